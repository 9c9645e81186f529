"""Per-tract statistics across samples (tjamd_tract_stats / tjamd_tract_sample_stats) without a GPU: the entry points are
exported and refuse bad arguments before any device call, and the numpy restatement of the reference's formulas that the
GPU tests (tests/test_tract_stats.py) compare against reproduces values computed by hand.

The restatement follows src/genome_set.c term by term, the histogram's bars in the reference's order:
descriptive_stats_of_histogram (:738-766), relative_difference_of_vector (:768-779),
update_descriptive_stats_for_this_trait (:692-710, the rule with the reference tract length only when lengths are given:
this project has no mapper).  A tract is a run of union rows with one id, a
sample's histogram in it is its rows with a non-zero count (length, count), one bar per row."""
import ctypes as C
import math

import numpy as np
import pytest

import tatajuba_amd as tj

N_STATS = 5                                     # DESC_STAT_avgelength, _modalfreq, _propcov, _covpercontext, _entropy (:23-24)
DBL_MIN = float(np.finfo(np.float64).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


def _div(a, b):
    """C's double division (inf / nan instead of an exception)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def signed_length(meta):
    v = (np.asarray(meta, dtype=np.uint64) >> np.uint64(2)) & np.uint64(0x3FF)
    v = v.astype(np.int64)
    return np.where(v >= 0x200, v - 0x400, v)


def descriptive_stats_of_histogram(bars, coverage, n_context):
    """src/genome_set.c:738-766.  bars: [(length, freq)] of one sample in one tract (freq != 0).  They are summed in the
    order of the reference's h->i[]: highest freq first, the larger length first among equal freqs (the empfreq order
    this project restates).  The device sums them in union row order instead: the same terms in another
    order, which the tests' tolerance of 1e-12 covers."""
    integral = sum(f for _, f in bars)
    bars = sorted(bars, key=lambda b: (-b[1], -b[0]))
    result = [0.0] * N_STATS
    for length, freq in bars:                                               # :746-747
        if integral:
            result[0] += _div(freq * length, integral)
    modal = bars[0]                                                         # h->i[0]
    result[1] = _div(modal[1], integral)                                    # :749
    result[2] = _div(integral, coverage)                                    # :752
    result[3] = _div(integral, n_context)                                   # :755
    x = 0.0
    for _, freq in bars:                                                    # :757-761
        if integral:
            x = _div(freq, integral)
        result[4] += x * math.log(x)
    result[4] *= -1.0                                                       # :762
    return result, modal[0]


def relative_difference_of_vector(vec):
    """src/genome_set.c:768-779"""
    x_max, x_min = -FLT_MAX, FLT_MAX
    for v in vec:
        if x_max < v:
            x_max = v
        if x_min > v:
            x_min = v
    return (x_max - x_min) if x_max > DBL_MIN else 0.0


def restate_tract_stats(keys, mat, coverage, tract_ids=None, ref_length=None):
    """Every tract of a union (keys uint64 [n, 3], mat int32 [n, n_samples]): dict of first, n_rows, n_present, variable,
    reldiff [n_tracts, 5], values [n_tracts, 5, n_samples] (samples_per_trait, :696-698), modal_len, n_context, and
    difference (the sum that :703-706 compares with 1e-5)."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    mat = np.asarray(mat, dtype=np.int64)
    n, ns = mat.shape
    if tract_ids is None:                                                   # context-keyed ids (tjamd_tract_ids)
        ctx = np.zeros(n, bool)
        ctx[1:] = (keys[1:, 0] != keys[:-1, 0]) | (keys[1:, 1] != keys[:-1, 1]) | (((keys[1:, 2] ^ keys[:-1, 2]) & np.uint64(3)) != 0)
        tract_ids = np.cumsum(ctx)
    tract_ids = np.asarray(tract_ids)
    lengths = signed_length(keys[:, 2]).tolist()
    ctxkey = [(int(a), int(b), int(c) & 3) for a, b, c in keys]
    heads = [0] + [i for i in range(1, n) if tract_ids[i] != tract_ids[i - 1]] + [n]
    nt = len(heads) - 1
    out = {"first": np.array(heads[:-1], np.int64), "n_rows": np.diff(heads), "n_present": np.zeros(nt, np.int64),
           "variable": np.zeros(nt, np.int64), "reldiff": np.zeros((nt, N_STATS)), "difference": np.zeros(nt),
           "values": np.zeros((nt, N_STATS, ns)), "modal_len": np.zeros((nt, ns), np.int64), "n_context": np.zeros((nt, ns), np.int64)}
    cols = mat.tolist()
    for t in range(nt):
        lo, hi = heads[t], heads[t + 1]
        samples_per_trait = [0.0] * (N_STATS * ns)                          # :696
        present = []
        for s in range(ns):
            rows = [r for r in range(lo, hi) if cols[r][s] != 0]
            if not rows:
                continue
            bars = [(lengths[r], cols[r][s]) for r in rows]
            n_context = len({ctxkey[r] for r in rows})
            stats, modal_len = descriptive_stats_of_histogram(bars, coverage[s], n_context)
            for j in range(N_STATS):                                        # :697-698
                samples_per_trait[s + ns * j] = stats[j]
            present.append(s)
            out["modal_len"][t, s], out["n_context"][t, s] = modal_len, n_context
        for j in range(N_STATS):
            out["values"][t, j] = samples_per_trait[ns * j: ns * (j + 1)]
            out["reldiff"][t, j] = relative_difference_of_vector([samples_per_trait[ns * j + s] for s in present])
        out["n_present"][t] = len(present)
        difference = out["reldiff"][t, 0]                                   # :703-705
        difference += out["reldiff"][t, 1]
        difference += out["reldiff"][t, 4]
        out["difference"][t] = difference
        ref = int(ref_length[t]) if ref_length is not None else 0
        out["variable"][t] = int(len(present) < ns                          # :700
                                 or difference > 1.e-5                      # :706
                                 or (ref > 0 and any(out["modal_len"][t, s] != ref for s in present)))   # :707
    return out


def tsv_field(v, precision):
    """print_descriptive_stats_per_sample (:728-729): "%.*lf" if > 0, else empty"""
    return "%.*f" % (precision, v) if v > 0. else ""


def record(base, ctx0, ctx1, length, count=1):
    meta = (base & 3) | ((length & 0x3FF) << 2) | ((count & 0xFFFFF) << 12) | (0xffe << 32)
    return (ctx0, ctx1, meta)


def test_tract_stats_entries_are_exported():
    L = tj.lib()
    for s in ("tjamd_tract_stats", "tjamd_tract_sample_stats", "tjamd_last_tract_stats_ms"):
        assert s in tj.EXPORTS and hasattr(L, s)
    assert tj.TRACT_SUMMARY_DTYPE.itemsize == 56
    assert L.tjamd_last_tract_stats_ms(None) == -1.0


def test_tract_stats_entries_check_their_arguments_without_a_gpu():
    """every bad argument is refused with a message before any device call (so: also without a GPU)"""
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    cov = (C.c_int * 4)(5, 5, 5, 5)
    nv = C.c_long(7)

    def stats(c=None, keys=fake, counts=fake, n=10, ns=2, ids=None, coverage=cov, summ=fake, var=fake, cap=10):
        rc = L.tjamd_tract_stats(c, keys, counts, n, ns, ids, coverage, None, summ, var, cap, C.byref(nv))
        return rc, L.tjamd_last_error().decode()

    def sample(c=None, keys=fake, counts=fake, n=10, ns=2, coverage=cov, summ=fake, nt=3, lst=fake, nl=2, vals=fake):
        rc = L.tjamd_tract_sample_stats(c, keys, counts, n, ns, coverage, summ, nt, lst, nl, vals, None, None)
        return rc, L.tjamd_last_error().decode()

    ERR_ARG, ERR_CAP = 3, 4
    for kw, rc, msg in [({}, ERR_ARG, "null counter"),
                        ({"ns": 0}, ERR_ARG, "n_samples 0 outside 1..4096"),
                        ({"ns": 4097}, ERR_ARG, "n_samples 4097 outside 1..4096"),
                        ({"keys": None}, ERR_ARG, "null union buffers"),
                        ({"counts": None}, ERR_ARG, "null union buffers"),
                        ({"coverage": None}, ERR_ARG, "null coverage"),
                        ({"summ": None}, ERR_ARG, "null summary buffer"),
                        ({"n": -1}, ERR_ARG, "n_union -1 < 0"),
                        ({"cap": 0}, ERR_CAP, "capacity 0 for a union of 10 rows"),
                        ({"cap": -3}, ERR_CAP, "capacity -3")]:
        got, err = stats(**kw)
        assert got == -rc and err.startswith("tjamd_tract_stats") and msg in err, (kw, got, err)
    for kw, rc, msg in [({}, ERR_ARG, "null counter"),
                        ({"ns": 0}, ERR_ARG, "n_samples 0 outside 1..4096"),
                        ({"ns": 5000}, ERR_ARG, "outside 1..4096"),
                        ({"keys": None}, ERR_ARG, "null union buffers"),
                        ({"coverage": None}, ERR_ARG, "null coverage"),
                        ({"lst": None}, ERR_ARG, "null summary, list or values buffer"),
                        ({"vals": None}, ERR_ARG, "null summary, list or values buffer"),
                        ({"nt": 11}, ERR_ARG, "n_tracts 11"),
                        ({"nl": -1}, ERR_ARG, "n_list -1")]:
        got, err = sample(**kw)
        assert got == -rc and err.startswith("tjamd_tract_sample_stats") and msg in err, (kw, got, err)
    # an empty union is no error, and touches nothing
    assert L.tjamd_tract_stats(None, None, None, 0, 2, None, cov, None, None, None, 0, None) == -ERR_ARG   # (still: no counter)


def three_row_union():
    """two samples; tract 0 = rows 0-1 (one context, lengths 6 and 5), tract 1 = row 2 (another context, length 7)"""
    keys = np.array([record(1, 0xAB, 0xCD, 6), record(1, 0xAB, 0xCD, 5), record(0, 0x12, 0x34, 7)], dtype=np.uint64)
    mat = np.array([[3, 0], [1, 4], [2, 2]], dtype=np.int32)
    return keys, mat, [8, 4]


def test_restatement_reproduces_hand_computed_values():
    keys, mat, cov = three_row_union()
    r = restate_tract_stats(keys, mat, cov)
    assert list(r["first"]) == [0, 2] and list(r["n_rows"]) == [2, 1] and list(r["n_present"]) == [2, 2]
    h0 = -(0.75 * math.log(0.75) + 0.25 * math.log(0.25))                   # sample 0 of tract 0: bars (6, 3), (5, 1)
    want = [[5.75, 5.0], [0.75, 1.0], [0.5, 1.0], [4.0, 4.0], [h0, 0.0]]    # sample 1: one bar (5, 4)
    assert np.allclose(r["values"][0], want, rtol=0, atol=1e-15)
    assert r["values"][0, 4, 1] == 0.0                                      # one bar: entropy exactly 0
    assert list(r["modal_len"][0]) == [6, 5] and list(r["n_context"][0]) == [1, 1]
    assert np.allclose(r["reldiff"][0], [0.75, 0.25, 0.5, 0.0, h0], rtol=0, atol=1e-15)
    assert r["variable"][0] == 1
    assert np.array_equal(r["values"][1], [[7.0, 7.0], [1.0, 1.0], [0.25, 0.5], [2.0, 2.0], [0.0, 0.0]])
    assert list(r["reldiff"][1]) == [0.0, 0.0, 0.25, 0.0, 0.0] and r["variable"][1] == 0
    assert restate_tract_stats(keys, mat, cov, ref_length=[0, 8])["variable"][1] == 1     # modal length 7 != reference 8
    assert restate_tract_stats(keys, mat, cov, ref_length=[0, 7])["variable"][1] == 0
    # one id for both tracts: two contexts for sample 0 and 1, coverage per context = integral / 2
    r1 = restate_tract_stats(keys, mat, cov, tract_ids=[0, 0, 0])
    assert list(r1["n_context"][0]) == [2, 2] and list(r1["values"][0, 3]) == [3.0, 3.0]
    # absent sample: zeros, and the tract is variable
    r2 = restate_tract_stats(keys, np.array([[3, 0], [1, 0], [2, 2]], np.int32), cov)
    assert r2["n_present"][0] == 1 and r2["variable"][0] == 1 and not r2["values"][0, :, 1].any()
    # count tie: the larger length is modal
    r3 = restate_tract_stats(keys, np.array([[2, 2], [2, 2], [2, 2]], np.int32), cov)
    assert list(r3["modal_len"][0]) == [6, 6]
    assert [tsv_field(v, p) for v, p in [(5.75, 2), (0.0, 2), (-0.0, 5), (0.123456, 5)]] == ["5.75", "", "", "0.12346"]
