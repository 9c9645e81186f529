"""Tracts across samples by grouping (tjamd_union_tracts / tjamd_union_tract_stats / tjamd_union_tract_sample_stats)
without a GPU: the entries are exported and refuse bad arguments before any device call, the structures match the
header, and the numpy restatement that the GPU tests (tests/test_union_tracts.py) compare against reproduces values
computed by hand.

The restatement: the tracts are the context histograms of new_genomic_context_list's grouping (the oracle,
orc.genomic_context_list) on the union rows pooled as one sample, a row's count being its total over the samples; a
sample's histogram in a tract is its non-zero rows summed per length (the reference's h, src/context_histogram.c:278-286),
summarised by descriptive_stats_of_histogram (src/genome_set.c:738-766) and relative_difference_of_vector (:768-779), as
fill_g_tract_summary_tables (:347-378) does; the tract is variable by the rule of tjamd_tract_stats and selected by
print_selected_g_tract_vector's (:390-397)."""
import ctypes as C
import math

import numpy as np

import tatajuba_amd as tj
from oracle import orc
from tests.test_tract_stats_cabi import N_STATS, descriptive_stats_of_histogram, relative_difference_of_vector, record, signed_length

AVG, MODAL, PROP, CPC, ENT = range(N_STATS)                 # TJAMD_STAT_* order
ERR_ARG, ERR_CAP = 3, 4


def pooled_elements(keys, counts_of_rows):
    """the union rows as one sample's hopo_elements (orc.ELEM_DTYPE), count field = counts_of_rows (each < 2^19)"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    cnt = np.asarray(counts_of_rows, dtype=np.int64)
    assert (cnt >= 0).all() and (cnt < (1 << 19)).all()
    e = np.zeros(len(keys), dtype=orc.ELEM_DTYPE)
    e["ctx0"], e["ctx1"] = keys[:, 0], keys[:, 1]
    meta = keys[:, 2] & ~np.uint64(0xFFFFF << 12)
    e["meta"] = meta | (cnt.astype(np.uint64) << np.uint64(12))
    e["read_offset"] = 0
    e["loc_ref_id"] = e["loc_pos"] = e["loc_last"] = -1
    return e


def count_ranks(totals):
    """1 + dense rank of each total: the grouping compares counts only, so the oracle (20-bit counts) groups by the ranks
    as by the exact totals"""
    t = np.asarray(totals, dtype=np.int64)
    _, inv = np.unique(t, return_inverse=True)
    return inv.astype(np.int64) + 1


def oracle_union_grouping(keys, mat, k, maxd, lev, free_end=False):
    """orc.genomic_context_list on the union pooled by exact totals: dict of tract_id, join_type, groups (orc) and
    lev_distance per tract (the edit distance between the name of each row joined by the retry and the modal name at
    that moment, by orc.levenshtein), mode (by totals) and integral (summed totals)"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    totals = np.asarray(mat, dtype=np.int64).sum(axis=1)
    orc.set_edit_free_end(free_end)
    r = orc.genomic_context_list(pooled_elements(keys, count_ranks(totals)), k, maxd, lev, 1)
    gof, jt = r["group_of"], r["join_type"]
    ng = len(r["groups"])
    name = lambda i: orc.name_of(keys[i, 0], keys[i, 1], int(keys[i, 2]) & 3, k)
    lev_d, mode, integral = np.zeros(ng, np.int64), np.zeros(ng, np.int64), np.zeros(ng, np.int64)
    first = r["groups"]["first"]
    for g in range(ng):
        lo = int(first[g])
        hi = int(first[g + 1]) if g + 1 < ng else len(keys)
        best = lo
        for i in range(lo, hi):
            if i > lo and jt[i] == 2:
                lev_d[g] = max(lev_d[g], orc.levenshtein(name(best), name(i), free_end=free_end))
            if totals[i] > totals[best]:
                best = i
        mode[g] = int(np.argmax(totals[lo:hi])) + lo            # (argmax: the first of equal totals)
        integral[g] = int(totals[lo:hi].sum())
    return {"tract_id": gof, "join_type": jt, "groups": r["groups"], "lev_distance": lev_d, "mode": mode, "integral": integral}


def restate_union_tract_stats(keys, mat, coverage, tract_ids, lev_distance, ref_length=None):
    """Every tract (tract_ids: one per row, contiguous) of a union: dict of first, n_rows, n_present, variable, selected,
    lev_distance, reldiff [nt, 5] (TJAMD_STAT_* order), values [nt, 5, ns], modal_len, n_context, n_len, difference"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    mat = np.asarray(mat, dtype=np.int64)
    n, ns = mat.shape
    tract_ids = np.asarray(tract_ids)
    lengths = signed_length(keys[:, 2]).tolist()
    ctxkey = [(int(a), int(b), int(c) & 3) for a, b, c in keys]
    heads = [0] + [i for i in range(1, n) if tract_ids[i] != tract_ids[i - 1]] + [n]
    nt = len(heads) - 1
    out = {"first": np.array(heads[:-1], np.int64), "n_rows": np.diff(heads), "n_present": np.zeros(nt, np.int64),
           "variable": np.zeros(nt, np.int64), "selected": np.zeros(nt, np.int64), "lev_distance": np.asarray(lev_distance, np.int64),
           "reldiff": np.zeros((nt, N_STATS)), "difference": np.zeros(nt), "values": np.zeros((nt, N_STATS, ns)),
           "modal_len": np.zeros((nt, ns), np.int64), "n_context": np.zeros((nt, ns), np.int64), "n_len": np.zeros((nt, ns), np.int64)}
    cols = mat.tolist()
    for t in range(nt):
        lo, hi = heads[t], heads[t + 1]
        present = []
        for s in range(ns):
            rows = [r for r in range(lo, hi) if cols[r][s] != 0]
            if not rows:
                continue
            per_length = {}
            for r in rows:                                                  # one bar per length (the reference's h)
                per_length[lengths[r]] = per_length.get(lengths[r], 0) + cols[r][s]
            bars = list(per_length.items())
            n_context = len({ctxkey[r] for r in rows})
            stats, modal_len = descriptive_stats_of_histogram(bars, coverage[s], n_context)
            out["values"][t, :, s] = stats
            out["modal_len"][t, s], out["n_context"][t, s], out["n_len"][t, s] = modal_len, n_context, len(bars)
            present.append(s)
        for j in range(N_STATS):
            out["reldiff"][t, j] = relative_difference_of_vector([out["values"][t, j, s] for s in present])
        out["n_present"][t] = len(present)
        difference = out["reldiff"][t, AVG]
        difference += out["reldiff"][t, MODAL]
        difference += out["reldiff"][t, ENT]
        out["difference"][t] = difference
        ref = int(ref_length[t]) if ref_length is not None else 0
        out["variable"][t] = int(len(present) < ns or difference > 1.e-5 or (ref > 0 and any(out["modal_len"][t, s] != ref for s in present)))
        rd = out["reldiff"][t]
        out["selected"][t] = int(len(present) < ns or out["lev_distance"][t] > 0 or rd[MODAL] > 1e-6 or rd[AVG] > 1e-6 or rd[ENT] > 1e-6)
    return out


SELECTED_HEADER = "tract_id\tbegin_context\tn_genomes\tlev_distance\t|\trd_frequency\trd_avge_tract_length\trd_coverage\trd_context_covge\trd_entropy\n"
ANNOTATED_HEADER = ("tract_id\tGFF3_info\tbegin_context\tn_genomes\tlev_distance\t|\trd_frequency\trd_avge_tract_length\trd_coverage\t"
                    "rd_context_covge\trd_entropy\n")


def selected_line(t, n_present, lev_distance, reldiff):
    """one line of selected_tracts_unknown.tsv (print_selected_g_tract_vector, src/genome_set.c:406-411): location -1,
    reldiff in the reference's order (modal freq, avg length, prop coverage, coverage per context, entropy)"""
    ref_order = [reldiff[MODAL], reldiff[AVG], reldiff[PROP], reldiff[CPC], reldiff[ENT]]
    return "tid_%06d\t%8d\t%5d\t%5d\t|\t" % (t, -1, n_present, lev_distance) + "".join("%8.6f\t" % v for v in ref_order) + "\n"


# ---- a two-sample union by hand, k = 4, base C, left flank TTTT ----------------------------------------------------
#   row 0  right ACGT  len 6  counts [3, 0]   opens tract 0
#   row 1  right ACGT  len 5  counts [1, 2]   same context: joins (type 1)
#   row 2  right ACGA  len 5  counts [0, 4]   one substitution: joins within max_distance_per_flank 2 (type 1, a new context)
#   row 3  right TACG  len 7  counts [2, 2]   4 substitutions from ACGT: fails the flank test; the modal row is row 2 (total
#                                             4), edit distance TTTT.C.ACGA -> TTTT.C.TACG = 2 < 3: joins by the retry
#   row 4  base A, AAAA|AAAA, len 8, counts [5, 5]: opens tract 1
K, MAXD, LEV = 4, 2, 3
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
pack = lambda s: sum(_CODE[ch] << (2 * i) for i, ch in enumerate(s))


def hand_union():
    keys = np.array([record(1, pack("TTTT"), pack("ACGT"), 6), record(1, pack("TTTT"), pack("ACGT"), 5),
                     record(1, pack("TTTT"), pack("ACGA"), 5), record(1, pack("TTTT"), pack("TACG"), 7),
                     record(0, pack("AAAA"), pack("AAAA"), 8)], dtype=np.uint64)
    mat = np.array([[3, 0], [1, 2], [0, 4], [2, 2], [5, 5]], dtype=np.int32)
    return keys, mat, [10, 8]


def test_union_tract_entries_are_exported_and_laid_out_as_the_header():
    L = tj.lib()
    for s in ("tjamd_union_tracts", "tjamd_union_tract_stats", "tjamd_union_tract_sample_stats", "tjamd_last_union_tracts_ms",
              "tjamd_last_union_tract_stats_ms", "tjamd_last_union_tract_candidates"):
        assert s in tj.EXPORTS and hasattr(L, s)
    assert tj.UNION_TRACT_DTYPE.itemsize == 32 and tj.UNION_TRACT_SUMMARY_DTYPE.itemsize == 64
    f = tj.UNION_TRACT_DTYPE.fields
    assert [f[x][1] for x in ("first", "n_rows", "n_context", "mode", "indel", "lev_distance", "integral")] == [0, 4, 8, 12, 16, 20, 24]
    f = tj.UNION_TRACT_SUMMARY_DTYPE.fields
    assert [f[x][1] for x in ("first", "n_rows", "n_present", "variable", "selected", "lev_distance", "reldiff")] == [0, 4, 8, 12, 16, 20, 24]
    assert L.tjamd_last_union_tracts_ms(None) == -1.0 and L.tjamd_last_union_tract_stats_ms(None) == -1.0
    assert L.tjamd_last_union_tract_candidates(None) == -1


def test_union_tract_entries_check_their_arguments_without_a_gpu():
    """every bad argument is refused with a message before any device call (so: also without a GPU)"""
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    cov = (C.c_int * 4)(5, 5, 5, 5)
    nv, nsel = C.c_long(7), C.c_long(7)

    def tracts(c=None, keys=fake, counts=fake, n=10, ns=2, maxd=1, lev=2, ids=fake, tr=fake, cap=10):
        rc = L.tjamd_union_tracts(c, keys, counts, n, ns, maxd, lev, ids, None, tr, cap)
        return rc, L.tjamd_last_error().decode()

    def stats(c=None, keys=fake, counts=fake, n=10, ns=2, tr=fake, nt=3, coverage=cov, summ=fake):
        rc = L.tjamd_union_tract_stats(c, keys, counts, n, ns, tr, nt, coverage, None, summ, fake, C.byref(nv), fake, C.byref(nsel))
        return rc, L.tjamd_last_error().decode()

    def sample(c=None, keys=fake, counts=fake, n=10, ns=2, coverage=cov, summ=fake, nt=3, lst=fake, nl=2, vals=fake):
        rc = L.tjamd_union_tract_sample_stats(c, keys, counts, n, ns, coverage, summ, nt, lst, nl, vals, None, None, None)
        return rc, L.tjamd_last_error().decode()

    for fn, call, cases in [
        ("tjamd_union_tracts", tracts, [({}, ERR_ARG, "null counter"),
                                        ({"ns": 0}, ERR_ARG, "n_samples 0 outside 1..4096"),
                                        ({"ns": 4097}, ERR_ARG, "n_samples 4097 outside 1..4096"),
                                        ({"keys": None}, ERR_ARG, "null union buffers"),
                                        ({"counts": None}, ERR_ARG, "null union buffers"),
                                        ({"ids": None}, ERR_ARG, "null tract id or tract buffer"),
                                        ({"tr": None}, ERR_ARG, "null tract id or tract buffer"),
                                        ({"n": -1}, ERR_ARG, "n_union -1 < 0"),
                                        ({"n": 1 << 31}, ERR_CAP, "union rows"),
                                        ({"maxd": -1}, ERR_ARG, "negative distance"),
                                        ({"lev": -2}, ERR_ARG, "negative distance"),
                                        ({"cap": 0}, ERR_CAP, "capacity 0 for a union of 10 rows"),
                                        ({"cap": -3}, ERR_CAP, "capacity -3")]),
        ("tjamd_union_tract_stats", stats, [({}, ERR_ARG, "null counter"),
                                            ({"ns": 0}, ERR_ARG, "n_samples 0 outside 1..4096"),
                                            ({"ns": 4097}, ERR_ARG, "outside 1..4096"),
                                            ({"keys": None}, ERR_ARG, "null union buffers"),
                                            ({"counts": None}, ERR_ARG, "null union buffers"),
                                            ({"coverage": None}, ERR_ARG, "null coverage"),
                                            ({"tr": None}, ERR_ARG, "null tract or summary buffer"),
                                            ({"summ": None}, ERR_ARG, "null tract or summary buffer"),
                                            ({"nt": 0}, ERR_ARG, "n_tracts 0 for a union of 10 rows"),
                                            ({"nt": 11}, ERR_ARG, "n_tracts 11 for a union of 10 rows"),
                                            ({"n": -1}, ERR_ARG, "n_union -1 < 0")]),
        ("tjamd_union_tract_sample_stats", sample, [({}, ERR_ARG, "null counter"),
                                                    ({"ns": 0}, ERR_ARG, "n_samples 0 outside 1..4096"),
                                                    ({"ns": 5000}, ERR_ARG, "outside 1..4096"),
                                                    ({"keys": None}, ERR_ARG, "null union buffers"),
                                                    ({"coverage": None}, ERR_ARG, "null coverage"),
                                                    ({"summ": None}, ERR_ARG, "null summary, list or values buffer"),
                                                    ({"lst": None}, ERR_ARG, "null summary, list or values buffer"),
                                                    ({"vals": None}, ERR_ARG, "null summary, list or values buffer"),
                                                    ({"nt": 11}, ERR_ARG, "n_tracts 11"),
                                                    ({"nl": -1}, ERR_ARG, "n_list -1")])]:
        for kw, rc, msg in cases:
            got, err = call(**kw)
            assert got == -rc and err.startswith(fn) and msg in err, (fn, kw, got, err)
    assert nv.value == 7 and nsel.value == 7                 # (untouched: every call failed before reaching them)


def test_oracle_groups_the_hand_built_union():
    keys, mat, _ = hand_union()
    g = oracle_union_grouping(keys, mat, K, MAXD, LEV)
    assert g["tract_id"].tolist() == [0, 0, 0, 0, 1] and g["join_type"].tolist() == [0, 1, 1, 2, 0]
    assert g["groups"]["n_context"].tolist() == [3, 1] and g["groups"]["indel"].tolist() == [1, 0]
    assert g["lev_distance"].tolist() == [2, 0] and orc.levenshtein("TTTT.C.ACGA", "TTTT.C.TACG") == 2
    assert g["mode"].tolist() == [2, 4] and g["integral"].tolist() == [14, 10]
    # without the retry, row 3 opens a tract of its own; with counts of 20 bits the ranks stand for the totals
    assert oracle_union_grouping(keys, mat, K, MAXD, 0)["tract_id"].tolist() == [0, 0, 0, 1, 2]
    assert count_ranks([5, (1 << 40) + 1, 5, 0]).tolist() == [2, 3, 2, 1]


def test_restatement_reproduces_hand_computed_values():
    keys, mat, cov = hand_union()
    g = oracle_union_grouping(keys, mat, K, MAXD, LEV)
    r = restate_union_tract_stats(keys, mat, cov, g["tract_id"], g["lev_distance"])
    assert r["first"].tolist() == [0, 4] and r["n_rows"].tolist() == [4, 1] and r["n_present"].tolist() == [2, 2]
    # sample 0: rows 0, 1, 3 -> bars (6, 3), (7, 2), (5, 1), integral 6, contexts ACGT and TACG
    # sample 1: rows 1, 2, 3 -> lengths 5 + 5 summed: bars (5, 6), (7, 2), integral 8, contexts ACGT, ACGA, TACG
    h0 = -(0.5 * math.log(0.5) + (1 / 3) * math.log(1 / 3) + (1 / 6) * math.log(1 / 6))
    h1 = -(0.75 * math.log(0.75) + 0.25 * math.log(0.25))
    want = [[37 / 6, 5.5], [0.5, 0.75], [0.6, 1.0], [3.0, 8 / 3], [h0, h1]]
    assert np.allclose(r["values"][0], want, rtol=0, atol=1e-15)
    assert r["modal_len"][0].tolist() == [6, 5] and r["n_context"][0].tolist() == [2, 3] and r["n_len"][0].tolist() == [3, 2]
    assert np.allclose(r["reldiff"][0], [37 / 6 - 5.5, 0.25, 0.4, 1 / 3, abs(h0 - h1)], rtol=0, atol=1e-15)
    assert r["variable"][0] == 1 and r["selected"][0] == 1 and r["lev_distance"][0] == 2
    # tract 1: the same histogram in both samples; only the coverage differs, which neither rule reads
    assert r["values"][1].tolist() == [[8.0, 8.0], [1.0, 1.0], [0.5, 0.625], [5.0, 5.0], [0.0, 0.0]]
    assert r["variable"][1] == 0 and r["selected"][1] == 0 and r["reldiff"][1, PROP] == 0.125
    # lev_distance alone selects a tract; a modal length off the reference length makes it variable
    assert restate_union_tract_stats(keys[:4], np.array([[1, 1]] * 4), cov, [0] * 4, [1])["selected"].tolist() == [1]
    assert restate_union_tract_stats(keys[:4], np.array([[1, 1]] * 4), cov, [0] * 4, [0])["selected"].tolist() == [0]
    assert restate_union_tract_stats(keys, mat, cov, g["tract_id"], g["lev_distance"], ref_length=[0, 9])["variable"].tolist() == [1, 1]
    # per row (one bar per row, as tjamd_tract_stats) sample 1's modal frequency would be 4 / 8, not 6 / 8
    assert selected_line(0, 2, 2, r["reldiff"][0]) == "tid_000000\t      -1\t    2\t    2\t|\t0.250000\t0.666667\t0.400000\t0.333333\t%8.6f\t\n" % abs(h0 - h1)
