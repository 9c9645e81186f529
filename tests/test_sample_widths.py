"""Every segment width of the cross-sample kernels.  tract_stats_kernel, tract_sample_stats_kernel, union_totals_kernel
and the union statistics kernels give a tract (or a row) a segment of S = min(64, next_pow2(n_samples)) lanes, a lane
taking samples lane, lane + S, ...; the other tests run 1, 2, 3, 8 and 70 samples, so S = 1, 2, 4, 8 and 64 with two
strides at most.  Here: S = 2, 4, 16, 32 and 64, sample counts just beyond a power of two, three and four strides, and the
4096 samples that the entries accept at most -- through tjamd_tract_stats / tjamd_tract_sample_stats, tjamd_union_tracts
and its two statistics entries, and tjamd_located_tracts (union_totals_kernel, lt_gather_counts_kernel), against the
restatements at the suite's tolerances, every output in a guarded buffer (tests/bounds_calls.py).

What can go wrong with the width is a reduction over the segment that stops short of S lanes and a lane's walk over
its samples that loses a stride; the choice of S itself is one of speed (a segment of 64 lanes for every sample count
gives the same values).  Planted in every union, for what those two would get wrong:
  last      a tract whose samples are all in the last stride (s >= S * floor((n_samples - 1) / S))
  one       a tract present in exactly one sample, the last
  off_ref   a tract whose samples agree in average length, modal frequency and entropy, so that it is variable only by the
            reference length, and only through the last sample's modal length
  big       a tract whose first row totals more than 2^31 over the samples (2^32 at 4096 samples of 2^20): totals, integral
            and the modal row are exact in 64 bits
The seeds are such that the restatement alone puts no tract within 1e-9 of the 1e-5 threshold: asserted below."""
import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests import bounds_calls as bc
from tests.bounds_calls import Union
from tests.test_locate import check_located_tracts
from tests.test_locate_cabi import restate_located_tracts
from tests.test_tract_stats import check_against_restatement
from tests.test_tract_stats_cabi import restate_tract_stats, signed_length
from tests.test_union_tracts import check_grouping, check_stats, family_rows, sample_records, union_of_samples
from tests.test_union_tracts_cabi import oracle_union_grouping, restate_union_tract_stats

pytestmark = pytest.mark.gpu

K, MAXD, LEV = 10, 1, 2
N_SAMPLES = (2, 4, 9, 16, 17, 32, 33, 64, 65, 129, 200, 4096)
PLANTS = {"last": (1, 0x3AAAA, 0x15555), "one": (0, 0x2BCDE, 0x0F0F0), "off_ref": (1, 0x1C3A5, 0x2D4B6), "big": (0, 0x0ACE1, 0x3BDF2)}
OFF_REF_LENGTH, BIG_LENGTH = 7, 10


def segment(ns):
    S = 1
    while S < ns and S < 64:
        S <<= 1
    return S


def build(ns):
    """-> (Union, {plant: its rows in the union}, the big row's count per sample)"""
    S = segment(ns)
    s0 = S * ((ns - 1) // S)
    rows = family_rows(K, ns, 1000 + ns, n_fam=120 if ns < 4096 else 6)      # a few hundred rows; a few dozen at 4096 samples
    assert not any(key[:3] in PLANTS.values() for key in rows)
    for length in (6, 5):
        rows[PLANTS["last"] + (length,)] = [0 if s < s0 else 5 + (s + length) % 7 for s in range(ns)]
    rows[PLANTS["one"] + (9,)] = [0] * (ns - 1) + [13]
    for length in (4, 5, 7, 8):                                               # all but the last sample: 5 and 7, ten each; the last: 4 and 8
        rows[PLANTS["off_ref"] + (length,)] = [10 if (s == ns - 1) == (length in (4, 8)) else 0 for s in range(ns)]
    rows[PLANTS["big"] + (BIG_LENGTH,)] = [1] * ns                           # (the merge's count field has 20 bits: the counts come below)
    rows[PLANTS["big"] + (6,)] = [100] * ns
    keys, mat = union_of_samples(sample_records(rows, ns))
    keys, mat = np.asarray(keys, np.uint64).reshape(-1, 3), np.array(mat, np.int32)
    where = {name: np.flatnonzero((keys[:, 0] == c0) & (keys[:, 1] == c1) & ((keys[:, 2] & np.uint64(3)) == base)) for name, (base, c0, c1) in PLANTS.items()}
    assert [len(where[name]) for name in ("last", "one", "off_ref", "big")] == [2, 1, 4, 2]
    per = max(1 << 20, (1 << 31) // ns + 7)
    big_row = where["big"][0]
    assert signed_length(keys[big_row: big_row + 1, 2])[0] == BIG_LENGTH and per < (1 << 31) and per * ns > (1 << 31)
    mat[big_row, :] = per
    cov = np.random.default_rng(ns).integers(20, 80, ns).tolist()
    return Union(keys, mat, cov), where, per


def reference_lengths(nt, off_ref_tract, seed):
    ref = np.random.default_rng(seed).integers(-1, 12, nt).astype(np.int32)
    ref[off_ref_tract] = OFF_REF_LENGTH
    return ref


@pytest.mark.parametrize("ns", N_SAMPLES)
def test_segment_widths(ns):
    u, where, per = build(ns)
    S = segment(ns)
    s0 = S * ((ns - 1) // S)
    big_total = ns * per
    assert big_total > (1 << 31) and (ns != 4096 or (per == 1 << 20 and big_total == 1 << 32))
    c = tj.Counter(K)

    # ---- the context-keyed tracts: tjamd_tract_stats, tjamd_tract_sample_stats
    ids, nt = orc.tract_ids(u.keys)
    tract = {name: int(ids[r[0]]) for name, r in where.items()}
    assert all((ids[r] == tract[name]).all() and (ids == tract[name]).sum() == len(r) for name, r in where.items())
    ref = reference_lengths(nt, tract["off_ref"], ns)
    for given in (None, ref):
        want = restate_tract_stats(u.keys, u.mat, u.cov, ref_length=given)
        assert not (np.abs(want["difference"] - 1e-5) <= 1e-9).any()
        got_nt, got = bc.tract_stats_of(c, u, nt, ref=bc.dev(given, np.int32) if given is not None else None)
        assert got_nt == nt, got
        assert check_against_restatement(got, want) == 0
        s = got["summary"]
        assert s["n_present"][tract["last"]] == ns - s0 and not got["values"][tract["last"], :, :s0].any() and (got["values"][tract["last"], 0, s0:] > 0).all()
        assert s["n_present"][tract["one"]] == 1 and got["modal_len"][tract["one"]].tolist() == [0] * (ns - 1) + [9]
        t = tract["off_ref"]
        assert s["n_present"][t] == ns and (s["reldiff"][t][[0, 1, 4]] == 0.0).all() and s["variable"][t] == (1 if given is not None else 0)
        assert got["modal_len"][t].tolist() == [7] * (ns - 1) + [8]
        t = tract["big"]
        assert s["n_present"][t] == ns and (got["values"][t, 3] == per + 100.0).all()            # coverage per context: the integral, one context

    # ---- the grouped tracts: tjamd_union_tracts and its statistics
    want_g = oracle_union_grouping(u.keys, u.mat, K, MAXD, LEV)
    tracts = bc.tracts_from_grouping(want_g, u.n)
    nt = len(tracts)
    gid = want_g["tract_id"]
    tract = {name: int(gid[r[0]]) for name, r in where.items()}
    assert all((gid[r] == tract[name]).all() and (gid == tract[name]).sum() == len(r) for name, r in where.items())   # each plant a tract of its own
    got_nt, got = bc.union_tracts_of(c, u, MAXD, LEV, nt)
    assert got_nt == nt, got
    check_grouping(got, want_g)
    check_stats(got, restate_union_tract_stats(u.keys, u.mat, u.cov, gid, want_g["lev_distance"]))
    big = got["tracts"][tract["big"]]
    assert big["integral"] == big_total + 100 * ns > (1 << 31) and big["mode"] == where["big"][0] and big["first"] == where["big"][0]
    assert got["summary"]["variable"][tract["off_ref"]] == 0 and got["summary"]["n_present"][tract["last"]] == ns - s0
    ref = reference_lengths(nt, tract["off_ref"], ns + 1)
    again = bc.union_stats_of(c, u, got["d_tracts"], nt, ref=bc.dev(ref, np.int32))
    check_stats(again, restate_union_tract_stats(u.keys, u.mat, u.cov, gid, want_g["lev_distance"], ref_length=ref))
    assert again["summary"]["variable"][tract["off_ref"]] == 1 and again["modal_len"][tract["off_ref"]].tolist() == [7] * (ns - 1) + [8]

    # ---- tracts by location: union_totals_kernel picks each tract's place and modal row, lt_gather_counts_kernel moves the rows
    loc = bc.planted_locations(u.keys, ns)
    loc[where["big"][0]] = (123456, 1, 456, 9, 0, 0, 1)                       # the big row is located, its tract's other row elsewhere:
    loc[where["big"][1]] = (77, 0, 77, 5, 1, 0, 2)                            # by exact totals the tract lies at the big row's place
    ld = bc.dev(loc)
    for given in (None, tracts):
        want = restate_located_tracts(u.keys, u.mat, given, loc)
        need = len(want["tracts"])
        got_nt, got = bc.located_tracts_of(c, u, bc.dev(given) if given is not None else None, nt if given is not None else 0, ld, need)
        assert got_nt == need, got
        check_located_tracts(got, want, u.keys, u.mat)
        at = int(np.flatnonzero(got["perm"] == where["big"][0])[0])
        t = int(np.searchsorted(got["tracts"]["first"], at, side="right")) - 1
        assert got["tract_loc"]["flat"][t] == 123456 and got["tracts"]["mode"][t] == at and got["tracts"]["integral"][t] >= big_total
        r = got["raw"]
        pu = Union(got["keys"], got["mat"], u.cov)
        stats = bc.union_stats_of(c, pu, r["d_out_tracts"].payload, need, ref=r["d_ref_length"].payload.view(bc.torch().int32))
        new_ids = np.repeat(np.arange(need), got["tracts"]["n_rows"])
        check_stats(stats, restate_union_tract_stats(got["keys"], got["mat"], u.cov, new_ids, got["tracts"]["lev_distance"], ref_length=got["ref_length"]))
    c.close()
