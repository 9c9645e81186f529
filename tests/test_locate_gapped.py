"""tjamd_reference_add_seeds / tjamd_locate_gapped on the GPU against the brute-force restatement of
tests/test_locate_gapped_cabi.py: the seed order leaves the index and tjamd_locate as they were, the lookup field for field
on exact, substituted, indel-bearing, inner-mutated, random and repeated queries at three (max_edits, max_shift), seed ranges
on both sides of the lane walk at row counts around the wavefront, rows all located or none located on entry, the
eight-sample pipeline of tests/test_locate.py, and examples/located_tracts.c with and without -g."""
import ctypes as C
import functools
import os
import random
import re
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests.test_locate import (_dev, _p, _raw, check_located_tracts, dev_locate, dev_located_tracts, queries_for, random_genome, same_entries,
                               selected_line_at)
from tests.test_locate_cabi import (CODE, LOCATIONS_HEADER, NOWHERE, _pack, contigs_of, location_line, restate_located_tracts, restate_locate,
                                    restate_reference_index)
from tests.test_locate_gapped_cabi import restate_locate_gapped, seed_ranges
from tests.test_union_tracts import DNA, _oracle_sample, device_union, make_genome, reads_of, sample_of
from tests.test_union_tracts_cabi import SELECTED_HEADER, oracle_union_grouping, restate_union_tract_stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 3
LOC, TR = tj.LOCATION_DTYPE, tj.UNION_TRACT_DTYPE
# the longest range a lane walks alone, as the kernels have it
LC_LANE_WALK = int(re.search(r"^#define\s+LC_LANE_WALK\s+(\d+)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "hopo_device.hip")).read(), re.M).group(1))
SETTINGS = ((1, 0), (2, 1), (4, 3))                      # (max_edits, max_shift)


def _torch():
    return pytest.importorskip("torch")


def dev_locate_gapped(counter, ref, keys, loc, max_edits, max_shift, n=None, with_how=True, on_device=False):
    """-> (rows located by the call, LOCATION_DTYPE per row, how per row or None), or (negative code, message, None)"""
    torch = _torch()
    kd = keys if on_device else _dev(np.asarray(keys, np.uint64).reshape(-1, 3))
    n = kd.numel() // 24 if n is None else n
    ld = _dev(np.asarray(loc, LOC)) if len(loc) else torch.zeros(32, dtype=torch.uint8, device="cuda")
    how = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda") if with_how else None
    torch.cuda.synchronize()
    got = tj.lib().tjamd_locate_gapped(counter._h, ref._h, _p(kd), n, max_edits, max_shift, _p(ld), _p(how))
    if got < 0:
        return got, tj.lib().tjamd_last_error().decode(), None
    return got, _raw(ld, LOC, len(loc)), how[:n].cpu().numpy() if with_how else None


def canonical(lc, rc, b):
    """a forward (left flank, right flank, base) as the scan stores it (restate_reference_index's rule) -> (ctx0, ctx1, base)"""
    if b < 2:
        return _pack(lc), _pack(rc), b
    return _pack([3 - c for c in reversed(rc)]), _pack([3 - c for c in reversed(lc)]), 3 - b


def gapped_queries(rng, stream, entries, k, n_each=100):
    """exact entries; one substitution in each flank; an insertion or deletion of 1 ... 3 bases in one flank, cut from the
    mutated genome window (a deletion pulls in the genome's next bases); a substitution in the inner half of both flanks;
    random keys; and every seventh context again with another length"""
    contigs = contigs_of(stream)
    h = (k + 1) // 2
    q = []

    def windows(e):
        """the forward flanks of an entry with 3 spare bases each, inner first, or None where the contig or ACGT ends"""
        s, pos, end = contigs[int(e["contig"])], int(e["pos"]), int(e["pos"]) + int(e["length"])
        if pos - k - 3 < 0 or end + k + 3 > len(s):
            return None
        lw, rw = s[pos - k - 3: pos][::-1], s[end: end + k + 3]
        if not all(c in CODE for c in lw + rw):
            return None
        return [CODE[c] for c in lw], [CODE[c] for c in rw], CODE[s[pos]]

    def key(lw, rw, b):
        c0, c1, base = canonical(list(reversed(lw[:k])), rw[:k], b)
        return (c0, c1, base | (rng.randrange(3, 12) << 2))

    kinds = {"exact": 0, "subs": 0, "indel": 0, "inner": 0}
    while min(kinds.values()) < n_each:
        w = windows(entries[rng.randrange(len(entries))])
        if w is None:
            continue
        lw, rw, b = list(w[0]), list(w[1]), w[2]
        kind = min(kinds, key=kinds.get)
        if kind == "subs":
            for f in (lw, rw):
                p = rng.randrange(k)
                f[p] = (f[p] + rng.randrange(1, 4)) & 3
        elif kind == "indel":
            f, p, s = rng.choice((lw, rw)), rng.randrange(k), rng.randrange(1, 4)
            if rng.random() < 0.5:
                f[p:p] = [rng.randrange(4) for _ in range(s)]
            else:
                del f[p:p + s]
        elif kind == "inner":
            for f in (lw, rw):
                p = rng.randrange(h)
                f[p] = (f[p] + rng.randrange(1, 4)) & 3
        kinds[kind] += 1
        q.append(key(lw, rw, b))
    q += [(rng.getrandbits(2 * k), rng.getrandbits(2 * k), rng.randrange(2) | (rng.randrange(3, 12) << 2)) for _ in range(n_each // 2)]
    q += [(a, b, (m & 3) | (20 << 2)) for a, b, m in q[::7]]
    return np.array(q, dtype=np.uint64)


def check_gapped(c, ref, entries, keys, first, k, max_edits, max_shift, n=None):
    """one call against the restatement: every field of every row, the rows located before byte for byte, d_how, the return
    value; -> (locations, how)"""
    n = len(keys) if n is None else n
    want, how = restate_locate_gapped(entries, keys[:n], first[:n], max_edits, max_shift, k)
    rc, got, got_how = dev_locate_gapped(c, ref, keys, first, max_edits, max_shift, n=n)
    assert rc >= 0, got
    assert got[:n].tobytes() == want.tobytes(), (k, max_edits, max_shift, np.flatnonzero(got[:n] != want)[:5])
    assert got[n:].tobytes() == first[n:].tobytes()                          # rows behind n are not touched
    assert (got_how == how).all() and rc == int((how == 1).sum()) and c.last_locate_gapped_ms() > 0
    before = first[:n]["flat"] >= 0
    assert got[:n][before].tobytes() == first[:n][before].tobytes() and (how[before] == 0).all() and (how[~before] != 0).all()
    return want, how


# ---- the seed order ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 13, 32])
def test_seed_order_leaves_the_index_and_the_first_pass_as_they_were(k):
    rng = random.Random(11 * k)
    g = random_genome(rng, 30000, k)
    entries, _ = restate_reference_index(g, k)
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    keys = queries_for(rng, entries, k, 100, 400)
    n1, loc1 = dev_locate(c, ref, keys, 1)
    assert not ref.has_seeds and c.last_seed_order_ms() == -1.0
    rc, err, _ = dev_locate_gapped(c, ref, keys, loc1, 2, 1)                  # refused before the order is there, nothing written
    assert rc == -ERR_ARG and err.startswith("tjamd_locate_gapped") and "no seed order" in err
    assert ref.add_seeds(c) == len(entries) == ref.n_entries and ref.has_seeds and c.last_seed_order_ms() > 0
    same_entries(ref.download(), entries)
    n2, loc2 = dev_locate(c, ref, keys, 1)
    assert n2 == n1 and loc2.tobytes() == loc1.tobytes() == restate_locate(entries, keys, 1).tobytes()
    assert ref.add_seeds(c) == len(entries) and ref.has_seeds                 # the second call returns at once
    check_gapped(c, ref, entries, keys, loc1, k, 2, 1)
    # the refusals that need both objects: another k, max_edits above k
    other = tj.Counter(k - 1)
    rc, err, _ = dev_locate_gapped(other, ref, keys, loc1, 1, 1)
    assert rc == -ERR_ARG and f"built with k = {k}, the counter has k = {k - 1}" in err
    assert tj.lib().tjamd_reference_add_seeds(other._h, ref._h) == -ERR_ARG and f"built with k = {k}" in tj.lib().tjamd_last_error().decode()
    other.close()
    rc, err, _ = dev_locate_gapped(c, ref, keys, loc1, k + 1, 1)
    assert rc == -ERR_ARG and f"max_edits {k + 1} outside 0..{k}" in err
    # an index without entries
    empty = tj.Reference(c, b"")
    assert empty.add_seeds(c) == 0 and empty.has_seeds
    rc, got, how = dev_locate_gapped(c, empty, keys, loc1, 2, 1)
    assert rc == 0 and got.tobytes() == loc1.tobytes() and ((how == 0) == (loc1["flat"] >= 0)).all() and ((how == -1) == (loc1["flat"] < 0)).all()
    empty.close()
    ref.close()
    c.close()


# ---- parity with the restatement -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,total", [(13, 60000), (25, 60000), (32, 30000), (7, 60000)])
def test_locate_gapped_matches_the_restatement(k, total):
    rng = random.Random(37 * k)
    g = random_genome(rng, total, k)
    entries, _ = restate_reference_index(g, k)
    keys = gapped_queries(rng, g, entries, k)
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    assert ref.add_seeds(c) == len(entries)
    n1, first = dev_locate(c, ref, keys, 1)
    assert first.tobytes() == restate_locate(entries, keys, 1).tobytes() and (first["flat"] >= 0).any() and (first["flat"] < 0).any()
    seen = set()
    for max_edits, max_shift in SETTINGS:
        want, how = check_gapped(c, ref, entries, keys, first, k, max_edits, max_shift)
        rc, again, how2 = dev_locate_gapped(c, ref, keys, first, max_edits, max_shift)
        assert again.tobytes() == want.tobytes() and (how2 == how).all()                          # two runs, identical bytes
        seen |= set(want["mismatches"][how == 1].tolist())
        # (one edit without a shift is one exact flank: the first pass has those rows already)
        assert (how == 1).any() == (max_edits > 1) and (how == -1).any() and (how == 0).any()
    assert {2, 3} <= seen                                                     # a substitution in each flank; a three-base indel
    # without d_how
    rc, got, _ = dev_locate_gapped(c, ref, keys, first, 4, 3, with_how=False)
    assert rc == int((how == 1).sum()) and got.tobytes() == want.tobytes()
    ref.close()
    c.close()


# ---- seed ranges around the lane walk, row counts around the wavefront -----------------------------------------------------------

@functools.lru_cache(None)
def long_range_case(k, total):
    rng = random.Random(100 + k)
    g = random_genome(rng, total, k)
    entries, _ = restate_reference_index(g, k)
    keys = gapped_queries(rng, g, entries, k, n_each=55)[:257]
    assert len(keys) == 257
    todo = np.flatnonzero(restate_locate(entries, keys, 1)["flat"] < 0)
    for at, j in ((0, todo[0]), (256, todo[-1])):        # the wavefronts of one lane have a row to try
        keys[[at, j]] = keys[[j, at]]
    return g, entries, keys, restate_locate(entries, keys, 1)


@pytest.mark.parametrize("k,total", [(5, 40000), (9, 60000), (9, 34000)])
def test_locate_gapped_with_ranges_on_both_sides_of_the_lane_walk(k, total):
    """a flank's inner base is never the tract's base, so three quarters of the seeds occur: at k = 9 (h = 5) 60 kB give
    about 28 entries per range, all of them handed to the wavefront and none as long as one stride of it; 34 kB give about 16,
    on both sides of the lane walk.  A row whose mutation made its inner base the tract's base has an empty range."""
    g, entries, keys, first = long_range_case(k, total)
    todo = first["flat"] < 0
    r0, r1 = seed_ranges(entries, keys, k)
    if k == 5:                                           # h = 3: every range of a row that is tried goes to the wavefront, for several strides
        for r in (r0[todo], r1[todo]):
            assert ((r == 0) | (r > 10 * LC_LANE_WALK)).all() and (r > 10 * LC_LANE_WALK).mean() > 0.8
    elif total == 60000:
        for r in (r0[todo], r1[todo]):
            assert ((r == 0) | (r > LC_LANE_WALK)).all() and (r < 64).all() and (r > LC_LANE_WALK).mean() > 0.8
    else:                                                # both paths in every wavefront, and within one row
        short0, short1 = (r0 > 0) & (r0 <= LC_LANE_WALK), (r1 > 0) & (r1 <= LC_LANE_WALK)
        for short, r in ((short0, r0), (short1, r1)):
            assert short[todo].mean() > 0.2 and (r > LC_LANE_WALK)[todo].mean() > 0.2
            for w in range(0, 256, 64):
                sel = todo[w: w + 64]
                assert short[w: w + 64][sel].any() and (r[w: w + 64][sel] > LC_LANE_WALK).any()
        assert (short0 != short1)[todo].mean() > 0.2
    assert todo[0] and todo[256] and todo.sum() > 100 and (~todo).sum() > 20
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    ref.add_seeds(c)
    for n in (1, 63, 64, 65, 257):
        want, how = check_gapped(c, ref, entries, keys, first, k, 3, 3, n=n)
    assert (how == 1).sum() > 50 and want["n_hits"].max() > 1
    check_gapped(c, ref, entries, keys, first, k, 1, 1)
    ref.close()
    c.close()


def test_both_lookups_at_the_edge_of_the_lane_walk():
    """k = 2, the smallest the counter takes.  A contig of 2 + length + 2 bases holds one entry (its other runs lack a flank inside
    the contig), so every bucket is built by hand from repeated A tracts that share one flank and differ in the other (and in
    length): 16 and 17 tracts behind the left flanks CG and GT, 16 and 17 in front of the right flanks TC and CT.  The flanks'
    inner bases keep the four groups apart as well, so the buckets of tjamd_locate (the whole flank) and the seed ranges of
    tjamd_locate_gapped (h = 1: the inner base) both have exactly LC_LANE_WALK and LC_LANE_WALK + 1 entries, in either order of
    the index.  One wavefront holds a row of each, rows that own a range of both lengths, and rows of base C, whose ranges are
    empty.  The random cases of the tests above pass both lengths only by chance."""
    k, W = 2, LC_LANE_WALK
    rights, lefts = ("GA", "GC", "GG", "GT"), ("AC", "CC", "GC", "TC")       # (inner bases G and C: no other group has them)
    contigs = [("CG", 3 + i % 5, rights[i % 4]) for i in range(W)] + [("GT", 3 + i % 6, rights[i % 4]) for i in range(W + 1)]
    contigs += [(lefts[i % 4], 3 + i % 7, "TC") for i in range(W)] + [(lefts[i % 4], 3 + i % 4, "CT") for i in range(W + 1)]
    g = "".join(f"{l}{'A' * n}{r}\n" for l, n, r in contigs).encode()
    entries, n_contigs = restate_reference_index(g, k)
    assert len(entries) == n_contigs == 4 * W + 2 and (entries["base"] == 0).all()
    A, C_ = 0, 1
    rows = [("CG", "GA", A), ("AA", "AA", C_), ("GT", "GG", A), ("AC", "TC", A), ("GC", "CT", A), ("CG", "CT", A), ("GT", "TC", A),
            ("CG", "TT", A), ("GT", "AT", A), ("TT", "TC", A), ("CA", "CT", A), ("TG", "GG", C_), ("CG", "GT", A), ("GT", "GA", A), ("CG", "AC", A), ("TA", "TC", A)]
    keys = np.array([canonical([CODE[ord(x)] for x in l], [CODE[ord(x)] for x in r], b)[:2] + (b | (5 << 2),) for l, r, b in rows], dtype=np.uint64)
    assert len(keys) < 64
    size = [dict(zip(*(x.tolist() for x in np.unique(entries[side], return_counts=True)))) for side in ("ctx0", "ctx1")]
    b0 = np.array([size[0].get(int(a), 0) if int(m) & 3 == A else 0 for a, _, m in keys])
    b1 = np.array([size[1].get(int(b), 0) if int(m) & 3 == A else 0 for _, b, m in keys])
    r0, r1 = seed_ranges(entries, keys, k)
    for own, other in ((b0, b1), (b1, b0), (r0, r1), (r1, r0)):              # each length on each side, alone in its row and beside the other
        assert (own == W).any() and (own == W + 1).any() and ((own == W) & (other == W + 1)).any()
        assert ((own == W) & (other < W)).any() and ((own == W + 1) & (other < W)).any()
    assert (b0[[1, 11]] == 0).all() and (b1[[1, 11]] == 0).all() and (r0[[1, 11]] == 0).all() and (r1[[1, 11]] == 0).all()
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    assert ref.add_seeds(c) == len(entries)
    same_entries(ref.download(), entries)
    for mm in (0, 1, 2):
        want = restate_locate(entries, keys, mm)
        n, got = dev_locate(c, ref, keys, mm)
        assert got.tobytes() == want.tobytes() and n == int((want["flat"] >= 0).sum()) > 0, (mm, np.flatnonzero(got != want)[:5])
    assert want["n_hits"].max() > W + 1 and (want["flat"][[1, 11]] < 0).all()
    nowhere = np.zeros(len(keys), LOC)
    nowhere[:] = NOWHERE
    for max_edits, max_shift in ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1)):
        want, how = check_gapped(c, ref, entries, keys, nowhere, k, max_edits, max_shift)
        assert (how[[1, 11]] == -1).all() and (how == 1).any()
    assert want["n_hits"].max() > W + 1
    ref.close()
    c.close()


# ---- every row located on entry, or none -------------------------------------------------------------------------------------

def test_all_rows_located_already_and_none_located():
    k = 13
    rng = random.Random(13)
    g = random_genome(rng, 30000, k)
    entries, _ = restate_reference_index(g, k)
    keys = gapped_queries(rng, g, entries, k, n_each=40)
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    ref.add_seeds(c)
    everywhere = np.zeros(len(keys), LOC)
    everywhere[:] = (5, 0, 5, 3, 9, 1, 2)
    everywhere["flat"] = np.arange(len(keys))
    rc, got, how = dev_locate_gapped(c, ref, keys, everywhere, 4, 3)
    assert rc == 0 and got.tobytes() == everywhere.tobytes() and (how == 0).all()
    nowhere = np.zeros(len(keys), LOC)
    nowhere[:] = NOWHERE
    want, how = check_gapped(c, ref, entries, keys, nowhere, k, 2, 2)
    assert (how != 0).all() and (want["mismatches"][how == 1] == 0).any() and (how == -1).any()
    ref.close()
    c.close()


# ---- the pipeline ------------------------------------------------------------------------------------------------------------

def test_eight_sample_pipeline_with_the_second_pass(monkeypatch):
    torch = _torch()
    monkeypatch.delenv("TATAJUBA_AMD_EDIT_DISTANCE", raising=False)
    k, m, ns, maxd, lev, mm = 15, 4, 8, 1, 2, 1
    rng = random.Random(2024)
    pieces = make_genome(rng, n_tracts=2000)
    genome = "".join(left + DNA[b] * length + right for left, b, length, right in pieces)
    counters, ocov = [], []
    for smp in range(ns):
        s = reads_of(sample_of(pieces, rng, smp), rng)
        c = tj.Counter(k)
        c.scan_host(s, m)
        assert c.finalise(1, 5) == 0
        counters.append(c); ocov.append(c.coverage)
    L = tj.lib()
    hs = (C.c_void_p * ns)(*[c._h for c in counters])
    drec, counts = C.c_void_p(), (C.c_long * ns)()
    merger = tj.Counter(k)
    total = L.tjamd_gather_histograms(merger._h, hs, ns, C.byref(drec), counts)
    keys = torch.empty(total * 24, dtype=torch.uint8, device="cuda")
    mat = torch.empty((total, ns), dtype=torch.int32, device="cuda")
    nu = L.tjamd_merge_samples(merger._h, drec, counts, ns, C.c_void_p(keys.data_ptr()), C.c_void_p(mat.data_ptr()), total)
    keys, mat = keys[: nu * 24], mat[:nu]
    keys_cpu, mat_cpu = np.frombuffer(keys.cpu().numpy().tobytes(), np.uint64).reshape(-1, 3), mat.cpu().numpy()
    nt0, grouped = device_union(merger, keys, mat, ocov, maxd, lev, on_device=True)

    stream = (genome + "\n").encode()
    ref = tj.Reference(merger, stream)
    ms_ref = merger.last_reference_ms()
    entries, _ = restate_reference_index(stream, k)
    assert ref.add_seeds(merger) == len(entries)
    ms_seed = merger.last_seed_order_ms()
    n1, first = dev_locate(merger, ref, keys, mm, on_device=True)
    ms_locate = merger.last_locate_ms()
    assert first.tobytes() == restate_locate(entries, keys_cpu, mm).tobytes()
    want, how = restate_locate_gapped(entries, keys_cpu, first, 3, 3, k)
    rc, got, got_how = dev_locate_gapped(merger, ref, keys, first, 3, 3, on_device=True)
    ms_gapped = merger.last_locate_gapped_ms()
    assert rc == int((how == 1).sum()) > 0 and got.tobytes() == want.tobytes() and (got_how == how).all()
    assert (np.frombuffer(keys.cpu().numpy().tobytes(), np.uint64).reshape(-1, 3) == keys_cpu).all()
    nt_first, _ = dev_located_tracts(merger, keys, mat, grouped["tracts"], first, on_device=True)
    nt, lt = dev_located_tracts(merger, keys, mat, grouped["tracts"], got, on_device=True)
    check_located_tracts(lt, restate_located_tracts(keys_cpu, mat_cpu, grouped["tracts"], want), keys_cpu, mat_cpu)
    ctx_ids, _ = orc.tract_ids(keys_cpu)
    heads = np.flatnonzero(np.r_[True, ctx_ids[1:] != ctx_ids[:-1]])
    before, after = int((first["flat"][heads] >= 0).sum()), int((got["flat"][heads] >= 0).sum())
    print(f"\n[locate_gapped] contexts located: {before} of {len(heads)} ({100.0 * before / len(heads):.1f} %) by tjamd_locate at {mm} mismatch, "
          f"{after} ({100.0 * after / len(heads):.1f} %) after tjamd_locate_gapped at 3 edits, shift 3; rows {n1} -> {n1 + rc} of {nu}; "
          f"tracts by location {nt_first} -> {nt} (grouped: {nt0})")
    print(f"[locate_gapped] genome {len(genome)} bases, {ref.n_entries} entries: tjamd_last_reference_ms {ms_ref:.3f} ms, tjamd_last_seed_order_ms "
          f"{ms_seed:.3f} ms; union {nu} rows: tjamd_last_locate_ms {ms_locate:.3f} ms, tjamd_last_locate_gapped_ms {ms_gapped:.3f} ms")
    assert ms_seed > 0 and ms_gapped > 0 and ms_locate > 0
    ref.close()
    for c in counters + [merger]:
        c.close()


# ---- examples/located_tracts.c -----------------------------------------------------------------------------------------------

def test_located_tracts_c_example_with_and_without_the_second_pass(tmp_path):
    exe, libdir = str(tmp_path / "located_tracts"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "located_tracts.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", exe])
    k, m, mm = 10, 3, 1
    rng = random.Random(7)
    pieces = make_genome(rng, n_tracts=200)
    contigs = ["".join(left + DNA[b] * length + right for left, b, length, right in part) for part in (pieces[:120], pieces[120:])]
    fasta = str(tmp_path / "ref.fa")
    with open(fasta, "w") as fh:
        fh.write("".join(">contig%d some text\n%s\n" % (i, "\n".join(s[j: j + 70] for j in range(0, len(s), 70))) for i, s in enumerate(contigs)))
    files, recs, covs = [], [], []
    for smp in range(2):
        s = reads_of(sample_of(pieces, rng, smp), rng)
        reads = bytes(s).split(b"\n")[:-1]
        f = str(tmp_path / f"s{smp}.fq")
        with open(f, "wb") as fh:
            fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rd, b"I" * len(rd)) for i, rd in enumerate(reads)))
        files.append(f)
        rec, cov = _oracle_sample(s, k, m)
        recs.append(rec); covs.append(cov)
    _, _, keys_o, mat_o = orc.merge_samples(np.frombuffer(np.concatenate(recs).tobytes(), np.uint64).reshape(-1, 3), [len(x) for x in recs])
    g = oracle_union_grouping(keys_o, mat_o, k, 1, 2)
    first = np.asarray(g["groups"]["first"], np.int64)
    tracts = np.zeros(len(first), TR)
    tracts["first"], tracts["n_rows"] = first, np.diff(np.r_[first, len(keys_o)])
    tracts["n_context"], tracts["indel"] = g["groups"]["n_context"], g["groups"]["indel"]
    tracts["mode"], tracts["lev_distance"], tracts["integral"] = g["mode"], g["lev_distance"], g["integral"]
    entries, _ = restate_reference_index(("\n".join(contigs) + "\n").encode(), k)
    loc1 = restate_locate(entries, keys_o, mm)
    loc2, how = restate_locate_gapped(entries, keys_o, loc1, 3, 3, k)
    assert (how == 1).sum() > 0
    lines = {}
    for name, extra, loc in (("plain", [], loc1), ("gapped", ["-g", "3"], loc2), ("narrow", ["-g", "2", "-s", "1"], restate_locate_gapped(entries, keys_o, loc1, 2, 1, k)[0])):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, "-x", str(mm), "-k", str(k), "-m", str(m), "-c", "5", "-d", "1", "-l", "-1", "-o", str(out)] + extra + files,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lt = restate_located_tracts(keys_o, mat_o, tracts, loc)
        perm, nt = lt["perm"], len(lt["tracts"])
        ids = np.repeat(np.arange(nt), lt["tracts"]["n_rows"])
        want = restate_union_tract_stats(keys_o[perm], mat_o[perm], covs, ids, lt["tracts"]["lev_distance"], ref_length=lt["ref_length"])
        sel = np.flatnonzero(want["selected"])
        lines[name] = r.stdout.strip().splitlines()
        assert lines[name][-1] == f"From {nt} tracts, 0 interesting ones are annotated and {len(sel)} interesting ones are not annotated"
        assert (out / "tract_locations.tsv").read_text() == LOCATIONS_HEADER + "".join(location_line(t, lt["tract_loc"][t]) for t in range(nt)), name
        assert (out / "selected_tracts_unknown.tsv").read_text() == SELECTED_HEADER + "".join(
            selected_line_at(t, lt["tract_loc"]["flat"][t], want["n_present"][t], want["lev_distance"][t], want["reldiff"][t]) for t in sel), name
    assert len(lines["plain"]) == 2 and len(lines["gapped"]) == 3 and len(lines["narrow"]) == 3
    assert lines["gapped"][1] == f"{int((how == 1).sum())} more union rows located within 3 edits and a shift of 3"
    assert lines["narrow"][1].endswith("more union rows located within 2 edits and a shift of 1")
    # examples/sample_vcfs.c takes the same two options and reports the same rows, behind its own summary line
    vcfs = str(tmp_path / "sample_vcfs")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sample_vcfs.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", vcfs])
    said = {}
    for name, extra in (("vcf_plain", []), ("vcf_gapped", ["-g", "3"])):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([vcfs, "-r", fasta, "-x", str(mm), "-k", str(k), "-m", str(m), "-c", "5", "-d", "1", "-l", "-1", "-o", str(out)] + extra + files,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        said[name] = r.stdout.strip().splitlines()
        assert len(os.listdir(out)) == 2                                       # one VCF per sample
    assert len(said["vcf_gapped"]) == len(said["vcf_plain"]) + 1 and said["vcf_gapped"][-1] == lines["gapped"][1]
    assert f"{int((loc1['flat'] >= 0).sum())} of {len(keys_o)} union rows located" in said["vcf_plain"][-1]
