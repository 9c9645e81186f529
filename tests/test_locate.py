"""tjamd_reference_create / tjamd_locate / tjamd_located_tracts on the GPU against the brute-force restatement of
tests/test_locate_cabi.py: the index on random multi-contig genomes (N runs, lowercase, homopolymers beyond 1023) and
against the located scan the oracle already checks, the lookup field for field (random and mutated queries, every
max_mismatches, buckets thousands long), the tracts by location (hand union, random families, statistics on the permuted
union), the eight-sample pipeline of tests/test_union_tracts.py with its reference genome, and examples/located_tracts.c."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests.test_tract_stats_cabi import N_STATS
from tests.test_locate_cabi import (LOCATIONS_HEADER, NOWHERE, hand_tracts_and_locations, location_line, restate_located_tracts, restate_locate,
                                    restate_reference_index)
from tests.test_union_tracts import BAD_SPANS, DNA, _oracle_sample, check_stats, device_union, make_genome, random_families, reads_of, sample_of
from tests.test_union_tracts_cabi import SELECTED_HEADER, hand_union, oracle_union_grouping, restate_union_tract_stats, AVG, MODAL, PROP, CPC, ENT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAP = 3, 4
BAD_SPANS_LOCATED = tuple(s for s in BAD_SPANS if s != [(0, 5), (5, 0)])      # (the test below never sent this one)
assert len(BAD_SPANS_LOCATED) == 6
TR, SU, LOC = tj.UNION_TRACT_DTYPE, tj.UNION_TRACT_SUMMARY_DTYPE, tj.LOCATION_DTYPE
ENTRY_FIELDS = ("ctx0", "ctx1", "flat", "contig", "pos", "length", "base", "neg_strand")


def _torch():
    return pytest.importorskip("torch")


def _p(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def _dev(a, dt=np.uint8):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()


def _raw(t, dt, n):
    return np.frombuffer(t[: n * dt.itemsize].cpu().numpy().tobytes(), dtype=dt)


def same_entries(got, want):
    assert len(got) == len(want)
    for f in ENTRY_FIELDS:
        assert (got[f] == want[f]).all(), f


def dev_locate(counter, ref, keys, mm, on_device=False):
    """-> (number of located rows, LOCATION_DTYPE per row), or (negative code, message)"""
    torch = _torch()
    kd = keys if on_device else _dev(np.asarray(keys, np.uint64).reshape(-1, 3))
    n = kd.numel() // 24
    loc = torch.full((max(n, 1) * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = tj.lib().tjamd_locate(counter._h, ref._h, _p(kd), n, mm, _p(loc))
    if got < 0:
        return got, tj.lib().tjamd_last_error().decode()
    return got, _raw(loc, LOC, n)


def dev_located_tracts(counter, keys, mat, tracts, loc, capacity=None, on_device=False):
    """-> (n_tracts, dict: perm, keys, mat, tracts, tract_loc, ref_length as numpy, and the device tensors under d_*)"""
    torch = _torch()
    kd = keys if on_device else _dev(np.asarray(keys, np.uint64).reshape(-1, 3))
    md = mat if on_device else torch.from_numpy(np.ascontiguousarray(mat, np.int32)).cuda()
    nu, ns = int(md.shape[0]), int(md.shape[1])
    cap = nu if capacity is None else capacity
    td = _dev(tracts) if tracts is not None else None
    ld = _dev(loc)
    perm = torch.full((max(nu, 1),), -7, dtype=torch.int32, device="cuda")
    ok, om = torch.zeros_like(kd), torch.full_like(md, -7)
    otr = torch.zeros(max(cap, 1) * 32, dtype=torch.uint8, device="cuda")
    otl = torch.zeros(max(cap, 1) * 32, dtype=torch.uint8, device="cuda")
    orl = torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nt = tj.lib().tjamd_located_tracts(counter._h, _p(kd), _p(md), nu, ns, _p(td), len(tracts) if tracts is not None else 0, _p(ld), _p(perm), _p(ok), _p(om),
                                       _p(otr), _p(otl), _p(orl), cap)
    if nt < 0:
        return nt, tj.lib().tjamd_last_error().decode()
    return nt, {"perm": perm[:nu].cpu().numpy(), "keys": np.frombuffer(ok.cpu().numpy().tobytes(), np.uint64).reshape(-1, 3), "mat": om.cpu().numpy(),
                "tracts": _raw(otr, TR, nt), "tract_loc": _raw(otl, LOC, nt), "ref_length": orl[:nt].cpu().numpy(),
                "d_keys": ok, "d_mat": om, "d_tracts": otr, "d_ref_length": orl}


def check_located_tracts(got, want, keys, mat):
    keys, mat = np.asarray(keys, np.uint64).reshape(-1, 3), np.asarray(mat)
    assert (got["perm"] == want["perm"]).all()
    assert got["tracts"].tobytes() == want["tracts"].tobytes() and got["tract_loc"].tobytes() == want["tract_loc"].tobytes()
    assert (got["ref_length"] == want["ref_length"]).all()
    assert (got["keys"] == keys[want["perm"]]).all() and (got["mat"] == mat[want["perm"]]).all()


def stats_on(counter, got, nt, ns, coverage):
    """tjamd_union_tract_stats / _sample_stats (every tract) on the permuted union a tjamd_located_tracts call wrote"""
    torch = _torch()
    L = tj.lib()
    kd, md, tr, ref = got["d_keys"], got["d_mat"], got["d_tracts"], got["d_ref_length"]
    nu = int(md.shape[0])
    cov = (C.c_int * ns)(*[int(x) for x in coverage])
    summ = torch.zeros(max(nt, 1) * 64, dtype=torch.uint8, device="cuda")
    var = torch.full((max(nt, 1),), -1, dtype=torch.int32, device="cuda")
    sel = torch.full((max(nt, 1),), -1, dtype=torch.int32, device="cuda")
    nv, nsel = C.c_long(-1), C.c_long(-1)
    rc = L.tjamd_union_tract_stats(counter._h, _p(kd), _p(md), nu, ns, _p(tr), nt, cov, _p(ref), _p(summ), _p(var), C.byref(nv), _p(sel), C.byref(nsel))
    assert rc == nt, L.tjamd_last_error()
    lst = torch.arange(max(nt, 1), dtype=torch.int32, device="cuda")
    vals = torch.full((max(nt, 1), N_STATS, ns), -7.0, dtype=torch.float64, device="cuda")
    ml, nc, nl = (torch.full((max(nt, 1), ns), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    rc = L.tjamd_union_tract_sample_stats(counter._h, _p(kd), _p(md), nu, ns, cov, _p(summ), nt, _p(lst), nt, _p(vals), _p(ml), _p(nc), _p(nl))
    assert rc == nt, L.tjamd_last_error()
    return {"summary": _raw(summ, SU, nt), "variable": var[: nv.value].cpu().numpy(), "selected": sel[: nsel.value].cpu().numpy(),
            "values": vals[:nt].cpu().numpy(), "modal_len": ml[:nt].cpu().numpy(), "n_context": nc[:nt].cpu().numpy(), "n_len": nl[:nt].cpu().numpy()}


def restate_stats_on(got, coverage):
    """the numpy restatement on the same permuted arrays, tract ids from the new tiling, ref_length from the call"""
    ids = np.repeat(np.arange(len(got["tracts"])), got["tracts"]["n_rows"])
    return restate_union_tract_stats(got["keys"], got["mat"], coverage, ids, got["tracts"]["lev_distance"], ref_length=got["ref_length"])


def random_genome(rng, total, k, acgt_only=False):
    """contigs of random bases with homopolymers (one beyond 1023), N runs, lowercase stretches, an empty contig and one
    shorter than 2k + 1; as a stream of reads"""
    def contig(n):
        out = []
        while sum(map(len, out)) < n:
            r = rng.random()
            if r < 0.02:
                out.append(rng.choice("ACGT") * rng.randrange(4, 40))
            elif r < 0.03 and not acgt_only:
                out.append("N" * rng.randrange(1, 2 * k + 3))
            elif r < 0.04 and not acgt_only:
                out.append("".join(rng.choice("acgtu") for _ in range(rng.randrange(1, 30))))
            elif r < 0.045 and not acgt_only:
                out.append(rng.choice("RYKMnx-*"))
            else:
                out.append("".join(rng.choice("ACGT") for _ in range(rng.randrange(1, 50))))
        return "".join(out)
    if acgt_only:
        return (contig(total) + "\n").encode()
    parts = [contig(total // 3), "", contig(2 * k), contig(total // 3) + "ACGT" * 8 + "G" * 1500 + "TACG" * 8 + contig(100), "acgtn" * 3, contig(total // 3)]
    return ("\n".join(parts) + "\n").encode()


# ---- the index ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 12, 13, 25, 32])
def test_reference_index_matches_the_restatement(k):
    c = tj.Counter(k)
    for seed, total in ((k, 3000), (100 + k, 40000)):
        g = random_genome(random.Random(seed), total, k)
        want, n_contigs = restate_reference_index(g, k)
        ref = tj.Reference(c, g)
        assert ref.n_contigs == n_contigs == 6 and ref.n_entries == len(want) > 0
        same_entries(ref.download(), want)
        assert want["length"].max() >= 1500 and (want["length"] == 1).any() and want["neg_strand"].any() and c.last_reference_ms() > 0
        ref.close()
    # a last contig without its delimiter; an empty stream; streams too short for any entry
    ref = tj.Reference(c, g[:-1])
    assert ref.n_contigs == 6
    same_entries(ref.download(), restate_reference_index(g[:-1], k)[0])
    ref.close()
    for s in (b"", b"\n", b"A", b"ACGT" * (k // 2) + b"\n", b"\n\n\n"):
        ref = tj.Reference(c, s)
        assert ref.n_entries == 0 and ref.n_contigs == restate_reference_index(s, k)[1] and len(ref.download()) == 0
        ref.close()
    c.close()


@pytest.mark.parametrize("k", [4, 13, 32])
def test_reference_index_is_the_located_scan(k):
    """ACGT only, one contig: the entries of length >= 2 are the located scan's tracts (m = 2), those of length 1 its monomers"""
    g = random_genome(random.Random(7 * k), 30000, k, acgt_only=True)
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    e = ref.download()
    stream = np.frombuffer(g, np.uint8)
    for sel, m in ((e["length"] >= 2, 2), (e["length"] == 1, 0)):
        rec = np.zeros(len(stream), tj.LOCATED_DTYPE)                    # (room for the monomers: more than half the bases)
        n = tj.lib().tjamd_scan_host_located(c._h, stream.ctypes.data, len(stream), m, rec.ctypes.data, len(rec))
        assert n > 0, tj.lib().tjamd_last_error()
        rec = rec[:n]
        d = orc.decode_meta(rec["meta"])
        x = e[sel]
        assert len(rec) == len(x) > 0
        assert (rec["ctx0"] == x["ctx0"]).all() and (rec["ctx1"] == x["ctx1"]).all() and (rec["pos"] == x["pos"].astype(np.uint64)).all()
        assert (d["base"] == x["base"]).all() and (d["length"] == x["length"]).all() and ((d["canon_flag"] == 2) == (x["neg_strand"] == 1)).all()
    ref.close()
    c.close()


# ---- the lookup --------------------------------------------------------------------------------------------------------

def queries_for(rng, entries, k, n_random, n_mutated):
    """random contexts, and entries with 0-3 substitutions in one flank or in both; some contexts twice (two lengths)"""
    mask = (1 << (2 * k)) - 1
    q = [(rng.getrandbits(2 * k), rng.getrandbits(2 * k), rng.randrange(2) | (rng.randrange(3, 12) << 2)) for _ in range(n_random)]

    def mutate(x, n):
        for p in rng.sample(range(k), n):
            x ^= rng.randrange(1, 4) << (2 * p)
        return x & mask
    for _ in range(n_mutated):
        e = entries[rng.randrange(len(entries))]
        c0, c1 = int(e["ctx0"]), int(e["ctx1"])
        n0, n1 = rng.choice([(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (0, 3), (3, 0), (1, 1), (2, 1), (0, min(k, 4))])
        q.append((mutate(c0, min(n0, k)), mutate(c1, min(n1, k)), int(e["base"]) | (rng.randrange(3, 12) << 2)))
    q += [(a, b, (m & 3) | (20 << 2)) for a, b, m in q[::7]]
    return np.array(q, dtype=np.uint64)


@pytest.mark.parametrize("k,total", [(13, 60000), (25, 60000), (32, 30000), (7, 60000)])
def test_locate_matches_the_restatement(k, total):
    rng = random.Random(31 * k)
    g = random_genome(rng, total, k)
    entries, _ = restate_reference_index(g, k)
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    keys = queries_for(rng, entries, k, 300, 1500)
    seen = set()
    for mm in range(4):
        want = restate_locate(entries, keys, mm)
        n, got = dev_locate(c, ref, keys, mm)
        assert got.tobytes() == want.tobytes(), (k, mm, np.flatnonzero(got != want)[:5])
        assert n == int((want["flat"] >= 0).sum()) and c.last_locate_ms() > 0
        seen |= set(want["mismatches"].tolist())
        if mm >= 1:
            assert (want["flat"] < 0).any() and (want["mismatches"] == mm).any()
    assert seen == {0, 1, 2, 3}
    # refusals: another k, max_mismatches outside 0 .. k, and nothing to do
    other = tj.Counter(k - 1)
    rc, err = dev_locate(other, ref, keys, 1)
    assert rc == -ERR_ARG and err.startswith("tjamd_locate") and f"built with k = {k}, the counter has k = {k - 1}" in err
    other.close()
    for bad in (-1, k + 1):
        rc, err = dev_locate(c, ref, keys, bad)
        assert rc == -ERR_ARG and f"max_mismatches {bad} outside 0..{k}" in err
    assert dev_locate(c, ref, keys[:0], 1)[0] == 0
    empty = tj.Reference(c, b"")
    n, got = dev_locate(c, empty, keys, 2)
    assert n == 0 and all(tuple(x.tolist()) == NOWHERE for x in got[:10]) and (got["flat"] == -1).all()
    empty.close()
    ref.close()
    c.close()


def test_locate_with_buckets_thousands_long():
    """k = 4: 512 (base, flank) buckets for about 1.1 million entries, so every query walks buckets of some 2000 entries on
    each side, and repeats give n_hits in the hundreds"""
    k = 4
    rng = random.Random(4)
    g = ("".join(rng.choice("ACGT") for _ in range(1_500_000)) + "\n").encode()
    entries, _ = restate_reference_index(g, k)
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    ms_build = c.last_reference_ms()
    assert ref.n_entries == len(entries) > 1_000_000
    same_entries(ref.download(), entries)
    keys = queries_for(rng, entries, k, 100, 200)
    for mm in (0, 1, 3):
        want = restate_locate(entries, keys, mm)
        n, got = dev_locate(c, ref, keys, mm)
        assert got.tobytes() == want.tobytes() and n == int((want["flat"] >= 0).sum()) > 0
    assert want["n_hits"].max() > 1000
    print(f"\n[locate] k = 4, {ref.n_entries} entries: index {ms_build:.3f} ms, lookup of {len(keys)} rows at 3 mismatches {c.last_locate_ms():.3f} ms")
    ref.close()
    c.close()


@pytest.mark.parametrize("k,total", [(5, 40000), (6, 150000)])
def test_locate_with_buckets_on_both_sides_of_the_lane_walk(k, total):
    """buckets of about 14 entries: in one wavefront some lanes walk their bucket alone (up to 16 entries) while others hand
    theirs to the wavefront, and a query may take one path for ctx0 and the other for ctx1"""
    rng = random.Random(k)
    g = random_genome(rng, total, k)
    entries, _ = restate_reference_index(g, k)
    keys = queries_for(rng, entries, k, 200, 1200)
    size = {}
    for side in ("ctx0", "ctx1"):
        flank, n = np.unique(entries[side].astype(np.int64) * 2 + entries["base"], return_counts=True)
        size[side] = dict(zip(flank.tolist(), n.tolist()))
    b0 = np.array([size["ctx0"].get(int(a) * 2 + (int(m) & 3), 0) for a, _, m in keys])
    b1 = np.array([size["ctx1"].get(int(b) * 2 + (int(m) & 3), 0) for _, b, m in keys])
    for b in (b0, b1):                                                        # a fifth of the queries at least on either path
        assert (b <= 16).mean() > 0.2 and (b > 16).mean() > 0.2
    assert ((b0 <= 16) != (b1 <= 16)).mean() > 0.2
    for w in range(0, len(keys) - 63, 64):                                    # and both paths inside every full wavefront
        assert (b0[w: w + 64] <= 16).any() and (b0[w: w + 64] > 16).any()
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    for mm in range(4):
        want = restate_locate(entries, keys, mm)
        n, got = dev_locate(c, ref, keys, mm)
        assert got.tobytes() == want.tobytes() and n == int((want["flat"] >= 0).sum()) > 0
    assert want["n_hits"].max() > 16
    ref.close()
    c.close()


# ---- tracts by location ------------------------------------------------------------------------------------------------

def test_located_tracts_on_the_hand_union():
    keys, mat, cov = hand_union()
    c = tj.Counter(4)
    for located in (True, False):
        tracts, loc = hand_tracts_and_locations(located)
        want = restate_located_tracts(keys, mat, tracts, loc)
        nt, got = dev_located_tracts(c, keys, mat, tracts, loc)
        assert nt == 2 and c.last_located_tracts_ms() > 0
        check_located_tracts(got, want, keys, mat)
        assert got["perm"].tolist() == [4, 0, 1, 2, 3] and got["tracts"]["mode"].tolist() == [0, 3] and got["ref_length"].tolist() == [8 if located else 0, 6]
        check_stats(stats_on(c, got, nt, 2, cov), restate_stats_on(got, cov))
    tracts, loc = hand_tracts_and_locations()
    nt, got = dev_located_tracts(c, keys, mat, None, loc)
    assert nt == 3
    check_located_tracts(got, restate_located_tracts(keys, mat, None, loc), keys, mat)
    assert got["perm"].tolist() == [2, 4, 0, 1, 3]
    loc[3] = NOWHERE
    loc[4] = (100, 1, 40, 8, 0, 0, 1)
    nt, got = dev_located_tracts(c, keys, mat, tracts, loc)
    assert nt == 3 and got["perm"].tolist() == [3, 4, 0, 1, 2]
    check_located_tracts(got, restate_located_tracts(keys, mat, tracts, loc), keys, mat)
    # a capacity below the tracts found; tracts that do not tile the union
    rc, err = dev_located_tracts(c, keys, mat, tracts, loc, capacity=2)
    assert rc == -ERR_CAP and err.startswith("tjamd_located_tracts") and "3 tracts, caller capacity 2" in err and c.last_located_tracts_ms() == -1.0
    far = loc.copy()
    far["flat"][0] = 1 << 45                                                 # beyond what the ordering sorts on: refused, not mis-ordered
    rc, err = dev_located_tracts(c, keys, mat, tracts, far)
    assert rc == -ERR_ARG and "flat >= 2^45" in err
    far["flat"][0] = (1 << 45) - 1
    assert dev_located_tracts(c, keys, mat, tracts, far)[0] == 3
    for spans in BAD_SPANS_LOCATED:
        bad = np.zeros(len(spans), TR)
        bad["first"], bad["n_rows"] = [s[0] for s in spans], [s[1] for s in spans]
        rc, err = dev_located_tracts(c, keys, mat, bad, loc)
        assert rc == -ERR_ARG and "do not tile the union" in err, (spans, rc, err)
    c.close()


@pytest.mark.parametrize("k,ns,seed", [(10, 3, 1), (12, 8, 2), (10, 70, 3)])
def test_located_tracts_on_random_families(k, ns, seed):
    """context-keyed tracts (no tracts given) and grouped tracts, locations planted so that many tracts share a place,
    some rows of one tract sit at different places and a fifth of the contexts have none"""
    keys, mat = random_families(k, ns, seed)
    rng = random.Random(seed)
    cov = rng.choices(range(20, 80), k=ns)
    place = {}
    loc = np.zeros(len(keys), LOC)
    for i, (c0, c1, meta) in enumerate(keys.tolist()):
        ctx = (c0, c1, meta & 3)
        if ctx not in place:
            flat = rng.randrange(0, 400) if rng.random() < 0.5 else (1 << 33) + rng.randrange(0, 1 << 20)
            place[ctx] = NOWHERE if rng.random() < 0.2 else (flat, flat % 7, flat % 1000, rng.randrange(1, 15), rng.randrange(3), rng.randrange(2), rng.randrange(1, 3))
        loc[i] = place[ctx]
    c = tj.Counter(k)
    nt0, g = device_union(c, keys, mat, cov, 1, 2)
    for tracts in (None, g["tracts"]):
        want = restate_located_tracts(keys, mat, tracts, loc)
        nt, got = dev_located_tracts(c, keys, mat, tracts, loc)
        assert nt == len(want["tracts"]) and nt < (nt0 if tracts is not None else len(place))
        check_located_tracts(got, want, keys, mat)
        assert (got["tracts"]["n_rows"] > 1).any() and (got["tract_loc"]["flat"] < 0).any() and (got["tract_loc"]["flat"] > (1 << 33)).any()
        check_stats(stats_on(c, got, nt, ns, cov), restate_stats_on(got, cov))
        nt2, again = dev_located_tracts(c, keys, mat, tracts, loc)
        assert nt2 == nt and all(got[f].tobytes() == again[f].tobytes() for f in ("perm", "keys", "mat", "tracts", "tract_loc", "ref_length"))
    c.close()


# ---- the pipeline ------------------------------------------------------------------------------------------------------

def test_eight_sample_pipeline_with_a_reference(monkeypatch):
    torch = _torch()
    monkeypatch.delenv("TATAJUBA_AMD_EDIT_DISTANCE", raising=False)
    k, m, ns, maxd, lev, mm = 15, 4, 8, 1, 2, 1
    rng = random.Random(2024)
    pieces = make_genome(rng, n_tracts=2000)
    genome = "".join(left + DNA[b] * length + right for left, b, length, right in pieces)      # the unmodified pieces joined
    counters, ocov = [], []
    for smp in range(ns):
        s = reads_of(sample_of(pieces, rng, smp), rng)
        c = tj.Counter(k)
        c.scan_host(s, m)
        assert c.finalise(1, 5) == 0
        counters.append(c); ocov.append(c.coverage)
    kept_before = [c.download_kept().tobytes() for c in counters]
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
    ms_tracts, ms_stats = merger.last_union_tracts_ms(), merger.last_union_tract_stats_ms()

    stream = (genome + "\n").encode()
    ref = tj.Reference(merger, stream)
    ms_ref = merger.last_reference_ms()
    entries, _ = restate_reference_index(stream, k)
    same_entries(ref.download(), entries)
    n_located, loc = dev_locate(merger, ref, keys, mm, on_device=True)
    ms_locate = merger.last_locate_ms()
    want_loc = restate_locate(entries, keys_cpu, mm)
    assert loc.tobytes() == want_loc.tobytes() and n_located == int((want_loc["flat"] >= 0).sum())
    nt, got = dev_located_tracts(merger, keys, mat, grouped["tracts"], loc, on_device=True)
    ms_located = merger.last_located_tracts_ms()
    check_located_tracts(got, restate_located_tracts(keys_cpu, mat_cpu, grouped["tracts"], want_loc), keys_cpu, mat_cpu)
    stats = stats_on(merger, got, nt, ns, ocov)
    ms_stats_located = merger.last_union_tract_stats_ms()
    check_stats(stats, restate_stats_on(got, ocov))

    # the pairs test_eight_sample_pipeline counts as split (one right flank, left flanks one substitution apart, two tracts
    # of tjamd_union_tracts) now share a tract
    new_row = np.empty(nu, np.int64)
    new_row[got["perm"]] = np.arange(nu)
    new_id = np.searchsorted(got["tracts"]["first"], new_row, side="right") - 1
    ctx_ids, _ = orc.tract_ids(keys_cpu)
    k0 = keys_cpu[:, 0].astype(object); k1 = keys_cpu[:, 1].astype(object); kb = keys_cpu[:, 2] & np.uint64(3)
    heads = np.flatnonzero(np.r_[True, ctx_ids[1:] != ctx_ids[:-1]])
    ham = lambda a, b: bin(((a ^ b) | ((a ^ b) >> 1)) & int("01" * 32, 2)).count("1")
    by_right = {}
    for h in heads:
        by_right.setdefault((int(kb[h]), k1[h]), []).append(h)
    left_pairs_split = still_split = 0
    for hs_ in by_right.values():
        for i in range(len(hs_)):
            for j in range(i + 1, len(hs_)):
                a, b = hs_[i], hs_[j]
                if ham(k0[a], k0[b]) == 1 and grouped["tract_id"][a] != grouped["tract_id"][b]:
                    left_pairs_split += 1
                    still_split += int(new_id[a] != new_id[b])
    assert left_pairs_split > 0 and still_split == 0
    assert nt < nt0                                                          # fewer tracts than by grouping alone
    tl = got["tract_loc"]
    assert (tl["n_hits"] <= 1).all() and (tl["n_hits"][tl["flat"] >= 0] == 1).all()
    located_ctx = sum(1 for h in heads if loc["flat"][h] >= 0)
    print(f"\n[locate] {located_ctx} of {len(heads)} union contexts located ({100.0 * located_ctx / len(heads):.1f} %), {n_located} of {nu} rows")
    assert located_ctx >= 0.85 * len(heads)
    # the reference length: the genome's own run at the place; at a planted tract without a length variant, the piece's length
    starts, off = {}, 0
    for i, (left, b, length, right) in enumerate(pieces):
        starts[off + len(left)] = (i, length)
        off += len(left) + length + len(right)
    planted = 0
    for t in np.flatnonzero(tl["flat"] >= 0):
        f = int(tl["flat"][t])
        e = f
        while e + 1 < len(genome) and genome[e + 1] == genome[f]:
            e += 1
        assert genome[f - 1] != genome[f] and got["ref_length"][t] == tl["ref_length"][t] == e - f + 1
        if f in starts and starts[f][0] % 8 != 4:
            planted += 1
            assert got["ref_length"][t] == starts[f][1]
    assert planted > 1000 and (got["ref_length"][tl["flat"] < 0] == 0).all()
    # the variable rule reads the reference length: tracts whose samples all show one length that is not the reference's
    assert len(stats["variable"]) > 0
    # nothing the calls read has changed; a second call is bitwise identical
    assert [c.download_kept().tobytes() for c in counters] == kept_before
    assert (np.frombuffer(keys.cpu().numpy().tobytes(), np.uint64).reshape(-1, 3) == keys_cpu).all() and (mat.cpu().numpy() == mat_cpu).all()
    n2, loc2 = dev_locate(merger, ref, keys, mm, on_device=True)
    nt2, again = dev_located_tracts(merger, keys, mat, grouped["tracts"], loc2, on_device=True)
    assert n2 == n_located and loc2.tobytes() == loc.tobytes() and nt2 == nt
    assert all(got[f].tobytes() == again[f].tobytes() for f in ("perm", "keys", "mat", "tracts", "tract_loc", "ref_length"))
    from tatajuba_amd.dist import located_tracts_device
    a = located_tracts_device(merger, ref, keys, mat, mm, tracts=grouped["tracts"])
    assert a["n_located"] == n_located and a["loc"].tobytes() == loc.tobytes() and a["tracts"].tobytes() == got["tracts"].tobytes()
    assert (a["perm"] == got["perm"]).all() and a["tract_loc"].tobytes() == got["tract_loc"].tobytes()
    print(f"[locate] genome {len(genome)} bases, {ref.n_entries} entries: tjamd_last_reference_ms {ms_ref:.3f} ms; union {nu} rows x {ns} samples: "
          f"tjamd_last_locate_ms {ms_locate:.3f} ms, tjamd_last_located_tracts_ms {ms_located:.3f} ms ({nt0} grouped tracts -> {nt}); beside "
          f"tjamd_last_union_tracts_ms {ms_tracts:.3f} ms, tjamd_last_union_tract_stats_ms {ms_stats:.3f} ms ({ms_stats_located:.3f} ms on the permuted union)")
    assert ms_ref > 0 and ms_locate > 0 and ms_located > 0
    ref.close()
    for c in counters + [merger]:
        c.close()


def selected_line_at(t, flat, n_present, lev_distance, reldiff):
    """one line of selected_tracts_unknown.tsv as examples/located_tracts.c writes it: begin_context = the flat location"""
    ref_order = [reldiff[MODAL], reldiff[AVG], reldiff[PROP], reldiff[CPC], reldiff[ENT]]
    return "tid_%06d\t%8d\t%5d\t%5d\t|\t" % (t, flat, n_present, lev_distance) + "".join("%8.6f\t" % v for v in ref_order) + "\n"


def test_located_tracts_c_example(tmp_path):
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
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, "-r", fasta, "-x", str(mm), "-k", str(k), "-m", str(m), "-c", "5", "-d", "1", "-l", "-1", "-o", str(out)] + files,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    _, _, keys_o, mat_o = orc.merge_samples(np.frombuffer(np.concatenate(recs).tobytes(), np.uint64).reshape(-1, 3), [len(x) for x in recs])
    g = oracle_union_grouping(keys_o, mat_o, k, 1, 2)
    first = np.asarray(g["groups"]["first"], np.int64)
    tracts = np.zeros(len(first), TR)
    tracts["first"], tracts["n_rows"] = first, np.diff(np.r_[first, len(keys_o)])
    tracts["n_context"], tracts["indel"] = g["groups"]["n_context"], g["groups"]["indel"]
    tracts["mode"], tracts["lev_distance"], tracts["integral"] = g["mode"], g["lev_distance"], g["integral"]
    entries, n_contigs = restate_reference_index(("\n".join(contigs) + "\n").encode(), k)
    loc = restate_locate(entries, keys_o, mm)
    lt = restate_located_tracts(keys_o, mat_o, tracts, loc)
    perm = lt["perm"]
    ids = np.repeat(np.arange(len(lt["tracts"])), lt["tracts"]["n_rows"])
    want = restate_union_tract_stats(keys_o[perm], mat_o[perm], covs, ids, lt["tracts"]["lev_distance"], ref_length=lt["ref_length"])
    sel = np.flatnonzero(want["selected"])
    nt = len(lt["tracts"])
    assert len(sel) > 0 and nt < len(tracts) and n_contigs == 2 and (lt["tract_loc"]["contig"] == 1).any()
    assert r.stdout.strip().splitlines()[-1] == f"From {nt} tracts, 0 interesting ones are annotated and {len(sel)} interesting ones are not annotated"
    assert (out / "selected_tracts_unknown.tsv").read_text() == SELECTED_HEADER + "".join(
        selected_line_at(t, lt["tract_loc"]["flat"][t], want["n_present"][t], want["lev_distance"][t], want["reldiff"][t]) for t in sel)
    assert (out / "tract_locations.tsv").read_text() == LOCATIONS_HEADER + "".join(location_line(t, lt["tract_loc"][t]) for t in range(nt))
