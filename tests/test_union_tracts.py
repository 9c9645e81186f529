"""tjamd_union_tracts / tjamd_union_tract_stats / tjamd_union_tract_sample_stats on the GPU against the oracle's grouping of
the pooled union (orc.genomic_context_list) and the numpy restatement of tests/test_union_tracts_cabi.py: hand-built and
random unions with no scan, exact totals above the 20-bit count field, the degenerate rule (the context-keyed tracts of
tjamd_tract_ids / tjamd_tract_stats), large tracts (the global-memory path), the eight-sample pipeline scan -> finalise ->
gather -> merge -> union tracts -> stats, and examples/selected_tracts.c."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests.test_tract_stats_cabi import N_STATS, record, restate_tract_stats
from tests.test_union_tracts_cabi import (ANNOTATED_HEADER, SELECTED_HEADER, hand_union, oracle_union_grouping, pack, restate_union_tract_stats,
                                          selected_line, K, MAXD, LEV)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAP = 3, 4
# (first, n_rows) of tracts that do not tile a union of five rows; tests/test_locate.py and tests/test_buffer_bounds.py send them too
BAD_SPANS = ([(0, 3), (4, 1)], [(1, 3), (4, 1)], [(0, 4), (4, 2)], [(0, 4), (3, 2)], [(0, 5), (5, 0)], [(-1, 5), (4, 1)], [(0, 2), (2, 2)])
TR, SU = tj.UNION_TRACT_DTYPE, tj.UNION_TRACT_SUMMARY_DTYPE


def _torch():
    return pytest.importorskip("torch")


def device_union(counter, keys, mat, coverage, maxd, lev, ref_length=None, on_device=False, capacity=None):
    """the three entries, per-sample values for EVERY tract (list = 0 .. n_tracts-1).  keys / mat: numpy or CUDA tensors.
    Returns (n_tracts, dict) or (negative code, error) if tjamd_union_tracts fails."""
    torch = _torch()
    L = tj.lib()
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1)).to(dev)
    kd = keys if on_device else t(np.asarray(keys, np.uint64), np.uint8)
    md = mat if on_device else torch.from_numpy(np.ascontiguousarray(mat, np.int32)).to(dev)
    nu, ns = int(md.shape[0]), int(md.shape[1])
    cap = nu if capacity is None else capacity
    ids = torch.full((max(nu, 1),), -7, dtype=torch.int32, device=dev)
    jt = torch.full((max(nu, 1),), -7, dtype=torch.int32, device=dev)
    tr = torch.zeros(max(cap, 1) * 32, dtype=torch.uint8, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    torch.cuda.synchronize()
    nt = L.tjamd_union_tracts(counter._h, p(kd), p(md), nu, ns, maxd, lev, p(ids), p(jt), p(tr), cap)
    if nt < 0:
        return nt, L.tjamd_last_error().decode()
    cov = (C.c_int * ns)(*[int(x) for x in coverage])
    ref = t(np.asarray(ref_length, np.int32), np.int32) if ref_length is not None else None
    summ = torch.zeros(max(nt, 1) * 64, dtype=torch.uint8, device=dev)
    var = torch.full((max(nt, 1),), -1, dtype=torch.int32, device=dev)
    sel = torch.full((max(nt, 1),), -1, dtype=torch.int32, device=dev)
    nv, nsel = C.c_long(-1), C.c_long(-1)
    got = L.tjamd_union_tract_stats(counter._h, p(kd), p(md), nu, ns, p(tr), nt, cov, p(ref), p(summ), p(var), C.byref(nv), p(sel), C.byref(nsel))
    assert got == nt, L.tjamd_last_error()
    lst = torch.arange(max(nt, 1), dtype=torch.int32, device=dev)
    vals = torch.full((max(nt, 1), N_STATS, ns), -7.0, dtype=torch.float64, device=dev)
    ml, nc, nl = (torch.full((max(nt, 1), ns), -7, dtype=torch.int32, device=dev) for _ in range(3))
    got = L.tjamd_union_tract_sample_stats(counter._h, p(kd), p(md), nu, ns, cov, p(summ), nt, p(lst), nt, p(vals), p(ml), p(nc), p(nl))
    assert got == nt, L.tjamd_last_error()
    raw = lambda x, dt: np.frombuffer(x[: nt * dt.itemsize].cpu().numpy().tobytes(), dtype=dt)
    return nt, {"tract_id": ids[:nu].cpu().numpy(), "join_type": jt[:nu].cpu().numpy(), "tracts": raw(tr, TR), "summary": raw(summ, SU),
                "variable": var[: nv.value].cpu().numpy(), "selected": sel[: nsel.value].cpu().numpy(), "values": vals[:nt].cpu().numpy(),
                "modal_len": ml[:nt].cpu().numpy(), "n_context": nc[:nt].cpu().numpy(), "n_len": nl[:nt].cpu().numpy()}


def check_grouping(got, want):
    """device ids, join types and tract fields against oracle_union_grouping"""
    tr, g = got["tracts"], want["groups"]
    assert len(tr) == len(g)
    assert (got["tract_id"] == want["tract_id"]).all() and (got["join_type"] == want["join_type"]).all()
    assert (tr["first"] == g["first"]).all() and (tr["n_rows"] == g["n_elem"]).all()
    assert (tr["n_context"] == g["n_context"]).all() and (tr["indel"] == g["indel"]).all()
    assert (tr["mode"] == want["mode"]).all() and (tr["integral"] == want["integral"]).all()
    assert (tr["lev_distance"] == want["lev_distance"]).all()


def check_stats(got, want):
    s = got["summary"]
    for f in ("first", "n_rows", "n_present", "lev_distance", "selected"):
        assert (s[f] == want[f]).all(), f
    assert np.allclose(s["reldiff"], want["reldiff"], rtol=1e-12, atol=1e-12)
    assert np.allclose(got["values"], want["values"], rtol=1e-12, atol=1e-12)
    for f in ("modal_len", "n_context", "n_len"):
        assert (got[f] == want[f]).all(), f
    near = np.abs(want["difference"] - 1e-5) <= 1e-9
    assert (s["variable"][~near] == want["variable"][~near]).all() and not near.any()
    assert list(got["variable"]) == list(np.flatnonzero(s["variable"])) and list(got["selected"]) == list(np.flatnonzero(s["selected"]))


def check_all(counter, keys, mat, cov, k, maxd, lev, free_end=False, ref_length=None):
    nt, got = device_union(counter, keys, mat, cov, maxd, lev, ref_length=ref_length)
    assert nt > 0, got
    want = oracle_union_grouping(keys, mat, k, maxd, lev, free_end=free_end)
    check_grouping(got, want)
    check_stats(got, restate_union_tract_stats(keys, mat, cov, want["tract_id"], want["lev_distance"], ref_length=ref_length))
    return got, want


def sample_records(rows, ns):
    """rows: {(base, ctx0, ctx1, length): [count per sample]} -> each sample's tjamd_records (count field = its count), in
    the finalised order that the merge expects (base, ctx0, ctx1, length, each descending)"""
    recs = []
    order = sorted(rows, key=lambda x: (-x[0], -x[1], -x[2], -x[3]))
    for s in range(ns):
        r = [record(b, c0, c1, ln, rows[(b, c0, c1, ln)][s]) for (b, c0, c1, ln) in order if rows[(b, c0, c1, ln)][s] > 0]
        recs.append(np.array(r, np.uint64).reshape(-1, 3))
    return recs


def union_of_samples(recs):
    """the union in the merge's order (orc.merge_samples)"""
    _, _, keys, mat = orc.merge_samples(np.concatenate(recs), [len(r) for r in recs])
    return keys, mat


def family_rows(k, ns, seed, n_fam=600):
    """families of near-identical contexts (right-flank substitutions and one-base indels, first bases of the left flank),
    a few lengths each, counts per sample: {(base, ctx0, ctx1, length): [count per sample]}"""
    rng = random.Random(seed)
    mask = (1 << (2 * k)) - 1
    rows = {}
    for fam in range(n_fam):
        c0, c1, base = rng.getrandbits(2 * k), rng.getrandbits(2 * k), rng.randrange(2)
        for member in range(rng.choice([1, 1, 2, 3, 5])):
            a, b = c0, c1
            for _ in range(rng.choice([0, 1, 1, 2])):
                r = rng.random()
                if r < 0.25:
                    a ^= rng.randrange(1, 4) << (2 * rng.randrange(2))
                elif r < 0.5:
                    b ^= rng.randrange(1, 4) << (2 * rng.randrange(k))
                elif r < 0.75:
                    p = rng.randrange(k)
                    b = ((b & ((1 << (2 * p)) - 1)) | (rng.randrange(4) << (2 * p)) | ((b >> (2 * p)) << (2 * p + 2))) & mask
                else:
                    p = rng.randrange(k)
                    b = ((b & ((1 << (2 * p)) - 1)) | ((b >> (2 * p + 2)) << (2 * p)) | (rng.randrange(4) << (2 * k - 2))) & mask
            for length in rng.sample(range(3, 12), rng.choice([1, 2, 3])):
                rows[(base, a, b, length)] = [rng.randrange(1, 30) if rng.random() < 0.8 else 0 for _ in range(ns)]
    for key in list(rows):
        if not any(rows[key]):
            rows[key][0] = 1
    return rows


def random_families(k, ns, seed, n_fam=600):
    """the union of family_rows, in the merge's order"""
    return union_of_samples(sample_records(family_rows(k, ns, seed, n_fam), ns))


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(K)
    yield c
    c.close()


def test_hand_built_union(counter):
    keys, mat, cov = hand_union()
    got, want = check_all(counter, keys, mat, cov, K, MAXD, LEV)
    assert got["tract_id"].tolist() == [0, 0, 0, 0, 1] and got["join_type"].tolist() == [0, 1, 1, 2, 0]
    assert got["tracts"]["lev_distance"].tolist() == [2, 0] and got["tracts"]["mode"].tolist() == [2, 4]
    assert got["summary"]["selected"].tolist() == [1, 0] and list(got["selected"]) == [0] and list(got["variable"]) == [0]
    assert got["n_len"][0].tolist() == [3, 2] and got["modal_len"][0].tolist() == [6, 5]            # lengths summed over contexts
    assert counter.last_union_tracts_ms() > 0 and counter.last_union_tract_stats_ms() > 0 and counter.last_union_tract_candidates() == 1
    # without the retry row 3 is a tract of its own, absent from no sample, and lev_distance 0
    nt, g0 = device_union(counter, keys, mat, cov, MAXD, 0)
    assert nt == 3 and g0["tract_id"].tolist() == [0, 0, 0, 1, 2] and (g0["tracts"]["lev_distance"] == 0).all()
    # capacity below the tracts found; bad tracts (not tiling the union) are refused
    rc, err = device_union(counter, keys, mat, cov, MAXD, LEV, capacity=1)
    assert rc == -ERR_CAP and err.startswith("tjamd_union_tracts") and "2 tracts, caller capacity 1" in err
    assert counter.last_union_tracts_ms() == -1.0
    torch = _torch()
    L = tj.lib()
    kd = torch.from_numpy(keys.view(np.uint8).reshape(-1)).cuda()
    md = torch.from_numpy(mat).cuda()
    cv = (C.c_int * 2)(*cov)
    summ = torch.zeros(64 * 3, dtype=torch.uint8, device="cuda")
    def stats_of(spans):
        tr = np.zeros(len(spans), TR)
        tr["first"], tr["n_rows"] = [b[0] for b in spans], [b[1] for b in spans]
        td = torch.from_numpy(tr.view(np.uint8)).cuda()
        rc = L.tjamd_union_tract_stats(counter._h, C.c_void_p(kd.data_ptr()), C.c_void_p(md.data_ptr()), 5, 2, C.c_void_p(td.data_ptr()), len(spans), cv,
                                       None, C.c_void_p(summ.data_ptr()), None, None, None, None)
        return rc, L.tjamd_last_error().decode()

    assert stats_of([(0, 4), (4, 1)])[0] == 2
    for bad in BAD_SPANS:
        rc, err = stats_of(bad)
        assert rc == -ERR_ARG and err.startswith("tjamd_union_tract_stats") and "must tile the union" in err, (bad, rc, err)
        assert counter.last_union_tract_stats_ms() == -1.0


@pytest.mark.parametrize("k,ns,maxd,lev,free_end", [(10, 3, 1, 2, 0), (10, 8, 2, 3, 0), (12, 70, 1, 3, 0), (10, 3, 1, 2, 1), (10, 8, 2, 3, 1)])
def test_random_unions_match_the_oracle(k, ns, maxd, lev, free_end, monkeypatch):
    """both readings of the absent edit distance (TATAJUBA_AMD_EDIT_DISTANCE, read per call), 3 / 8 / 70 samples"""
    if free_end:
        monkeypatch.setenv("TATAJUBA_AMD_EDIT_DISTANCE", "free_end")
    else:
        monkeypatch.delenv("TATAJUBA_AMD_EDIT_DISTANCE", raising=False)
    keys, mat = random_families(k, ns, 1000 * k + 10 * maxd + lev + free_end)
    cov = random.Random(ns).choices(range(20, 80), k=ns)
    c = tj.Counter(k)
    ref = np.random.default_rng(ns).integers(-1, 12, len(keys))   # (one per tract at most: only the first n_tracts are read)
    got, want = check_all(c, keys, mat, cov, k, maxd, lev, free_end=free_end)
    nt = len(got["tracts"])
    assert (got["join_type"] == 2).sum() > 0 and 0 < len(got["selected"]) and 0 < len(got["variable"])
    if ns < 70:                                                   # (with 70 samples nearly every tract is absent from one)
        assert len(got["selected"]) < nt and len(got["variable"]) < nt
    got2, _ = check_all(c, keys, mat, cov, k, maxd, lev, free_end=free_end, ref_length=ref[:nt])
    assert len(got2["variable"]) >= len(got["variable"]) and (ns == 70 or len(got2["variable"]) > len(got["variable"]))
    # the grouped ids are caller ids tjamd_tract_stats accepts
    from tests.test_tract_stats import device_stats
    nt2, ts = device_stats(c, keys, mat, cov, tract_ids=got["tract_id"])
    assert nt2 == nt and (ts["summary"]["n_present"] == got["summary"]["n_present"]).all()
    c.close()


def test_totals_above_the_20_bit_count_field(counter):
    """row 2's total is 2^20 + 4: the union key's field holds 4.  By exact totals row 2 is modal when row 3 is tried, and
    row 3 (TTTT.C.GGTC) is 2 edits from its name TTTT.C.AGGT: it joins.  By the field, row 0 (TTTT.C.ACGT, 3 edits) would be
    modal and row 3 would open a tract of its own."""
    big = (1 << 19) + 2
    keys = np.array([record(1, pack("TTTT"), pack("ACGT"), 6, 10), record(1, pack("TTTT"), pack("ACGT"), 5, 3),
                     record(1, pack("TTTT"), pack("AGGT"), 5, (2 * big) & 0xFFFFF), record(1, pack("TTTT"), pack("GGTC"), 7, 2)], dtype=np.uint64)
    mat = np.array([[10, 0], [1, 2], [big, big], [1, 1]], dtype=np.int32)
    cov = [big, big]
    assert orc.levenshtein("TTTT.C.AGGT", "TTTT.C.GGTC") == 2 and orc.levenshtein("TTTT.C.ACGT", "TTTT.C.GGTC") == 3
    got, want = check_all(counter, keys, mat, cov, K, MAXD, LEV)
    assert got["tract_id"].tolist() == [0, 0, 0, 0] and got["join_type"].tolist() == [0, 1, 1, 2]
    tr = got["tracts"][0]
    assert tr["mode"] == 2 and tr["integral"] == 2 * big + 15 and tr["lev_distance"] == 2
    field = orc.genomic_context_list(orc_elements_from_field(keys), K, MAXD, LEV, 1)   # what the wrapped field would give
    assert field["group_of"].tolist() == [0, 0, 0, 1]


def orc_elements_from_field(keys):
    e = np.zeros(len(keys), dtype=orc.ELEM_DTYPE)
    e["ctx0"], e["ctx1"], e["meta"] = keys[:, 0], keys[:, 1], keys[:, 2]
    e["loc_ref_id"] = e["loc_pos"] = e["loc_last"] = -1
    return e


def test_degenerate_rule_is_the_context_keyed_tracts(counter):
    """max_distance_per_flank 1, levenshtein_distance 0: a tract per context, as tjamd_tract_ids / tjamd_tract_stats"""
    from tests.test_tract_stats import device_stats
    keys, mat = random_families(10, 5, 77)
    cov = [30, 40, 50, 60, 70]
    c = tj.Counter(10)
    nt, got = device_union(c, keys, mat, cov, 1, 0)
    _, ts = device_stats(c, keys, mat, cov)                     # (the context-keyed ids of tjamd_tract_ids, computed there)
    torch = _torch()
    kd = torch.from_numpy(np.ascontiguousarray(keys).view(np.uint8).reshape(-1)).cuda()
    ids = np.full(len(keys), -1, np.int32)
    assert tj.lib().tjamd_tract_ids(c._h, C.c_void_p(kd.data_ptr()), len(keys), None, ids.ctypes.data) == nt
    assert (got["tract_id"] == ids).all() and (got["tracts"]["lev_distance"] == 0).all() and (got["join_type"] != 2).all()
    s, t = got["summary"], ts["summary"]
    assert len(t) == nt and (s["n_present"] == t["n_present"]).all() and (s["variable"] == t["variable"]).all()
    assert np.allclose(s["reldiff"], t["reldiff"], rtol=1e-12, atol=1e-12)
    assert np.allclose(got["values"], ts["values"], rtol=1e-12, atol=1e-12)
    c.close()


def test_large_tracts_take_the_global_path(counter):
    """a tract of one context with 141 lengths, and one of 16 contexts (two right-flank positions: pairwise within 2
    substitutions, joined at max_distance_per_flank 3) x 320 lengths = 5120 rows, beside small tracts"""
    rng = random.Random(5)
    ns, k = 3, 10
    rows = {}
    for ln in range(-20, 121):
        rows[(1, 0x1234, 0x5678, ln)] = [rng.randrange(1, 50) for _ in range(ns)]
    for x in range(4):
        for y in range(4):
            for ln in range(1, 321):
                rows[(0, 0xABCDE, 0x31000 | (x << 2) | (y << 6), ln)] = [rng.randrange(0, 9) for _ in range(ns)]
    for f in range(40):
        for ln in range(3, 3 + rng.randrange(1, 6)):
            rows[(1, rng.getrandbits(20), rng.getrandbits(20), ln)] = [rng.randrange(1, 9) for _ in range(ns)]
    for key in list(rows):
        if not any(rows[key]):
            rows[key][0] = 1
    keys, mat = union_of_samples(sample_records(rows, ns))
    cov = [100, 200, 300]
    c = tj.Counter(k)
    got, want = check_all(c, keys, mat, cov, k, 3, 4)
    n = got["tracts"]["n_rows"]
    assert n.max() == 5120 and 141 in n.tolist()
    big = int(np.argmax(n))
    assert (got["n_len"][big] == 320).all() and (got["n_context"][big] == 16).all()
    assert got["n_len"].max() == 320 and (got["n_len"] == 141).sum() == ns
    c.close()


# ---- the pipeline -------------------------------------------------------------------------------------------------
DNA = "ACGT"


def make_genome(rng, n_tracts=400, k=15):
    """random flanks of 40 bases around homopolymer tracts of 6-12 bases; returns the pieces (left, base, length, right)"""
    pieces = []
    for _ in range(n_tracts):
        b = rng.randrange(4)
        other = [x for x in DNA if x != DNA[b]]
        flank = lambda: "".join(rng.choice(DNA) for _ in range(40))
        left, right = flank(), flank()
        left = left[:-1] + rng.choice(other)                   # (the tract is exactly `length` long)
        right = rng.choice(other) + right[1:]
        pieces.append([left, b, rng.randrange(6, 13), right])
    return pieces


def sample_of(pieces, rng, smp):
    """a sample's copy: per-sample right-flank SNPs (3 bases after the tract), one-base right-flank deletions, left-flank
    SNPs next to the tract (2 bases before it), tract-length variants; which tracts carry which variant is fixed by the
    tract's index so that several samples share each allele"""
    out = []
    for i, (left, b, length, right) in enumerate(pieces):
        kind, carriers = i % 8, (i // 8) % 4
        has = (smp + carriers) % 3 == 0
        if has and kind == 1:                                   # right-flank SNP
            right = right[:3] + DNA[(DNA.index(right[3]) + 1) % 4] + right[4:]
        elif has and kind == 2:                                 # left-flank SNP next to the tract
            c = [x for x in DNA if x not in (left[-2], DNA[b])][0]
            left = left[:-2] + c + left[-1]
        elif has and kind == 3:                                 # one-base deletion in the right flank
            right = right[:5] + right[6:] + "A"
        elif has and kind == 4:                                 # tract length
            length += 1
        out.append(left + DNA[b] * length + right)
    return "".join(out)


_RC = str.maketrans("ACGT", "TGCA")


def reads_of(genome, rng, depth=30, read_len=150):
    """reads from both strands"""
    n = depth * len(genome) // read_len
    out = []
    for _ in range(n):
        s = rng.randrange(0, len(genome) - read_len)
        r = genome[s: s + read_len]
        out.append((r if rng.random() < 0.5 else r.translate(_RC)[::-1]) + "\n")
    return np.frombuffer("".join(out).encode(), np.uint8)


def _oracle_sample(stream, k, m):
    o = orc.Oracle(k)
    o.scan_stream(stream, m)
    o.finalise(1, 5)
    e = o.elems()
    rec = np.zeros(len(e), dtype=tj.RECORD_DTYPE)
    for f in ("ctx0", "ctx1", "meta"):
        rec[f] = e[f]
    cov = o.c.coverage
    o.close()
    return rec, cov


def test_eight_sample_pipeline(monkeypatch):
    torch = _torch()
    from tatajuba_amd.dist import union_tracts_device
    monkeypatch.delenv("TATAJUBA_AMD_EDIT_DISTANCE", raising=False)
    k, m, ns, maxd, lev = 15, 4, 8, 1, 2                      # the reference's -d 1 and its levenshtein default, d + 1
    rng = random.Random(2024)
    pieces = make_genome(rng, n_tracts=2000)
    counters, orecs, ocov = [], [], []
    for smp in range(ns):
        s = reads_of(sample_of(pieces, rng, smp), rng)
        c = tj.Counter(k)
        c.scan_host(s, m)
        assert c.finalise(1, 5) == 0
        rec, cov = _oracle_sample(s, k, m)
        assert c.coverage == cov
        counters.append(c); orecs.append(rec); ocov.append(cov)
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
    _, _, keys_o, mat_o = orc.merge_samples(np.frombuffer(np.concatenate(orecs).tobytes(), np.uint64).reshape(-1, 3), [len(r) for r in orecs])
    assert nu == len(keys_o)
    keys_cpu, mat_cpu = keys.cpu().numpy(), mat.cpu().numpy()
    mat_before = mat_cpu.tobytes()
    nt, got = device_union(merger, keys, mat, ocov, maxd, lev, on_device=True)
    ms_tracts, cand = merger.last_union_tracts_ms(), merger.last_union_tract_candidates()
    ms_stats = merger.last_union_tract_stats_ms()
    want = oracle_union_grouping(keys_o, mat_o, k, maxd, lev)
    check_grouping(got, want)
    check_stats(got, restate_union_tract_stats(keys_o, mat_o, ocov, want["tract_id"], want["lev_distance"]))
    # against the context-keyed tracts: fewer tracts, fewer absent from some sample
    ctx_ids, n_ctx = orc.tract_ids(keys_o)
    ctx = restate_tract_stats(keys_o, mat_o, ocov)
    assert nt < n_ctx
    assert (got["summary"]["n_present"] < ns).sum() < (ctx["n_present"] < ns).sum()
    # the planted variants, seen as pairs of neighbouring context-keyed tracts of one base that differ in one flank only
    k0 = keys_o[:, 0].astype(object); k1 = keys_o[:, 1].astype(object); kb = keys_o[:, 2] & np.uint64(3)
    heads = np.flatnonzero(np.r_[True, ctx_ids[1:] != ctx_ids[:-1]])
    ham = lambda a, b: bin(((a ^ b) | ((a ^ b) >> 1)) & int("01" * 32, 2)).count("1")
    right_pairs = left_pairs_split = right_joined = 0
    for a, b in zip(heads[:-1], heads[1:]):
        if kb[a] != kb[b]:
            continue
        if k0[a] == k0[b] and ham(k1[a], k1[b]) == 1:
            right_pairs += 1
            right_joined += int(got["tract_id"][a] == got["tract_id"][b])
    by_right = {}
    for h in heads:
        by_right.setdefault((int(kb[h]), k1[h]), []).append(h)
    for hs_ in by_right.values():
        for i in range(len(hs_)):
            for j in range(i + 1, len(hs_)):
                a, b = hs_[i], hs_[j]
                if ham(k0[a], k0[b]) == 1 and got["tract_id"][a] != got["tract_id"][b]:
                    left_pairs_split += 1
    assert right_pairs > 10 and right_joined >= 0.9 * right_pairs            # right-flank SNPs: one tract
    assert left_pairs_split > 0                                              # left-flank SNP next to the tract: the limitation
    # nothing the calls read has changed; a second call is bitwise identical
    assert [c.download_kept().tobytes() for c in counters] == kept_before
    assert (keys.cpu().numpy() == keys_cpu).all() and mat.cpu().numpy().tobytes() == mat_before
    nt2, again = device_union(merger, keys, mat, ocov, maxd, lev, on_device=True)
    assert nt2 == nt and all(got[f].tobytes() == again[f].tobytes() for f in got)
    ms_tracts2, ms_stats2 = merger.last_union_tracts_ms(), merger.last_union_tract_stats_ms()
    a = union_tracts_device(merger, keys, mat, ocov, maxd, lev)
    assert a["summary"].tobytes() == got["summary"].tobytes() and (a["selected"] == got["selected"]).all()
    assert a["values"].tobytes() == got["values"][a["selected"]].tobytes()
    print(f"\n[union tracts] union {nu} rows x {ns} samples, {nt} tracts ({n_ctx} context-keyed), {len(got['selected'])} selected, "
          f"{int((got['join_type'] == 2).sum())} joined by the retry: tjamd_last_union_tracts_ms {ms_tracts:.3f} ms "
          f"({cand} retry candidates), tjamd_last_union_tract_stats_ms {ms_stats:.3f} ms; second call {ms_tracts2:.3f} / {ms_stats2:.3f} ms")
    assert ms_tracts > 0 and ms_stats > 0 and cand > 0
    for c in counters + [merger]:
        c.close()


def test_selected_tracts_c_example(tmp_path, golden_dir):
    exe, libdir = str(tmp_path / "selected_tracts"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "selected_tracts.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", exe])
    g = os.path.join(golden_dir, "err1750956.fastq.gz")
    out = tmp_path / "same"
    out.mkdir()
    r = subprocess.run([exe, "-k", "10", "-m", "3", "-c", "5", "-o", str(out), g, g], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("From ") and last.endswith(" tracts, 0 interesting ones are annotated and 0 interesting ones are not annotated")
    assert (out / "selected_tracts_unknown.tsv").read_text() == SELECTED_HEADER
    assert (out / "selected_tracts_annotated.tsv").read_text() == ANNOTATED_HEADER
    # two different samples, -d 1 -l -1 (levenshtein d + 1 = 2): every line against the restatement on the oracle's union
    rng = random.Random(7)
    pieces = make_genome(rng, n_tracts=200)
    files, recs, covs = [], [], []
    for smp in range(2):
        s = reads_of(sample_of(pieces, rng, smp), rng)
        reads = bytes(s).split(b"\n")[:-1]
        f = str(tmp_path / f"s{smp}.fq")
        with open(f, "wb") as fh:
            fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rd, b"I" * len(rd)) for i, rd in enumerate(reads)))
        files.append(f)
        rec, cov = _oracle_sample(s, 10, 3)
        recs.append(rec); covs.append(cov)
    out = tmp_path / "two"
    out.mkdir()
    r = subprocess.run([exe, "-k", "10", "-m", "3", "-c", "5", "-d", "1", "-l", "-1", "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    _, _, keys_o, mat_o = orc.merge_samples(np.frombuffer(np.concatenate(recs).tobytes(), np.uint64).reshape(-1, 3), [len(x) for x in recs])
    g = oracle_union_grouping(keys_o, mat_o, 10, 1, 2)
    want = restate_union_tract_stats(keys_o, mat_o, covs, g["tract_id"], g["lev_distance"])
    sel = np.flatnonzero(want["selected"])
    nt = len(want["first"])
    assert len(sel) > 0
    assert r.stdout.strip().splitlines()[-1] == f"From {nt} tracts, 0 interesting ones are annotated and {len(sel)} interesting ones are not annotated"
    assert (out / "selected_tracts_unknown.tsv").read_text() == SELECTED_HEADER + "".join(
        selected_line(t, want["n_present"][t], want["lev_distance"][t], want["reldiff"][t]) for t in sel)
    assert (out / "selected_tracts_annotated.tsv").read_text() == ANNOTATED_HEADER
