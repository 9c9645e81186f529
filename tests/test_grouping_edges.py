"""The grouping of near-identical contexts on the device -- group_back_kernel, group_resolve_kernel, group_speculate_kernel
and group_repair_kernel under both count sources, name_edit_distance, group_summary_kernel, group_histogram_kernel,
union_tract_kernel -- against the CPU oracle on the grouping corpus (tests/grouping_edges.py), whose rows sit where the
kernels' walks change: long stretches, the repair's windows of GR_CHUNK rows, the second trip of the grid-stride loops, the
order effects of a replay and the edit distance at its threshold.  tests/test_grouping_edges_corpus.py shows on the CPU that
each planted row is where it is meant to be.

Integer work, nothing may differ.  Every case goes through the three entries: its rows as a union through tjamd_union_tracts
(group ids, join types, every tract field, and the number of candidates the speculation flagged against the restatement),
and as a finalised sample -- each row `count` times, the kept records being exactly the planted rows -- through
tjamd_group_contexts and tjamd_context_histograms, field by field.  Every case runs on one counter per k that the file's
cases share, the larger problems first, and on a fresh one.  Nothing in this file skips."""
import ctypes as C

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests import grouping_edges as G
from tests.test_gpu_parity import _hist_mask
from tests.test_union_tracts import check_grouping, device_union
from tests.test_union_tracts_cabi import oracle_union_grouping

pytestmark = pytest.mark.gpu

TR = tj.UNION_TRACT_DTYPE
GROUP_FIELDS = ("first", "n_elem", "n_context", "mode", "indel", "n_len", "modal_len", "modal_freq", "integral")


@pytest.fixture(scope="module")
def shared():
    """one counter per k, reused by every case of the file"""
    made = {}
    yield lambda k: made.setdefault(k, tj.Counter(k))
    for c in made.values():
        c.close()


def set_reading(monkeypatch, free_end):
    if free_end:
        monkeypatch.setenv("TATAJUBA_AMD_EDIT_DISTANCE", "free_end")
    else:
        monkeypatch.delenv("TATAJUBA_AMD_EDIT_DISTANCE", raising=False)
    orc.set_edit_free_end(free_end)


def union_route(c, r, maxd, lev, free_end, mat=None, what=""):
    """tjamd_union_tracts (and the statistics entries behind it) on the rows; returns the device's dict"""
    mat = G.split_counts(r.counts) if mat is None else mat
    nt, got = device_union(c, r.keys, mat, [30] * mat.shape[1], maxd, lev)
    assert nt > 0, (what, got)
    ref = oracle_union_grouping if len(r) <= 5000 else G.union_grouping
    check_grouping(got, ref(r.keys, mat, r.k, maxd, lev, free_end=free_end))
    totals = mat.astype(np.int64).sum(axis=1)
    flagged = int(G.candidates(r.keys, totals, G.heads_of(G.back_of(r.keys, maxd)), r.k, lev, free_end).sum())
    assert c.last_union_tract_candidates() == flagged, (what, c.last_union_tract_candidates(), flagged)
    return got


def load_sample(c, r):
    """the rows as a finalised sample: each `count` times; what is kept is exactly the planted rows"""
    c.reset()
    c.upload_raw(G.sample_raw(r, tj.ELEM_DTYPE))
    assert c.finalise(0, 0) == 0
    kept = c.download_kept()
    assert len(kept) == len(r) and (G.kept_table(kept) == G.planted(r)).all()
    return kept


def check_group_contexts(c, kept, maxd):
    gof, grp = c.group_contexts(maxd)
    ogof, first, nel, nctx, integ, mode = orc.group_contexts(kept, maxd)
    assert len(grp) == len(first) and (gof == ogof).all(), maxd
    assert (grp["first"] == first).all() and (grp["n_elem"] == nel).all() and (grp["n_context"] == nctx).all(), maxd
    assert (grp["integral"] == integ).all() and (grp["mode"] == mode).all(), maxd


def check_context_histograms(c, kept, k, maxd, lev, statistics=True):
    got = c.context_histograms(maxd, lev)
    want = orc.genomic_context_list(kept, k, maxd, lev, 3)
    g, w = got["groups"], want["groups"]
    assert len(g) == len(w) and (got["group_of"] == want["group_of"]).all(), (maxd, lev)
    assert ((got["join_type"] & 3) == want["join_type"]).all(), (maxd, lev)
    for f in GROUP_FIELDS if statistics else ("first", "n_elem", "n_context", "mode", "indel"):
        assert (g[f] == w[f]).all(), (f, maxd, lev)
    if statistics:
        m = _hist_mask(w, len(kept))
        assert (got["hist"]["length"][m] == want["hist_len"][m]).all() and (got["hist"]["freq"][m] == want["hist_freq"][m]).all()
    return got, want


def run_case(c, name, monkeypatch):
    r = G.get(name)
    _, params, both = G.CASES[name]
    kept = load_sample(c, r)
    for maxd in sorted({p[0] for p in params} | (set(G.STAIRCASE_MAXD) if name.startswith("staircase") else set())):
        check_group_contexts(c, kept, maxd)
    for maxd, lev in params:
        for fe in ((False, True) if both else (False,)):
            set_reading(monkeypatch, fe)
            what = "%s maxd %d lev %d free_end %d" % (name, maxd, lev, fe)
            got = union_route(c, r, maxd, lev, fe, what=what)
            _, want = check_context_histograms(c, kept, r.k, maxd, lev)
            if lev == 0:
                assert not (want["join_type"] == 2).any()
            if name == "all_join":
                assert len(got["tracts"]) == 2 == len(want["groups"]) and got["tracts"]["n_rows"].tolist() == [4500, 4500]   # one tract per base
                assert (got["join_type"][[0, 4500]] == 0).all() and (np.delete(got["join_type"], [0, 4500]) != 0).all()


def union_tracts_only(c, keys, mat, maxd, lev):
    """tjamd_union_tracts alone (no statistics): the part of device_union's dict that check_grouping reads"""
    import torch
    L = tj.lib()
    kd = torch.from_numpy(np.ascontiguousarray(keys).view(np.uint8).reshape(-1)).cuda()
    md = torch.from_numpy(np.ascontiguousarray(mat, np.int32)).cuda()
    n = len(keys)
    ids = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    jt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    tr = torch.zeros(n * TR.itemsize, dtype=torch.uint8, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    torch.cuda.synchronize()
    nt = L.tjamd_union_tracts(c._h, p(kd), p(md), n, mat.shape[1], maxd, lev, p(ids), p(jt), p(tr), n)
    assert nt > 0, L.tjamd_last_error()
    return {"tract_id": ids.cpu().numpy(), "join_type": jt.cpu().numpy(), "tracts": np.frombuffer(tr[: nt * TR.itemsize].cpu().numpy().tobytes(), dtype=TR)}


@pytest.mark.parametrize("which", ["staircase", "retry"])
def test_second_trip_of_the_grid_stride_loops(which, shared, monkeypatch):
    """GRID_CAP * BLOCK + 300 rows, the smallest shape at which `i += gridDim.x * blockDim.x` happens at all; the grouping only,
    no statistics.  staircase: one stretch across row GRID_CAP * BLOCK, heads and candidates on either side of it.  retry:
    candidates on the last row of the first trip and the first two of the second.  First in the file: every case on the shared
    counter of k = 10 then meets the scratch that a million rows left behind.  (A row inside the staircase cannot be a
    retry unit's candidate as well: two layouts of the one shape.)  Union route with one sample; sample route with counts of 2."""
    set_reading(monkeypatch, False)
    r = G.with_counts(G.grid_stride(which), 2)
    c = shared(r.k)
    maxd, lev = 2, 3
    mat = r.counts.astype(np.int32)[:, None]
    got = union_tracts_only(c, r.keys, mat, maxd, lev)
    want = G.union_grouping(r.keys, mat, r.k, maxd, lev)
    check_grouping(got, want)
    h1 = G.heads_of(G.back_of(r.keys, maxd))
    assert c.last_union_tract_candidates() == int(G.candidates(r.keys, r.counts, h1, r.k, lev).sum()) > 0
    assert (want["join_type"][G.ONE_TRIP - 1:] == 2).any()
    kept = load_sample(c, r)
    check_group_contexts(c, kept, maxd)
    check_context_histograms(c, kept, r.k, maxd, lev, statistics=False)


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_on_the_shared_counter(name, shared, monkeypatch):
    """the larger cases come first: what they leave in keep, grp_jt, ut_lev and the scan scratch is stale for the small ones"""
    run_case(shared(G.get(name).k), name, monkeypatch)


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_on_a_fresh_counter(name, monkeypatch):
    c = tj.Counter(G.get(name).k)
    try:
        run_case(c, name, monkeypatch)
    finally:
        c.close()


def test_planted_join_types(shared, monkeypatch):
    """what the corpus file shows of the oracle, asked of the device outright: the cascade's five cases, the threshold pairs
    under both readings at lev - 1, lev and lev + 1, the retry pair as the only two rows"""
    set_reading(monkeypatch, False)
    r = G.get("cascade")
    m = r.marks
    jt = union_route(shared(10), r, 2, 3, False)["join_type"]
    assert [int(jt[m[x]]) for x in ("new_name.R1", "new_name.R2", "old_name.R1", "old_name.R2", "absorbed.R1", "absorbed.S", "tie.H2", "tie.D",
                                    "base.first")] == [2, 2, 2, 0, 2, 0, 1, 2, 0]
    for k in (2, 10, 32):
        for r in (G.get("threshold-k%d" % k), G.get("shifted-k%d" % k)):
            load_sample(shared(k), r)
            for lev, fe, want in ((2, False, [0, 0, 0]), (2, True, [0, 0, 2]), (3, False, [2, 0, 2]), (3, True, [2, 0, 2]), (4, False, [2, 2, 2]), (4, True, [2, 2, 2])):
                set_reading(monkeypatch, fe)
                want = [w for w, x in zip(want, ("below", "at", "shifted")) if x in r.marks]
                got = union_route(shared(k), r, 1, lev, fe)
                assert [int(got["join_type"][i]) for i in r.marks.values()] == want, (k, lev, fe)
                h = shared(k).context_histograms(1, lev)
                assert [int(h["join_type"][i]) & 3 for i in r.marks.values()] == want, (k, lev, fe)
    set_reading(monkeypatch, False)
    got = union_route(shared(10), G.get("retry_pair"), 1, 3, False)
    assert got["join_type"].tolist() == [0, 2] and got["tracts"]["lev_distance"].tolist() == [2] and got["tracts"]["n_context"].tolist() == [2]


def test_count_field_wraps_in_a_sample_and_not_in_a_union(shared, monkeypatch):
    """X has 2^20 + 3 copies in the sample: its 20-bit field holds 3, its neighbour Y (5) is the histogram's name, as in the
    oracle, and Z -- within 3 edits of Y only -- is taken in.  The same rows as a union go by exact totals: X's total over two
    samples passes 2^31, X is the name and Z opens a tract.  Each route against its own reference."""
    set_reading(monkeypatch, False)
    r = G.count_wrap()
    c = shared(r.k)
    kept = load_sample(c, r)
    assert tj.decode_meta(kept["meta"])["count"].tolist() == [3, 5, 4]
    check_group_contexts(c, kept, 2)
    got, want = check_context_histograms(c, kept, r.k, 2, 3)
    assert (got["join_type"] & 3).tolist() == [0, 1, 2] and got["groups"]["mode"].tolist() == [r.marks["Y"]]
    mat = G.count_wrap_union_mat(r)
    u = union_route(c, r, 2, 3, False, mat=mat)
    assert u["join_type"].tolist() == [0, 1, 0] and u["tracts"]["mode"].tolist() == [r.marks["X"], r.marks["Z"]]
    assert u["tracts"]["integral"].tolist() == [int(mat[:2].astype(np.int64).sum()), int(mat[2].sum())] and u["tracts"]["integral"][0] > 1 << 31


def test_length_histogram_ties_with_negative_lengths(shared, monkeypatch):
    """Bars of equal summed count, a negative length on either side of the tie: the larger length comes first, (5, 6), (2, 6),
    (-3, 6), (-1, 4) and (-2, 5), (-7, 5), (3, 2), as orc.genomic_context_list orders them.  The order of equal counts is
    UNPINNED (new_empfreq_from_int_weighted is absent from the reference tree) and the same on both sides."""
    set_reading(monkeypatch, False)
    r = G.get("hist_ties")
    c = shared(r.k)
    kept = load_sample(c, r)
    got, _ = check_context_histograms(c, kept, r.k, 2, 3)
    h = got["hist"]
    assert list(zip(h["length"][:4].tolist(), h["freq"][:4].tolist())) == [(5, 6), (2, 6), (-3, 6), (-1, 4)]
    assert list(zip(h["length"][6:9].tolist(), h["freq"][6:9].tolist())) == [(-2, 5), (-7, 5), (3, 2)]
    assert got["groups"]["modal_len"].tolist() == [5, -2] and got["groups"]["modal_freq"].tolist() == [6, 5]
