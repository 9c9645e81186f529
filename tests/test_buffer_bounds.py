"""Where the device entries write.  Every output of every entry that writes caller memory (tests/bounds_calls.py: DEVICE
and HOST) sits in a guarded buffer (tests/guarded.py) of exactly the size the header asks for, at row, tract and query
counts on both sides of the kernels' constants; the results are checked against the suite's restatements and oracle as
elsewhere, and beside them: no byte outside a payload changed, no const input changed.  Then the same with one element of
capacity too few, with inputs the device refuses, with the optional outputs NULL, and with nothing to do."""
import ctypes as C
import functools
import os
import random
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from tatajuba_amd import capi
from oracle import orc
from tests import bounds_calls as bc
from tests.bounds_calls import ERR_ARG, ERR_CAP, LOC, SIZES, SU, TR, TS, Union
from tests.guarded import GuardedDevice, GuardedHost, frozen
from tests.test_locate import BAD_SPANS_LOCATED, check_located_tracts, queries_for, random_genome
from tests.test_locate_cabi import hand_tracts_and_locations, restate_located_tracts, restate_locate, restate_reference_index
from tests.test_tract_stats import BAD_TRACT_IDS, check_against_restatement, union_of
from tests.test_tract_stats_cabi import restate_tract_stats
from tests.test_union_tracts import BAD_SPANS, check_grouping, check_stats, random_families
from tests.test_union_tracts_cabi import hand_union, oracle_union_grouping, restate_union_tract_stats

pytestmark = pytest.mark.gpu

K, NS, MAXD, LEV = 10, 3, 1, 2
COV = [31, 47, 59]
CUTS = [(kind, v) for kind in ("rows", "ctx", "grp") for v in SIZES]
cut_ids = lambda cuts: [f"{kind}-{v}" for kind, v in cuts]


def test_the_table_names_every_case_below():
    elsewhere = {"tjamd_locate_gapped": "tests/test_locate_gapped_bounds.py"}    # the variant layer, N8-N13, has files of its own
    elsewhere.update({name: "tests/test_variant_bounds.py" for name in ("tjamd_tract_variants", "tjamd_tract_features", "tjamd_variant_effects", "tjamd_merge_variants",
                                                                        "tjamd_site_depths", "tjamd_annotation_download", "tjamd_coding_download")})
    assert all(os.path.exists(os.path.join(os.path.dirname(__file__), os.path.basename(f))) for f in elsewhere.values())
    assert set(bc.DEVICE) - set(elsewhere) == {"tjamd_merge_samples", "tjamd_tract_ids", "tjamd_tract_stats", "tjamd_tract_sample_stats", "tjamd_union_tracts",
                                               "tjamd_union_tract_stats", "tjamd_union_tract_sample_stats", "tjamd_locate", "tjamd_located_tracts"}
    assert set(bc.HOST) - set(elsewhere) == set(HOST_CASES) and set(elsewhere) <= set(bc.DEVICE) | set(bc.HOST)


# ---- the unions: prefixes of one union of random families, cut to a number of rows, of context-keyed tracts, of grouped tracts

@functools.lru_cache(None)
def base():
    keys, mat = random_families(K, NS, 4242, n_fam=5200)
    ids, _ = orc.tract_ids(np.ascontiguousarray(keys))
    ctx_heads = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
    grp_heads = np.asarray(oracle_union_grouping(keys, mat, K, MAXD, LEV)["groups"]["first"], np.int64)
    assert len(keys) > max(SIZES) and len(ctx_heads) > max(SIZES) and len(grp_heads) > max(SIZES)
    return Union(keys, mat, COV), ctx_heads, grp_heads


@functools.lru_cache(None)
def cut(kind, v):
    """the first v rows; the rows of the first v context-keyed tracts; the rows of the first v grouped tracts (a prefix of a
    union in merge order is a union, and the grouping of a prefix that ends with a tract is the prefix of the grouping)"""
    u, ctx_heads, grp_heads = base()
    return u.cut({"rows": v, "ctx": int(ctx_heads[v]), "grp": int(grp_heads[v])}[kind])


@functools.lru_cache(None)
def grouping(kind, v):
    u = cut(kind, v)
    g = oracle_union_grouping(u.keys, u.mat, K, MAXD, LEV)
    return g, bc.tracts_from_grouping(g, u.n)


@functools.lru_cache(None)
def locations(kind, v):
    return bc.planted_locations(cut(kind, v).keys, 7)


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(K)
    yield c
    c.close()


# ---- exact fit ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", SIZES)
def test_exact_fit_merge_samples(counter, v):
    u = cut("rows", v)
    records, counts = u.sample_records()
    _, _, keys_o, mat_o = orc.merge_samples(records, counts)
    assert len(keys_o) == v                                                   # the capacity the call turns out to need
    r = bc.call_merge_samples(counter, records, counts, NS, v)
    assert r.rc == v, r.err
    assert (r["d_out_keys"].view(np.uint64).reshape(-1, 3) == keys_o).all() and (r["d_out_counts"].view(np.int32).reshape(-1, NS) == mat_o).all()
    assert (mat_o == u.mat).all()


NOT_GRP = [kv for kv in CUTS if kv[0] != "grp"]
NOT_CTX = [kv for kv in CUTS if kv[0] != "ctx"]


@pytest.mark.parametrize("kind,v", NOT_GRP, ids=cut_ids(NOT_GRP))
def test_exact_fit_tract_ids_and_tract_stats(counter, kind, v):
    u = cut(kind, v)
    ids, nt = orc.tract_ids(u.keys)
    assert kind != "ctx" or nt == v
    r = bc.call_tract_ids(counter, u)
    assert r.rc == nt and (r["d_tract_id"].view(np.int32) == ids).all() and (r["h_tract_id"].view(np.int32) == ids).all()
    ref = np.random.default_rng(v).integers(-1, 12, nt).astype(np.int32)
    for given in (None, ref):
        want = restate_tract_stats(u.keys, u.mat, COV, ref_length=given)
        got_nt, got = bc.tract_stats_of(counter, u, nt, ref=bc.dev(given, np.int32) if given is not None else None)
        assert got_nt == nt == len(want["first"]), got
        assert check_against_restatement(got, want) == 0
        assert counter.last_tract_stats_ms() > 0


@pytest.mark.parametrize("kind,v", NOT_CTX, ids=cut_ids(NOT_CTX))
def test_exact_fit_union_tract_entries(counter, kind, v):
    u = cut(kind, v)
    want, tracts = grouping(kind, v)
    nt = len(tracts)
    assert kind != "grp" or nt == v
    got_nt, got = bc.union_tracts_of(counter, u, MAXD, LEV, nt)
    assert got_nt == nt, got
    check_grouping(got, want)
    assert got["tracts"].tobytes() == tracts.tobytes()
    check_stats(got, restate_union_tract_stats(u.keys, u.mat, COV, want["tract_id"], want["lev_distance"]))
    ref = np.random.default_rng(v).integers(-1, 12, nt).astype(np.int32)
    again = bc.union_stats_of(counter, u, got["d_tracts"], nt, ref=bc.dev(ref, np.int32))
    check_stats(again, restate_union_tract_stats(u.keys, u.mat, COV, want["tract_id"], want["lev_distance"], ref_length=ref))
    # the grouped ids are caller ids that tjamd_tract_stats takes: the same tracts, so the same capacity
    ids = bc.dev(want["tract_id"].astype(np.int32), np.int32)
    ts_nt, ts = bc.tract_stats_of(counter, u, nt, ids=ids)
    assert ts_nt == nt and check_against_restatement(ts, restate_tract_stats(u.keys, u.mat, COV, tract_ids=want["tract_id"])) == 0


@pytest.mark.parametrize("kind,v", CUTS, ids=cut_ids(CUTS))
def test_exact_fit_located_tracts(counter, kind, v):
    """with the caller's tracts (the grouped ones) and with none (d_tracts NULL: the context-keyed ones)"""
    u = cut(kind, v)
    loc = locations(kind, v)
    ld = bc.dev(loc)
    for tracts in ([None] if kind == "ctx" else [grouping(kind, v)[1]] if kind == "grp" else [None, grouping(kind, v)[1]]):
        want = restate_located_tracts(u.keys, u.mat, tracts, loc)
        need = len(want["tracts"])
        nt, got = bc.located_tracts_of(counter, u, bc.dev(tracts) if tracts is not None else None, len(tracts) if tracts is not None else 0, ld, need)
        assert nt == need, got
        check_located_tracts(got, want, u.keys, u.mat)
        assert counter.last_located_tracts_ms() > 0
        # the outputs feed the statistics: the permuted union, its new tiling and the reference lengths
        r = got["raw"]
        pu = Union(got["keys"], got["mat"], COV)
        stats = bc.union_stats_of(counter, pu, r["d_out_tracts"].payload, nt, ref=r["d_ref_length"].payload.view(bc.torch().int32))
        ids = np.repeat(np.arange(nt), got["tracts"]["n_rows"])
        check_stats(stats, restate_union_tract_stats(got["keys"], got["mat"], COV, ids, got["tracts"]["lev_distance"], ref_length=got["ref_length"]))


# ---- the lookup: query counts that end inside a wavefront one of whose lanes owns a bucket longer than LC_LANE_WALK ------

with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tatajuba_amd", "csrc", "hopo_device.hip")) as _src:
    LC_LANE_WALK = int(re.search(r"^#define LC_LANE_WALK (\d+)$", _src.read(), re.M).group(1))      # the kernel's own figure


@pytest.fixture(scope="module")
def lookup():
    k = 5
    rng = random.Random(k)
    g = random_genome(rng, 40000, k)
    entries, _ = restate_reference_index(g, k)
    keys = queries_for(rng, entries, k, 600, 3300)
    assert len(keys) >= max(SIZES)
    size = {}
    for side in ("ctx0", "ctx1"):
        flank, n = np.unique(entries[side].astype(np.int64) * 2 + entries["base"], return_counts=True)
        size[side] = dict(zip(flank.tolist(), n.tolist()))
    longest = lambda q: max(size["ctx0"].get(int(q[0]) * 2 + (int(q[2]) & 3), 0), size["ctx1"].get(int(q[1]) * 2 + (int(q[2]) & 3), 0))
    bucket = np.array([longest(q) for q in keys])
    spare = [i for i in np.flatnonzero(bucket > LC_LANE_WALK).tolist() if i % 64 not in (0, 1)]
    for at in [0, 1] + [v - 1 for v in SIZES if v % 64 == 1 and v > 1]:      # the wavefronts that end after one or two lanes
        if bucket[at] <= LC_LANE_WALK:
            j = spare.pop()
            keys[[at, j]] = keys[[j, at]]
            bucket[[at, j]] = bucket[[j, at]]
    for v in SIZES:                                                           # the precondition, from the restated index alone
        if v % 64:
            last = bucket[v - v % 64: v]
            assert (last > LC_LANE_WALK).any() and (v % 64 < 3 or (last <= LC_LANE_WALK).any()), v
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    assert ref.n_entries == len(entries)
    yield c, ref, entries, bc.dev(keys), keys, {mm: restate_locate(entries, keys, mm) for mm in (1, 3)}
    ref.close()
    c.close()


@pytest.mark.parametrize("v", SIZES)
def test_exact_fit_locate(lookup, v):
    c, ref, entries, kd, keys, want = lookup
    for mm in want:
        r = bc.call_locate(c, ref, kd, v, mm)                                 # (a row's result does not depend on the rows behind it)
        assert r["d_loc"].view(LOC).tobytes() == want[mm][:v].tobytes(), (v, mm)
        assert r.rc == int((want[mm][:v]["flat"] >= 0).sum()) and c.last_locate_ms() > 0


def test_locate_leaves_the_reference_as_it_was(lookup):
    c, ref, entries, kd, keys, want = lookup
    before = ref.download()
    for v in (65, 4097):
        assert bc.call_locate(c, ref, kd, v, 3).rc >= 0
    assert ref.download().tobytes() == before.tobytes()


# ---- one short ----------------------------------------------------------------------------------------------------------

def short_capacities(need):
    return [need - 1] + ([1] if need > 2 else [])


# the cuts put each entry's needed capacity beside 64, 256, 1024 and 4096 at least once: the rows for the merge, the
# context-keyed tracts ("ctx") for tjamd_tract_stats and tjamd_located_tracts without tracts, the grouped ones ("grp") for the rest
SHORT_CUTS = [("rows", 65), ("rows", 1025), ("ctx", 257), ("ctx", 1025), ("ctx", 4097), ("grp", 257), ("grp", 4097)]


@pytest.mark.parametrize("kind,v", SHORT_CUTS, ids=cut_ids(SHORT_CUTS))
def test_one_short_is_refused_and_nothing_is_written_past_the_capacity(counter, kind, v):
    """(every caller of tests/bounds_calls.py checks the guards behind a buffer of `capacity` elements, and the inputs)"""
    u = cut(kind, v)
    records, counts = u.sample_records()
    for cap in short_capacities(u.n):
        bc.call_merge_samples(counter, records, counts, NS, cap).refused(ERR_CAP, f"{u.n} union keys, caller capacity {cap}")
    _, n_ctx = orc.tract_ids(u.keys)
    for cap in short_capacities(n_ctx):
        bc.call_tract_stats(counter, u, cap).refused(ERR_CAP, "tjamd_tract_stats", f"{n_ctx} tracts, caller capacity {cap}")
        assert counter.last_tract_stats_ms() == -1.0
    want, tracts = grouping(kind, v)
    for cap in short_capacities(len(tracts)):
        bc.call_union_tracts(counter, u, MAXD, LEV, cap).refused(ERR_CAP, "tjamd_union_tracts", f"{len(tracts)} tracts, caller capacity {cap}")
        assert counter.last_union_tracts_ms() == -1.0
    ids = bc.dev(want["tract_id"].astype(np.int32), np.int32)
    for cap in short_capacities(len(tracts)):
        bc.call_tract_stats(counter, u, cap, ids=ids).refused(ERR_CAP, f"{len(tracts)} tracts, caller capacity {cap}")
    loc = locations(kind, v)
    for given in (None, tracts):
        need = len(restate_located_tracts(u.keys, u.mat, given, loc)["tracts"])
        for cap in short_capacities(need):
            r = bc.call_located_tracts(counter, u, bc.dev(given) if given is not None else None, len(tracts), bc.dev(loc), cap)
            r.refused(ERR_CAP, "tjamd_located_tracts", f"{need} tracts, caller capacity {cap}")
            assert counter.last_located_tracts_ms() == -1.0
    # capacity 0 for a union that has rows: refused before any launch
    bc.call_tract_stats(counter, u, 0).refused(ERR_CAP, "capacity 0")
    bc.call_union_tracts(counter, u, MAXD, LEV, 0).refused(ERR_CAP, "capacity 0")
    bc.call_located_tracts(counter, u, None, 0, bc.dev(loc), 0).refused(ERR_CAP, "capacity 0")


# ---- refusals that the device finds --------------------------------------------------------------------------------------



def spans(pairs):
    tr = np.zeros(len(pairs), TR)
    tr["first"], tr["n_rows"] = [p[0] for p in pairs], [p[1] for p in pairs]
    return tr


def test_bad_tract_ids_are_refused_inside_the_buffers(counter):
    keys, mat = union_of([(1, 0x10, 0x20, [(6, [3, 1]), (5, [1, 1])]), (1, 0x10, 0x30, [(6, [2, 0])]), (1, 0x11, 0x20, [(4, [0, 5])]), (0, 0x10, 0x20, [(8, [1, 1])])])
    u = Union(keys, mat, [7, 3])
    for bad in BAD_TRACT_IDS:
        for cap in (5, 2, 1):
            bc.call_tract_stats(counter, u, cap, ids=bc.dev(np.array(bad, np.int32), np.int32)).refused(ERR_ARG, "tract ids must start at 0 and go up by 0 or 1")
            assert counter.last_tract_stats_ms() == -1.0
    # the same kinds of fault far into a larger union: a jump, a step back, a negative id, ids beyond the capacity
    u = cut("grp", 1025)
    good = grouping("grp", 1025)[0]["tract_id"].astype(np.int32)
    nt = int(good[-1]) + 1
    for at, to in ((u.n // 2, lambda x: x + 2), (u.n // 2, lambda x: x - 3), (u.n - 1, lambda x: -1), (1, lambda x: 1 << 30), (u.n - 1, lambda x: (1 << 31) - 1)):
        bad = good.copy()
        bad[at:] = to(bad[at:])
        for cap in (nt, nt - 1, 64):
            bc.call_tract_stats(counter, u, cap, ids=bc.dev(bad, np.int32)).refused(ERR_ARG, "tract ids must start at 0")


def test_a_listed_tract_outside_the_tracts_is_refused_inside_the_buffers(counter):
    u = cut("grp", 257)
    _, tracts = grouping("grp", 257)
    nt = len(tracts)
    r = bc.call_tract_stats(counter, u, nt, ids=bc.dev(grouping("grp", 257)[0]["tract_id"].astype(np.int32), np.int32))
    s = bc.call_union_tract_stats(counter, u, bc.dev(tracts), nt)
    assert r.rc == nt and s.rc == nt
    for listed in ([0, nt], [-1], [nt - 1, 1 << 30, 0], list(range(100)) + [-(1 << 31)] + list(range(100))):
        lst = bc.dev(np.array(listed, np.int32), np.int32)
        bc.call_tract_sample_stats(counter, u, r["d_summary"].payload, nt, lst).refused(ERR_ARG, "tjamd_tract_sample_stats", f"outside [0, {nt})")
        bc.call_union_tract_sample_stats(counter, u, s["d_summary"].payload, nt, lst).refused(ERR_ARG, "tjamd_union_tract_sample_stats", f"outside [0, {nt})")
    # summaries whose rows lie outside the union (a caller's own, or of another union)
    for field, value in (("first", -5), ("first", u.n), ("n_rows", u.n + 1), ("n_rows", -1)):
        for dt, got, call in ((TS, r, bc.call_tract_sample_stats), (SU, s, bc.call_union_tract_sample_stats)):
            summ = got["d_summary"].view(dt, nt).copy()
            summ[field][nt // 2] = value
            call(counter, u, bc.dev(summ), nt, bc.arange_dev(nt)).refused(ERR_ARG, "rows outside the union")


def bad_tilings(tracts, n):
    """tilings of a large union gone wrong in one place or everywhere: the sums of their rows fall short of the union, or
    reach far beyond it"""
    out = []
    for change in (lambda t: t["n_rows"].__setitem__(len(t) // 2, t["n_rows"][len(t) // 2] + 1), lambda t: t["first"].__setitem__(len(t) // 3, n + 5),
                   lambda t: t["n_rows"].__imul__(3), lambda t: t["n_rows"].__setitem__(slice(None), n), lambda t: t["first"].__setitem__(slice(None), n - 1),
                   lambda t: t["n_rows"].__setitem__(len(t) - 1, 1 << 30), lambda t: t["first"].__setitem__(0, -(1 << 30)), lambda t: t["n_rows"].__setitem__(5, -7)):
        t = tracts.copy()
        change(t)
        out.append(t)
    return out


def test_tracts_that_do_not_tile_the_union_are_refused_inside_the_buffers(counter):
    keys, mat, cov = hand_union()
    u = Union(keys, mat, cov)
    _, loc = hand_tracts_and_locations()
    c4 = tj.Counter(4)
    assert bc.call_union_tract_stats(c4, u, bc.dev(spans([(0, 4), (4, 1)])), 2).rc == 2
    for bad in BAD_SPANS:
        bc.call_union_tract_stats(c4, u, bc.dev(spans(bad)), len(bad)).refused(ERR_ARG, "tjamd_union_tract_stats", "must tile the union")
        assert c4.last_union_tract_stats_ms() == -1.0
        if bad in BAD_SPANS_LOCATED:
            for cap in (5, 1):
                bc.call_located_tracts(c4, u, bc.dev(spans(bad)), len(bad), bc.dev(loc), cap).refused(ERR_ARG, "do not tile the union")
                assert c4.last_located_tracts_ms() == -1.0
    c4.close()
    # a large union: d_perm, d_out_keys and d_out_counts hold n_union rows whatever the spans say
    u = cut("grp", 1025)
    _, tracts = grouping("grp", 1025)
    ld = bc.dev(locations("grp", 1025))
    for bad in bad_tilings(tracts, u.n):
        bc.call_union_tract_stats(counter, u, bc.dev(bad), len(bad)).refused(ERR_ARG, "must tile the union")
        for cap in (len(bad), 3):
            bc.call_located_tracts(counter, u, bc.dev(bad), len(bad), ld, cap).refused(ERR_ARG, "do not tile the union")


def test_a_flat_too_large_is_refused_inside_the_buffers(counter):
    keys, mat, cov = hand_union()
    tracts, loc = hand_tracts_and_locations()
    c4 = tj.Counter(4)
    far = loc.copy()
    far["flat"][0] = 1 << 45
    bc.call_located_tracts(c4, Union(keys, mat, cov), bc.dev(tracts), len(tracts), bc.dev(far), 5).refused(ERR_ARG, "flat >= 2^45")
    c4.close()
    u = cut("rows", 1025)
    loc = locations("rows", 1025).copy()
    located = np.flatnonzero(loc["flat"] >= 0)
    loc["flat"][located[len(located) // 2:]] = (1 << 62) + 12345
    for given in (None, grouping("rows", 1025)[1]):
        for cap in (u.n, 2):
            r = bc.call_located_tracts(counter, u, bc.dev(given) if given is not None else None, len(given) if given is not None else 0, bc.dev(loc), cap)
            r.refused(ERR_ARG, "flat >= 2^45")
            assert counter.last_located_tracts_ms() == -1.0


# ---- the optional outputs as NULL ---------------------------------------------------------------------------------------

# (which pointers a call may go without does not depend on the size: a small cut, and one of each kind past a block of every scan)
NULL_CUTS = [("rows", 65), ("grp", 1025), ("ctx", 4097)]


@pytest.mark.parametrize("kind,v", NULL_CUTS, ids=cut_ids(NULL_CUTS))
def test_optional_outputs_may_be_null(counter, kind, v):
    u = cut(kind, v)
    same = lambda a, b, names: all(a.bytes_of(n) == b.bytes_of(n) for n in names)
    full = bc.call_tract_ids(counter, u)
    for null, rest in ((("d_tract_id",), ("h_tract_id",)), (("h_tract_id",), ("d_tract_id",)), (("d_tract_id", "h_tract_id"), ())):
        part = bc.call_tract_ids(counter, u, null=null)
        assert part.rc == full.rc and same(part, full, rest)
    _, n_ctx = orc.tract_ids(u.keys)
    full = bc.call_tract_stats(counter, u, n_ctx)
    part = bc.call_tract_stats(counter, u, n_ctx, null=("d_var", "n_var"))
    assert part.rc == full.rc == n_ctx and same(part, full, ("d_summary",))
    lst = bc.arange_dev(n_ctx)
    full_v = bc.call_tract_sample_stats(counter, u, full["d_summary"].payload, n_ctx, lst)
    part_v = bc.call_tract_sample_stats(counter, u, full["d_summary"].payload, n_ctx, lst, null=("d_modal_len", "d_n_context"))
    assert part_v.rc == full_v.rc == n_ctx and same(part_v, full_v, ("d_values",))
    _, tracts = grouping(kind, v)
    nt = len(tracts)
    full = bc.call_union_tracts(counter, u, MAXD, LEV, nt)
    part = bc.call_union_tracts(counter, u, MAXD, LEV, nt, null=("d_join_type",))
    assert part.rc == full.rc == nt and same(part, full, ("d_tract_id", "d_tracts"))
    full_s = bc.call_union_tract_stats(counter, u, full["d_tracts"].payload, nt)
    part_s = bc.call_union_tract_stats(counter, u, full["d_tracts"].payload, nt, null=("d_var", "n_var", "d_sel", "n_sel"))
    assert part_s.rc == full_s.rc == nt and same(part_s, full_s, ("d_summary",))
    lst = bc.arange_dev(nt)
    full_v = bc.call_union_tract_sample_stats(counter, u, full_s["d_summary"].payload, nt, lst)
    part_v = bc.call_union_tract_sample_stats(counter, u, full_s["d_summary"].payload, nt, lst, null=("d_modal_len", "d_n_context", "d_n_len"))
    assert part_v.rc == full_v.rc == nt and same(part_v, full_v, ("d_values",))
    ld = bc.dev(locations(kind, v))
    for given in (None, full["d_tracts"].payload):
        full_l = bc.call_located_tracts(counter, u, given, nt, ld, u.n)
        part_l = bc.call_located_tracts(counter, u, given, nt, ld, u.n, null=("d_out_keys", "d_out_counts", "d_tract_loc", "d_ref_length"))
        assert part_l.rc == full_l.rc > 0 and same(part_l, full_l, ("d_perm", "d_out_tracts"))
        for one in ("d_out_keys", "d_out_counts", "d_tract_loc", "d_ref_length"):
            part_l = bc.call_located_tracts(counter, u, given, nt, ld, u.n, null=(one,))
            assert part_l.rc == full_l.rc and same(part_l, full_l, [n for n in bc.DEVICE["tjamd_located_tracts"] if n != one])


# ---- nothing to do ------------------------------------------------------------------------------------------------------

def test_empty_inputs_touch_nothing(counter, lookup):
    u = cut("rows", 65)
    _, tracts = grouping("rows", 65)
    nt = len(tracts)
    ld = bc.dev(locations("rows", 65))
    empty_list = bc.torch().zeros(0, dtype=bc.torch().int32, device="cuda")
    summary = bc.call_union_tract_stats(counter, u, bc.dev(tracts), nt)
    ts = bc.call_tract_stats(counter, u, u.n)
    records, counts = u.sample_records()
    lc, ref, _, kd, _, _ = lookup
    calls = [bc.call_merge_samples(counter, records, [0] * NS, NS, 8),
             bc.call_tract_ids(counter, u, n=0),
             bc.call_tract_stats(counter, u, 8, n=0),
             bc.call_tract_stats(counter, u, 0, n=0),
             bc.call_tract_sample_stats(counter, u, ts["d_summary"].payload, ts.rc, empty_list),
             bc.call_union_tracts(counter, u, MAXD, LEV, 8, n=0),
             bc.call_union_tract_stats(counter, u, bc.dev(tracts), nt, n=0),
             bc.call_union_tract_sample_stats(counter, u, summary["d_summary"].payload, nt, empty_list),
             bc.call_locate(lc, ref, kd, 0, 1),
             bc.call_located_tracts(counter, u, bc.dev(tracts), 0, ld, 8, n=0),
             bc.call_located_tracts(counter, u, None, 0, ld, 8, n=0)]
    for r in calls:
        assert r.rc == 0, r.err
        # where an output of such a call has no bytes at all, untouched() has nothing to compare; the caller has checked the
        # guards on both sides of it all the same, and a store to element 0 of an empty payload lands in the back guard
        assert all(g.untouched() for g in r.outs.values())


# ---- the entries that write host memory ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sample():
    """one sample scanned and finalised on the device, and on the oracle"""
    k, m = 10, 3
    stream = tj.synth_stream(20000, 150, 60000, variant_seed=3)
    c = tj.Counter(k)
    c.scan_host(stream, m)
    raw = orc.Oracle(k)
    raw.scan_stream(stream, m)
    raw_elems = raw.elems()
    raw.close()
    o = orc.Oracle(k)
    o.scan_stream(stream, m)
    o.finalise(1, 5)
    yield c, o, stream, raw_elems, k, m
    o.close()
    c.close()


def refused_host(rc, *words):
    err = tj.lib().tjamd_last_error().decode()
    assert rc == -ERR_CAP and all(w in err for w in words), (rc, err)


def case_download_raw(sample):
    c, o, stream, raw_elems, k, m = sample
    from tests.test_gpu_parity import as_records, rec_sorted
    n = c.raw_count()
    assert n == len(raw_elems) > 1000
    out = GuardedHost(n * 24)
    assert tj.lib().tjamd_download_raw(c._h, out.c, n) == n
    out.check("out")
    assert (rec_sorted(out.view(tj.RECORD_DTYPE)) == rec_sorted(as_records(raw_elems))).all()
    for cap in (n - 1, 1, 0):
        short = GuardedHost(cap * 24)
        refused_host(tj.lib().tjamd_download_raw(c._h, short.c, cap), f"{n} raw records, caller capacity {cap}")
        short.check("out")
        assert short.untouched()


def finalised(sample):
    c, o = sample[0], sample[1]
    if c.n_kept <= 0:
        assert c.finalise(1, 5) == 0 and o.c.status == 0
    return c, o


def case_download_kept(sample):
    c, o = finalised(sample)
    n = c.n_kept
    assert n == o.c.n_elem > 100
    out = GuardedHost(n * 40)
    assert tj.lib().tjamd_download_kept(c._h, out.c, n) == n
    out.check("out")
    assert out.view(tj.ELEM_DTYPE).tobytes() == o.elems().tobytes()
    for cap in (n - 1, 1):
        short = GuardedHost(cap * 40)
        refused_host(tj.lib().tjamd_download_kept(c._h, short.c, cap), f"{n} kept records, caller capacity {cap}")
        short.check("out")
        assert short.untouched()


def case_download_idx(sample):
    c, o = finalised(sample)
    n = c.n_idx
    ei, ef = o.idx()
    assert n == o.c.n_idx > 10
    a, b = GuardedHost(n * 4), GuardedHost(n * 4)
    assert tj.lib().tjamd_download_idx(c._h, a.c, b.c, n) == n
    a.check("idx_initial"); b.check("idx_final")
    assert (a.view(np.int32) == ei).all() and (b.view(np.int32) == ef).all()
    for cap in (n - 1, 1):
        a, b = GuardedHost(cap * 4), GuardedHost(cap * 4)
        refused_host(tj.lib().tjamd_download_idx(c._h, a.c, b.c, cap), f"{n} index ranges, caller capacity {cap}")
        a.check("idx_initial"); b.check("idx_final")
        assert a.untouched() and b.untouched()


def case_scan_host_located(sample):
    c, o, stream, raw_elems, k, m = sample
    s = np.ascontiguousarray(stream[:30000])
    roomy = tj.Counter(k)
    want = roomy.scan_host_located(s, m)                                       # (checked against the oracle by tests/test_gpu_parity.py)
    n = len(want)
    assert n > 100
    out = GuardedHost(n * 32)
    with frozen(s):
        assert tj.lib().tjamd_scan_host_located(roomy._h, s.ctypes.data, s.size, m, out.c, n) == n
        out.check("out")
        assert out.view(tj.LOCATED_DTYPE).tobytes() == want.tobytes()
        ref = orc.Oracle(k)
        ref.scan_stream(s, m)
        e = ref.elems()
        ref.close()
        got = out.view(tj.LOCATED_DTYPE)                                       # the oracle's raw elements, in emission order
        assert len(e) == n and all((got[f] == e[f]).all() for f in ("ctx0", "ctx1", "meta"))
        for cap in (n - 1, 1):
            short = GuardedHost(cap * 32)
            refused_host(tj.lib().tjamd_scan_host_located(roomy._h, s.ctypes.data, s.size, m, short.c, cap), f"produced {n} records, caller capacity {cap}")
            short.check("out")
            assert short.untouched()
    roomy.close()


def case_group_contexts(sample):
    c, o = finalised(sample)
    n = c.n_kept
    gof, first, nel, nctx, integ, mode = orc.group_contexts(o.elems(), 1)
    ng = len(first)
    a, b = GuardedHost(n * 4), GuardedHost(ng * tj.GROUP_DTYPE.itemsize)
    assert tj.lib().tjamd_group_contexts(c._h, 1, a.c, b.c, ng) == ng
    a.check("group_of"); b.check("groups")
    g = b.view(tj.GROUP_DTYPE)
    assert (a.view(np.int32) == gof).all() and (g["first"] == first).all() and (g["n_elem"] == nel).all() and (g["n_context"] == nctx).all()
    assert (g["integral"] == integ).all() and (g["mode"] == mode).all()
    for cap in (ng - 1, 1):
        a, b = GuardedHost(n * 4), GuardedHost(cap * tj.GROUP_DTYPE.itemsize)
        refused_host(tj.lib().tjamd_group_contexts(c._h, 1, a.c, b.c, cap), f"{ng} groups, caller capacity {cap}")
        a.check("group_of"); b.check("groups")
        assert b.untouched()
    a = GuardedHost(n * 4)                                                     # groups NULL: the ids alone, whatever the capacity
    assert tj.lib().tjamd_group_contexts(c._h, 1, a.c, None, 0) == ng and (a.view(np.int32) == gof).all()
    a.check("group_of")


def case_context_histograms(sample):
    c, o = finalised(sample)
    n, k, m = c.n_kept, sample[4], sample[5]
    want = orc.genomic_context_list(o.elems(), k, 1, 2, m)
    ng = len(want["groups"])
    sizes = {"group_of": n * 4, "join_type": n * 4, "groups": ng * capi.CONTEXT_GROUP_DTYPE.itemsize, "hist": n * 8}
    full = {name: GuardedHost(nb) for name, nb in sizes.items()}
    assert tj.lib().tjamd_context_histograms(c._h, 1, 2, *[full[name].c for name in sizes], ng) == ng
    for name, g in full.items():
        g.check(name)
    grp, hist = full["groups"].view(capi.CONTEXT_GROUP_DTYPE), full["hist"].view(capi.LENGTH_FREQ_DTYPE)
    assert (full["group_of"].view(np.int32) == want["group_of"]).all() and (full["join_type"].view(np.int32) == want["join_type"]).all()
    for f in ("first", "n_elem", "n_context", "mode", "indel", "n_len", "modal_len", "modal_freq", "integral"):
        assert (grp[f] == want["groups"][f]).all(), f
    for g in range(ng):
        lo, hi = int(grp["first"][g]), int(grp["first"][g]) + int(grp["n_len"][g])
        assert (hist["length"][lo:hi] == want["hist_len"][lo:hi]).all() and (hist["freq"][lo:hi] == want["hist_freq"][lo:hi]).all()
    for cap in (ng - 1, 1):
        part = {name: GuardedHost(nb if name != "groups" else cap * capi.CONTEXT_GROUP_DTYPE.itemsize) for name, nb in sizes.items()}
        refused_host(tj.lib().tjamd_context_histograms(c._h, 1, 2, *[part[name].c for name in sizes], cap), f"{ng} groups, caller capacity {cap}")
        for name, g in part.items():
            g.check(name)
        assert part["groups"].untouched()
    for null in sizes:                                                         # each output may be NULL: the others are what they were
        part = {name: None if name == null else GuardedHost(nb) for name, nb in sizes.items()}
        assert tj.lib().tjamd_context_histograms(c._h, 1, 2, *[part[name].c if part[name] else None for name in sizes], ng) == ng
        for name, g in part.items():
            if g is not None:
                g.check(name)
                if name != "hist":                                             # (hist: only [first, first + n_len) of each group is defined)
                    assert g.payload.tobytes() == full[name].payload.tobytes(), (null, name)


def case_reference_download(sample):
    c, k = sample[0], sample[4]
    g = random_genome(random.Random(11), 20000, k)
    want, _ = restate_reference_index(g, k)
    for stream in (g, g[: len(g) // 3]):                                       # built, used, closed and built again, smaller
        want, _ = restate_reference_index(stream, k)
        ref = tj.Reference(c, stream)
        n = ref.n_entries
        assert n == len(want) > 100
        out = GuardedHost(n * 48)
        assert tj.lib().tjamd_reference_download(ref._h, out.c, n) == n
        out.check("out")
        got = out.view(tj.REF_ENTRY_DTYPE)
        for f in ("ctx0", "ctx1", "flat", "contig", "pos", "length", "base", "neg_strand"):
            assert (got[f] == want[f]).all(), f
        for cap in (n - 1, 1, 0):
            short = GuardedHost(cap * 48)
            refused_host(tj.lib().tjamd_reference_download(ref._h, short.c, cap), "tjamd_reference_download", f"{n} entries, caller capacity {cap}")
            short.check("out")
            assert short.untouched()
        ref.close()


def case_scan_windows(sample):
    rng = random.Random(3)
    k, nw = 8, 300
    wins = ["".join(rng.choice("ACGT") for _ in range(rng.randrange(60, 140))) for _ in range(nw)]
    wins[5], wins[6] = "ACGT", ""
    arr = (C.c_char_p * nw)(*[w.encode() for w in wins])
    lens = (C.c_int * nw)(*[len(w) for w in wins])
    for m in (2, 0):
        exp, expw = [], []
        for i, w in enumerate(wins):
            o = orc.Oracle(k)
            (o.scan_seq(w, m) if m else o.scan_seq_all_monomers(w))
            exp.append(o.elems().copy()); expw += [i] * len(exp[-1])
            o.close()
        exp = np.concatenate(exp)
        n = len(exp)
        out, wof = GuardedHost(n * 40), GuardedHost(n * 4)
        assert tj.lib().tjamd_scan_windows(k, arr, lens, nw, m, out.c, wof.c, n) == n
        out.check("out"); wof.check("window_of")
        assert out.view(tj.ELEM_DTYPE).tobytes() == exp.tobytes() and wof.view(np.int32).tolist() == expw
        only = GuardedHost(n * 40)                                             # window_of may be NULL
        assert tj.lib().tjamd_scan_windows(k, arr, lens, nw, m, only.c, None, n) == n
        only.check("out")
        assert only.payload.tobytes() == out.payload.tobytes()
        for cap in (n - 1, 1):
            out, wof = GuardedHost(cap * 40), GuardedHost(cap * 4)
            assert tj.lib().tjamd_scan_windows(k, arr, lens, nw, m, out.c, wof.c, cap) == -1
            out.check("out"); wof.check("window_of")
    tj.lib().tjamd_thread_cleanup()


def case_device_download(sample):
    c = sample[0]
    L = tj.lib()
    n = 1000003                                                                # (no multiple of anything)
    want = ((np.arange(n, dtype=np.int64) * 7 + 3) & 0xFF).astype(np.uint8)
    src = bc.dev(want)
    out = GuardedHost(n)
    assert L.tjamd_device_download(c._h, out.c, C.c_void_p(src.data_ptr()), n) == 0
    out.check("host")
    assert out.payload.tobytes() == want.tobytes()
    none = GuardedHost(64)
    assert L.tjamd_device_download(c._h, none.c, C.c_void_p(src.data_ptr()), 0) == 0 and none.untouched()
    none.check("host")


def case_gather_histograms(sample):
    c, o = finalised(sample)
    k = sample[4]
    L = tj.lib()
    for ns in (1, 3):
        hs = (C.c_void_p * ns)(*[c._h] * ns)
        counts = GuardedHost(ns * 8)
        drec = C.c_void_p()
        merger = tj.Counter(k)
        total = L.tjamd_gather_histograms(merger._h, hs, ns, C.byref(drec), C.cast(counts.c, C.POINTER(C.c_long)))
        counts.check("counts")
        assert total == ns * c.n_kept and counts.view(np.int64).tolist() == [c.n_kept] * ns
        got = np.zeros(total, tj.RECORD_DTYPE)
        assert L.tjamd_device_download(merger._h, got.ctypes.data, drec, total * 24) == 0
        e = o.elems()
        for s in range(ns):
            part = got[s * c.n_kept: (s + 1) * c.n_kept]
            assert all((part[f] == e[f]).all() for f in ("ctx0", "ctx1", "meta"))
        merger.close()


HOST_CASES = {"tjamd_download_raw": case_download_raw, "tjamd_download_kept": case_download_kept, "tjamd_download_idx": case_download_idx,
              "tjamd_scan_host_located": case_scan_host_located, "tjamd_group_contexts": case_group_contexts,
              "tjamd_context_histograms": case_context_histograms, "tjamd_reference_download": case_reference_download,
              "tjamd_scan_windows": case_scan_windows, "tjamd_device_download": case_device_download, "tjamd_gather_histograms": case_gather_histograms}


@pytest.mark.parametrize("entry", list(HOST_CASES))
def test_host_outputs_stay_inside_their_buffers(sample, entry):
    HOST_CASES[entry](sample)
