"""tjamd_replicate_trees on the GPU, with no difference allowed anywhere: every result is compared with the restatement of
tests/test_replicate_trees_cabi.py and with the existing entries run per replicate on the device (tjamd_sample_linkage or
tjamd_sample_agglomerate, then tjamd_linkage_tree).  Sample counts on both sides of the single-workgroup path (64), of the
key pass's tiles (32) and of a wavefront's 128 cells, 1025 samples once; replicate counts 1, 2, 3 and 5; all three linkages;
replicate groups of two; replicates of one call that end at different rounds, in every position, with batches of 32 and of 4
rounds; two pairs that merge in one round, in the middle replicate; forests of different sizes in one call; every refusal of
N15 and N18 planted in the last replicate and in the last replicate of the second group; a counter reused across sizes and
entries; and the chain of N19 on its planted corpus.  Outputs always sit in guarded buffers (tests/guarded.py), every input is
held frozen, and every call is made twice and must give the same bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, frozen, payload_pattern
from tests.test_agglomerate import CROSS, dev_agglomerate
from tests.test_agglomerate_cabi import AVERAGE, COMPLETE, KEY_MAX, cap_for_average
from tests.test_bootstrap import PLANTED_NS, PLANTED_REPLICATES, PLANTED_SEED, PLANTED_SITES, dev_support, dev_weighted, dev_weights, planted_chain
from tests.test_clades import dev_tree
from tests.test_distances import dev_distances
from tests.test_linkage import dev_linkage
from tests.test_linkage_cabi import DIFFER, LENGTH, as_tuples, fabricate_small, fabricate_wide, symmetric
from tests.test_locate import _dev, _p
from tests.test_replicate_trees_cabi import LINKAGES, SINGLE, UNSET, restate_replicate_trees

pytestmark = pytest.mark.gpu

ERR_ARG = 3
DIST, LINK, NODE = tj.SAMPLE_DISTANCE_DTYPE, tj.LINK_DTYPE, tj.TREE_NODE_DTYPE
CELL, MIRROR, KEY = "a cell has n_both < 0, n_differ < 0, n_differ > n_both or length_diff < 0", "differs from the cell (b, a)", "a key of 2^40 or more under TJAMD_AGGL_AVERAGE"


def _torch():
    return pytest.importorskip("torch")


def dev_rep_trees(counter, dist, metric, min_both, linkage, null_links=False):
    """two calls of tjamd_replicate_trees on dist [R, ns, ns] -> per replicate {"links", "n_rounds", "nodes", "order"} as numpy;
    or, when the call is refused, (negative code, message, the guarded buffers).  Entries past a replicate's n_nodes must
    hold what the buffer held before the call.  dist may be (device bytes of the matrices, R, ns), for an input laid out on the device."""
    torch = _torch()
    L = tj.lib()
    dd, R, ns = dist if isinstance(dist, tuple) else (_dev(dist),) + dist.shape[:2]
    runs = []
    for _ in range(2):
        bufs = {"links": GuardedDevice(R * (ns - 1) * LINK.itemsize), "nodes": GuardedDevice(R * (ns - 1) * NODE.itemsize), "order": GuardedDevice(R * ns * 4)}
        counts, rounds = (C.c_int * R)(*[UNSET] * R), (C.c_int * R)(*[UNSET] * R)
        torch.cuda.synchronize()
        with frozen(dd):
            rc = L.tjamd_replicate_trees(counter._h, _p(dd), ns, R, metric, min_both, linkage, None if null_links else bufs["links"].c, bufs["nodes"].c if ns > 1 else None,
                                         bufs["order"].c, counts, rounds)
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        for k, b in bufs.items():
            b.check("d_rep_" + k)
        if rc < 0:
            assert counter.last_replicate_trees_ms() == -1.0 and err.startswith("tjamd_replicate_trees")
            assert list(counts) == [UNSET] * R and list(rounds) == [UNSET] * R         # the host outputs too
            return rc, err, bufs
        assert rc == R and (ns == 1 or counter.last_replicate_trees_ms() > 0)
        raw = {k: b.payload.cpu().numpy() for k, b in bufs.items()}
        pattern = {k: payload_pattern(bufs[k].nbytes) for k in ("links", "nodes")}
        out = []
        for r in range(R):
            n = counts[r]
            assert 0 <= n <= ns - 1 and 0 <= rounds[r] <= n, (r, n, rounds[r])
            for k in ("links", "nodes"):                                                # entries from n_nodes on are not written
                lo, hi = (r * (ns - 1) + (0 if null_links and k == "links" else n)) * 16, (r + 1) * (ns - 1) * 16
                assert (raw[k][lo:hi] == pattern[k][lo:hi]).all(), (k, r, n)
            at = r * (ns - 1) * 16
            out.append({"links": raw["links"][at: at + n * 16].copy().view(LINK), "nodes": raw["nodes"][at: at + n * 16].copy().view(NODE),
                        "order": raw["order"][r * ns * 4: (r + 1) * ns * 4].copy().view(np.int32), "n_rounds": rounds[r]})
        runs.append(out)
    for a, b in zip(*runs):                                                             # two runs: the same bytes
        assert all(a[k].tobytes() == b[k].tobytes() for k in ("links", "nodes", "order")) and a["n_rounds"] == b["n_rounds"]
    return runs[0]


def loop_on_device(counter, dist, metric, min_both, linkage):
    """the per-replicate loop of the existing entries -> the same list"""
    out = []
    ns = dist.shape[1]
    for d in dist:
        d = np.ascontiguousarray(d)
        links, n_rounds = (dev_linkage(counter, d, metric, min_both), 0) if linkage == SINGLE else dev_agglomerate(counter, d, metric, min_both, linkage)
        out.append(dict(dev_tree(counter, links, ns), links=links, n_rounds=n_rounds))
    return out


def same(got, want, what=""):
    assert isinstance(got, list), (what, got[:2])
    assert len(got) == len(want), what
    for r, (g, w) in enumerate(zip(got, want)):
        assert g["n_rounds"] == w["n_rounds"], (what, r, g["n_rounds"], w["n_rounds"])
        for k in ("links", "nodes", "order"):
            assert len(g[k]) == len(w[k]) and g[k].tobytes() == w[k].tobytes(), (what, r, k, g[k][:6], w[k][:6])


def check(counter, dist, metric, min_both, linkage, what="", loop=None, want=None):
    """the call against the restatement and against the loop on the device (want, loop: their results where the caller has them)"""
    got = dev_rep_trees(counter, dist, metric, min_both, linkage)
    same(got, restate_replicate_trees(dist, metric, min_both, linkage) if want is None else want, (what, "restatement"))
    same(got, loop_on_device(counter, dist, metric, min_both, linkage) if loop is None else loop, (what, "loop"))
    return got


def _counter_under(**env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    c = tj.Counter(15)
    for k, v in saved.items():
        if v is None:
            del os.environ[k]
        else:
            os.environ[k] = v
    return c


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(15)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rounds_counter():
    """a counter whose calls never take the single-workgroup path"""
    c = _counter_under(TATAJUBA_AMD_LINKAGE_SMALL="0")
    yield c
    c.close()


@pytest.fixture(scope="module")
def group_counter():
    """replicates go through two at a time"""
    c = _counter_under(TATAJUBA_AMD_TREES_GROUP="2")
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch_counter():
    """four rounds between two looks at the flag words"""
    c = _counter_under(TATAJUBA_AMD_AGGL_BATCH="4")
    yield c
    c.close()


def stack_small(ns, R, rng):
    return np.stack([fabricate_small(ns, rng) for _ in range(R)])


COUNTS = [1, 2, 3, 33, 63, 64, 65, 66, 129, 257]
REPLICATES = [1, 2, 3, 5]


@pytest.mark.parametrize("ns,kind", [(ns, "default") for ns in COUNTS] + [(ns, "rounds") for ns in COUNTS if ns <= 64])
def test_sample_and_replicate_counts(counter, rounds_counter, ns, kind):
    c = counter if kind == "default" else rounds_counter
    rng = np.random.RandomState(2000 + ns)
    dist = stack_small(ns, max(REPLICATES), rng)          # keys in 0..3; under min_both 2 many pairs are no edge: ties and forests
    for linkage in LINKAGES:
        loop, want = loop_on_device(c, dist, DIFFER, 2, linkage), restate_replicate_trees(dist, DIFFER, 2, linkage)
        for R in REPLICATES:
            check(c, dist[:R], DIFFER, 2, linkage, (ns, R, linkage), loop=loop[:R], want=want[:R])
        wide = np.stack([cap_for_average(fabricate_wide(ns, rng)) if linkage == AVERAGE else fabricate_wide(ns, rng) for _ in range(2)])
        check(c, wide, LENGTH, 1, linkage, (ns, "wide", linkage))
    full = dev_rep_trees(c, dist[:3], DIFFER, 2, COMPLETE)                             # d_rep_links may be NULL: the same nodes and orders
    for g, f in zip(dev_rep_trees(c, dist[:3], DIFFER, 2, COMPLETE, null_links=True), full):
        assert g["nodes"].tobytes() == f["nodes"].tobytes() and g["order"].tobytes() == f["order"].tobytes() and g["n_rounds"] == f["n_rounds"]


def test_more_than_a_sample_per_thread(counter):
    """1025 samples: a workgroup of 1024 no longer holds a sample per thread in the pair kernel, the sort and the tree"""
    ns = 1025
    dist = stack_small(ns, 2, np.random.RandomState(1025))
    dist["n_both"][1] += 2                                                             # the second replicate: every pair an edge
    got = dev_rep_trees(counter, dist, DIFFER, 2, COMPLETE)
    same(got, restate_replicate_trees(dist, DIFFER, 2, COMPLETE), "restatement")
    same(got, loop_on_device(counter, dist, DIFFER, 2, COMPLETE), "loop")
    assert len(got[1]["links"]) == ns - 1


@pytest.mark.parametrize("ns", [40, 66])
def test_replicate_groups(group_counter, ns):
    rng = np.random.RandomState(3000 + ns)
    dist = stack_small(ns, 5, rng)
    for linkage in LINKAGES:
        loop = loop_on_device(group_counter, dist, DIFFER, 2, linkage)
        for R in (1, 2, 3, 5):
            check(group_counter, dist[:R], DIFFER, 2, linkage, (ns, R, linkage), loop=loop[:R])


def mixed_replicates(ns, rng):
    """all keys equal (ns - 1 rounds under the agglomerative linkages), keys in 0..3 (a handful of rounds), no edge at all"""
    full = np.ones((ns, ns), np.int64)
    equal = symmetric(ns, 3 * full, full - np.eye(ns, dtype=np.int64), 2 * (full - np.eye(ns, dtype=np.int64)))
    few = fabricate_small(ns, rng)
    few["n_both"] += 1
    none = symmetric(ns, 0 * full, 0 * full, 0 * full)
    return equal, few, none


@pytest.mark.parametrize("ns", [66, 40])
@pytest.mark.parametrize("kind", ["batches of 32", "batches of 4"])
def test_replicates_that_end_at_different_rounds(counter, batch_counter, ns, kind):
    """a replicate that is done must stay as it is while the others of its call go on: 65 rounds are three batches of 32"""
    c = counter if kind == "batches of 32" else batch_counter
    equal, few, none = mixed_replicates(ns, np.random.RandomState(4000 + ns))
    for linkage in LINKAGES:
        loops = {id(d): loop_on_device(c, d[None], DIFFER, 1, linkage)[0] for d in (equal, few, none)}
        assert linkage == SINGLE or (loops[id(equal)]["n_rounds"] == ns - 1 and 0 < loops[id(few)]["n_rounds"] < ns - 1)
        assert len(loops[id(none)]["links"]) == 0 and loops[id(none)]["n_rounds"] == 0
        for order in ((equal, few, none), (few, none, equal), (none, equal, few)):       # each of the three first, in the middle and last
            check(c, np.stack(order), DIFFER, 1, linkage, (ns, linkage), loop=[loops[id(d)] for d in order])


@pytest.mark.parametrize("cross", sorted(CROSS))
@pytest.mark.parametrize("ns,at", [(66, (0, 65, 20, 40)), (40, (1, 39, 2, 38))])
def test_two_pairs_of_one_round_in_the_middle_replicate(counter, ns, at, cross):
    """N18's planted case (tests/test_agglomerate.py) as replicate 1 of 3: the cell of the two unions holds all four cells"""
    s0, s1, s2, s3 = at
    k01, k23, k02, k03, k12, k13 = CROSS[cross]
    rng = np.random.RandomState(ns)
    nd = 1000 + rng.randint(0, 100, (ns, ns))
    for (a, b), v in {(s0, s1): k01, (s2, s3): k23, (s0, s2): k02, (s0, s3): k03, (s1, s2): k12, (s1, s3): k13}.items():
        nd[min(a, b), max(a, b)] = v
    np.fill_diagonal(nd, 0)
    planted = symmetric(ns, np.full((ns, ns), 5000), nd, nd)
    others = stack_small(ns, 2, rng)
    others["n_both"] += 1
    dist = np.stack([others[0], planted, others[1]])
    first = [(a, b, k) for k, a, b in sorted([(k01, min(s0, s1), max(s0, s1)), (k23, min(s2, s3), max(s2, s3))])]
    union = tuple(sorted((min(s0, s1), min(s2, s3))))
    for linkage, key in ((AVERAGE, (k02 + k03 + k12 + k13) // 4), (COMPLETE, max(k02, k03, k12, k13))):
        got = check(counter, dist, DIFFER, 1, linkage, (ns, linkage))
        assert as_tuples(got[1]["links"])[:3] == first + [(union[0], union[1], key)]


@pytest.mark.parametrize("ns", [9, 70])
def test_forests_of_different_sizes_share_a_call(counter, ns):
    rng = np.random.RandomState(5000 + ns)
    whole = fabricate_small(ns, rng)
    whole["n_both"] += 2
    halves = whole.copy()                                                               # two cliques: ns - 2 links
    for f in DIST.names:
        halves[f][: ns // 2, ns // 2:] = 0
        halves[f][ns // 2:, : ns // 2] = 0
    alone = whole.copy()                                                                # the last sample has no edge: ns - 2 links, another shape
    alone["n_both"][ns - 1, : ns - 1] = alone["n_both"][: ns - 1, ns - 1] = 1
    alone["n_differ"][ns - 1, : ns - 1] = alone["n_differ"][: ns - 1, ns - 1] = 0
    none = symmetric(ns, np.zeros((ns, ns)), np.zeros((ns, ns)), np.zeros((ns, ns)))
    dist = np.stack([halves, none, whole, alone])
    for linkage in LINKAGES:
        got = check(counter, dist, DIFFER, 2, linkage, (ns, linkage))
        assert [len(g["nodes"]) for g in got] == [ns - 2, 0, ns - 1, ns - 2]
        assert got[1]["order"].tolist() == list(range(ns))


def refusal_cases(d, ns):
    """(message, linkage or None for any, metric, [(field, cell, value)]): what N15 refuses, and N18's bound"""
    last = ns - 1
    nb = lambda at: int(d["n_both"][at])
    cases = [(MIRROR, None, DIFFER, [("n_both", (last, 3), nb((last, 3)) + 1)]),
             (MIRROR, None, DIFFER, [("n_differ", (0, ns - 30), int(d["n_differ"][0, ns - 30]) + 1)]),
             (MIRROR, None, DIFFER, [("length_diff", (33, 34), int(d["length_diff"][33, 34]) + 1)]),
             (CELL, None, DIFFER, [("n_differ", (5, ns - 10), nb((5, ns - 10)) + 1), ("n_differ", (ns - 10, 5), nb((5, ns - 10)) + 1)]),
             (CELL, None, DIFFER, [("n_both", (last, last), -3)]),
             (CELL, None, DIFFER, [("n_differ", (last, last - 1), -1), ("n_differ", (last - 1, last), -1)]),
             (CELL, None, DIFFER, [("length_diff", (31, 31), -(1 << 62))]),
             (KEY, AVERAGE, LENGTH, [("length_diff", (2, last), KEY_MAX), ("length_diff", (last, 2), KEY_MAX), ("n_both", (2, last), 5), ("n_both", (last, 2), 5)])]
    return cases


@pytest.mark.parametrize("ns", [40, 70])
def test_device_refusals(counter, group_counter, ns):
    """each refusal planted in the last replicate alone (one group), and in the last replicate of the second group (groups of
    two): the whole call is refused, the replicate is named, nothing is written for the good replicates before it"""
    rng = np.random.RandomState(6000 + ns)
    good = stack_small(ns, 4, rng)
    good["n_both"] += 1
    for c, R in ((counter, 3), (group_counter, 4)):
        for i, (msg, only, metric, changes) in enumerate(refusal_cases(good[R - 1], ns)):
            linkage = LINKAGES[i % 3] if only is None else only
            bad = good[:R].copy()
            for field, at, value in changes:
                bad[field][R - 1][at] = value
            with pytest.raises(ValueError) as e:
                restate_replicate_trees(bad, metric, 2, linkage)
            assert e.value.replicate == R - 1
            rc, err, bufs = dev_rep_trees(c, bad, metric, 2, linkage)
            assert rc == -ERR_ARG and msg in err and err.endswith("(replicate %d)" % (R - 1)), (msg, R, rc, err)
            assert all(b.untouched() for b in bufs.values()), (msg, R)                 # nothing was written, for no replicate
    for c in (counter, group_counter):                                                  # the counters serve the next good call
        check(c, good, DIFFER, 2, AVERAGE)
    # COMPLETE and single linkage have no bound on a key
    big = good[:3].copy()
    big["length_diff"][2][2, ns - 1] = big["length_diff"][2][ns - 1, 2] = KEY_MAX
    for linkage in (SINGLE, COMPLETE):
        check(counter, big, LENGTH, 2, linkage)


@pytest.mark.parametrize("ns", [40, 70])
def test_two_device_refusals_in_different_replicates(counter, group_counter, ns):
    """a cell that differs from its mirror in replicate 1 and a cell with n_differ > n_both in replicate 3: replicate 1's message"""
    good = stack_small(ns, 4, np.random.RandomState(7000 + ns))
    good["n_both"] += 1
    bad = good.copy()
    bad["n_both"][1][ns - 1, 3] += 1
    bad["n_differ"][3][5, ns - 10] = bad["n_differ"][3][ns - 10, 5] = int(good["n_both"][3][5, ns - 10]) + 1
    for c in (counter, group_counter):
        for linkage in LINKAGES:
            rc, err, bufs = dev_rep_trees(c, bad, DIFFER, 2, linkage)
            assert rc == -ERR_ARG and MIRROR in err and err.endswith("(replicate 1)"), (linkage, rc, err)
            assert all(b.untouched() for b in bufs.values())
    both = good.copy()                                                                  # two rules in one replicate: the first in N15's order
    both["n_both"][2][ns - 1, 3] += 1
    both["n_differ"][2][5, ns - 10] = both["n_differ"][2][ns - 10, 5] = int(good["n_both"][2][5, ns - 10]) + 1
    rc, err, bufs = dev_rep_trees(counter, both, DIFFER, 2, COMPLETE)
    assert rc == -ERR_ARG and CELL in err and err.endswith("(replicate 2)"), (rc, err)


def test_a_reused_counter_gives_the_bytes_of_a_fresh_one():
    rng = np.random.RandomState(8000)
    large, small = stack_small(130, 3, rng), stack_small(20, 5, rng)
    fresh = []
    for dist in (large, small):
        c = tj.Counter(15)
        fresh.append({linkage: dev_rep_trees(c, dist, DIFFER, 2, linkage) for linkage in LINKAGES})
        c.close()
    c = tj.Counter(15)
    try:
        for linkage in LINKAGES:
            same(dev_rep_trees(c, large, DIFFER, 2, linkage), fresh[0][linkage], "large")
            same(dev_rep_trees(c, small, DIFFER, 2, linkage), fresh[1][linkage], "small")
            one = loop_on_device(c, large[1:2], DIFFER, 2, AVERAGE)                    # tjamd_sample_agglomerate and tjamd_linkage_tree on the same scratch
            same(one, fresh[0][AVERAGE][1:2], "the entries between")
            same(dev_rep_trees(c, large, DIFFER, 2, linkage), fresh[0][linkage], "large again")
    finally:
        c.close()


def test_the_chain_on_the_planted_corpus(counter):
    """weights, weighted matrices, the trees of all replicates in one call, the support: equal to the per-replicate loop's"""
    ns, n_sites, R = PLANTED_NS, PLANTED_SITES, PLANTED_REPLICATES
    x = planted_chain()
    w = dev_weights(counter, n_sites, R, PLANTED_SEED)
    rep_dist = dev_weighted(counter, x["sites"], x["alleles"], x["g"], ns, w)
    dist = dev_distances(counter, x["sites"], x["alleles"], x["g"], ns)
    base = dev_tree(counter, dev_linkage(counter, dist, DIFFER, 1), ns)
    got = dev_rep_trees(counter, rep_dist, DIFFER, 1, SINGLE)
    for r in range(R):
        assert got[r]["links"].tobytes() == x["rep_links"][r].tobytes(), r
        assert got[r]["nodes"].tobytes() == x["rep_trees"][r]["nodes"].tobytes() and got[r]["order"].tobytes() == x["rep_trees"][r]["order"].tobytes(), r
    loop = loop_on_device(counter, rep_dist, DIFFER, 1, SINGLE)
    same(got, loop, "loop")
    support = dev_support(counter, base["nodes"], base["order"], [(g["nodes"], g["order"]) for g in got])
    assert support.tolist() == dev_support(counter, base["nodes"], base["order"], [(g["nodes"], g["order"]) for g in loop]).tolist() == x["support"].tolist()
    # the wrapper, on device pointers, feeding tjamd_clade_support as it stands
    torch = _torch()
    dd = _dev(rep_dist)
    links, nodes, order = (torch.zeros(R * ns * 16, dtype=torch.uint8, device="cuda") for _ in range(3))
    counts, rounds = counter.replicate_trees(_p(dd), ns, R, tj.LINK_DIFFER, 1, tj.TREE_SINGLE, _p(links), _p(nodes), _p(order))
    assert counts == [len(g["nodes"]) for g in got] and rounds == [0] * R and counter.last_replicate_trees_ms() > 0
    bn, bo, out = _dev(base["nodes"]), _dev(base["order"]), torch.zeros(len(base["nodes"]) * 4, dtype=torch.uint8, device="cuda")
    assert counter.clade_support(_p(bn), len(base["nodes"]), _p(bo), ns, _p(nodes), _p(order), counts, _p(out)) == len(base["nodes"])
    assert out.cpu().numpy().view(np.int32).tolist() == x["support"].tolist()
    print(f"\n[replicate trees] {ns} samples, {R} replicates, single linkage: {counter.last_replicate_trees_ms():.3f} ms in one call")
