"""tjamd_clade_support up to the 4096 samples it holds, and the bootstrap chain at the sample counts that switch on the large forms.

The support.  tests/test_bootstrap.py stops at 130 samples; the kernel walks the samples 1024 at a time, keeps positions as
unsigned shorts, packs a node as first << 13 | size and looks it up in a set of 8192 places.  Here: 1023, 1024 and 1025 samples
(the second trip of the 1024-thread loops), 2049, 4095 and 4096; caterpillars (all keys share `first`, or `first` runs to
n_samples - 2; sizes to n_samples: 4095 nodes in the 8192 places, keys that differ in their low bits alone) and a balanced tree;
seven replicates per case.  Every case is against restate_clade_support_by_positions, which tests/test_bootstrap_cabi.py holds to
the set-per-node restatement.

The counts cannot be trivial, and cannot reach 7 or 0 either: replicates 1 and 2 (the base, and the base over the reversed order)
hold every node, replicate 5 holds none, so a count lies in 2 .. 6.  test_the_cases_are_not_trivial asserts, without a device,
that every case has a node at 6, a node at 2 and a node in between; the all-and-nothing ends are test_one_replicate_at_the_limit
(0 and 1) and test_4096_replicates (4096).

The chain.  tjamd_bootstrap_weights -> tjamd_sample_distances_weighted -> per replicate tjamd_sample_linkage and
tjamd_sample_agglomerate (both linkages) -> tjamd_linkage_tree -> tjamd_clade_support on a planted corpus of 70 samples (tiles of
edge 32, the key pass and the rounds of both tree builders) and of 130 (more than one tile a side), every step against its
restatement.  Outputs sit in guarded buffers, inputs are frozen, every call is made twice (the dev_* helpers)."""
import functools

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.test_agglomerate import dev_agglomerate
from tests.test_agglomerate_cabi import AVERAGE, COMPLETE, restate_sample_agglomerate
from tests.test_bootstrap import (check_weighted, dev_support, dev_weighted, dev_weights, nested_family, planted_distances, planted_trees)
from tests.test_bootstrap_cabi import nodes_of, restate_clade_support, restate_clade_support_by_positions
from tests.test_clades import check_tree, dev_tree
from tests.test_distances import check_distances, dev_distances
from tests.test_linkage import check_links, dev_linkage
from tests.test_linkage_cabi import DIFFER, restate_sample_linkage

ERR_ARG = 3
LIMIT = 4096
SAMPLE_COUNTS = (1023, 1024, 1025, 2049, 4095, 4096)
TREES = ("caterpillar", "reversed caterpillar", "balanced")
PERMUTATION = "d_order or a replicate's order is not a permutation of 0 .. n_samples - 1"
NODE = "a node has size < 2, first < 0 or first + size above n_samples %d"


def tree_intervals(kind, ns):
    """the ns - 1 nodes of a tree over the positions 0 .. ns - 1, as (first, size), the root last"""
    if kind == "caterpillar":
        return [(0, s) for s in range(2, ns + 1)]
    if kind == "reversed caterpillar":
        return [(ns - s, s) for s in range(2, ns + 1)]
    out = []

    def split(lo, hi):                                                        # balanced: children before their parent
        if hi - lo >= 2:
            split(lo, (lo + hi) // 2)
            split((lo + hi) // 2, hi)
            out.append((lo, hi - lo))

    split(0, ns)
    return out


def broken_by_swap(iv, p):
    """the nodes that hold one of the leaves at positions p and p + 1 and not the other: swapping the two takes their sets apart"""
    return [(f, s) for f, s in iv if (f <= p < f + s) != (f <= p + 1 < f + s)]


def swap_position(iv, ns):
    """where replicate 4 swaps two neighbouring leaves: 1023 | 1024, the edge of the kernel's first trip, where the samples reach
    it and a node ends there (1025 samples: the reversed caterpillar has no node of one leaf); the middle otherwise"""
    return 1023 if ns >= 1025 and broken_by_swap(iv, 1023) else ns // 2 - 1


@functools.lru_cache(maxsize=None)
def case(kind, ns):
    """-> nodes, order, the seven replicates, the expected support"""
    rng = np.random.RandomState(ns * 3 + TREES.index(kind))
    iv = tree_intervals(kind, ns)
    assert len(iv) == ns - 1 and iv[-1] == (0, ns)
    nodes, order = nodes_of(iv), rng.permutation(ns).astype(np.int32)
    p = swap_position(iv, ns)
    swapped = order.copy()
    swapped[[p, p + 1]] = order[[p + 1, p]]
    broken = broken_by_swap(iv, p)
    whole = [x for x in iv[:-1] if x not in frozenset(broken)]
    assert broken and len(whole) >= (ns - 1) // 2
    half = whole[: (ns - 1) // 2]
    other = tree_intervals("reversed caterpillar" if kind == "caterpillar" else "caterpillar", ns)
    reps = [(nodes, order),                                                   # 1 the base itself
            (nodes_of([(ns - f - s, s) for f, s in iv]), order[::-1].copy()),  # 2 over the reversed order: every set is a node again, elsewhere
            (nodes, rng.permutation(ns).astype(np.int32)),                    # 3 its nodes over a random order: the root alone, almost surely
            (nodes, swapped),                                                 # 4 two neighbouring leaves swapped: every set but the broken ones
            (nodes[:0], rng.permutation(ns).astype(np.int32)),                # 5 no node
            (nodes_of([iv[-1]] * (ns - 1 - len(half)) + half), order),        # 6 ns - 1 nodes, half of them the root again and again; no broken set
            (nodes_of(other), order)]                                         # 7 the other caterpillar: the root, and the prefixes of a balanced tree
    want = restate_clade_support_by_positions(nodes, order, reps)
    return nodes, order, reps, want


@pytest.mark.parametrize("kind", TREES)
@pytest.mark.parametrize("ns", SAMPLE_COUNTS)
def test_the_cases_are_not_trivial(kind, ns):
    """on the restatement alone, before a device is asked.  The root is in every replicate that has a node: 6; a set that replicate
    4 breaks is in replicates 1 and 2 alone (a prefix of a balanced tree also in 7): 2; the others lie in between"""
    nodes, order, reps, want = case(kind, ns)
    assert len(nodes) == ns - 1 and len(reps) == 7 and [len(rn) for rn, _ in reps] == [ns - 1] * 4 + [0] + [ns - 1] * 2
    assert want[-1] == 6 == want.max() and want.min() == 2 and ((want > 2) & (want < 6)).any(), np.bincount(want)
    assert len(set(want.tolist())) >= 3
    if kind == "balanced" or ns == 1023:                                      # ... and the fast restatement is the plain one, where that is affordable
        assert restate_clade_support(nodes, order, reps).tolist() == want.tolist()


def test_the_edge_cases_are_not_trivial():
    for make in (one_replicate_case, most_nodes_case, many_replicates_case):
        nodes, order, reps, want = make()
        assert want.min() < want.max(), make.__name__
    assert set(one_replicate_case()[3].tolist()) == {0, 1} and many_replicates_case()[3].max() == 4096 and many_replicates_case()[3].min() == 0


@functools.lru_cache(maxsize=None)
def one_replicate_case():
    """4096 samples, one replicate: the reversed caterpillar's nodes over the base's order; the root and nothing else is held"""
    nodes, order = case("caterpillar", LIMIT)[:2]
    reps = [(nodes_of(tree_intervals("reversed caterpillar", LIMIT)), order)]
    return nodes, order, reps, restate_clade_support_by_positions(nodes, order, reps)


@functools.lru_cache(maxsize=None)
def most_nodes_case():
    """n_nodes 4096, the entry's limit: the 4095 nodes of the caterpillar and one of them again"""
    nodes, order, reps, want = case("caterpillar", LIMIT)
    nodes = np.concatenate([nodes, nodes[2000: 2001]])
    return nodes, order, reps, np.concatenate([want, want[2000: 2001]])


@functools.lru_cache(maxsize=None)
def many_replicates_case():
    """three samples, 4096 replicates.  The base over the order 2 0 1: {0, 1}, the root and {2, 0}.  Every replicate holds the
    root; of every four, one holds {0, 1} at places 0 and 1, one has it side by side but as no node, one holds it at places 1 and
    2, and one holds {2, 1}, which is no set of the base.  {2, 0} is in none"""
    nodes, order = nodes_of([(1, 2), (0, 3), (0, 2)]), np.array([2, 0, 1], np.int32)
    four = [([(0, 3), (0, 2)], [0, 1, 2]), ([(0, 3)], [1, 0, 2]), ([(0, 3), (1, 2)], [2, 1, 0]), ([(0, 3), (1, 2)], [0, 2, 1])]
    reps = [(nodes_of(four[r % 4][0]), np.array(four[r % 4][1], np.int32)) for r in range(4096)]
    want = restate_clade_support(nodes, order, reps)
    assert want.tolist() == [2048, 4096, 0] == restate_clade_support_by_positions(nodes, order, reps).tolist()
    return nodes, order, reps, want


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(15)
    yield c
    c.close()


def check_support(got, want):
    assert isinstance(got, np.ndarray), got[:2]
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", TREES)
@pytest.mark.parametrize("ns", SAMPLE_COUNTS)
def test_support_of_large_trees(counter, kind, ns):
    nodes, order, reps, want = case(kind, ns)
    check_support(dev_support(counter, nodes, order, reps), want)


@pytest.mark.gpu
def test_the_limit_of_nodes(counter):
    nodes, order, reps, want = most_nodes_case()
    assert len(nodes) == LIMIT
    check_support(dev_support(counter, nodes, order, reps), want)


@pytest.mark.gpu
def test_one_replicate_at_the_limit(counter):
    nodes, order, reps, want = one_replicate_case()
    check_support(dev_support(counter, nodes, order, reps), want)


@pytest.mark.gpu
def test_4096_replicates(counter):
    nodes, order, reps, want = many_replicates_case()
    check_support(dev_support(counter, nodes, order, reps), want)


@pytest.mark.gpu
def test_refusals_at_the_limit(counter):
    nodes, order, reps, want = case("balanced", LIMIT)
    twice = order.copy()
    twice[int(np.flatnonzero(order == 0)[0])] = LIMIT - 1                      # sample 4095 twice, sample 0 missing
    rep_twice = reps[2][1].copy()
    rep_twice[int(np.flatnonzero(rep_twice == 0)[0])] = LIMIT - 1
    beyond = reps[3][0].copy()
    beyond[LIMIT - 2]["first"], beyond[LIMIT - 2]["size"] = LIMIT - 1, 2       # a replicate's node (4095, 2)
    too_large = nodes.copy()
    too_large[LIMIT - 2]["size"] = LIMIT + 1                                   # a base node of 4097
    cases = [(PERMUTATION, nodes, twice, reps), (PERMUTATION, nodes, order, reps[:2] + [(reps[2][0], rep_twice)] + reps[3:]),
             (NODE % LIMIT, nodes, order, reps[:3] + [(beyond, reps[3][1])] + reps[4:]), (NODE % LIMIT, too_large, order, reps)]
    for msg, n, o, rr in cases:
        with pytest.raises(ValueError):
            restate_clade_support_by_positions(n, o, rr)
        rc, err, buf = dev_support(counter, n, o, rr)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert buf.untouched(), msg
    check_support(dev_support(counter, nodes, order, reps), want)             # the counter serves the next good call


# ---- the chain ------------------------------------------------------------------------------------------------------------

CHAIN_REPLICATES = 9
BUILDERS = {"single": (lambda d: restate_sample_linkage(d, DIFFER, 1), lambda c, d: dev_linkage(c, d, DIFFER, 1)),
            "complete": (lambda d: restate_sample_agglomerate(d, DIFFER, 1, COMPLETE)[0], lambda c, d: dev_agglomerate(c, d, DIFFER, 1, COMPLETE)[0]),
            "average": (lambda d: restate_sample_agglomerate(d, DIFFER, 1, AVERAGE)[0], lambda c, d: dev_agglomerate(c, d, DIFFER, 1, AVERAGE)[0])}


@functools.lru_cache(maxsize=None)
def chain(ns):
    """the restated chain: ns samples, 4 ns sites on the halves, quarters, ... and pairs of the samples, 15 % of the cells
    missing, 9 replicates; the trees of all three builders"""
    x = planted_distances(ns=ns, n_sites=4 * ns, R=CHAIN_REPLICATES, seed=ns, family=nested_family(ns), corpus_seed=ns)
    x["trees"] = {name: planted_trees(x, restate, restate_clade_support_by_positions) for name, (restate, _) in BUILDERS.items()}
    return x


@pytest.mark.parametrize("ns", [70, 130])
def test_the_chain_is_not_trivial(ns):
    """on the restatement: every builder has a clade in every replicate and one in some of them only; and the fast
    restatement of the support is the plain one"""
    x = chain(ns)
    assert len(nested_family(ns)) >= ns - 2 and min(len(f) for f in nested_family(ns)) == 2
    assert (x["g"] == -1).mean() > 0.1
    for name, t in x["trees"].items():
        s = t["support"]
        assert len(t["base"]["nodes"]) == ns - 1 and s.max() == CHAIN_REPLICATES and ((s > 0) & (s < CHAIN_REPLICATES)).any(), (name, s)
        assert restate_clade_support(t["base"]["nodes"], t["base"]["order"], [(r["nodes"], r["order"]) for r in t["rep_trees"]]).tolist() == s.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [70, 130])
def test_the_chain_at_the_large_forms(counter, ns):
    x = chain(ns)
    sites, alleles, g = x["sites"], x["alleles"], x["g"]
    got_w = dev_weights(counter, len(sites), CHAIN_REPLICATES, ns)
    assert got_w.tobytes() == x["w"].tobytes()
    got_dist = dev_weighted(counter, sites, alleles, g, ns, got_w)
    check_weighted(got_dist, x["rep_dist"])
    dist = dev_distances(counter, sites, alleles, g, ns)
    check_distances(dist, x["dist"])
    for name, (_, build) in BUILDERS.items():
        t = x["trees"][name]
        links = build(counter, dist)
        check_links(links, t["base_links"])
        tree = dev_tree(counter, links, ns)
        check_tree(tree, t["base"], name)
        reps = []
        for r in range(CHAIN_REPLICATES):
            links = build(counter, got_dist[r])
            check_links(links, t["rep_links"][r])
            rt = dev_tree(counter, links, ns)
            check_tree(rt, t["rep_trees"][r], (name, r))
            reps.append((rt["nodes"], rt["order"]))
        check_support(dev_support(counter, tree["nodes"], tree["order"], reps), t["support"])
