"""Where tjamd_consensus_tree writes, in the manner of tests/test_buffer_bounds.py: d_nodes, d_order and d_rep_count sit in
guarded buffers (tests/guarded.py) of exactly the size the header asks for, the inputs are held frozen, and the sample counts
lie on both sides of every edge the kernels have: the 16 wavefronts that share a replicate's nodes (15 to 17 nodes), a
wavefront's 64 lanes over the members of a clade and over the candidates for a parent (63 to 66 samples), the blocks of 256
records and the four kept classes a block of wavefronts takes (256 to 258 samples of one replicate), the sort's blocks of 1024
records and the workgroups of 1024 that order and lay out the kept classes (1024 to 1026), and the limit of 4096 samples with
four positions a thread (4095 and 4096).

The replicates are one tree under different leaf orders, so the answer is known without the restatement, whose frozensets
take seconds at 4096 samples (6.5 s for five replicates: affordable once, not at fifteen sizes; tests/test_consensus_limits.py
runs it there, on replicates that disagree): the consensus is that tree, every count is the number of replicates, a node's
interval starts with its smallest member, and its parent is the tree's.  A caterpillar, the most members a call can hold, runs
once at each limit.  Up to 258 samples the restatement is compared as well, on replicates that disagree."""
import numpy as np
import pytest

import tatajuba_amd as tj
from tests import bounds_calls as bc
from tests.test_consensus import caterpillar, check, cross_check, dev_consensus, laid_out, nested
from tests.test_consensus_cabi import NODE, fabricate_replicates, majority

pytestmark = pytest.mark.gpu

EDGES = [16, 17, 18, 63, 64, 65, 66, 256, 257, 258, 1024, 1025, 1026, 4095, 4096]
assert set(EDGES) & set(bc.SIZES) and max(EDGES) == max(s for s in bc.SIZES if s <= 4096)


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(15)
    yield c
    c.close()


def clades(tree, out):
    """the sets of the nested pairs, each with its parent's -> the set of `tree`"""
    if not isinstance(tree, tuple):
        return frozenset([tree])
    kids = [clades(child, out) for child in tree]
    mine = frozenset().union(*kids)
    for child, k in zip(tree, kids):
        if isinstance(child, tuple):
            out[k] = mine
    out.setdefault(mine, None)
    return mine


def check_one_tree(got, tree, ns, R):
    nodes, order = got["nodes"], got["order"].tolist()
    parent_of = {}
    clades(tree, parent_of)
    assert len(nodes) == ns - 1 == len(parent_of) and got["n_classes"] == ns - 1 and (nodes["count"] == R).all()
    assert sorted(order) == list(range(ns)) and all((c == R).all() for c in got["rep_count"])
    sets = [frozenset(order[f: f + s]) for f, s in zip(nodes["first"].tolist(), nodes["size"].tolist())]
    keys = [(len(s), min(s)) for s in sets]
    assert keys == sorted(keys) and len(set(sets)) == ns - 1 and set(sets) == set(parent_of)
    index = {s: j for j, s in enumerate(sets)}
    for j, s in enumerate(sets):
        assert order[nodes["first"][j]] == min(s), j                     # children ascending by smallest member: the smallest comes first
        assert nodes["parent"][j] == (-1 if parent_of[s] is None else index[parent_of[s]]), j


@pytest.mark.parametrize("ns", EDGES)
def test_one_tree_at_every_edge(counter, ns):
    rng = np.random.RandomState(ns)
    tree = nested([int(x) for x in rng.permutation(ns)], rng)
    for R in (1, 2):
        reps = [laid_out(tree, rng) for _ in range(R)]
        got = dev_consensus(counter, reps, ns, R)
        assert isinstance(got, dict), got[:2]
        check_one_tree(got, tree, ns, R)
        got_null = dev_consensus(counter, reps, ns, R, null=("rep_count", "classes"))
        assert got_null["nodes"].tobytes() == got["nodes"].tobytes() and got_null["order"].tobytes() == got["order"].tobytes()
    cross_check(counter, reps, ns, got, bases=1)
    if ns <= 258:                                                         # replicates that disagree, against the restatement
        reps = fabricate_replicates(ns, 3, 1 + ns // 64, 300 + ns)
        check(counter, reps, ns, 2)
        # a refused call at this size writes nothing: a node that ends one behind the samples, in the last replicate
        bad = reps[:2] + [(reps[2][0][:-1] + [(ns - 1, 2)], reps[2][1])]
        rc, err, _ = dev_consensus(counter, bad, ns, 2)
        assert rc == -3 and "replicate 2" in err, (rc, err)


@pytest.mark.parametrize("ns", [4095, 4096])
def test_a_caterpillar_at_the_limit(counter, ns):
    """ns - 1 nested clades of up to ns members: the most the comparison, the parents and the layout can be asked for"""
    rng = np.random.RandomState(ns)
    orders = [rng.permutation(ns).astype(np.int32)]
    orders.append(np.r_[orders[0][:2][::-1], orders[0][2:]].astype(np.int32))     # the same sets, the first two samples swapped
    got = dev_consensus(counter, [(caterpillar(ns, True), o) for o in orders], ns, 2)
    assert isinstance(got, dict), got[:2]
    want = sorted(orders[0][:2].tolist())
    for x in orders[0][2:].tolist():                                      # a node's children: the node below it and one sample, the smaller first
        want = [x] + want if x < want[0] else want + [x]
    assert got["order"].tolist() == want and got["n_classes"] == ns - 1
    nodes = got["nodes"]
    assert nodes["parent"].tolist() == list(range(1, ns - 1)) + [-1] and (nodes["count"] == 2).all() and nodes["size"].tolist() == list(range(2, ns + 1))
    # a node's interval holds the first `size` samples of the replicates' order
    at = {s: p for p, s in enumerate(want)}
    place = np.array([at[s] for s in orders[0].tolist()])
    lo, hi = np.minimum.accumulate(place), np.maximum.accumulate(place)
    assert nodes["first"].tolist() == lo[1:].tolist() and (hi[1:] - lo[1:] + 1).tolist() == nodes["size"].tolist()
    assert all((c == 2).all() for c in got["rep_count"])
    assert nodes.view(NODE)["first"].tolist() == nodes["first"].tolist() and majority(2) == 2
