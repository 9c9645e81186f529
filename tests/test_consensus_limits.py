"""tjamd_consensus_tree at the limits of what it admits, with no difference allowed anywhere: every result is compared with the
restatement of tests/test_consensus_cabi.py through check of tests/test_consensus.py.  tests/test_consensus.py stops at 8
replicates, and tests/test_consensus_bounds.py reaches 4096 samples on one tree under different leaf orders, where every run of
equal keys is one class; here:

  many replicates    9 samples x 4096 replicates, 66 x 512 and 257 x 1024 (262 144 records), each at the majority, one above it
                     and at n_replicates: the replicate found by the binary search over the offsets, counts between the
                     majority and all, classes that are rejected;
  the sample limit   replicates that disagree at 2049 samples x 3 and at 4096 x 5: runs of several classes, rejected classes and
                     a second round of comparisons at the size where a thread holds four positions;
  the comparison     1025 samples x 3 under TATAJUBA_AMD_CONSENSUS_KEY_BITS 0, 3 and the default: with no bit of the hash every
                     class of a size is told apart by comparison alone, over hundreds of rounds;
  equal offsets      replicates without a node at the front, in the middle and at the back, several in a row;
  a twin node        a node listed twice in a replicate with a node of another class, of the same size and (under KEY_BITS 0) the
                     same key, between the two: the replicate counts once for the class;
  the chain          tjamd_replicate_trees at 1025 samples x 5 under complete linkage into tjamd_consensus_tree.

What the shapes need to hold is asserted without a device.  Outputs always sit in guarded buffers (tests/guarded.py), every input
is held frozen, and every call is made twice and must give the same bytes (tests/test_consensus.py: dev_consensus)."""
import collections
import functools

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.test_agglomerate_cabi import COMPLETE
from tests.test_consensus import _counter_under, check, cross_check, dev_consensus, same
from tests.test_consensus_cabi import fabricate_replicates, majority, pack, restate_consensus
from tests.test_linkage_cabi import DIFFER, fabricate_small
from tests.test_replicate_trees import dev_rep_trees

# (ns, R, k, seed)
MANY = [(9, 4096, 1, 1), (66, 512, 2, 1), (257, 1024, 5, 1)]
LIMIT = [(2049, 3, 8, 2049), (4096, 5, 8, 4096)]
COMPARED = (1025, 3, 5, 1025)
GAPS = (20, 70, 1, 20)
EMPTY = (0, 1, 2, 31, 32, 33, 34, 35, 67, 68, 69)          # the replicates of GAPS without a node


@functools.lru_cache(maxsize=None)
def replicates(shape):
    ns, R, k, seed = shape
    return fabricate_replicates(ns, R, k, seed)


@functools.lru_cache(maxsize=None)
def wanted(shape, min_count):
    return restate_consensus(*pack(replicates(shape), shape[0]), shape[0], min_count)


def three_thresholds(R):
    return [majority(R), majority(R) + 1, R]


def classes_by_size(reps):
    """the distinct sets of the replicates' nodes -> {size: how many}"""
    sets = {frozenset(np.asarray(order)[f: f + s].tolist()) for iv, order in reps for f, s in iv}
    return collections.Counter(len(s) for s in sets)


@pytest.mark.parametrize("shape", MANY + LIMIT, ids=str)
def test_the_replicates_disagree(shape):
    """at the majority: a kept count strictly between the majority and all the replicates, and a rejected class"""
    ns, R = shape[:2]
    most = wanted(shape, majority(R))
    counts = most["nodes"]["count"]
    if shape in MANY:
        assert ((counts > majority(R)) & (counts < R)).any(), sorted(set(counts.tolist()))
    else:
        assert len(counts) >= ns // 2                       # (three replicates: no count lies between two and three)
    assert most["n_classes"] > len(most["nodes"]) > 0
    assert max(classes_by_size(replicates(shape)).values()) > 1                            # several classes of one size


def gap_replicates():
    ns, R = GAPS[:2]
    return [([], order) if r in EMPTY else (iv, order) for r, (iv, order) in enumerate(replicates(GAPS))]


def test_the_replicates_without_a_node_leave_a_consensus():
    ns, R = GAPS[:2]
    reps = gap_replicates()
    counts = pack(reps, ns)[2]
    offsets = np.r_[0, np.cumsum(counts)[:-1]].tolist()
    assert offsets[:4] == [0, 0, 0, 0] and len(set(offsets[31:37])) == 1 and offsets[67:] == [offsets[67]] * 3 and offsets[67] == sum(counts)
    want = restate_consensus(*pack(reps, ns), ns, majority(R))
    assert len(want["nodes"]) > 0 and want["n_classes"] > len(want["nodes"]) and want["nodes"]["count"].max() <= R - len(EMPTY)
    assert want["nodes"]["count"].min() < R - len(EMPTY)


def twin_replicates(mirrored):
    """8 samples, 3 replicates.  Replicate 1 lists {0,1} (mirrored: {2,3}) twice with the other pair between the two; the others
    hold every set once, at other places of other orders"""
    a, b = ((2, 2), (0, 2)) if mirrored else ((0, 2), (2, 2))
    twin = ([(4, 2), a, b, a, (0, 4), (0, 8)], [0, 1, 2, 3, 4, 5, 6, 7])
    return [([(0, 2), (2, 2), (0, 4), (0, 8)], [1, 0, 3, 2, 5, 4, 7, 6]), twin, ([(6, 2), (4, 2), (4, 4), (0, 8)], [7, 6, 5, 4, 3, 2, 1, 0])], 8


@pytest.mark.parametrize("mirrored", [False, True])
def test_a_twin_node_counts_once_in_the_restatement(mirrored):
    reps, ns = twin_replicates(mirrored)
    want = restate_consensus(*pack(reps, ns), ns, 2)
    # {0,1}, {2,3} and {0,1,2,3} in all three replicates, {4,5} in one, the full set in three
    assert [tuple(int(x) for x in n) for n in want["nodes"]] == [(2, 3, 0, 2), (2, 3, 2, 2), (3, 3, 0, 4), (-1, 3, 0, 8)] and want["n_classes"] == 5
    assert want["rep_count"][1].tolist() == [1, 3, 3, 3, 3, 3]


# ---- on the device --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def _inputs_released():
    """the replicates and their restatements are made once per shape and shared, and given back with the module"""
    yield
    replicates.cache_clear()
    wanted.cache_clear()


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(15)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hook_counters():
    """every clade of a size in one run; eight keys a size; and the keys as they are"""
    cs = {"0": _counter_under(TATAJUBA_AMD_CONSENSUS_KEY_BITS="0"), "3": _counter_under(TATAJUBA_AMD_CONSENSUS_KEY_BITS="3"), "default": tj.Counter(15)}
    yield cs
    for c in cs.values():
        c.close()


def held(counter, shape, min_count):
    got = dev_consensus(counter, replicates(shape), shape[0], min_count)
    same(got, wanted(shape, min_count), (shape, min_count))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2], ids=["the majority", "one above it", "all replicates"])
@pytest.mark.parametrize("shape", MANY, ids=str)
def test_many_replicates(counter, shape, which):
    ns, R = shape[:2]
    got = held(counter, shape, three_thresholds(R)[which])
    if which == 0 and R == 512:                             # (cheap there: a call of tjamd_clade_support takes its replicates one by one on the host side of the test)
        cross_check(counter, replicates(shape), ns, got, bases=1)


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [False, True], ids=["the majority", "all replicates"])
@pytest.mark.parametrize("shape", LIMIT, ids=str)
def test_disagreeing_replicates_at_the_sample_limit(counter, shape, strict):
    ns, R = shape[:2]
    got = held(counter, shape, R if strict else majority(R))
    assert strict or len(got["nodes"]) >= ns // 2


@pytest.mark.gpu
def test_the_comparison_path_at_1025_samples(hook_counters):
    ns, R = COMPARED[:2]
    sizes = classes_by_size(replicates(COMPARED))
    assert sizes[2] > 64 and max(sizes.values()) == sizes[2]                               # with no bit of the hash: a run of that many classes, a round each
    got = {bits: held(c, COMPARED, majority(R)) for bits, c in hook_counters.items()}
    for g in got.values():
        assert g["nodes"].tobytes() == got["default"]["nodes"].tobytes() and g["order"].tobytes() == got["default"]["order"].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g["rep_count"], got["default"]["rep_count"]))


@pytest.mark.gpu
def test_replicates_without_a_node_at_the_front_in_the_middle_and_at_the_back(counter):
    ns, R = GAPS[:2]
    reps = gap_replicates()
    for m in (majority(R), R - len(EMPTY)):
        got = check(counter, reps, ns, m, m)
        assert len(got["nodes"]) > 0 and all(len(got["rep_count"][r]) == 0 for r in EMPTY)
    cross_check(counter, reps, ns, check(counter, reps, ns, majority(R)), bases=4)       # (the bases: replicates 3, of 0 to 3, alone has nodes)


@pytest.mark.gpu
@pytest.mark.parametrize("mirrored", [False, True])
def test_a_twin_node_behind_a_node_of_another_class(hook_counters, mirrored):
    """under KEY_BITS 0 the four nodes of size 2 of replicate 1 share a run, and the walk back from the second twin passes a
    record of its replicate and run that is of another class"""
    reps, ns = twin_replicates(mirrored)
    for bits in ("0", "default"):
        got = check(hook_counters[bits], reps, ns, 2, (mirrored, bits))
        assert got["nodes"]["count"].tolist() == [3, 3, 3, 3] and got["rep_count"][1].tolist() == [1, 3, 3, 3, 3, 3], bits
        assert check(hook_counters[bits], reps, ns, 3, (mirrored, bits, "strict"))["nodes"]["count"].tolist() == [3, 3, 3, 3]


def chain_input():
    """1025 samples, 5 replicates: one matrix with keys in 0..3, in every replicate 300 pairs drawn again"""
    ns, R = 1025, 5
    rng = np.random.RandomState(1025)
    base = fabricate_small(ns, rng)
    out = []
    for _ in range(R):
        d = base.copy()
        a, b = rng.randint(0, ns, 300), rng.randint(0, ns, 300)
        keep = a != b
        a, b = a[keep], b[keep]
        nd = rng.randint(0, 4, len(a))
        d["n_differ"][a, b] = d["n_differ"][b, a] = nd
        d["n_both"][a, b] = d["n_both"][b, a] = nd + rng.randint(0, 3, len(a))
        out.append(d)
    return np.stack(out)


@pytest.mark.gpu
def test_the_chain_at_1025_samples(counter):
    """the trees of tjamd_replicate_trees as they come from the device, forests among them, into tjamd_consensus_tree"""
    ns, R = 1025, 5
    trees = dev_rep_trees(counter, chain_input(), DIFFER, 2, COMPLETE)
    reps = [(t["nodes"], t["order"]) for t in trees]
    assert min(len(t["nodes"]) for t in trees) < ns - 1
    got = check(counter, reps, ns, majority(R), "the chain")
    assert got["n_classes"] > len(got["nodes"]) > 0
    cross_check(counter, reps, ns, got, bases=1)
