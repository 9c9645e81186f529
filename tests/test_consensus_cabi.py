"""The majority-rule consensus tree of the bootstrap replicates (include/tatajuba_consensus.h: tjamd_consensus_tree) without a
GPU: the entry is declared in its own header, exported and prototyped and refuses bad arguments before any device call; the
restatement that the GPU tests (tests/test_consensus.py) compare against is pinned by answers worked out by hand; and the
fabricated corpus those tests run on is shown here to hold what they need it to hold.

restate_consensus is the rule of the header in plain Python on frozensets: classes are dictionary keys, so equality is set
equality and nothing else."""
import ctypes as C
import fnmatch
import glob
import os
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedHost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_consensus_tree", "tjamd_last_consensus_tree_ms"]
ERR_NO_DEVICE, ERR_ARG = 1, 3
NODE, CNODE = tj.TREE_NODE_DTYPE, tj.CONSENSUS_NODE_DTYPE
PERMUTATION, RANGE, CROSS = "is not a permutation", "has size < 2, first < 0 or first + size above n_samples", "cross"


def majority(R):
    return R // 2 + 1


def nodes_of(intervals):
    out = np.zeros(len(intervals), NODE)
    out["left"], out["right"] = -9, -9                                    # never read
    for i, (first, size) in enumerate(intervals):
        out[i]["first"], out[i]["size"] = first, size
    return out


def pack(reps, ns):
    """reps: [(intervals or NODE array, order)] -> rep_nodes NODE [R * (ns - 1)], rep_orders int32 [R * ns], counts"""
    rep_nodes = np.zeros(len(reps) * max(ns - 1, 0), NODE)
    rep_nodes["first"], rep_nodes["size"] = -7, -7                        # beyond a replicate's count: never read
    rep_orders = np.zeros(len(reps) * ns, np.int32)
    counts = []
    for r, (rn, ro) in enumerate(reps):
        rn = rn if isinstance(rn, np.ndarray) else nodes_of(rn)
        rep_nodes[r * (ns - 1): r * (ns - 1) + len(rn)] = rn
        rep_orders[r * ns: (r + 1) * ns] = ro
        counts.append(len(rn))
    return rep_nodes, rep_orders, counts


def restate_consensus(rep_nodes, rep_orders, counts, ns, min_count):
    """-> {"nodes": CNODE [n], "order": int32 [ns], "rep_count": [int32 [counts[r]]], "n_classes"}.  ValueError for what the
    entry refuses on the device: .replicate is the smallest refused replicate, the text its first broken rule."""
    R = len(counts)
    assert 2 * min_count > R and min_count <= R
    refused, sets = None, []
    for r in range(R):
        order = [int(x) for x in rep_orders[r * ns: (r + 1) * ns]]
        iv = [(int(n["first"]), int(n["size"])) for n in rep_nodes[r * (ns - 1): r * (ns - 1) + counts[r]]]
        why = None
        if sorted(order) != list(range(ns)):
            why = PERMUTATION
        elif any(s < 2 or f < 0 or f + s > ns for f, s in iv):
            why = RANGE
        elif any(a < b < a + s < b + t for a, s in iv for b, t in iv):
            why = CROSS
        if why and refused is None:
            refused = ValueError(why)
            refused.replicate = r
        sets.append([] if why else [frozenset(order[f: f + s]) for f, s in iv])
    if refused is not None:
        raise refused
    holders = {}
    for r, clades in enumerate(sets):
        for s in clades:
            holders.setdefault(s, set()).add(r)                           # two equal nodes of one replicate: once
    count = {s: len(h) for s, h in holders.items()}
    kept = sorted((s for s in count if count[s] >= min_count), key=lambda s: (len(s), min(s)))
    for i, a in enumerate(kept):
        for b in kept[i + 1:]:
            assert a < b or a.isdisjoint(b), (sorted(a), sorted(b))       # nested or disjoint (and never equal, nor b inside a: the order)
    parent = [next((i for i in range(j + 1, len(kept)) if s < kept[i]), -1) for j, s in enumerate(kept)]
    children = {j: [] for j in range(-1, len(kept))}                      # (smallest member, node or None for a sample)
    for j, p in enumerate(parent):
        children[p].append((min(kept[j]), j))
    for t in range(ns):
        children[next((j for j, s in enumerate(kept) if t in s), -1)].append((t, None))
    order, first = [], {}
    stack = [iter(sorted(children[-1], key=lambda c: c[0]))]
    while stack:
        item = next(stack[-1], None)
        if item is None:
            stack.pop()
        elif item[1] is None:
            order.append(item[0])
        else:
            first[item[1]] = len(order)
            stack.append(iter(sorted(children[item[1]], key=lambda c: c[0])))
    nodes = np.zeros(len(kept), CNODE)
    for j, s in enumerate(kept):
        nodes[j] = (parent[j], count[s], first[j], len(s))
        assert frozenset(order[first[j]: first[j] + len(s)]) == s         # the node's interval of the order is the node's set
    assert sorted(order) == list(range(ns)) and order[0] == 0
    return {"nodes": nodes, "order": np.array(order, np.int32), "rep_count": [np.array([count[s] for s in c], np.int32) for c in sets], "n_classes": len(count),
            "n_children": [len(children[j]) for j in range(len(kept))]}


def as_rows(nodes):
    return [tuple(int(x) for x in n) for n in nodes]


# ---- answers by hand ---------------------------------------------------------------------------------------------------------

def one_differing_replicate():
    """5 samples, 3 replicates: two caterpillars from the left and one from the right, which shares the full set alone"""
    left = [(0, 2), (0, 3), (0, 4), (0, 5)]
    right = [(3, 2), (2, 3), (1, 4), (0, 5)]
    return [(left, [0, 1, 2, 3, 4]), (left, [1, 0, 2, 3, 4]), (right, [0, 1, 2, 3, 4])], 5


def test_a_resolved_tree_at_the_majority_and_a_star_at_the_strict_threshold():
    reps, ns = one_differing_replicate()
    got = restate_consensus(*pack(reps, ns), ns, 2)
    # {0,1} {0,1,2} {0,1,2,3} twice each, the full set three times; (size, smallest member) is their order, each the next one's child
    assert as_rows(got["nodes"]) == [(1, 2, 0, 2), (2, 2, 0, 3), (3, 2, 0, 4), (-1, 3, 0, 5)] and got["order"].tolist() == [0, 1, 2, 3, 4]
    assert got["n_classes"] == 7 and [c.tolist() for c in got["rep_count"]] == [[2, 2, 2, 3], [2, 2, 2, 3], [1, 1, 1, 3]]
    star = restate_consensus(*pack(reps, ns), ns, 3)
    assert as_rows(star["nodes"]) == [(-1, 3, 0, 5)] and star["order"].tolist() == [0, 1, 2, 3, 4] and star["n_children"] == [5]
    assert star["n_classes"] == 7 and [c.tolist() for c in star["rep_count"]] == [c.tolist() for c in got["rep_count"]]


def three_children():
    """6 samples, 3 replicates: {0,1} in all, {2,3} and {0..4} in two, {0,1,2,3} in one.  {0..4} has the children {0,1}, {2,3}
    and the sample 4; the sample 5 is a root beside it.  The third replicate holds {0,1} at another place of another order."""
    return [([(0, 2), (2, 2), (0, 5)], [0, 1, 2, 3, 4, 5]), ([(0, 2), (2, 2), (0, 4), (0, 5)], [1, 0, 3, 2, 4, 5]), ([(1, 2)], [5, 1, 0, 3, 2, 4])], 6


def test_a_node_with_three_children():
    reps, ns = three_children()
    got = restate_consensus(*pack(reps, ns), ns, 2)
    assert as_rows(got["nodes"]) == [(2, 3, 0, 2), (2, 2, 2, 2), (-1, 2, 0, 5)] and got["order"].tolist() == [0, 1, 2, 3, 4, 5]
    assert got["n_children"] == [2, 2, 3] and got["n_classes"] == 4
    assert [c.tolist() for c in got["rep_count"]] == [[3, 2, 2], [3, 2, 1, 2], [3]]
    strict = restate_consensus(*pack(reps, ns), ns, 3)
    assert as_rows(strict["nodes"]) == [(-1, 3, 0, 2)] and strict["order"].tolist() == [0, 1, 2, 3, 4, 5]


def two_roots():
    """5 samples, 1 replicate: {0,3} and {2,4}, and the sample 1 in neither: it lies between them, by its own number"""
    return [([(0, 2), (3, 2)], [4, 2, 1, 3, 0])], 5


def test_two_roots_and_a_lone_sample_between_them():
    reps, ns = two_roots()
    got = restate_consensus(*pack(reps, ns), ns, 1)
    assert as_rows(got["nodes"]) == [(-1, 1, 0, 2), (-1, 1, 3, 2)] and got["order"].tolist() == [0, 3, 1, 2, 4]
    assert got["n_classes"] == 2
    # two equal nodes in one replicate count once, and each gets the count; no node at all: the identity
    twice = restate_consensus(*pack([([(0, 2), (3, 2), (0, 2)], [4, 2, 1, 3, 0])], ns), ns, 1)
    assert as_rows(twice["nodes"]) == as_rows(got["nodes"]) and twice["rep_count"][0].tolist() == [1, 1, 1] and twice["n_classes"] == 2
    none = restate_consensus(*pack([([], [4, 2, 1, 3, 0]), ([], [0, 1, 2, 3, 4])], ns), ns, 2)
    assert len(none["nodes"]) == 0 and none["order"].tolist() == [0, 1, 2, 3, 4] and none["n_classes"] == 0


def test_the_restatement_refuses_what_the_device_refuses():
    reps, ns = three_children()
    for change, why in [(([(0, 2)], [0, 1, 2, 3, 4, 4]), PERMUTATION), (([(0, 2), (5, 2)], [0, 1, 2, 3, 4, 5]), RANGE), (([(0, 1)], [0, 1, 2, 3, 4, 5]), RANGE),
                        (([(0, 3), (2, 3)], [0, 1, 2, 3, 4, 5]), CROSS)]:
        with pytest.raises(ValueError, match=re.escape(why)) as e:
            restate_consensus(*pack(reps[:2] + [change], ns), ns, 2)
        assert e.value.replicate == 2
    with pytest.raises(ValueError, match=re.escape(RANGE)) as e:                    # the smallest refused replicate, and its first broken rule
        restate_consensus(*pack([reps[0], ([(0, 3), (2, 3), (-1, 2)], reps[0][1]), ([(0, 2)], [0] * 6)], ns), ns, 2)
    assert e.value.replicate == 1
    restate_consensus(*pack([([(0, 3), (0, 3), (3, 3), (0, 6), (1, 2)], list(range(6)))], ns), ns, 1)   # touching, nested and equal nodes do not cross


# ---- the fabricated corpus of the GPU tests -----------------------------------------------------------------------------------

def fabricate_tree(ns, rng):
    """a random order, and the intervals of a tree of recursive random splits over it, children before parents"""
    order = rng.permutation(ns).astype(np.int32)
    iv, todo = [], [(0, ns)]
    while todo:
        first, size = todo.pop()
        if size < 2:
            continue
        iv.append((first, size))
        cut = int(rng.randint(1, size))
        todo += [(first, cut), (first + cut, size - cut)]
    return order, sorted(iv, key=lambda n: (n[1], n[0]))


def fabricate_replicates(ns, R, k, seed):
    """R replicates of one tree, each over the tree's order with k random transpositions applied"""
    rng = np.random.RandomState(seed)
    order, iv = fabricate_tree(ns, rng)
    reps = []
    for _ in range(R):
        o = order.copy()
        for _ in range(k if ns > 1 else 0):
            a, b = rng.randint(0, ns, 2)
            o[a], o[b] = o[b], o[a]
        reps.append((iv, o))
    return reps


# (ns, R, k) -> seed: the shapes at which the GPU tests need the corpus to be a consensus worth the name
CORPUS = {(5, 3, 1): 4, (9, 5, 1): 1, (65, 5, 2): 1, (65, 8, 3): 1, (130, 5, 3): 1, (257, 7, 4): 1}


def corpus_properties(ns, R, k, seed):
    reps = fabricate_replicates(ns, R, k, seed)
    packed = pack(reps, ns)
    most, strict = restate_consensus(*packed, ns, majority(R)), restate_consensus(*packed, ns, R)
    return {"keeps a quarter": 4 * len(most["nodes"]) >= ns, "three children": max(most["n_children"], default=0) >= 3,
            "rejects a class": most["n_classes"] > len(most["nodes"]), "strict keeps fewer": len(strict["nodes"]) < len(most["nodes"])}


@pytest.mark.parametrize("shape", sorted(CORPUS))
def test_the_fabricated_corpus_is_worth_a_consensus(shape):
    ns, R, k = shape
    held = corpus_properties(ns, R, k, CORPUS[shape])
    assert all(held.values()), f"seed {CORPUS[shape]} at (ns, R, k) = {shape} does not give a corpus that {[w for w, ok in held.items() if not ok]}: choose another seed"


# ---- declarations and argument checks --------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    own_path = os.path.join(ROOT, "include", "tatajuba_consensus.h")
    own = strip(own_path)
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.CONSENSUS_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    assert re.search(r"typedef struct \{ int parent, count, first, size; \} tjamd_consensus_node;", own)
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_consensus.h"]
    assert len(others) >= 15
    earlier = (tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS + tj.EFFECT_EXPORTS + tj.SITE_EXPORTS + tj.DEPTH_EXPORTS + tj.DISTANCE_EXPORTS
               + tj.LINKAGE_EXPORTS + tj.AGGLOMERATE_EXPORTS + tj.GROUP_EXPORTS + tj.CLADE_EXPORTS + tj.BOOTSTRAP_EXPORTS + tj.REPLICATE_TREE_EXPORTS)
    for s in NEW_ENTRIES:
        for path in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(path)), (s, path)   # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in earlier and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert '#include "tatajuba_replicate_trees.h"' in own
    assert CNODE.names == ("parent", "count", "first", "size") and CNODE.itemsize == 16
    assert [CNODE.fields[f][1] for f in ("first", "size")] == [NODE.fields[f][1] for f in ("first", "size")]   # where tjamd_tree_node has them
    assert L.tjamd_last_consensus_tree_ms(None) == -1.0
    for name in ("consensus_tree", "last_consensus_tree_ms"):
        assert hasattr(tj.Counter, name)
    text = open(own_path).read()
    for what in ("Of a node only first and size are read", "same set of samples", "two equal nodes of one replicate count once", "2 * min_count > n_replicates",
                 "strict consensus", "(size, smallest member)", "a child always comes before its parent", "d_order[0] == 0", "identity order",
                 "rests on no hash", "TATAJUBA_AMD_CONSENSUS_KEY_BITS", "not a permutation", "cross", "names the smallest refused replicate",
                 "*h_n_classes is left alone", "Two runs give the same bytes", "cast to tjamd_tree_node", "44 bytes per clade", "caterpillar",
                 "Not built", "greedy", "branch lengths", "Robinson-Foulds", "base tree", "Ward", "neighbour joining"):
        assert what in text, what
    # the headers before this one stay as they were written, their "Not built" lists included
    assert "support written into the Newick file; Ward and neighbour joining. */" in open(os.path.join(ROOT, "include", "tatajuba_replicate_trees.h")).read()
    assert "support written into the Newick file" in open(os.path.join(ROOT, "include", "tatajuba_bootstrap.h")).read()


def _caller():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call fails its argument checks first
    classes = GuardedHost(8)
    classes_before = classes.payload.copy()

    def call(c=fake, rep_nodes=fake, rep_order=fake, counts=(4, 0, 3), ns=5, n_rep=3, min_count=2, nodes=fake, order=fake, rep_count=fake, null_classes=False):
        h_counts = None if counts is None else (C.c_int * max(len(counts), 1))(*counts)
        rc = L.tjamd_consensus_tree(c, rep_nodes, rep_order, h_counts, ns, n_rep, min_count, nodes, order, rep_count,
                                    None if null_classes else C.cast(classes.c, C.POINTER(C.c_long)))
        return rc, L.tjamd_last_error().decode()

    def untouched():
        classes.check("h_n_classes")
        return bool((classes.payload == classes_before).all())

    return call, untouched


def test_consensus_tree_checks_its_arguments_without_a_gpu():
    call, untouched = _caller()
    for kw, msg in [({"c": None}, "null counter"), ({"rep_order": None}, "null d_rep_order"), ({"counts": None}, "null h_rep_n_nodes"), ({"order": None}, "null d_order"),
                    ({"nodes": None}, "null d_nodes"), ({"nodes": None, "ns": 2, "counts": (1, 0, 1)}, "null d_nodes"),
                    ({"rep_nodes": None}, "null d_rep_nodes"), ({"rep_nodes": None, "counts": (0, 0, 1)}, "null d_rep_nodes"),
                    ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": -3}, "n_samples -3 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"),
                    ({"n_rep": 0}, "n_replicates 0 outside 1..4096"), ({"n_rep": -1}, "n_replicates -1 outside 1..4096"), ({"n_rep": 4097}, "n_replicates 4097 outside 1..4096"),
                    ({"counts": (4, 5, 0)}, "replicate 1 has 5 nodes, outside 0..n_samples - 1 = 4"), ({"counts": (4, 0, -1)}, "replicate 2 has -1 nodes"),
                    ({"ns": 1, "counts": (0, 1, 0), "nodes": None}, "replicate 1 has 1 nodes, outside 0..n_samples - 1 = 0"),
                    ({"min_count": 1}, "min_count 1 outside 2..3"), ({"min_count": 4}, "min_count 4 outside 2..3"), ({"min_count": 0}, "min_count 0 outside 2..3"),
                    ({"min_count": -2}, "min_count -2 outside 2..3"), ({"n_rep": 2, "counts": (1, 1), "min_count": 1}, "min_count 1 outside 2..2"),
                    ({"n_rep": 1, "counts": (1,), "min_count": 2}, "min_count 2 outside 1..1"), ({"n_rep": 1, "counts": (1,), "min_count": 0}, "min_count 0 outside 1..1")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_consensus_tree") and msg in err, (kw, got, err)
        assert untouched()
    if tj.device_count() == 0:                     # good arguments, but nothing to run on: named, before the handles are read
        for kw in ({}, {"min_count": 3}, {"rep_count": None, "null_classes": True}, {"rep_nodes": None, "counts": (0, 0, 0)}, {"ns": 1, "counts": (0, 0, 0), "nodes": None, "rep_nodes": None},
                   {"ns": 4096, "n_rep": 4096, "counts": (4095,) * 4096, "min_count": 2049}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_consensus_tree") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
            assert untouched()


def test_consensus_tree_reports_the_first_of_two_broken_rules_without_a_gpu():
    call, untouched = _caller()
    for kw, msg in [({"c": None, "rep_order": None}, "null counter"), ({"rep_order": None, "counts": None}, "null d_rep_order"), ({"counts": None, "order": None}, "null h_rep_n_nodes"),
                    ({"order": None, "ns": 0}, "null d_order"), ({"ns": 0, "n_rep": 0}, "n_samples 0 outside 1..4096"), ({"n_rep": 4097, "nodes": None}, "n_replicates 4097 outside 1..4096"),
                    ({"nodes": None, "counts": (9, 0, 0)}, "null d_nodes"), ({"counts": (9, 0, 0), "min_count": 1}, "replicate 0 has 9 nodes"),
                    ({"rep_nodes": None, "min_count": 1}, "null d_rep_nodes")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_consensus_tree") and msg in err, (kw, got, err)
    assert untouched()
