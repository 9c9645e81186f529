"""The clade step (include/tatajuba_clades.h: tjamd_linkage_tree, tjamd_clade_sites) without a GPU: the entries are declared in
their own header, exported and prototyped and refuse bad arguments before any device call, the node record matches the header,
and the restatements that the GPU tests (tests/test_clades.py) compare against are pinned by a hand case whose expected records
are written out here, by second forms of themselves and by properties on random inputs.

restate_linkage_tree is written from the rule in the header in two independent forms that must agree byte for byte: one is a
union-find over the links that hands first positions down from the roots, one takes node j's clade as the component of a in
restate_linkage_clusters (tests/test_linkage_cabi.py) applied to the first j + 1 links and lays the leaves out by recursion.
restate_clade_sites has three: per node with the smallest and the largest genotype of the clade's called samples (the one the GPU
tests use at any size), site by site with sets, and per node through restate_group_sites_table (tests/test_groups_cabi.py) with
the clade as group 0 and the rest as group 1.  The device reads a site by prefix counts over the leaf order."""
import ctypes as C
import fnmatch
import glob
import os
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedHost
from tests.test_depths_cabi import _fields
from tests.test_groups_cabi import as_tuples, restate_group_sites_table
from tests.test_linkage_cabi import restate_linkage_clusters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_linkage_tree", "tjamd_clade_sites", "tjamd_last_linkage_tree_ms", "tjamd_last_clade_sites_ms"]
ERR_NO_DEVICE, ERR_ARG, ERR_CAPACITY = 1, 3, 4
LINK, NODE, CALL, GSITE, MARK = tj.LINK_DTYPE, tj.TREE_NODE_DTYPE, tj.GROUP_CALL_DTYPE, tj.GROUP_SITE_DTYPE, tj.GROUP_MARK_DTYPE
OUTPUTS = ("calls", "sites", "node_marks", "marks")


def links_of(pairs):
    """LINK records of (a, b) pairs; the keys ascend, and the tree does not read them"""
    out = np.zeros(len(pairs), LINK)
    for j, (a, b) in enumerate(pairs):
        out[j] = (a, b, j)
    return out


# ---- the tree ---------------------------------------------------------------------------------------------------------------

def _checked_links(links, ns):
    links = np.asarray(links, LINK)
    assert 1 <= ns <= 4096 and len(links) <= ns - 1
    if len(links) and ((links["a"] < 0) | (links["a"] >= links["b"]) | (links["b"] >= ns)).any():
        raise ValueError("link")
    return links


def restate_linkage_tree(links, ns):
    """union-find over the links -> {"nodes": NODE [n_links], "order": int32 [ns]}; ValueError for what is refused on the device"""
    links = _checked_links(links, ns)
    parent, node_of, members = list(range(ns)), [-1 - s for s in range(ns)], [1] * ns      # per label: the node that is the component, its size
    smallest = list(range(ns))
    nodes = np.zeros(len(links), NODE)

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for j, l in enumerate(links):
        ra, rb = find(int(l["a"])), find(int(l["b"]))
        if ra == rb:
            raise ValueError("cycle")
        if smallest[rb] < smallest[ra]:
            ra, rb = rb, ra                                                       # ra: the side with the smaller smallest member
        if members[ra] < members[rb]:                                             # union by size: the label is not the smallest member
            keep, gone = rb, ra
        else:
            keep, gone = ra, rb
        nodes[j] = (node_of[ra], node_of[rb], -1, members[ra] + members[rb])
        smallest[keep], members[keep], node_of[keep] = smallest[ra], members[ra] + members[rb], j
        parent[gone] = keep
    order = np.full(ns, -1, np.int32)
    at = 0
    for r in sorted((s for s in range(ns) if parent[s] == s), key=lambda s: smallest[s]):
        if node_of[r] >= 0:
            nodes[node_of[r]]["first"] = at
        else:
            order[at] = -1 - node_of[r]
        at += members[r]
    for j in range(len(links) - 1, -1, -1):                                       # a parent before its children
        first = int(nodes[j]["first"])
        for child in (int(nodes[j]["left"]), int(nodes[j]["right"])):
            if child >= 0:
                nodes[child]["first"] = first
                first += int(nodes[child]["size"])
            else:
                order[first] = -1 - child
                first += 1
    return {"nodes": nodes, "order": order}


def restate_linkage_tree_by_clusters(links, ns):
    """the same from the components of the first j + 1 links, every key 0 and the threshold 0; the leaves by recursion"""
    links = _checked_links(links, ns)
    flat = links.copy()
    flat["key"] = 0
    labels = [restate_linkage_clusters(flat[:j], ns, 0) for j in range(len(links) + 1)]      # labels[j]: before link j
    clade, nodes = [], np.zeros(len(links), NODE)

    def as_child(members):
        if len(members) == 1:
            return -1 - members[0]
        return max(k for k in range(len(clade)) if clade[k] == members)                  # the latest node that is this component

    for j, l in enumerate(links):
        a, b = int(l["a"]), int(l["b"])
        if labels[j][a] == labels[j][b]:
            raise ValueError("cycle")
        sides = sorted([np.flatnonzero(labels[j] == labels[j][a]).tolist(), np.flatnonzero(labels[j] == labels[j][b]).tolist()], key=min)
        nodes[j]["left"], nodes[j]["right"] = as_child(sides[0]), as_child(sides[1])
        clade.append(np.flatnonzero(labels[j + 1] == labels[j + 1][a]).tolist())
        assert clade[j] == sorted(sides[0] + sides[1])
        nodes[j]["size"] = len(clade[j])

    def leaves(child):
        return [-1 - child] if child < 0 else leaves(int(nodes[child]["left"])) + leaves(int(nodes[child]["right"]))

    last = labels[len(links)]
    order = []
    for c in range(int(last.max()) + 1):                                          # components are numbered by smallest member
        order += leaves(as_child(np.flatnonzero(last == c).tolist()))
    place = {s: p for p, s in enumerate(order)}
    for j in range(len(links)):
        nodes[j]["first"] = min(place[s] for s in clade[j])
        assert sorted(place[s] for s in clade[j]) == list(range(int(nodes[j]["first"]), int(nodes[j]["first"]) + len(clade[j])))
    return {"nodes": nodes, "order": np.array(order, np.int32)}


def same_tree(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in ("nodes", "order"))


def tree_links(kind, ns, rng=None):
    """the link lists of the tests: a chain, the reverse chain, a balanced tree, a random forest with singletons and several roots,
    no link at all"""
    if kind == "chain":
        pairs = [(i, i + 1) for i in range(ns - 1)]
    elif kind == "reverse chain":
        pairs = [(ns - 2 - i, ns - 1 - i) for i in range(ns - 1)]
    elif kind == "balanced":
        pairs, step = [], 1
        while step < ns:
            pairs += [(i, i + step) for i in range(0, ns - step, 2 * step)]
            step *= 2
    elif kind == "forest":
        shuffled = rng.permutation(ns).tolist()
        in_play = shuffled[max(1, ns // 8) if ns > 2 else 0:]                     # the others are in no link
        pairs = []
        for part in (in_play[0::3], in_play[1::3], in_play[2::3]):                # three trees, each a random one over its samples
            pairs += [tuple(sorted((part[k], part[rng.randint(k)]))) for k in range(1, len(part))]
        pairs = [pairs[k] for k in rng.permutation(len(pairs))]                   # (any order of a forest's links is a list without a cycle)
    else:
        assert kind == "none"
        pairs = []
    return links_of(pairs)


TREE_KINDS = ("chain", "reverse chain", "balanced", "forest", "none")


# ---- the clade sites --------------------------------------------------------------------------------------------------------

def _clade_inputs(n_alleles, genotype, nodes, order, min_called):
    """the arrays of a call, checked as the device checks them: ValueError names what is refused there"""
    na, order = np.asarray(n_alleles, np.int64), np.asarray(order, np.int64)
    nodes = np.asarray(nodes, NODE)
    ns = len(order)
    gt = np.asarray(genotype, np.int64).reshape(len(na), ns)
    assert 1 <= ns <= 4096 and len(nodes) <= 4096 and min_called >= 1
    if sorted(order.tolist()) != list(range(ns)):
        raise ValueError("order")
    first, size = nodes["first"].astype(np.int64), nodes["size"].astype(np.int64)
    if (size < 2).any() or (first < 0).any() or (first + size > ns).any():
        raise ValueError("node")
    if (na < 1).any() or (na > ns).any():
        raise ValueError("n_alleles")
    if (gt < -1).any() or (gt > na[:, None]).any():
        raise ValueError("cell")
    return na, gt, nodes, order, ns


def _clade_result(calls, sites, marks):
    marks = np.array(marks, MARK) if len(marks) else np.zeros(0, MARK)
    node_marks = np.bincount(marks["group"], minlength=calls.shape[1]).astype(np.int32)
    return {"calls": calls, "sites": sites, "node_marks": node_marks, "marks": marks}


def restate_clade_sites(n_alleles, genotype, nodes, order, min_called):
    """the rule, node by node over all sites at once: the called members' smallest and largest genotype -> calls CALL [n_sites,
    n_nodes], sites GSITE [n_sites], node_marks int32 [n_nodes], marks MARK [n_marks] ascending in (site, node)"""
    na, gt, nodes, order, ns = _clade_inputs(n_alleles, genotype, nodes, order, min_called)
    n_sites, n_nodes, X = len(na), len(nodes), 4097
    laid = gt[:, order].astype(np.int32)                                          # the genotypes in leaf order
    rows = np.arange(n_sites)
    i, s = np.nonzero(gt >= 0)
    carriers = np.bincount(i * X + gt[i, s], minlength=n_sites * X).reshape(n_sites, X)   # per (site, genotype)
    site_called = (gt >= 0).sum(1)
    calls, sites = np.zeros((n_sites, n_nodes), CALL), np.zeros(n_sites, GSITE)
    for j in range(n_nodes):
        sub = laid[:, int(nodes[j]["first"]): int(nodes[j]["first"]) + int(nodes[j]["size"])]
        n_called = (sub >= 0).sum(1)
        low, high = np.where(sub >= 0, sub, X).min(1), sub.max(1)
        fixed = np.where(n_called == 0, -1, np.where(low == high, high, -2))
        n_outside = np.where(fixed >= 0, carriers[rows, np.maximum(fixed, 0)] - n_called, 0)
        calls["n_called"][:, j], calls["fixed"][:, j], calls["n_outside"][:, j] = n_called, fixed, n_outside
        calls["mark"][:, j] = (fixed >= 0) & (n_called >= min_called) & (n_outside == 0) & (site_called > n_called)
    m2 = calls["mark"] != 0
    sites["n_called"], sites["n_genotypes"], sites["n_marks"] = site_called, (carriers > 0).sum(1), m2.sum(1)
    sites["first_group"] = np.where(m2.any(1), m2.argmax(1), -1) if n_nodes else -1
    at_i, at_j = np.nonzero(m2)
    marks = np.zeros(len(at_i), MARK)
    marks["site"], marks["group"], marks["genotype"], marks["n_called"] = at_i, at_j, calls["fixed"][at_i, at_j], calls["n_called"][at_i, at_j]
    return _clade_result(calls, sites, marks)


def restate_clade_sites_sets(n_alleles, genotype, nodes, order, min_called):
    """the same, site by site with sets of samples"""
    na, gt, nodes, order, ns = _clade_inputs(n_alleles, genotype, nodes, order, min_called)
    calls, sites, marks = np.zeros((len(na), len(nodes)), CALL), np.zeros(len(na), GSITE), []
    members = [set(order[int(n["first"]): int(n["first"]) + int(n["size"])].tolist()) for n in nodes]
    for i in range(len(na)):
        called = {s for s in range(ns) if gt[i, s] >= 0}
        marked = []
        for j, clade in enumerate(members):
            mine, others = called & clade, called - clade
            carried = {int(gt[i, s]) for s in mine}
            fixed = -1 if not mine else carried.pop() if len(carried) == 1 else -2
            n_outside = sum(1 for s in others if gt[i, s] == fixed) if fixed >= 0 else 0
            mark = int(fixed >= 0 and len(mine) >= min_called and n_outside == 0 and len(others) > 0)
            calls[i, j] = (len(mine), fixed, n_outside, mark)
            if mark:
                marked.append(j)
                marks.append((i, j, fixed, len(mine)))
        sites[i] = (len(called), len({int(gt[i, s]) for s in called}), len(marked), marked[0] if marked else -1)
    return _clade_result(calls, sites, marks)


def restate_clade_sites_by_groups(n_alleles, genotype, nodes, order, min_called):
    """the same from N16's restatement: per node the two-group labelling (the clade 0, the rest 1), and group 0's record"""
    na, gt, nodes, order, ns = _clade_inputs(n_alleles, genotype, nodes, order, min_called)
    calls, sites = np.zeros((len(na), len(nodes)), CALL), np.zeros(len(na), GSITE)
    for j, n in enumerate(nodes):
        labels = np.ones(ns, np.int64)
        labels[order[int(n["first"]): int(n["first"]) + int(n["size"])]] = 0
        r = restate_group_sites_table(na, gt, labels, 2, min_called)
        calls[:, j] = r["calls"][:, 0]
        sites["n_called"], sites["n_genotypes"] = r["sites"]["n_called"], r["sites"]["n_genotypes"]      # (every sample takes part: the same for every node)
    if not len(nodes):
        r = restate_group_sites_table(na, gt, np.zeros(ns, np.int64), 1, min_called)
        sites["n_called"], sites["n_genotypes"] = r["sites"]["n_called"], r["sites"]["n_genotypes"]
    marks = []
    for i in range(len(na)):
        marked = np.flatnonzero(calls["mark"][i]).tolist()
        sites[i]["n_marks"], sites[i]["first_group"] = len(marked), marked[0] if marked else -1
        marks += [(i, j, int(calls[i, j]["fixed"]), int(calls[i, j]["n_called"])) for j in marked]
    return _clade_result(calls, sites, marks)


def same_result(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in OUTPUTS)


def random_matrix(rng, n_sites, ns, tree, p_missing=0.25, max_alleles=3, planted=4):
    """few alleles, so that clades are often fixed; every `planted`-th site gives one node's clade the site's last allele and
    nobody else (random cells mark nothing once the clades are large)"""
    na = rng.randint(1, min(max_alleles, ns) + 1, n_sites)
    gt = (rng.random_sample((n_sites, ns)) ** 2 * (na[:, None] + 1)).astype(np.int64)   # 0 most often
    gt[rng.random_sample((n_sites, ns)) < p_missing] = -1
    nodes, order = tree["nodes"], tree["order"]
    for i in range(0, n_sites, planted):
        if len(nodes):
            n = nodes[rng.randint(len(nodes))]
            gt[i, gt[i] == na[i]] = 0
            gt[i, order[int(n["first"]): int(n["first"]) + int(n["size"])]] = na[i]
    return na, gt


# ---- the hand case ----------------------------------------------------------------------------------------------------------
# seven samples; sample 6 is in no link.  Link (4, 5) joins {3, 4} and {0, 5}: the left child is the component of b.
HAND_LINKS = [(0, 5), (3, 4), (4, 5), (1, 2), (2, 3)]
HAND_NODES = [(-1, -6, 0, 2), (-4, -5, 2, 2), (0, 1, 0, 4), (-2, -3, 4, 2), (2, 3, 0, 6)]
HAND_ORDER = [0, 5, 3, 4, 1, 2, 6]
HAND_NODES_4 = HAND_NODES[:4]                     # without the last link: two roots and a sample alone, the same order
HAND_N_ALLELES = [2, 1, 3, 1, 1]
HAND_GENOTYPE = [[1, 0, 0, 0, 0, 1, 2], [1, -1, -1, 1, 1, 1, -1], [0, 2, 2, 3, -1, 0, 0], [-1] * 7, [1, 1, 1, 1, 1, 1, 0]]
HAND_CALLS_1 = [[(2, 1, 0, 1), (2, 0, 2, 0), (4, -2, 0, 0), (2, 0, 2, 0), (6, -2, 0, 0)],
                [(2, 1, 2, 0), (2, 1, 2, 0), (4, 1, 0, 0), (0, -1, 0, 0), (4, 1, 0, 0)],      # node 2: fixed and private, but nobody outside is called
                [(2, 0, 1, 0), (1, 3, 0, 1), (3, -2, 0, 0), (2, 2, 0, 1), (5, -2, 0, 0)],
                [(0, -1, 0, 0)] * 5,
                [(2, 1, 4, 0), (2, 1, 4, 0), (4, 1, 2, 0), (2, 1, 4, 0), (6, 1, 0, 1)]]       # the root does not cover sample 6, which is called
HAND_SITES = {1: [(7, 3, 1, 0), (4, 1, 0, -1), (6, 3, 2, 1), (0, 0, 0, -1), (7, 2, 1, 4)],
              2: [(7, 3, 1, 0), (4, 1, 0, -1), (6, 3, 1, 3), (0, 0, 0, -1), (7, 2, 1, 4)]}
HAND_MARKS = {1: [(0, 0, 1, 2), (2, 1, 3, 1), (2, 3, 2, 2), (4, 4, 1, 6)], 2: [(0, 0, 1, 2), (2, 3, 2, 2), (4, 4, 1, 6)], 3: [(4, 4, 1, 6)]}
HAND_NODE_MARKS = {1: [1, 1, 0, 1, 1], 2: [1, 0, 0, 1, 1], 3: [0, 0, 0, 0, 1]}


@pytest.mark.parametrize("restate", [restate_linkage_tree, restate_linkage_tree_by_clusters])
def test_the_rule_of_the_tree_on_the_hand_case(restate):
    t = restate(links_of(HAND_LINKS), 7)
    assert as_tuples(t["nodes"]) == HAND_NODES and t["order"].tolist() == HAND_ORDER
    t = restate(links_of(HAND_LINKS[:4]), 7)
    assert as_tuples(t["nodes"]) == HAND_NODES_4 and t["order"].tolist() == HAND_ORDER
    t = restate(links_of([]), 3)
    assert len(t["nodes"]) == 0 and t["order"].tolist() == [0, 1, 2]              # no link: the identity
    assert restate(links_of([]), 1)["order"].tolist() == [0]
    for what, pairs in (("link", [(0, 5), (-1, 4)]), ("link", [(3, 3)]), ("link", [(4, 3)]), ("link", [(0, 7)]),
                        ("cycle", [(0, 5), (0, 5)]), ("cycle", HAND_LINKS + [(0, 1)]), ("cycle", [(0, 1), (1, 2), (0, 2), (3, 4)])):
        with pytest.raises(ValueError, match=what):
            restate(links_of(pairs), 7)


@pytest.mark.parametrize("restate", [restate_clade_sites, restate_clade_sites_sets, restate_clade_sites_by_groups])
def test_the_rule_of_the_clade_sites_on_the_hand_case(restate):
    nodes = np.array(HAND_NODES, NODE)
    for min_called in (1, 2, 3):
        r = restate(HAND_N_ALLELES, HAND_GENOTYPE, nodes, HAND_ORDER, min_called)
        assert as_tuples(r["marks"]) == HAND_MARKS[min_called], min_called
        assert r["node_marks"].tolist() == HAND_NODE_MARKS[min_called]
        if min_called in HAND_SITES:
            assert as_tuples(r["sites"]) == HAND_SITES[min_called]
    r = restate(HAND_N_ALLELES, HAND_GENOTYPE, nodes, HAND_ORDER, 1)
    assert [as_tuples(row) for row in r["calls"]] == HAND_CALLS_1
    # only first and size are read; any intervals over any permutation do
    loose = np.array([(77, -99, 1, 3), (0, 0, 1, 3), (5, 5, 0, 7)], NODE)
    r = restate(HAND_N_ALLELES, HAND_GENOTYPE, loose, [6, 5, 4, 3, 2, 1, 0], 1)   # {5, 4, 3} twice, then everyone
    assert as_tuples(r["calls"][0]) == [(3, -2, 0, 0), (3, -2, 0, 0), (7, -2, 0, 0)]
    assert as_tuples(r["calls"][4]) == [(3, 1, 3, 0), (3, 1, 3, 0), (7, -2, 0, 0)] and len(r["marks"]) == 0
    # what is refused on the device
    bad_gt = [HAND_GENOTYPE[0][:6] + [3]] + HAND_GENOTYPE[1:]
    for what, na, gt, nd, order in (("order", HAND_N_ALLELES, HAND_GENOTYPE, nodes, [0, 5, 3, 4, 1, 2, 2]), ("order", HAND_N_ALLELES, HAND_GENOTYPE, nodes, [0, 5, 3, 4, 1, 2, 7]),
                                    ("order", HAND_N_ALLELES, HAND_GENOTYPE, nodes, [0, 5, 3, 4, 1, 2, -1]),
                                    ("node", HAND_N_ALLELES, HAND_GENOTYPE, np.array([(0, 0, 6, 2)], NODE), HAND_ORDER),
                                    ("node", HAND_N_ALLELES, HAND_GENOTYPE, np.array([(0, 0, 3, 1)], NODE), HAND_ORDER),
                                    ("node", HAND_N_ALLELES, HAND_GENOTYPE, np.array([(0, 0, -1, 3)], NODE), HAND_ORDER),
                                    ("n_alleles", [2, 0, 3, 1, 1], HAND_GENOTYPE, nodes, HAND_ORDER), ("n_alleles", [2, 1, 8, 1, 1], HAND_GENOTYPE, nodes, HAND_ORDER),
                                    ("cell", HAND_N_ALLELES, bad_gt, nodes, HAND_ORDER),
                                    ("cell", HAND_N_ALLELES, HAND_GENOTYPE[:3] + [[-1] * 6 + [-2]] + HAND_GENOTYPE[4:], nodes, HAND_ORDER)):
        with pytest.raises(ValueError, match=what):
            restate(na, gt, nd, order, 1)


@pytest.mark.parametrize("ns,seed", [(1, 1), (2, 2), (3, 3), (7, 4), (16, 5), (33, 6), (70, 7)])
def test_two_forms_of_the_tree_agree_and_the_properties_hold(ns, seed):
    rng = np.random.RandomState(seed)
    for kind in TREE_KINDS:
        links = tree_links(kind, ns, rng)
        t = restate_linkage_tree(links, ns)
        assert same_tree(t, restate_linkage_tree_by_clusters(links, ns)), kind
        nodes, order = t["nodes"], t["order"]
        assert sorted(order.tolist()) == list(range(ns)) and order[0] == 0
        clades = [set(order[int(n["first"]): int(n["first"]) + int(n["size"])].tolist()) for n in nodes]
        for j, n in enumerate(nodes):
            assert order[n["first"]] == min(clades[j]) and n["size"] >= 2         # the clade's smallest member comes first
            kids = [clades[c] if c >= 0 else {-1 - c} for c in (int(n["left"]), int(n["right"]))]
            assert kids[0] | kids[1] == clades[j] and not kids[0] & kids[1] and min(kids[0]) < min(kids[1])
            assert all(c < j for c in (int(n["left"]), int(n["right"])))
            assert {int(links[j]["a"]), int(links[j]["b"])} <= clades[j]
        for j in range(len(nodes)):
            for k in range(j):
                assert clades[k] <= clades[j] or not clades[k] & clades[j], (kind, j, k)     # the intervals nest
        if kind in ("chain", "reverse chain", "balanced") and ns > 1:
            assert len(links) == ns - 1 and int(nodes[-1]["first"]) == 0 and int(nodes[-1]["size"]) == ns
        if kind == "forest" and ns >= 16:
            roots = set(range(len(nodes))) - {int(c) for n in nodes for c in (n["left"], n["right"]) if c >= 0}
            assert len(roots) == 3 and len(set().union(*clades)) < ns            # several roots, and samples alone


@pytest.mark.parametrize("n_sites,ns,kind,seed", [(30, 7, "forest", 1), (24, 12, "chain", 2), (24, 12, "reverse chain", 3), (20, 16, "balanced", 4), (12, 70, "forest", 5),
                                                  (8, 66, "chain", 6), (10, 5, "none", 7), (6, 1, "none", 8), (16, 2, "chain", 9)])
def test_three_forms_of_the_clade_sites_agree_and_the_properties_hold(n_sites, ns, kind, seed):
    rng = np.random.RandomState(seed)
    tree = restate_linkage_tree(tree_links(kind, ns, rng), ns)
    nodes, order = tree["nodes"], tree["order"]
    na, gt = random_matrix(rng, n_sites, ns, tree)
    found = {}
    for min_called in (1, 2, 3):
        r = restate_clade_sites(na, gt, nodes, order, min_called)
        assert same_result(r, restate_clade_sites_sets(na, gt, nodes, order, min_called)), min_called
        assert same_result(r, restate_clade_sites_by_groups(na, gt, nodes, order, min_called)), min_called
        marks = as_tuples(r["marks"])
        assert marks == sorted(marks) and len(set(m[:2] for m in marks)) == len(marks)
        assert int(r["node_marks"].sum()) == len(marks) == int(r["sites"]["n_marks"].sum())
        for i, j, x, n in marks:
            inside = np.zeros(ns, bool)
            inside[order[int(nodes[j]["first"]): int(nodes[j]["first"]) + int(nodes[j]["size"])]] = True
            mine, others = inside & (gt[i] >= 0), ~inside & (gt[i] >= 0)
            assert mine.sum() == n >= min_called and (gt[i][mine] == x).all()    # every called member carries it ...
            assert others.any() and not (gt[i][others] == x).any()               # ... and no called sample outside the clade
            assert int(nodes[j]["size"]) < ns                                     # a node that covers every sample is never marked
        found[min_called] = set(m[:3] for m in marks)
    assert found[3] <= found[2] <= found[1]                                       # raising min_called only removes marks
    if kind in ("chain", "reverse chain", "balanced") and ns > 1:
        assert int(nodes[-1]["size"]) == ns and restate_clade_sites(na, gt, nodes, order, 1)["node_marks"][-1] == 0
    # the tree's own order and another order with the same clades give the same records where the intervals say the same sets
    if len(nodes):
        reordered = restate_clade_sites(na, gt[:, ::-1], nodes, (ns - 1 - order), 1)       # the samples renamed s -> ns - 1 - s
        assert same_result(reordered, restate_clade_sites(na, gt, nodes, order, 1))


def test_marks_exist_in_the_random_cases():
    """the properties above are about marks: the cases have some"""
    for n_sites, ns, kind, seed in ((30, 7, "forest", 1), (24, 12, "chain", 2), (20, 16, "balanced", 4)):
        rng = np.random.RandomState(seed)
        tree = restate_linkage_tree(tree_links(kind, ns, rng), ns)
        na, gt = random_matrix(rng, n_sites, ns, tree)
        assert len(restate_clade_sites(na, gt, tree["nodes"], tree["order"], 1)["marks"]) >= 3, kind


# ---- helpers of the GPU tests, pinned here ------------------------------------------------------------------------------------

def other_links_of(want_tree, rng):
    """the links of a restated tree, read back from its nodes: a link joins a member of the left child and one of the right"""
    nodes, order = want_tree["nodes"], want_tree["order"]
    pairs = []
    for n in nodes:
        f, size = int(n["first"]), int(n["size"])
        left = int(nodes[n["left"]]["size"]) if n["left"] >= 0 else 1
        a, b = int(order[f + rng.randint(left)]), int(order[f + left + rng.randint(size - left)])
        pairs.append((min(a, b), max(a, b)))
    return links_of(pairs)


def test_other_links_are_the_same_tree():
    rng = np.random.RandomState(5)
    for kind in TREE_KINDS:
        t = restate_linkage_tree(tree_links(kind, 40, rng), 40)
        again = restate_linkage_tree(other_links_of(t, rng), 40)
        assert again["nodes"].tobytes() == t["nodes"].tobytes() and again["order"].tobytes() == t["order"].tobytes(), kind


def newick_text(names, links, tree, node_marks):
    """sample_tree.nwk as examples/merged_vcf.c -N writes it, from the restatements"""
    nodes, order = tree["nodes"], tree["order"]

    def clade(child, parent_key):
        if child < 0:
            return "%s:%d" % (names[-1 - child], parent_key)
        key = int(links[child]["key"])
        return "(%s,%s)%d:%d" % (clade(int(nodes[child]["left"]), key), clade(int(nodes[child]["right"]), key), node_marks[child], parent_key - key)

    children = {int(c) for n in nodes for c in (n["left"], n["right"])}
    roots = [j for j in range(len(nodes)) if j not in children] + [-1 - s for s in range(len(order)) if -1 - s not in children]
    smallest = lambda r: int(order[nodes[r]["first"]]) if r >= 0 else -1 - r
    return "".join(clade(r, int(links[r]["key"]) if r >= 0 else 0) + ";\n" for r in sorted(roots, key=smallest))


def clade_sites_text(contig_names, m, marks):
    """clade_sites.tsv as examples/merged_vcf.c -N writes it: cluster_sites.tsv's columns with the node in the first"""
    out = ""
    for mk in marks:
        site = m["sites"][mk["site"]]
        ref, alts = m["text"][mk["site"]]
        out += "%d\t%s\t%d\t%s\t%s\t%d\n" % (mk["group"], contig_names[site["contig"]], site["pos"], ref, ref if mk["genotype"] == 0 else alts[mk["genotype"] - 1], mk["n_called"])
    return out


def test_newick_text_on_the_hand_case():
    """the text the example is held to, written out once"""
    tree = {"nodes": np.array(HAND_NODES, NODE), "order": np.array(HAND_ORDER, np.int32)}
    links = links_of(HAND_LINKS)
    links["key"] = [1, 1, 3, 2, 7]
    names = ["s%d" % s for s in range(7)]
    assert newick_text(names, links, tree, [4, 0, 1, 9, 2]) == "(((s0:1,s5:1)4:2,(s3:1,s4:1)0:2)1:4,(s1:2,s2:2)9:5)2:0;\ns6:0;\n"
    four = {"nodes": tree["nodes"][:4], "order": tree["order"]}
    assert newick_text(names, links[:4], four, [4, 0, 1, 9]) == "((s0:1,s5:1)4:2,(s3:1,s4:1)0:2)1:0;\n(s1:2,s2:2)9:0;\ns6:0;\n"


# ---- declarations and argument checks --------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    own_path = os.path.join(ROOT, "include", "tatajuba_clades.h")
    own = strip(own_path)
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.CLADE_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these functions and no other
    assert re.findall(r"typedef struct \{[^}]*\}\s*(\w+)\s*;", own) == ["tjamd_tree_node"]   # ... and this one record
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_clades.h"]
    assert len(others) >= 12
    for s in NEW_ENTRIES + ["tjamd_tree_node"]:
        for path in others:
            assert not re.search(r"\b%s\b\s*[(;]" % s, strip(path)), (s, path)   # ... and no other header any of them
    for s in NEW_ENTRIES:
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in (tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS + tj.EFFECT_EXPORTS + tj.SITE_EXPORTS
                         + tj.DEPTH_EXPORTS + tj.DISTANCE_EXPORTS + tj.LINKAGE_EXPORTS + tj.GROUP_EXPORTS) and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert "tatajuba_clades.h" in open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read()
    assert '#include "tatajuba_groups.h"' in own
    assert _fields(own, "tjamd_tree_node") == list(NODE.names)
    assert NODE.itemsize == 16 and [NODE.fields[x][1] for x in NODE.names] == [0, 4, 8, 12]
    assert L.tjamd_last_linkage_tree_ms(None) == -1.0 and L.tjamd_last_clade_sites_ms(None) == -1.0
    for name in ("linkage_tree", "clade_sites", "last_linkage_tree_ms", "last_clade_sites_ms"):
        assert hasattr(tj.Counter, name)
    text = open(own_path).read()
    for what in ("Reference interface replaced: none", "N17 of DESIGN.md section 3.5", "Not built:", "leaves as nodes", "samples left out", "weights", "share of exceptions",
                 "read depths", "bootstrap support", "other linkages", "the rule of the tree", "the rule of the clade sites"):
        assert what in text, what


def test_linkage_tree_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    outs = {"nodes": GuardedHost(64 * 16), "order": GuardedHost(64 * 4)}

    def call(c=fake, links=fake, n_links=5, ns=7, null=()):
        o = {k: (None if k in null else v.c) for k, v in outs.items()}
        rc = L.tjamd_linkage_tree(c, links, n_links, ns, o["nodes"], o["order"])
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"null": ("order",)}, "null d_order"), ({"null": ("order",), "n_links": 0}, "null d_order"),
                    ({"links": None}, "null link or node buffer"), ({"null": ("nodes",)}, "null link or node buffer"), ({"null": ("nodes",), "n_links": 1}, "null link or node buffer"),
                    ({"n_links": -1}, "n_links -1 outside 0..n_samples - 1 = 6"), ({"n_links": 7}, "n_links 7 outside 0..n_samples - 1 = 6"),
                    ({"n_links": 1, "ns": 1}, "n_links 1 outside 0..n_samples - 1 = 0"), ({"n_links": 1 << 40, "ns": 4096}, "outside 0..n_samples - 1 = 4095"),
                    ({"ns": 0, "n_links": 0}, "n_samples 0 outside 1..4096"), ({"ns": -3, "n_links": 0}, "n_samples -3 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_linkage_tree") and msg in err, (kw, got, err)
    if tj.device_count() == 0:                     # good arguments, but nothing to run on: named, before the handles are read
        for kw in ({}, {"n_links": 6}, {"n_links": 0, "links": None, "null": ("nodes",)}, {"n_links": 0, "ns": 1, "links": None, "null": ("nodes",)}, {"n_links": 4095, "ns": 4096}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_linkage_tree") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    for name, buf in outs.items():
        assert buf.untouched(), name               # host memory handed in as an output stays as it was
        buf.check(name)


def test_clade_sites_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)
    outs = {"calls": GuardedHost(64 * 16), "site_out": GuardedHost(64 * 16), "node_marks": GuardedHost(64 * 4), "marks": GuardedHost(64 * 16)}
    n_marks = C.c_long(-77)

    def call(c=fake, sites=fake, n_sites=4, gt=fake, ns=7, nodes=fake, nn=5, order=fake, min_called=1, cap=64, null=(), no_count=False):
        o = {k: (None if k in null else v.c) for k, v in outs.items()}
        rc = L.tjamd_clade_sites(c, sites, n_sites, gt, ns, nodes, nn, order, min_called, o["calls"], o["site_out"], o["node_marks"], o["marks"], cap,
                                 None if no_count else C.byref(n_marks))
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"n_sites": -1}, "n_sites -1 below 0"),
                    ({"sites": None}, "null site or genotype buffer"), ({"gt": None}, "null site or genotype buffer"), ({"gt": None, "n_sites": 1}, "null site or genotype buffer"),
                    ({"order": None}, "null d_order"), ({"order": None, "n_sites": 0}, "null d_order"), ({"order": None, "nn": 0}, "null d_order"),
                    ({"nodes": None}, "null d_nodes"), ({"nodes": None, "n_sites": 0}, "null d_nodes"),
                    ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": -2}, "n_samples -2 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"),
                    ({"nn": -1}, "n_nodes -1 outside 0..4096"), ({"nn": 4097}, "n_nodes 4097 outside 0..4096"),
                    ({"min_called": 0}, "min_called 0 below 1"), ({"min_called": -5}, "min_called -5 below 1"),
                    ({"cap": -1}, "mark_capacity -1 below 0"), ({"null": ("marks",), "cap": 1}, "null d_marks with a capacity of 1"),
                    ({"n_sites": 1 << 20, "ns": 2048}, "1048576 sites x 2048 samples: 2^31 cells or more"),
                    ({"n_sites": (1 << 31) // 7 + 1, "ns": 7}, "2^31 cells or more"), ({"n_sites": 1 << 62, "ns": 4}, "2^31 cells or more"),
                    ({"n_sites": 1 << 20, "ns": 7, "nn": 2048}, "1048576 sites x 2048 nodes: 2^31 calls or more")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_clade_sites") and msg in err, (kw, got, err)
    if tj.device_count() == 0:
        for kw in ({}, {"n_sites": 0, "sites": None, "gt": None}, {"nn": 0, "nodes": None}, {"null": ("calls", "site_out", "node_marks", "marks"), "cap": 0, "no_count": True},
                   {"n_sites": 1 << 20, "ns": 7, "nn": 2048, "null": ("calls",)},              # without d_calls the calls are not counted
                   {"n_sites": (1 << 31) // 4096 - 1, "ns": 4096, "nn": 4096, "null": ("calls",), "min_called": (1 << 31) - 1}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_clade_sites") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    assert n_marks.value == -77                    # *h_n_marks is left alone by every refusal
    for name, buf in outs.items():
        assert buf.untouched(), name
        buf.check(name)


def test_clade_sites_reports_the_first_of_two_broken_rules_without_a_gpu():
    """two rules broken in one call: the message is that of the rule that is checked first, for every pair of neighbours in the
    order of the checks (a pair that cannot be broken together takes the next rule)"""
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    outs = {"calls": GuardedHost(64 * 16), "site_out": GuardedHost(64 * 16), "node_marks": GuardedHost(64 * 4), "marks": GuardedHost(64 * 16)}
    n_marks = C.c_long(-77)

    def call(c=fake, sites=fake, n_sites=4, gt=fake, ns=7, nodes=fake, nn=5, order=fake, min_called=1, cap=64, null=()):
        o = {k: (None if k in null else v.c) for k, v in outs.items()}
        rc = L.tjamd_clade_sites(c, sites, n_sites, gt, ns, nodes, nn, order, min_called, o["calls"], o["site_out"], o["node_marks"], o["marks"], cap, C.byref(n_marks))
        return rc, L.tjamd_last_error().decode()

    cells = {"n_sites": 1 << 20, "ns": 2048}
    for kw, msg in [({"c": None, "n_sites": -1}, "null counter"), ({"n_sites": -1, "order": None}, "n_sites -1 below 0"), ({"n_sites": -1, "ns": 0}, "n_sites -1 below 0"),
                    ({"sites": None, "order": None}, "null site or genotype buffer"), ({"gt": None, "ns": 0}, "null site or genotype buffer"),
                    ({"order": None, "ns": 0}, "null d_order"), ({"order": None, "nodes": None}, "null d_order"),
                    ({"ns": 0, "nn": -1}, "n_samples 0 outside 1..4096"), ({"ns": 4097, "nodes": None}, "n_samples 4097 outside 1..4096"),
                    ({"nn": 4097, "nodes": None}, "n_nodes 4097 outside 0..4096"), ({"nn": 4097, "min_called": 0}, "n_nodes 4097 outside 0..4096"),
                    ({"nodes": None, "min_called": 0}, "null d_nodes"), ({"nodes": None, "cap": -1}, "null d_nodes"),
                    ({"min_called": 0, "cap": -1}, "min_called 0 below 1"), ({"min_called": 0, "null": ("marks",), "cap": 1}, "min_called 0 below 1"),
                    ({"cap": -1, **cells}, "mark_capacity -1 below 0"), ({"cap": -1, "null": ("marks",)}, "mark_capacity -1 below 0"),
                    ({"null": ("marks",), "cap": 1, **cells}, "null d_marks with a capacity of 1"),
                    ({"n_sites": 1 << 20, "ns": 2048, "nn": 2048}, "1048576 sites x 2048 samples: 2^31 cells or more")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_clade_sites") and msg in err, (kw, got, err)
    assert n_marks.value == -77
    for name, buf in outs.items():
        assert buf.untouched(), name
        buf.check(name)
