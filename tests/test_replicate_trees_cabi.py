"""The trees of all bootstrap replicates in one call (include/tatajuba_replicate_trees.h: tjamd_replicate_trees) without a GPU:
the entry is declared in its own header, exported and prototyped and refuses bad arguments before any device call, and the
restatement that the GPU tests (tests/test_replicate_trees.py) compare against is pinned by N18's hand case stacked with a
second replicate that is a forest.

restate_replicate_trees restates nothing of its own: it is the per-replicate composition of restate_sample_linkage
(tests/test_linkage_cabi.py), restate_sample_agglomerate (tests/test_agglomerate_cabi.py) and restate_linkage_tree
(tests/test_clades_cabi.py), which is the rule of the header."""
import ctypes as C
import fnmatch
import glob
import os
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedHost
from tests.test_agglomerate_cabi import AVERAGE, COMPLETE, HAND_LINKS, HAND_ROUNDS, KEY_MAX, hand_case, restate_sample_agglomerate
from tests.test_clades_cabi import restate_linkage_tree
from tests.test_linkage_cabi import DIFFER, DIFFER_RATE, LENGTH, as_tuples, restate_sample_linkage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_replicate_trees", "tjamd_last_replicate_trees_ms"]
ERR_NO_DEVICE, ERR_ARG = 1, 3
LINK, NODE = tj.LINK_DTYPE, tj.TREE_NODE_DTYPE
SINGLE = tj.TREE_SINGLE                                    # (0: test_new_entries_are_declared_exported_and_prototyped)
LINKAGES = (SINGLE, COMPLETE, AVERAGE)
UNSET = -77


def restate_replicate_trees(dist, metric, min_both, linkage):
    """dist: [n_replicates, ns, ns] -> per replicate {"links", "n_rounds", "nodes", "order"}: the builder of the linkage on the
    replicate's matrix, then the tree of its links.  ValueError for what the entry refuses on the device, whichever replicate
    holds it; .replicate of the error is the smallest refused one."""
    assert linkage in LINKAGES and dist.ndim == 3 and dist.shape[1] == dist.shape[2]
    ns, out, refused = dist.shape[1], [], None
    for r, d in enumerate(dist):
        try:
            links, n_rounds = (restate_sample_linkage(d, metric, min_both), 0) if linkage == SINGLE else restate_sample_agglomerate(d, metric, min_both, linkage)
        except ValueError as e:
            if refused is None:
                refused = ValueError(*e.args)
                refused.replicate = r
            continue
        out.append(dict(restate_linkage_tree(links, ns), links=links, n_rounds=n_rounds))
    if refused is not None:
        raise refused
    return out


def hand_replicates():
    """N18's hand case, and behind it the same four samples with (0, 3) and (1, 2) alone left as edges: a forest of two links"""
    forest = hand_case()
    for a in (0, 3):
        for b in (1, 2):
            forest["n_both"][a, b] = forest["n_both"][b, a] = forest["n_differ"][a, b] = forest["n_differ"][b, a] = 0
    return np.stack([hand_case(), forest])


def test_the_restatement_on_the_hand_case_and_a_forest():
    dist = hand_replicates()
    for linkage in (COMPLETE, AVERAGE):
        whole, forest = restate_replicate_trees(dist, DIFFER, 1, linkage)
        assert as_tuples(whole["links"]) == HAND_LINKS[linkage] and whole["n_rounds"] == HAND_ROUNDS
        # (0, 3) is node 0, (1, 2) node 1, their union node 2 over the order 0 3 1 2
        assert [tuple(int(x) for x in n) for n in whole["nodes"]] == [(-1, -4, 0, 2), (-2, -3, 2, 2), (0, 1, 0, 4)] and whole["order"].tolist() == [0, 3, 1, 2]
        assert as_tuples(forest["links"]) == HAND_LINKS[linkage][:2] and forest["n_rounds"] == 1
        assert [tuple(int(x) for x in n) for n in forest["nodes"]] == [(-1, -4, 0, 2), (-2, -3, 2, 2)] and forest["order"].tolist() == [0, 3, 1, 2]
    whole, forest = restate_replicate_trees(dist, DIFFER, 1, SINGLE)
    assert as_tuples(whole["links"]) == [(0, 3, 0), (1, 2, 1), (1, 3, 1)] and whole["n_rounds"] == 0   # (key, a, b): the cheapest pair across is (1, 3)
    assert [tuple(int(x) for x in n) for n in whole["nodes"]] == [(-1, -4, 0, 2), (-2, -3, 2, 2), (0, 1, 0, 4)]
    assert as_tuples(forest["links"]) == [(0, 3, 0), (1, 2, 1)] and forest["n_rounds"] == 0 and forest["order"].tolist() == [0, 3, 1, 2]
    assert [len(t["links"]) for t in restate_replicate_trees(dist, DIFFER, 11, SINGLE)] == [0, 0]       # no edge anywhere: identity orders
    assert all(t["order"].tolist() == [0, 1, 2, 3] and len(t["nodes"]) == 0 for t in restate_replicate_trees(dist, DIFFER, 11, AVERAGE))
    # a bad cell in the last replicate refuses the whole call; two of them: the smaller replicate is named
    bad = np.concatenate([dist, dist[:1]])
    bad["n_both"][2, 1, 2] = 11
    with pytest.raises(ValueError, match="mirror") as e:
        restate_replicate_trees(bad, DIFFER, 1, SINGLE)
    assert e.value.replicate == 2
    bad["n_differ"][1, 0, 3] = bad["n_differ"][1, 3, 0] = -1
    with pytest.raises(ValueError, match="cell") as e:
        restate_replicate_trees(bad, DIFFER, 1, COMPLETE)
    assert e.value.replicate == 1
    big = dist.copy()
    big["length_diff"][1, 0, 3] = big["length_diff"][1, 3, 0] = KEY_MAX
    with pytest.raises(ValueError, match="key"):
        restate_replicate_trees(big, LENGTH, 1, AVERAGE)
    assert len(restate_replicate_trees(big, LENGTH, 1, COMPLETE)) == 2 and len(restate_replicate_trees(big, LENGTH, 1, SINGLE)) == 2


# ---- declarations and argument checks --------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    own_path = os.path.join(ROOT, "include", "tatajuba_replicate_trees.h")
    own = strip(own_path)
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.REPLICATE_TREE_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    assert "struct" not in own                                                              # ... and adds no struct
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_replicate_trees.h"]
    assert len(others) >= 14
    for s in NEW_ENTRIES:
        for path in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(path)), (s, path)   # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in (tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS + tj.EFFECT_EXPORTS + tj.SITE_EXPORTS + tj.DEPTH_EXPORTS
                         + tj.DISTANCE_EXPORTS + tj.LINKAGE_EXPORTS + tj.AGGLOMERATE_EXPORTS + tj.GROUP_EXPORTS + tj.CLADE_EXPORTS + tj.BOOTSTRAP_EXPORTS) and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert '#include "tatajuba_bootstrap.h"' in own
    assert re.search(r"enum\s*\{\s*TJAMD_TREE_SINGLE = 0\s*\}", own)
    assert (tj.TREE_SINGLE, tj.AGGL_COMPLETE, tj.AGGL_AVERAGE) == (0, 1, 2) == LINKAGES
    assert L.tjamd_last_replicate_trees_ms(None) == -1.0
    for name in ("replicate_trees", "last_replicate_trees_ms"):
        assert hasattr(tj.Counter, name)
    text = open(own_path).read()
    for what in ("byte for byte", "tjamd_sample_linkage under TJAMD_TREE_SINGLE", "tjamd_sample_agglomerate under the other two", "under TJAMD_TREE_SINGLE it is 0",
                 "Entries past a replicate's n_nodes are not written", "(key, a, b)", "(key, round, a, b)", "refuses the whole call", "2^40",
                 "names the smallest refused replicate", "Nothing of the caller's is written", "identity orders", "Two runs give the same bytes", "1 GiB",
                 "once per batch of rounds", "rounds of the slowest replicate",                    # the rule, the refusals, the waits
                 "parallel walk", "different n_samples", "base tree", "Newick", "Ward", "neighbour joining"):   # named as not built
        assert what in text, what
    # the header before this one stays as it was written, its "Not built" list included
    assert "Not built: a batched tree builder (the caller runs the tree entries per replicate)" in open(os.path.join(ROOT, "include", "tatajuba_bootstrap.h")).read()


def _caller():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call fails its argument checks first
    nodes_h, rounds_h = GuardedHost(8 * 4), GuardedHost(8 * 4)

    def call(c=fake, dist=fake, ns=5, n_rep=3, metric=DIFFER, min_both=1, linkage=COMPLETE, links=fake, nodes=fake, order=fake, null_counts=False, null_rounds=False):
        rc = L.tjamd_replicate_trees(c, dist, ns, n_rep, metric, min_both, linkage, links, nodes, order,
                                     None if null_counts else C.cast(nodes_h.c, C.POINTER(C.c_int)), None if null_rounds else C.cast(rounds_h.c, C.POINTER(C.c_int)))
        return rc, L.tjamd_last_error().decode()

    return call, nodes_h, rounds_h


def test_replicate_trees_checks_its_arguments_without_a_gpu():
    call, nodes_h, rounds_h = _caller()
    for kw, msg in [({"c": None}, "null counter"), ({"dist": None}, "null d_dist"), ({"order": None}, "null d_rep_order"), ({"null_counts": True}, "null h_rep_n_nodes"),
                    ({"nodes": None}, "null d_rep_nodes"), ({"nodes": None, "ns": 2}, "null d_rep_nodes"),
                    ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": -3}, "n_samples -3 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"),
                    ({"ns": 0, "nodes": None}, "n_samples 0 outside 1..4096"),
                    ({"n_rep": 0}, "n_replicates 0 outside 1..4096"), ({"n_rep": -1}, "n_replicates -1 outside 1..4096"), ({"n_rep": 4097}, "n_replicates 4097 outside 1..4096"),
                    ({"metric": -1}, "metric -1 outside 0..2"), ({"metric": 3}, "metric 3 outside 0..2"),
                    ({"min_both": 0}, "min_both 0 below 1"), ({"min_both": -7}, "min_both -7 below 1"),
                    ({"linkage": -1}, "linkage -1 outside 0..2"), ({"linkage": 3}, "linkage 3 outside 0..2"), ({"linkage": 3, "null_rounds": True, "links": None}, "linkage 3 outside 0..2")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_replicate_trees") and msg in err, (kw, got, err)
    if tj.device_count() == 0:                     # good arguments, but nothing to run on: named, before the handles are read
        for kw in ({}, {"linkage": SINGLE}, {"linkage": AVERAGE, "links": None, "null_rounds": True}, {"ns": 1}, {"ns": 1, "nodes": None, "links": None},
                   {"ns": 4096, "n_rep": 4096, "metric": DIFFER_RATE, "min_both": (1 << 31) - 1, "linkage": AVERAGE}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_replicate_trees") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    assert nodes_h.untouched() and rounds_h.untouched()   # host memory handed in as the outputs stays as it was
    nodes_h.check("h_rep_n_nodes")
    rounds_h.check("h_rep_n_rounds")


def test_replicate_trees_reports_the_first_of_two_broken_rules_without_a_gpu():
    """two rules broken in one call: the message is that of the rule that is checked first, for every pair of neighbours in the
    order of the checks"""
    call, nodes_h, rounds_h = _caller()
    for kw, msg in [({"c": None, "dist": None}, "null counter"), ({"dist": None, "order": None}, "null d_dist"), ({"order": None, "null_counts": True}, "null d_rep_order"),
                    ({"null_counts": True, "nodes": None}, "null h_rep_n_nodes"), ({"nodes": None, "ns": 4097}, "null d_rep_nodes"),
                    ({"ns": 0, "n_rep": 0}, "n_samples 0 outside 1..4096"), ({"n_rep": 4097, "metric": 3}, "n_replicates 4097 outside 1..4096"),
                    ({"metric": -1, "min_both": 0}, "metric -1 outside 0..2"), ({"min_both": 0, "linkage": 3}, "min_both 0 below 1")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_replicate_trees") and msg in err, (kw, got, err)
    assert nodes_h.untouched() and rounds_h.untouched()
    nodes_h.check("h_rep_n_nodes")
    rounds_h.check("h_rep_n_rounds")
