"""The linkage step (include/tatajuba_linkage.h: tjamd_sample_linkage, tjamd_linkage_clusters) without a GPU: the entries are
declared in their own header, exported and prototyped and refuse bad arguments before any device call, the record matches the
header, and the restatements that the GPU tests (tests/test_linkage.py) compare against are pinned by a hand case whose expected
links and clusters are written out here, by a second form of the tree (Prim) and by properties on random matrices.

restate_sample_linkage is written from the rule in the header: Kruskal over the edges sorted by (key, a, b) with a union-find.
The device runs Boruvka rounds over a key matrix and sorts the chosen edges at the end."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_sample_linkage", "tjamd_linkage_clusters", "tjamd_last_sample_linkage_ms", "tjamd_last_linkage_clusters_ms"]
ERR_NO_DEVICE, ERR_ARG = 1, 3
DIST, LINK = tj.SAMPLE_DISTANCE_DTYPE, tj.LINK_DTYPE
DIFFER, LENGTH, DIFFER_RATE = 0, 1, 2
METRICS = (DIFFER, LENGTH, DIFFER_RATE)
NONE = np.uint64(2 ** 64 - 1)


def link_keys(dist, metric, min_both):
    """the checks of the rule and the key of every cell -> uint64 [ns, ns], NONE where (a, b) is no edge and on the diagonal.
    ValueError for what the entry refuses on the device."""
    ns = dist.shape[0]
    assert dist.shape == (ns, ns) and metric in METRICS and min_both >= 1
    nb, nd, ld = dist["n_both"].astype(np.int64), dist["n_differ"].astype(np.int64), dist["length_diff"].astype(np.int64)
    if (nb < 0).any() or (nd < 0).any() or (nd > nb).any() or (ld < 0).any():
        raise ValueError("cell")
    if (nb != nb.T).any() or (nd != nd.T).any() or (ld != ld.T).any():
        raise ValueError("mirror")
    key = nd if metric == DIFFER else ld if metric == LENGTH else (nd << 32) // np.maximum(nb, 1)   # (nd <= nb < 2^31: below 2^63)
    edge = (nb >= min_both) & ~np.eye(ns, dtype=bool)
    return np.where(edge, key.astype(np.uint64), NONE)


def _links(triples):
    out = np.zeros(len(triples), LINK)
    for i, (key, a, b) in enumerate(triples):
        out[i] = (a, b, key)
    return out


def restate_sample_linkage(dist, metric, min_both):
    """Kruskal: the edges ascending in (key, a, b), each taken if its ends are in two components -> LINK_DTYPE [n_links]"""
    K = link_keys(dist, metric, min_both)
    ns = K.shape[0]
    a, b = np.triu_indices(ns, 1)
    k = K[a, b]
    keep = k != NONE
    a, b, k = a[keep], b[keep], k[keep]
    order = np.lexsort((b, a, k))
    parent = list(range(ns))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    taken = []
    for i in order.tolist():
        ra, rb = find(int(a[i])), find(int(b[i]))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            taken.append((int(k[i]), int(a[i]), int(b[i])))
            if len(taken) == ns - 1:
                break
    return _links(taken)


def restate_sample_linkage_prim(dist, metric, min_both):
    """Prim under the same total order, a tree per component of the edge graph, the edges sorted at the end: the forest is
    unique, so this is the same list.  n_samples steps of vector operations: what the largest case can afford."""
    K = link_keys(dist, metric, min_both)
    ns = K.shape[0]
    idx = np.arange(ns, dtype=np.int64)
    out_of_tree = np.ones(ns, bool)
    best_key = np.full(ns, NONE)                           # per vertex outside the tree: its smallest edge into it
    best_pair = np.full(ns, 1 << 62, np.int64)            # lo * 4096 + hi of that edge
    taken = []
    while out_of_tree.any():
        cand = np.flatnonzero(out_of_tree & (best_key != NONE))
        if len(cand) == 0:
            u = int(np.flatnonzero(out_of_tree)[0])        # a new tree
        else:
            kmin = best_key[cand].min()
            cand = cand[best_key[cand] == kmin]
            u = int(cand[np.argmin(best_pair[cand])])
            taken.append((int(kmin), int(best_pair[u] >> 12), int(best_pair[u] & 4095)))
        out_of_tree[u] = False
        pair = np.minimum(idx, u) * 4096 + np.maximum(idx, u)
        better = out_of_tree & (K[u] != NONE) & ((K[u] < best_key) | ((K[u] == best_key) & (pair < best_pair)))
        best_key[better], best_pair[better] = K[u][better], pair[better]
    return _links(sorted(taken))


def _dense(find, n_samples):
    ids, out = {}, np.zeros(n_samples, np.int32)
    for s in range(n_samples):                            # components numbered in the order of their smallest member
        out[s] = ids.setdefault(find(s), len(ids))
    return out


def restate_linkage_clusters(links, n_samples, threshold):
    """-> int32 [n_samples]: the dense id of every sample's component in the graph of the links with key <= threshold.
    ValueError for what the entry refuses on the device."""
    links = np.asarray(links, LINK)
    if len(links) and ((links["a"] < 0) | (links["a"] >= links["b"]) | (links["b"] >= n_samples) | (links["key"] < 0)).any():
        raise ValueError("link")
    parent = list(range(n_samples))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for l in links[links["key"] <= threshold] if len(links) else []:
        ra, rb = find(int(l["a"])), find(int(l["b"]))
        parent[max(ra, rb)] = min(ra, rb)
    return _dense(find, n_samples)


def components_of_all_pairs(dist, metric, min_both, threshold):
    """the same ids from the full graph: every pair with n_both >= min_both and key <= threshold"""
    K = link_keys(dist, metric, min_both)
    ns = K.shape[0]
    a, b = np.nonzero(np.triu((K != NONE) & (K <= np.uint64(max(threshold, 0))), 1) & (threshold >= 0))
    return restate_linkage_clusters(_links([(0, int(x), int(y)) for x, y in zip(a, b)]), ns, 0)


def planted_root_pairs(ns):
    """(a, b) pairs for ns >= 1023 whose roots (the smallest members of the components) sit so that four consecutive samples
    4t .. 4t + 3 hold no root, one root and four roots, and the 256 samples from 256 on no root at all: 0 takes 511, the 256
    samples 255 .. 510 are one chain, some t have their four samples joined, everyone else is alone"""
    assert ns >= 1023
    pairs = [(0, 511)] + [(s, s + 1) for s in range(255, 510)]
    for t in sorted({1, 5, 130, 200, 254, ns // 4 - 1}):                    # (the last: the last thread that has four samples)
        pairs += [(4 * t + j, 4 * t + j + 1) for j in range(3)]
    return pairs


def symmetric(ns, n_both, n_differ, length_diff):
    """a DIST matrix from three [ns, ns] arrays whose upper triangles and diagonals are used"""
    d = np.zeros((ns, ns), DIST)
    for f, m in (("n_both", n_both), ("n_differ", n_differ), ("length_diff", length_diff)):
        m = np.asarray(m, np.int64)
        d[f] = np.triu(m) + np.triu(m, 1).T
    return d


def fabricate_small(ns, rng):
    """keys in 0..3 under every metric's own field, so that ties abound: n_differ and length_diff in 0..3, n_both in n_differ ..
    n_differ + 2 (0, 1 or 2 and so below a min_both of 2 or 3 in many pairs; few distinct rates)"""
    nd = rng.randint(0, 4, (ns, ns))
    d = symmetric(ns, nd + rng.randint(0, 3, (ns, ns)), nd, rng.randint(0, 4, (ns, ns)))
    d["n_differ"][np.arange(ns), np.arange(ns)] = 0
    d["length_diff"][np.arange(ns), np.arange(ns)] = 0
    return d


def fabricate_wide(ns, rng):
    """keys over the full range: n_both up to 2^31 - 1, n_differ up to n_both, length_diff up to 2^63 - 1"""
    nb = rng.randint(0, 1 << 31, (ns, ns), dtype=np.int64)
    nb[rng.random_sample((ns, ns)) < 0.1] = 0
    nd = (nb * rng.random_sample((ns, ns))).astype(np.int64)
    ld = rng.randint(0, (1 << 63) - 1, (ns, ns), dtype=np.int64)
    return symmetric(ns, nb, np.minimum(nd, nb), ld)


# ---- the hand case ---------------------------------------------------------------------------------------------------------
# five samples; (n_both, n_differ, length_diff) of the pairs, min_both 2:
#   (0,1) (10, 2,  7)   rate 0.2        (0,2) ( 4, 1,  9)   rate 0.25       (0,3) (10, 5, 20)   rate 0.5
#   (1,2) (10, 2,  3)   rate 0.2        (1,3) ( 8, 3, 30)   rate 0.375      (2,3) (10, 3,  5)   rate 0.3
#   (x,4) ( 1, 0,  0)   below min_both: sample 4 has no edge
# DIFFER: (0,2) at 1; then (0,1) and (1,2) tie at 2 and the indices put (0,1) first, (1,2) closes a cycle; (1,3) and (2,3) tie
#   at 3, (1,3) first.  DIFFER_RATE: (0,1) and (1,2) tie at floor (0.2 * 2^32) and come before (0,2), which DIFFER put first;
#   then (2,3) at floor (0.3 * 2^32).  LENGTH: (1,2) 3, (2,3) 5, (0,1) 7.
HAND_MIN_BOTH = 2
HAND_LINKS = {DIFFER: [(0, 2, 1), (0, 1, 2), (1, 3, 3)],
              DIFFER_RATE: [(0, 1, 858993459), (1, 2, 858993459), (2, 3, 1288490188)],
              LENGTH: [(1, 2, 3), (2, 3, 5), (0, 1, 7)]}
# the DIFFER tree cut at thresholds -1 .. 3: (clusters, n_clusters)
HAND_CLUSTERS = {-1: ([0, 1, 2, 3, 4], 5), 0: ([0, 1, 2, 3, 4], 5), 1: ([0, 1, 0, 2, 3], 4), 2: ([0, 0, 0, 1, 2], 3), 3: ([0, 0, 0, 0, 1], 2)}
# with min_both 1 sample 4 is at n_differ 0 from everyone: four links at key 0, the indices alone decide
HAND_LINKS_MIN_BOTH_1 = [(0, 4, 0), (1, 4, 0), (2, 4, 0), (3, 4, 0)]


def hand_case():
    nb = [[10, 10, 4, 10, 1], [0, 10, 10, 8, 1], [0, 0, 10, 10, 1], [0, 0, 0, 10, 1], [0, 0, 0, 0, 1]]
    nd = [[0, 2, 1, 5, 0], [0, 0, 2, 3, 0], [0, 0, 0, 3, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    ld = [[0, 7, 9, 20, 0], [0, 0, 3, 30, 0], [0, 0, 0, 5, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    return symmetric(5, nb, nd, ld)


def as_tuples(links):
    return [(int(l["a"]), int(l["b"]), int(l["key"])) for l in links]


def test_the_rule_on_the_hand_case():
    d = hand_case()
    for metric in METRICS:
        for restate in (restate_sample_linkage, restate_sample_linkage_prim):
            assert as_tuples(restate(d, metric, HAND_MIN_BOTH)) == HAND_LINKS[metric], (metric, restate.__name__)
    assert as_tuples(restate_sample_linkage(d, DIFFER, 1)) == HAND_LINKS_MIN_BOTH_1
    assert as_tuples(restate_sample_linkage_prim(d, DIFFER, 1)) == HAND_LINKS_MIN_BOTH_1
    assert len(restate_sample_linkage(d, DIFFER, 11)) == 0                       # no pair has that much in common
    links = restate_sample_linkage(d, DIFFER, HAND_MIN_BOTH)
    for t, (want, n) in HAND_CLUSTERS.items():
        got = restate_linkage_clusters(links, 5, t)
        assert got.tolist() == want and got.max() + 1 == n, t
        assert components_of_all_pairs(d, DIFFER, HAND_MIN_BOTH, t).tolist() == want, t
    # what is refused
    for field, at, value, what in (("n_both", (1, 1), -1, "cell"), ("n_differ", (0, 3), -1, "cell"), ("length_diff", (2, 2), -5, "cell"),
                                   ("n_differ", (4, 4), 2, "cell"), ("n_both", (0, 1), 11, "mirror"), ("n_differ", (3, 1), 2, "mirror"),
                                   ("length_diff", (4, 0), 1, "mirror")):
        bad = d.copy()
        bad[field][at] = value
        with pytest.raises(ValueError, match=what):
            restate_sample_linkage(bad, DIFFER, HAND_MIN_BOTH)
    for a, b, key in ((-1, 2, 0), (2, 2, 0), (3, 2, 0), (0, 5, 0), (0, 1, -1)):
        with pytest.raises(ValueError, match="link"):
            restate_linkage_clusters(_links([(0, 0, 1), (key, a, b)]), 5, 3)


@pytest.mark.parametrize("ns,seed", [(2, 1), (7, 2), (20, 3), (33, 4), (70, 5)])
def test_properties_on_random_matrices(ns, seed):
    rng = np.random.RandomState(seed)
    for d, min_both in ((fabricate_small(ns, rng), 2), (fabricate_small(ns, rng), 3), (fabricate_wide(ns, rng), 1)):
        for metric in METRICS:
            links = restate_sample_linkage(d, metric, min_both)
            assert links.tobytes() == restate_sample_linkage_prim(d, metric, min_both).tobytes()   # the second form
            t = as_tuples(links)
            assert [(k, a, b) for a, b, k in t] == sorted((k, a, b) for a, b, k in t) and len(set(t)) == len(t)   # ascending
            assert all(a < b for a, b, k in t)
            K = link_keys(d, metric, min_both)
            assert all(int(K[a, b]) == k for a, b, k in t)
            whole = components_of_all_pairs(d, metric, min_both, (1 << 63) - 1)
            assert len(links) == ns - (whole.max() + 1)                           # n_links = n - components
            keys = sorted(set(int(x) for x in K[K != NONE]))
            if len(keys) > 8:
                keys = keys[:3] + keys[len(keys) // 2: len(keys) // 2 + 2] + keys[-3:]
            for k in keys:
                for thr in (k - 1, k):                                            # either side of every key
                    assert restate_linkage_clusters(links, ns, thr).tolist() == components_of_all_pairs(d, metric, min_both, thr).tolist(), (metric, thr)


def any_list():
    """(key, a, b) of nine links over eight samples: (0,3) twice, the cycle 0-3-6-0 at key 1, (1,2) at two keys, sample 7 in none"""
    return _links([(5, 4, 6), (1, 0, 3), (1, 3, 6), (1, 0, 6), (1, 0, 3), (9, 1, 2), (0, 2, 5), (2, 1, 5), (2, 1, 2)])


# at 0: {2,5}; at 1: {0,3,6} as well; at 2: {1,2,5}; from 5 on: {0,3,4,6}
ANY_LIST_CLUSTERS = {-1: [0, 1, 2, 3, 4, 5, 6, 7], 0: [0, 1, 2, 3, 4, 2, 5, 6], 1: [0, 1, 2, 0, 3, 2, 0, 4], 2: [0, 1, 1, 0, 2, 1, 0, 3],
                     4: [0, 1, 1, 0, 2, 1, 0, 3], 5: [0, 1, 1, 0, 0, 1, 0, 2], 9: [0, 1, 1, 0, 0, 1, 0, 2]}


def test_cuts_of_any_list():
    """unsorted, cyclic, duplicated, longer than n - 1: components are defined for all of these, labels by the smallest member"""
    links = any_list()
    assert len(links) > 8 - 1
    for thr, want in ANY_LIST_CLUSTERS.items():
        assert restate_linkage_clusters(links, 8, thr).tolist() == want, thr
    assert restate_linkage_clusters(links[:0], 3, 7).tolist() == [0, 1, 2]


# ---- declarations and argument checks --------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    own = strip(os.path.join(ROOT, "include", "tatajuba_linkage.h"))
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.LINKAGE_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_linkage.h"]
    assert len(others) >= 10
    for s in NEW_ENTRIES:
        for path in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(path)), (s, path)   # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in (tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS + tj.EFFECT_EXPORTS + tj.SITE_EXPORTS
                         + tj.DEPTH_EXPORTS + tj.DISTANCE_EXPORTS) and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert "tatajuba_linkage.h" in open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read()
    assert '#include "tatajuba_distances.h"' in own
    assert _fields(own, "tjamd_link") == list(LINK.names)
    assert LINK.itemsize == 16 and [LINK.fields[x][1] for x in LINK.names] == [0, 4, 8]
    assert re.search(r"enum\s*\{\s*TJAMD_LINK_DIFFER = 0, TJAMD_LINK_LENGTH = 1, TJAMD_LINK_DIFFER_RATE = 2\s*\}", own)
    assert (tj.LINK_DIFFER, tj.LINK_LENGTH, tj.LINK_DIFFER_RATE) == METRICS
    assert L.tjamd_last_sample_linkage_ms(None) == -1.0 and L.tjamd_last_linkage_clusters_ms(None) == -1.0
    for name in ("sample_linkage", "linkage_clusters", "last_sample_linkage_ms", "last_linkage_clusters_ms"):
        assert hasattr(tj.Counter, name)
    for what in ("complete", "average", "Ward", "neighbour joining", "Newick", "length_diff per site", "cophenetic", "bootstrap"):   # named as not built
        assert what in open(os.path.join(ROOT, "include", "tatajuba_linkage.h")).read(), what


def test_sample_linkage_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    out = GuardedHost(64 * LINK.itemsize)

    def call(c=fake, dist=fake, ns=5, metric=DIFFER, min_both=1, null_out=False):
        rc = L.tjamd_sample_linkage(c, dist, ns, metric, min_both, None if null_out else out.c)
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"dist": None}, "null d_dist"), ({"null_out": True}, "null d_links"),
                    ({"null_out": True, "ns": 2}, "null d_links"),
                    ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": -3}, "n_samples -3 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"),
                    ({"ns": 0, "null_out": True}, "n_samples 0 outside 1..4096"),
                    ({"metric": -1}, "metric -1 outside 0..2"), ({"metric": 3}, "metric 3 outside 0..2"),
                    ({"min_both": 0}, "min_both 0 below 1"), ({"min_both": -7}, "min_both -7 below 1")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_sample_linkage") and msg in err, (kw, got, err)
    if tj.device_count() == 0:                     # good arguments, but nothing to run on: named, before the handles are read
        for kw in ({}, {"ns": 1}, {"ns": 1, "null_out": True}, {"ns": 4096, "metric": DIFFER_RATE, "min_both": (1 << 31) - 1}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_sample_linkage") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    assert out.untouched()                         # host memory handed in as the output stays as it was
    out.check("d_links")


def test_linkage_clusters_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)
    out = GuardedHost(64 * 4)

    def call(c=fake, links=fake, n_links=4, ns=5, threshold=3, null_out=False):
        rc = L.tjamd_linkage_clusters(c, links, n_links, ns, threshold, None if null_out else out.c)
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"null_out": True}, "null d_cluster"),
                    ({"n_links": -1}, "n_links -1 outside 0..2^24"), ({"n_links": (1 << 24) + 1}, "n_links 16777217 outside 0..2^24"),
                    ({"links": None}, "null d_links"), ({"links": None, "n_links": 1}, "null d_links"),
                    ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": -1}, "n_samples -1 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_linkage_clusters") and msg in err, (kw, got, err)
    if tj.device_count() == 0:
        for kw in ({}, {"links": None, "n_links": 0}, {"n_links": 1 << 24, "ns": 4096}, {"threshold": -1}, {"threshold": (1 << 63) - 1}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_linkage_clusters") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    assert out.untouched()
    out.check("d_cluster")


def test_sample_linkage_reports_the_first_of_two_broken_rules_without_a_gpu():
    """two rules broken in one call: the message is that of the rule that is checked first, for every pair of neighbours in the
    order of the checks"""
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    out = GuardedHost(64 * LINK.itemsize)

    def call(c=fake, dist=fake, ns=5, metric=DIFFER, min_both=1, null_out=False):
        rc = L.tjamd_sample_linkage(c, dist, ns, metric, min_both, None if null_out else out.c)
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None, "dist": None}, "null counter"), ({"dist": None, "null_out": True}, "null d_dist"), ({"dist": None, "ns": 0}, "null d_dist"),
                    ({"null_out": True, "ns": 4097}, "null d_links"), ({"null_out": True, "metric": 3}, "null d_links"),
                    ({"ns": 0, "metric": 3}, "n_samples 0 outside 1..4096"), ({"ns": 4097, "min_both": 0}, "n_samples 4097 outside 1..4096"),
                    ({"metric": -1, "min_both": 0}, "metric -1 outside 0..2"), ({"metric": 3, "min_both": -7}, "metric 3 outside 0..2")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_sample_linkage") and msg in err, (kw, got, err)
    assert out.untouched()
    out.check("d_links")
