"""The complete and average linkage trees (include/tatajuba_agglomerate.h: tjamd_sample_agglomerate) without a GPU: the entry is
declared in its own header, exported and prototyped and refuses bad arguments before any device call, and the restatement that
the GPU tests (tests/test_agglomerate.py) compare against is pinned by a hand case whose links are written out here, by a
second, naive form that recomputes every distance from the clusters' member lists, and by properties on random matrices.

restate_sample_agglomerate is written from the rule in the header, in vectorised numpy over the uint64 key matrix: the row
minimum, the mutual pairs, the update in two phases (rows, then columns), and a merged-away cluster loses its edges.  The
device keeps sizes instead, with 0 for a retired cluster, and never writes a retired row again."""
import ctypes as C
import fnmatch
import glob
import os
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedHost
from tests.test_linkage_cabi import DIFFER, DIFFER_RATE, LENGTH, METRICS, NONE, _links, as_tuples, fabricate_small, fabricate_wide, link_keys, symmetric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_sample_agglomerate", "tjamd_last_sample_agglomerate_ms"]
ERR_NO_DEVICE, ERR_ARG = 1, 3
LINK = tj.LINK_DTYPE
COMPLETE, AVERAGE = tj.AGGL_COMPLETE, tj.AGGL_AVERAGE     # (1 and 2: test_new_entries_are_declared_exported_and_prototyped)
LINKAGES = (COMPLETE, AVERAGE)
KEY_MAX = 1 << 40                                          # AVERAGE: a key of a pair of samples stays below this


def _f(x, y, linkage):
    """max or + with NONE absorbing, on uint64 arrays"""
    return np.where((x == NONE) | (y == NONE), NONE, np.maximum(x, y) if linkage == COMPLETE else x + y)


def restate_sample_agglomerate(dist, metric, min_both, linkage):
    """-> (LINK_DTYPE [n_links] ascending in (key, round, a, b), the rounds that merged).  ValueError for what the entry
    refuses on the device."""
    assert linkage in LINKAGES
    K = link_keys(dist, metric, min_both).copy()           # the maximum or the sum over the pairs across two clusters
    ns = K.shape[0]
    if linkage == AVERAGE and ((K != NONE) & (K >= np.uint64(KEY_MAX))).any():
        raise ValueError("key")
    size = np.ones(ns, np.uint64)
    idx = np.arange(ns)
    merged, n_rounds = [], 0
    while True:
        if linkage == AVERAGE:                             # the division is taken here and never stored
            D = np.where(K != NONE, K // np.maximum(size[:, None] * size[None, :], np.uint64(1)), NONE)
        else:
            D = K
        nn = D.argmin(axis=1)                              # the first of equal distances: the smallest id
        has = D[idx, nn] != NONE
        X = np.flatnonzero(has & (nn[nn] == idx) & (idx < nn))
        if len(X) == 0:
            break
        Y = nn[X]
        merged += [(int(k), n_rounds, int(a), int(b)) for k, a, b in zip(D[X, Y], X, Y)]
        K[X, :] = _f(K[X, :], K[Y, :], linkage)            # phase A: rows, over all columns
        K[:, X] = _f(K[:, X], K[:, Y], linkage)            # phase B: columns, over all rows, reading what phase A wrote
        K[Y, :] = NONE                                     # retired
        K[:, Y] = NONE
        size[X] += size[Y]
        size[Y] = 0
        n_rounds += 1
    return _links([(k, a, b) for k, r, a, b in sorted(merged)]), n_rounds


def restate_sample_agglomerate_naive(dist, metric, min_both, linkage):
    """the same rounds with every D recomputed from the clusters' member lists and the keys of the pairs of samples"""
    K0 = link_keys(dist, metric, min_both)
    ns = K0.shape[0]
    members = {s: [s] for s in range(ns)}
    merged, n_rounds = [], 0

    def D(x, y):
        P = [int(K0[a, b]) for a in members[x] for b in members[y]]
        if int(NONE) in P:
            return None
        return max(P) if linkage == COMPLETE else sum(P) // len(P)

    while True:
        nn = {}
        for x in members:
            cand = [(D(x, y), y) for y in members if y != x]
            cand = [c for c in cand if c[0] is not None]
            if cand:
                nn[x] = min(cand)
        pairs = [(d, x, y) for x, (d, y) in nn.items() if x < y and y in nn and nn[y][1] == x]
        if not pairs:
            break
        for d, x, y in pairs:
            merged.append((d, n_rounds, x, y))
        for d, x, y in pairs:
            members[x] = members[x] + members.pop(y)
        n_rounds += 1
    return _links([(k, a, b) for k, r, a, b in sorted(merged)]), n_rounds, members


def greedy_complete(dist, metric, min_both):
    """the textbook loop: the smallest pair of clusters merges, one at a time -> the links in the order of the merges"""
    K = link_keys(dist, metric, min_both).copy()
    out = []
    while True:
        at = int(K.argmin())
        x, y = divmod(at, K.shape[0])
        if K[x, y] == NONE:
            break
        x, y = min(x, y), max(x, y)
        out.append((int(K[x, y]), x, y))
        K[x, :] = _f(K[x, :], K[y, :], COMPLETE)
        K[:, x] = K[x, :]
        K[y, :] = NONE
        K[:, y] = NONE
    return _links(out)


def replay(links, ns):
    """the list replayed in order: every link's a and b must be the smallest members of two distinct components -> the
    components as {smallest member: members}, or None where a link is neither"""
    comp = {s: [s] for s in range(ns)}
    for a, b, key in as_tuples(links):
        if a not in comp or b not in comp or a >= b:
            return None
        comp[a] = comp[a] + comp.pop(b)
    return comp


def cap_for_average(d):
    """the same matrix with length_diff below 2^40: every metric's key is then below the bound of AVERAGE"""
    d = d.copy()
    d["length_diff"] %= KEY_MAX
    return d


# ---- the hand case ---------------------------------------------------------------------------------------------------------
# four samples, metric DIFFER, n_both 10 everywhere, min_both 1; n_differ: (0,1) 3, (0,2) 2, (0,3) 0, (1,2) 1, (1,3) 1, (2,3) 1.
# Round 0: nn (0) = 3, nn (3) = 0, nn (1) = 2, nn (2) = 1: (0,3) merges at 0 and (1,2) at 1.  Round 1: {0,3} and {1,2}, the pairs
# across them 3, 2, 1, 1: AVERAGE floor (7 / 4) = 1, COMPLETE 3.  Under AVERAGE (0,1,1) of round 1 stands behind (1,2,1) of
# round 0: by (key, a, b) it would stand before it.
HAND_LINKS = {AVERAGE: [(0, 3, 0), (1, 2, 1), (0, 1, 1)], COMPLETE: [(0, 3, 0), (1, 2, 1), (0, 1, 3)]}
HAND_ROUNDS = 2


def hand_case():
    nd = [[0, 3, 2, 0], [0, 0, 1, 1], [0, 0, 0, 1], [0, 0, 0, 0]]
    return symmetric(4, np.full((4, 4), 10), nd, np.zeros((4, 4)))


def test_the_rule_on_the_hand_case():
    d = hand_case()
    for linkage in LINKAGES:
        links, n_rounds = restate_sample_agglomerate(d, DIFFER, 1, linkage)
        assert as_tuples(links) == HAND_LINKS[linkage] and n_rounds == HAND_ROUNDS, linkage
        links, n_rounds, members = restate_sample_agglomerate_naive(d, DIFFER, 1, linkage)
        assert as_tuples(links) == HAND_LINKS[linkage] and n_rounds == HAND_ROUNDS and members == {0: [0, 3, 1, 2]}, linkage
        assert replay(links, 4) is not None
    assert len(restate_sample_agglomerate(d, DIFFER, 11, COMPLETE)[0]) == 0 and restate_sample_agglomerate(d, DIFFER, 11, AVERAGE)[1] == 0
    # the order is not (key, a, b): sorted that way, the AVERAGE list no longer replays, so the replay property can fail
    by_key = _links(sorted((k, a, b) for a, b, k in HAND_LINKS[AVERAGE]))
    assert as_tuples(by_key) == [(0, 3, 0), (0, 1, 1), (1, 2, 1)] and replay(by_key, 4) is None
    assert replay(_links([(k, a, b) for a, b, k in HAND_LINKS[AVERAGE]]), 4) == {0: [0, 3, 1, 2]}
    # what is refused: N15's cells, and a key of 2^40 under AVERAGE alone
    bad = d.copy()
    bad["n_both"][1, 2] = 11
    with pytest.raises(ValueError, match="mirror"):
        restate_sample_agglomerate(bad, DIFFER, 1, COMPLETE)
    big = d.copy()
    big["length_diff"][0, 1] = big["length_diff"][1, 0] = KEY_MAX
    with pytest.raises(ValueError, match="key"):
        restate_sample_agglomerate(big, LENGTH, 1, AVERAGE)
    assert len(restate_sample_agglomerate(big, LENGTH, 1, COMPLETE)[0]) == 3
    big["length_diff"][0, 1] = big["length_diff"][1, 0] = KEY_MAX - 1
    assert int(restate_sample_agglomerate(big, LENGTH, 1, AVERAGE)[0]["key"].max()) > 0


@pytest.mark.parametrize("ns,seed", [(2, 1), (3, 2), (5, 3), (9, 4), (17, 5), (26, 6), (40, 7)])
def test_two_forms_and_properties_on_random_matrices(ns, seed):
    rng = np.random.RandomState(seed)
    for d, min_both in ((fabricate_small(ns, rng), 1), (fabricate_small(ns, rng), 2), (fabricate_small(ns, rng), 3), (cap_for_average(fabricate_wide(ns, rng)), 1),
                        (fabricate_wide(ns, rng), 1)):
        for metric in METRICS:
            K = link_keys(d, metric, min_both)
            for linkage in LINKAGES:
                if linkage == AVERAGE and ((K != NONE) & (K >= np.uint64(KEY_MAX))).any():
                    with pytest.raises(ValueError, match="key"):
                        restate_sample_agglomerate(d, metric, min_both, linkage)
                    continue
                links, n_rounds = restate_sample_agglomerate(d, metric, min_both, linkage)
                naive, naive_rounds, members = restate_sample_agglomerate_naive(d, metric, min_both, linkage)
                assert links.tobytes() == naive.tobytes() and n_rounds == naive_rounds, (metric, linkage)   # the second form
                keys = [k for a, b, k in as_tuples(links)]
                assert keys == sorted(keys)                                     # keys ascend
                comp = replay(links, ns)                                        # a and b: smallest members of two components
                assert comp is not None and {x: sorted(m) for x, m in comp.items()} == {x: sorted(m) for x, m in members.items()}
                assert len(links) == ns - len(comp) and n_rounds <= len(links)
                roots = sorted(comp)
                for i, x in enumerate(roots):                                   # the rounds ended: no two clusters all of whose pairs are edges
                    for y in roots[i + 1:]:
                        assert (K[np.ix_(comp[x], comp[y])] == NONE).any(), (x, y)


@pytest.mark.parametrize("ns,seed", [(2, 11), (7, 12), (20, 13), (40, 14)])
def test_complete_with_distinct_keys_is_the_greedy_tree(ns, seed):
    rng = np.random.RandomState(seed)
    nd = np.zeros((ns, ns), np.int64)
    a, b = np.triu_indices(ns, 1)
    nd[a, b] = rng.permutation(len(a)) + 1                                      # every pair its own key
    nb = np.full((ns, ns), 10000)
    nb[rng.random_sample((ns, ns)) < 0.05] = 0                                  # a few pairs are no edge
    np.fill_diagonal(nb, 10000)
    d = symmetric(ns, nb, np.minimum(nd, np.triu(nb)), 3 * nd)
    for metric in (DIFFER, LENGTH):
        links, n_rounds = restate_sample_agglomerate(d, metric, 1, COMPLETE)
        assert links.tobytes() == greedy_complete(d, metric, 1).tobytes() and n_rounds <= len(links)


# ---- declarations and argument checks --------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    own_path = os.path.join(ROOT, "include", "tatajuba_agglomerate.h")
    own = strip(own_path)
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.AGGLOMERATE_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_agglomerate.h"]
    assert len(others) >= 11
    for s in NEW_ENTRIES:
        for path in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(path)), (s, path)   # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in (tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS + tj.EFFECT_EXPORTS + tj.SITE_EXPORTS + tj.DEPTH_EXPORTS
                         + tj.DISTANCE_EXPORTS + tj.LINKAGE_EXPORTS + tj.GROUP_EXPORTS + tj.CLADE_EXPORTS) and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert '#include "tatajuba_linkage.h"' in own
    assert re.search(r"enum\s*\{\s*TJAMD_AGGL_COMPLETE = 1, TJAMD_AGGL_AVERAGE = 2\s*\}", own)
    assert (tj.AGGL_COMPLETE, tj.AGGL_AVERAGE) == (1, 2) == LINKAGES
    assert L.tjamd_last_sample_agglomerate_ms(None) == -1.0
    for name in ("sample_agglomerate", "last_sample_agglomerate_ms"):
        assert hasattr(tj.Counter, name)
    text = open(own_path).read()
    for what in ("Keys ascend", "comes before any link", "(key, round, a, b)", "waits once per batch of", "2^40",   # the rule, its two properties, the waits
                 "Ward", "neighbour joining", "cache of nearest neighbours", "compaction", "edges only", "stars of equal keys", "bootstrap"):   # named as not built
        assert what in text, what


def test_sample_agglomerate_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    out = GuardedHost(64 * LINK.itemsize)
    rounds = C.c_int(-77)

    def call(c=fake, dist=fake, ns=5, metric=DIFFER, min_both=1, linkage=COMPLETE, null_out=False, null_rounds=False):
        rc = L.tjamd_sample_agglomerate(c, dist, ns, metric, min_both, linkage, None if null_out else out.c, None if null_rounds else C.byref(rounds))
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"dist": None}, "null d_dist"), ({"null_out": True}, "null d_links"),
                    ({"null_out": True, "ns": 2}, "null d_links"),
                    ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": -3}, "n_samples -3 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"),
                    ({"ns": 0, "null_out": True}, "n_samples 0 outside 1..4096"),
                    ({"metric": -1}, "metric -1 outside 0..2"), ({"metric": 3}, "metric 3 outside 0..2"),
                    ({"min_both": 0}, "min_both 0 below 1"), ({"min_both": -7}, "min_both -7 below 1"),
                    ({"linkage": 0}, "linkage 0 outside 1..2"), ({"linkage": 3}, "linkage 3 outside 1..2"), ({"linkage": -1, "null_rounds": True}, "linkage -1 outside 1..2")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_sample_agglomerate") and msg in err, (kw, got, err)
    if tj.device_count() == 0:                     # good arguments, but nothing to run on: named, before the handles are read
        for kw in ({}, {"ns": 1}, {"ns": 1, "null_out": True}, {"linkage": AVERAGE, "null_rounds": True},
                   {"ns": 4096, "metric": DIFFER_RATE, "min_both": (1 << 31) - 1, "linkage": AVERAGE}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_sample_agglomerate") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    assert out.untouched() and rounds.value == -77  # host memory handed in as the outputs stays as it was
    out.check("d_links")


def test_sample_agglomerate_reports_the_first_of_two_broken_rules_without_a_gpu():
    """two rules broken in one call: the message is that of the rule that is checked first, for every pair of neighbours in the
    order of the checks"""
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    out = GuardedHost(64 * LINK.itemsize)
    rounds = C.c_int(-77)

    def call(c=fake, dist=fake, ns=5, metric=DIFFER, min_both=1, linkage=COMPLETE, null_out=False):
        rc = L.tjamd_sample_agglomerate(c, dist, ns, metric, min_both, linkage, None if null_out else out.c, C.byref(rounds))
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None, "dist": None}, "null counter"), ({"dist": None, "null_out": True}, "null d_dist"), ({"dist": None, "ns": 0}, "null d_dist"),
                    ({"null_out": True, "ns": 4097}, "null d_links"), ({"null_out": True, "metric": 3}, "null d_links"),
                    ({"ns": 0, "metric": 3}, "n_samples 0 outside 1..4096"), ({"ns": 4097, "min_both": 0}, "n_samples 4097 outside 1..4096"),
                    ({"metric": -1, "min_both": 0}, "metric -1 outside 0..2"), ({"metric": 3, "linkage": 3}, "metric 3 outside 0..2"),
                    ({"min_both": 0, "linkage": 3}, "min_both 0 below 1"), ({"min_both": -7, "linkage": 0}, "min_both -7 below 1")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_sample_agglomerate") and msg in err, (kw, got, err)
    assert out.untouched() and rounds.value == -77
    out.check("d_links")
