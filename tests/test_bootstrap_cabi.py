"""The bootstrap step (include/tatajuba_bootstrap.h: tjamd_bootstrap_weights, tjamd_sample_distances_weighted,
tjamd_clade_support) without a GPU: the entries are declared in their own header, exported and prototyped and refuse bad
arguments before any device call, and the three restatements that the GPU tests (tests/test_bootstrap.py) compare against are
pinned by hand cases whose expected values are written out here, and by properties.

restate_bootstrap_weights is the header's rule in numpy uint64; restate_sample_distances_weighted a loop over the sites, as
N14's restatement, with every site's contribution multiplied by its weight; restate_clade_support compares Python sets.  The
device counts draws with atomic adds, walks tiles of sample pairs for two replicates per staged chunk, and compares clades as
intervals of a replicate's leaf order looked up in a hash set."""
import ctypes as C
import fnmatch
import glob
import os
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedHost
from tests.test_distances_cabi import HAND_EXPECTED, fabricate, hand_case, restate_sample_distances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_bootstrap_weights", "tjamd_sample_distances_weighted", "tjamd_clade_support",
               "tjamd_last_bootstrap_weights_ms", "tjamd_last_sample_distances_weighted_ms", "tjamd_last_clade_support_ms"]
ERR_NO_DEVICE, ERR_ARG = 1, 3
SITE, ALLELE, DIST, NODE = tj.SITE_DTYPE, tj.ALLELE_DTYPE, tj.SAMPLE_DISTANCE_DTYPE, tj.TREE_NODE_DTYPE
SEEDS = (0, 1, 2 ** 64 - 1)
PIN = [[3, 0, 1, 0, 1, 0, 2], [2, 0, 1, 1, 1, 1, 1], [1, 0, 1, 3, 1, 1, 0]]     # n_sites 7, seed 1, replicates 0 .. 2: the header's


# ---- the weights ------------------------------------------------------------------------------------------------------------

def _mix(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def restate_bootstrap_weights(n_sites, n_replicates, seed):
    """-> int32 [n_replicates, n_sites]: per replicate the counts of n_sites draws; all arithmetic in uint64, wrapping"""
    assert 1 <= n_sites < 2 ** 31 and 1 <= n_replicates <= 4096 and n_sites * n_replicates < 2 ** 31
    out = np.zeros((n_replicates, n_sites), np.int32)
    with np.errstate(over="ignore"):
        r = np.arange(1, n_replicates + 1, dtype=np.uint64)
        base = _mix(np.uint64(seed & (2 ** 64 - 1)) + np.uint64(0x9E3779B97F4A7C15) * r)
        j = np.arange(n_sites, dtype=np.uint64)
        for k in range(n_replicates):
            h = _mix(base[k] + j)
            pick = ((h >> np.uint64(32)) * np.uint64(n_sites)) >> np.uint64(32)
            out[k] = np.bincount(pick.astype(np.int64), minlength=n_sites)
    return out


def test_the_rule_of_the_weights():
    assert restate_bootstrap_weights(7, 3, 1).tolist() == PIN
    # the mixer by Python's own integers, one draw at a time
    M = 2 ** 64 - 1

    def mix(z):
        z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 & M; z ^= z >> 27; z = z * 0x94D049BB133111EB & M
        return z ^ (z >> 31)

    for seed in SEEDS:
        for n_sites, n_rep in ((1, 2), (7, 3), (257, 5), (5000, 2)):
            w = restate_bootstrap_weights(n_sites, n_rep, seed)
            assert w.dtype == np.int32 and w.shape == (n_rep, n_sites) and (w >= 0).all()
            assert (w.sum(1) == n_sites).all()                                # every replicate sums to n_sites
            for longer in (n_rep + 1, n_rep + 60):                            # a replicate does not depend on n_replicates
                assert restate_bootstrap_weights(n_sites, longer, seed)[:n_rep].tobytes() == w.tobytes()
            if n_sites <= 257:
                plain = np.zeros((n_rep, n_sites), np.int32)
                for r in range(n_rep):
                    base = mix((seed + 0x9E3779B97F4A7C15 * (r + 1)) & M)
                    for j in range(n_sites):
                        plain[r, ((mix((base + j) & M) >> 32) * n_sites) >> 32] += 1
                assert plain.tobytes() == w.tobytes()
    a, b, c = (restate_bootstrap_weights(300, 2, s) for s in SEEDS)
    assert a.tobytes() != b.tobytes() != c.tobytes() and a[0].tobytes() != a[1].tobytes()
    zero = (restate_bootstrap_weights(5000, 4, 1) == 0).mean()
    assert 0.33 < zero < 0.41                                                 # e^-1 of the sites are not drawn


# ---- the weighted distances -------------------------------------------------------------------------------------------------

def restate_sample_distances_weighted(sites, alleles, genotype, weights):
    """-> SAMPLE_DISTANCE_DTYPE [n_replicates, ns, ns].  weights is [n_replicates, n_sites].  ValueError for what the entry refuses
    on the device: all that restate_sample_distances refuses, whatever the weights; a weight below 0; a sum of 2^31 or more"""
    genotype = np.asarray(genotype)
    n_sites, ns = genotype.shape
    weights = np.asarray(weights, np.int64).reshape(-1, n_sites)
    restate_sample_distances(sites, alleles, genotype)                        # (its checks read every site and cell)
    if (weights < 0).any():
        raise ValueError("weight")
    if (weights.sum(1) >= 2 ** 31).any():
        raise ValueError("weight sum")
    out = np.zeros((len(weights), ns, ns), DIST)
    for i, s in enumerate(sites):
        g = genotype[i].astype(np.int64)
        L = np.zeros(ns, np.int64)
        L[g == 0] = int(s["ref_length"])
        L[g > 0] = alleles["alt_length"][int(s["first_allele"]) + g[g > 0] - 1]
        both = (g >= 0)[:, None] & (g >= 0)[None, :]
        differ = both & (g[:, None] != g[None, :])
        diff = np.where(both, np.abs(L[:, None] - L[None, :]), 0)
        for r in range(len(weights)):
            w = int(weights[r, i])
            out["n_both"][r] += (w * both).astype(np.int32)
            out["n_differ"][r] += (w * differ).astype(np.int32)
            out["length_diff"][r] += w * diff
    return out


# the hand case of tests/test_distances_cabi.py under the weights 2, 0, 3: site 1 drops out, site 0 counts twice, site 2 three times
#            sample 0   sample 1   sample 2
#   site 0   0 (5)      1 (6)      -1           x 2
#   site 2   1 (2)      1 (2)      0 (7)        x 3
# (0, 1): 2 + 3 in common, site 0 differs by 1, twice: (5, 2, 2).  (0, 2) and (1, 2): site 2 alone, three times, by 5: (3, 3, 15)
HAND_WEIGHTS = [2, 0, 3]
HAND_WEIGHTED = [[(5, 0, 0), (5, 2, 2), (3, 3, 15)],
                 [(5, 2, 2), (5, 0, 0), (3, 3, 15)],
                 [(3, 3, 15), (3, 3, 15), (3, 0, 0)]]


def as_triples(d):
    return [[tuple(int(v) for v in d[a, b]) for b in range(d.shape[1])] for a in range(d.shape[0])]


def repeat_sites(sites, alleles, genotype, w):
    """the corpus with site i repeated w[i] times, the allele chain rebuilt"""
    idx = np.repeat(np.arange(len(sites)), w)
    s = sites[idx].copy()
    s["first_allele"] = np.cumsum(s["n_alleles"]) - s["n_alleles"]
    parts = [alleles[int(sites["first_allele"][i]): int(sites["first_allele"][i]) + int(sites["n_alleles"][i])] for i in idx]
    a = np.concatenate(parts).copy() if len(parts) else alleles[:0].copy()
    a["site"] = np.repeat(np.arange(len(idx)), s["n_alleles"])
    return s, a, genotype[idx]


def test_the_rule_of_the_weighted_distances():
    sites, alleles, genotype = hand_case()
    got = restate_sample_distances_weighted(sites, alleles, genotype, [HAND_WEIGHTS, [1, 1, 1]])
    assert as_triples(got[0]) == HAND_WEIGHTED and as_triples(got[1]) == HAND_EXPECTED
    assert got[1].tobytes() == restate_sample_distances(sites, alleles, genotype).tobytes()
    with pytest.raises(ValueError, match="weight"):
        restate_sample_distances_weighted(sites, alleles, genotype, [[1, -1, 1]])
    with pytest.raises(ValueError, match="weight sum"):
        restate_sample_distances_weighted(sites, alleles, genotype, [[1, 1, 1], [2 ** 31 - 2, 1, 1]])
    restate_sample_distances_weighted(sites, alleles, genotype, [[2 ** 31 - 3, 1, 1]])      # 2^31 - 1: accepted
    bad = genotype.copy()
    bad[1, 0] = 7
    with pytest.raises(ValueError, match="genotype"):                         # in a site of weight 0
        restate_sample_distances_weighted(sites, alleles, bad, [HAND_WEIGHTS])


@pytest.mark.parametrize("n_sites,ns,seed", [(40, 7, 1), (25, 20, 2), (1, 3, 3)])
def test_weights_are_repeats_on_a_random_corpus(n_sites, ns, seed):
    rng = np.random.RandomState(seed)
    sites, alleles, g = fabricate(n_sites, ns, rng)
    weights = np.concatenate([restate_bootstrap_weights(n_sites, 2, seed), rng.randint(0, 4, (1, n_sites)), np.ones((1, n_sites), np.int64)])
    got = restate_sample_distances_weighted(sites, alleles, g, weights)
    for r, w in enumerate(weights):
        if w.sum() == 0:
            assert got[r].tobytes() == bytes(ns * ns * DIST.itemsize)
            continue
        assert got[r].tobytes() == restate_sample_distances(*repeat_sites(sites, alleles, g, w)).tobytes(), r
        for f in DIST.names:
            assert (got[r][f] == got[r][f].T).all()                           # full and symmetric: input to the tree builders
    assert got[3].tobytes() == restate_sample_distances(sites, alleles, g).tobytes()      # all weights 1


# ---- the support ------------------------------------------------------------------------------------------------------------

def nodes_of(intervals):
    out = np.zeros(len(intervals), NODE)
    for j, (first, size) in enumerate(intervals):
        out[j] = (0, 0, first, size)                                          # (children are not read)
    return out


def _checked_tree(nodes, order, ns):
    order = np.asarray(order, np.int64)
    if len(order) != ns or sorted(order.tolist()) != list(range(ns)):
        raise ValueError("order")
    for nd in nodes:
        first, size = int(nd["first"]), int(nd["size"])
        if size < 2 or first < 0 or first + size > ns:
            raise ValueError("node")
    return [frozenset(order[int(nd["first"]): int(nd["first"]) + int(nd["size"])].tolist()) for nd in nodes]


def restate_clade_support(nodes, order, replicates):
    """replicates: a list of (nodes, order) -> int32 [n_nodes], per node the replicates that hold its set; ValueError for what
    is refused on the device"""
    ns = len(order)
    base = _checked_tree(nodes, order, ns)
    held = [set(_checked_tree(rn, ro, ns)) for rn, ro in replicates]
    return np.array([sum(s in h for h in held) for s in base], np.int32)


# Seven samples.  The base: {0, 5}, {3, 4}, {0, 5, 3, 4}, {1, 2}, and all but sample 6, over the order 0 5 3 4 1 2 6.
#   replicate 0: the same tree over another order (4 3 5 0 6 2 1), with {0, 5} written twice: every node once, but {1, 2},
#                which lies side by side at positions 5 and 6 and is no node there, and the node of six, which is not side by side
#   replicate 1: a forest, {1, 2} and {3, 4} only, over the identity
#   replicate 2: no node at all
HAND_BASE = ([(0, 2), (2, 2), (0, 4), (4, 2), (0, 6)], [0, 5, 3, 4, 1, 2, 6])
HAND_REPLICATES = [([(2, 2), (0, 2), (2, 2), (0, 4)], [4, 3, 5, 0, 6, 2, 1]),
                   ([(1, 2), (3, 2)], [0, 1, 2, 3, 4, 5, 6]),
                   ([], [6, 5, 4, 3, 2, 1, 0])]
HAND_SUPPORT = [1, 2, 1, 1, 0]


def hand_support_case():
    return nodes_of(HAND_BASE[0]), np.array(HAND_BASE[1], np.int32), [(nodes_of(n), np.array(o, np.int32)) for n, o in HAND_REPLICATES]


def test_the_rule_of_the_support():
    nodes, order, reps = hand_support_case()
    assert restate_clade_support(nodes, order, reps).tolist() == HAND_SUPPORT
    assert restate_clade_support(nodes, order, [(nodes, order)] * 3).tolist() == [3] * 5
    assert restate_clade_support(nodes[:0], order, reps).tolist() == []
    for bad_order in ([0, 5, 3, 4, 1, 2, 2], [0, 5, 3, 4, 1, 2, 7], [0, 5, 3, 4, 1, 2, -1]):
        with pytest.raises(ValueError, match="order"):
            restate_clade_support(nodes, bad_order, reps)
        with pytest.raises(ValueError, match="order"):
            restate_clade_support(nodes, order, reps[:1] + [(reps[1][0], bad_order)])
    for bad_node in ((0, 1), (-1, 3), (6, 2), (0, 8)):
        with pytest.raises(ValueError, match="node"):
            restate_clade_support(nodes_of([bad_node]), order, reps)
        with pytest.raises(ValueError, match="node"):
            restate_clade_support(nodes, order, [(nodes_of([bad_node]), order)])


def fabricate_support(ns, n_rep, rng):
    """random intervals over random permutations; every replicate repeats some of the base's sets as intervals of its own order"""
    order = rng.permutation(ns).astype(np.int32)
    n_nodes = 0 if ns < 2 else int(rng.randint(1, ns))
    iv = []
    for _ in range(n_nodes):
        size = int(rng.randint(2, ns + 1)) if rng.rand() < 0.3 else int(rng.randint(2, min(ns, 5) + 1))
        iv.append((int(rng.randint(0, ns - size + 1)), size))
    nodes = nodes_of(iv)
    reps = []
    for r in range(n_rep):
        ro = order.copy()
        kind = r % 4
        if kind == 1:
            ro = ro[::-1].copy()                                              # every set is an interval again, elsewhere
        elif kind >= 2:
            ro = rng.permutation(ns).astype(np.int32)
        if kind == 3 and len(iv):                                             # keep some sets side by side in a random order
            first, size = iv[int(rng.randint(len(iv)))]
            members = order[first: first + size]
            rest = [s for s in ro.tolist() if s not in set(members.tolist())]
            at = int(rng.randint(0, len(rest) + 1))
            ro = np.array(rest[:at] + rng.permutation(members).tolist() + rest[at:], np.int32)
        pos = {int(s): p for p, s in enumerate(ro.tolist())}
        riv = []
        for first, size in iv:
            where = sorted(pos[int(s)] for s in order[first: first + size])
            if where[-1] - where[0] + 1 == size and rng.rand() < 0.7:
                riv.append((where[0], size))
        while ns >= 2 and len(riv) < ns - 1 and rng.rand() < 0.6:
            size = int(rng.randint(2, min(ns, 6) + 1))
            riv.append((int(rng.randint(0, ns - size + 1)), size))
        riv = riv[: max(ns - 1, 0)]
        reps.append((nodes_of([riv[i] for i in rng.permutation(len(riv))]), ro))
    return nodes, order, reps


def test_the_support_on_fabricated_intervals():
    seen = set()
    for ns, n_rep, seed in ((2, 1, 1), (3, 2, 2), (9, 8, 3), (40, 12, 4)):
        nodes, order, reps = fabricate_support(ns, n_rep, np.random.RandomState(seed))
        got = restate_clade_support(nodes, order, reps)
        assert len(got) == len(nodes) and (got >= 0).all() and (got <= n_rep).all()
        seen |= set(got.tolist())
        # by positions: the span of the members in the replicate's order, and a node at that place
        for j, nd in enumerate(nodes):
            members = order[int(nd["first"]): int(nd["first"]) + int(nd["size"])].tolist()
            n = 0
            for rn, ro in reps:
                where = [ro.tolist().index(s) for s in members]
                n += max(where) - min(where) + 1 == len(members) and any(int(x["first"]) == min(where) and int(x["size"]) == len(members) for x in rn)
            assert n == got[j]
    assert len(seen) >= 4 and max(seen) >= 3                                  # counts differ from node to node


def _checked_intervals(nodes, order, ns):
    """the refusals of _checked_tree, in its order -> (order int64 [ns], first int64 [n], size int64 [n])"""
    order = np.asarray(order, np.int64).reshape(-1)
    if len(order) != ns or (order < 0).any() or (order >= ns).any() or (np.bincount(order, minlength=ns) != 1).any():
        raise ValueError("order")
    first, size = np.asarray(nodes["first"], np.int64), np.asarray(nodes["size"], np.int64)
    if ((size < 2) | (first < 0) | (first + size > ns)).any():
        raise ValueError("node")
    return order, first, size


def restate_clade_support_by_positions(nodes, order, replicates):
    """restate_clade_support without a set per node, in numpy, for trees of thousands of samples (a caterpillar of 4096 has 8
    million members).  Per replicate pos = argsort(rep_order) is every sample's place in the replicate's order; a node of the base
    is held iff the places of its members pos[order[first: first + size]] are side by side (max - min + 1 == size) and (min, size)
    is among the replicate's (first, size) pairs.  The same refusals in the same order"""
    ns = len(order)
    order, first, size = _checked_intervals(nodes, order, ns)
    checked = [_checked_intervals(rn, ro, ns) for rn, ro in replicates]
    out = np.zeros(len(first), np.int32)
    if not len(first):
        return out
    cuts = np.stack([first, first + size], 1).reshape(-1)                     # reduceat: the slices [first, first + size) are its even results
    for ro, rfirst, rsize in checked:
        q = np.append(np.argsort(ro, kind="stable")[order], 0)                # (one more element, in odd results alone: a slice may end at ns)
        lo, hi = np.minimum.reduceat(q, cuts)[::2], np.maximum.reduceat(q, cuts)[::2]
        out += ((hi - lo + 1 == size) & np.isin(lo * (ns + 1) + size, rfirst * (ns + 1) + rsize)).astype(np.int32)
    return out


@pytest.mark.parametrize("ns", [2, 3, 9, 64, 65, 130, 257])
def test_the_support_by_positions_is_the_support_by_sets(ns):
    for seed in range(3):
        nodes, order, reps = fabricate_support(ns, 5, np.random.RandomState(1000 * ns + seed))
        want = restate_clade_support(nodes, order, reps)
        assert restate_clade_support_by_positions(nodes, order, reps).tolist() == want.tolist(), (ns, seed)
        assert restate_clade_support_by_positions(nodes, order, reps).dtype == want.dtype
        assert restate_clade_support_by_positions(nodes[:0], order, reps).tolist() == []
        whole = nodes_of([(0, ns)])                                           # a slice that ends at ns
        assert restate_clade_support_by_positions(whole, order, reps + [(whole, order)]).tolist() == restate_clade_support(whole, order, reps + [(whole, order)]).tolist()


def test_the_support_by_positions_on_the_hand_case_and_its_refusals():
    nodes, order, reps = hand_support_case()
    assert restate_clade_support_by_positions(nodes, order, reps).tolist() == HAND_SUPPORT
    assert restate_clade_support_by_positions(nodes, order, [(nodes, order)] * 3).tolist() == [3] * 5
    for bad_order in ([0, 5, 3, 4, 1, 2, 2], [0, 5, 3, 4, 1, 2, 7], [0, 5, 3, 4, 1, 2, -1], [0, 5, 3, 4, 1, 2]):
        for restate in (restate_clade_support, restate_clade_support_by_positions):
            with pytest.raises(ValueError, match="order"):
                restate(nodes, bad_order, reps)
            if len(bad_order) == 7:
                with pytest.raises(ValueError, match="order"):
                    restate(nodes, order, reps[:1] + [(reps[1][0], bad_order)])
    for bad_node in ((0, 1), (-1, 3), (6, 2), (0, 8), (1 << 30, 1 << 30)):
        for restate in (restate_clade_support, restate_clade_support_by_positions):
            with pytest.raises(ValueError, match="node"):
                restate(nodes_of([bad_node]), order, reps)
            with pytest.raises(ValueError, match="node"):
                restate(nodes, order, [(nodes_of([bad_node]), order)])
    for restate in (restate_clade_support, restate_clade_support_by_positions):   # a bad order is named before a bad node, the base before a replicate
        with pytest.raises(ValueError, match="order"):
            restate(nodes_of([(0, 1)]), [0, 5, 3, 4, 1, 2, 2], reps)
        with pytest.raises(ValueError, match="node"):
            restate(nodes_of([(0, 1)]), order, [(reps[0][0], [0] * 7)])


def clade_support_text(names, links, tree, node_marks, support, n_replicates):
    """clade_support.tsv of examples/merged_vcf.c -B: node, size, the name of its smallest member, key, supporting sites, support, R"""
    return "".join("%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (j, nd["size"], names[int(tree["order"][int(nd["first"])])], links["key"][j], node_marks[j], support[j], n_replicates)
                   for j, nd in enumerate(tree["nodes"]))


def test_clade_support_text_on_the_hand_case():
    from tests.test_clades_cabi import HAND_LINKS, links_of, restate_linkage_tree
    links = links_of(HAND_LINKS)
    tree = restate_linkage_tree(links, 7)
    assert [(int(n["first"]), int(n["size"])) for n in tree["nodes"]] == HAND_BASE[0] and tree["order"].tolist() == HAND_BASE[1]
    text = clade_support_text(["s%d" % i for i in range(7)], links, tree, [1, 1, 0, 1, 1], HAND_SUPPORT, 3)
    assert text == "0\t2\ts0\t0\t1\t1\t3\n1\t2\ts3\t1\t1\t2\t3\n2\t4\ts0\t2\t0\t1\t3\n3\t2\ts1\t3\t1\t1\t3\n4\t6\ts0\t4\t1\t0\t3\n"


# ---- declarations and argument checks --------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    path = os.path.join(ROOT, "include", "tatajuba_bootstrap.h")
    own, text = strip(path), " ".join(open(path).read().replace("*", " ").split())
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.BOOTSTRAP_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_bootstrap.h"]
    assert len(others) >= 14
    earlier = (tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS + tj.EFFECT_EXPORTS + tj.SITE_EXPORTS + tj.DEPTH_EXPORTS + tj.DISTANCE_EXPORTS
               + tj.LINKAGE_EXPORTS + tj.AGGLOMERATE_EXPORTS + tj.GROUP_EXPORTS + tj.CLADE_EXPORTS)
    for s in NEW_ENTRIES:
        for p in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(p)), (s, p)             # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in earlier and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert '#include "tatajuba_agglomerate.h"' in own and '#include "tatajuba_clades.h"' in own
    for name in ("bootstrap_weights", "sample_distances_weighted", "clade_support", "last_bootstrap_weights_ms", "last_sample_distances_weighted_ms",
                 "last_clade_support_ms"):
        assert hasattr(tj.Counter, name), name
    for timer in (L.tjamd_last_bootstrap_weights_ms, L.tjamd_last_sample_distances_weighted_ms, L.tjamd_last_clade_support_ms):
        assert timer(None) == -1.0
    for what in ("Reference interface replaced: none", "N19 of DESIGN.md section 3.5", "the rule of the weights", "the rule of the weighted distances",
                 "the rule of the clade support", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15", "((h >> 32) n_sites) >> 32",
                 "3 0 1 0 1 0 2, 2 0 1 1 1 1 1 and 1 0 1 3 1 1 0", "does not depend on n_replicates", "multiplied by w", "the bytes are tjamd_sample_distances'",
                 "a weight below 0", "sum to 2^31 or more", "counts once", "span `size`", "h_rep_n_nodes is host memory", "forests are fine",
                 "Not built:", "a batched tree builder", "jackknife", "real-valued weights", "support written into the Newick file", "MFMA for the 0/1 quantities"):
        assert what in text, what


def test_bootstrap_weights_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                      # never dereferenced: each call below fails its argument checks first
    out = GuardedHost(4096)

    def call(c=fake, n_sites=7, n_rep=3, null_out=False):
        rc = L.tjamd_bootstrap_weights(c, n_sites, n_rep, 1, None if null_out else out.c)
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"null_out": True}, "null d_weights"), ({"n_sites": 0}, "n_sites 0 outside 1..2^31 - 1"),
                    ({"n_sites": -4}, "n_sites -4 outside"), ({"n_sites": 1 << 31}, "n_sites 2147483648 outside"),
                    ({"n_rep": 0}, "n_replicates 0 outside 1..4096"), ({"n_rep": 4097}, "n_replicates 4097 outside 1..4096"),
                    ({"n_sites": 1 << 19, "n_rep": 4096}, "4096 replicates x 524288 sites: 2^31 weights or more")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_bootstrap_weights") and msg in err, (kw, got, err)
    if tj.device_count() == 0:
        for kw in ({}, {"n_sites": (1 << 19) - 1, "n_rep": 4096}, {"n_sites": (1 << 31) - 1, "n_rep": 1}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_bootstrap_weights") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    assert out.untouched()
    out.check("d_weights")


def test_sample_distances_weighted_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)
    out = GuardedHost(64 * DIST.itemsize)

    def call(c=fake, sites=fake, n_sites=3, alleles=fake, n_alleles=4, gt=fake, ns=2, null_out=False, w=fake, n_rep=2):
        rc = L.tjamd_sample_distances_weighted(c, sites, n_sites, alleles, n_alleles, gt, ns, None if null_out else out.c, w, n_rep)
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"null_out": True}, "null d_out"),
                    ({"n_sites": -1}, "n_sites -1, n_alleles 4: a count below 0"), ({"n_alleles": -1}, "n_sites 3, n_alleles -1: a count below 0"),
                    ({"sites": None}, "null site, allele or genotype buffer"), ({"alleles": None}, "null site, allele or genotype buffer"),
                    ({"gt": None}, "null site, allele or genotype buffer"),
                    ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": -3}, "n_samples -3 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"),
                    ({"n_alleles": 2}, "2 alleles for 3 sites"),
                    ({"n_alleles": 1 << 31}, "2147483648 alleles: 2^31 or more"),
                    ({"n_sites": 1 << 19, "n_alleles": 1 << 19, "ns": 4096}, "524288 sites x 4096 samples: 2^31 cells or more"),
                    ({"w": None}, "null d_weights"), ({"n_rep": 0}, "n_replicates 0 outside 1..4096"), ({"n_rep": 4097}, "n_replicates 4097 outside 1..4096"),
                    ({"n_sites": 1 << 19, "n_alleles": 1 << 19, "ns": 2, "n_rep": 4096}, "4096 replicates x 524288 sites: 2^31 weights or more")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_sample_distances_weighted") and msg in err, (kw, got, err)
    if tj.device_count() == 0:
        for kw in ({}, {"n_sites": 0, "n_alleles": 0}, {"n_sites": 0, "n_alleles": 0, "sites": None, "alleles": None, "gt": None, "w": None},
                   {"n_sites": (1 << 19) - 1, "n_alleles": (1 << 31) - 1, "ns": 4096, "n_rep": 4096}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_sample_distances_weighted") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    assert out.untouched()
    out.check("d_out")


def test_clade_support_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)
    out = GuardedHost(64 * 4)

    def call(c=fake, nodes=fake, n_nodes=3, order=fake, ns=7, rep_nodes=fake, rep_order=fake, counts=(2, 0, 6), n_rep=None, null_out=False):
        h = None if counts is None else (C.c_int * len(counts))(*counts)
        rc = L.tjamd_clade_support(c, nodes, n_nodes, order, ns, rep_nodes, rep_order, h, (len(counts) if counts is not None else 3) if n_rep is None else n_rep,
                                   None if null_out else out.c)
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"),
                    ({"n_nodes": -1}, "n_nodes -1 outside 0..4096"), ({"n_nodes": 4097}, "n_nodes 4097 outside 0..4096"),
                    ({"n_rep": 0}, "n_replicates 0 outside 1..4096"), ({"n_rep": 4097}, "n_replicates 4097 outside 1..4096"),
                    ({"order": None}, "null d_order or d_rep_order"), ({"rep_order": None}, "null d_order or d_rep_order"),
                    ({"counts": None}, "null h_rep_n_nodes"), ({"nodes": None}, "null d_nodes or d_support"), ({"null_out": True}, "null d_nodes or d_support"),
                    ({"rep_nodes": None}, "null d_rep_nodes"),
                    ({"counts": (2, -1, 6)}, "replicate 1 has -1 nodes, outside 0..n_samples - 1 = 6"),
                    ({"counts": (2, 0, 7)}, "replicate 2 has 7 nodes, outside 0..n_samples - 1 = 6"),
                    ({"counts": (1,), "ns": 1, "n_nodes": 0}, "replicate 0 has 1 nodes, outside 0..n_samples - 1 = 0")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_clade_support") and msg in err, (kw, got, err)
    if tj.device_count() == 0:
        for kw in ({}, {"n_nodes": 0, "nodes": None, "null_out": True}, {"counts": (0, 0), "rep_nodes": None}, {"ns": 4096, "n_nodes": 4096, "counts": (4095,)}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_clade_support") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    assert out.untouched()
    out.check("d_support")


def test_both_distance_entries_share_their_refusals_without_a_gpu():
    """every refusal that tjamd_sample_distances and tjamd_sample_distances_weighted share ahead of the device, by the same bad
    arguments through both (the weighted entry otherwise valid, one replicate): one code, one text behind the entry's name; the
    weighted entry's own three refusals come only where the shared ones pass"""
    L = tj.lib()
    fake = C.c_void_p(0x1000)                      # never dereferenced: each call below fails its argument checks first
    out = GuardedHost(64 * DIST.itemsize)
    names = ("tjamd_sample_distances", "tjamd_sample_distances_weighted")

    def call(weighted, sites=fake, n_sites=3, alleles=fake, n_alleles=4, gt=fake, ns=2, null_out=False, w=fake, n_rep=1):
        args = (fake, sites, n_sites, alleles, n_alleles, gt, ns, None if null_out else out.c)
        rc = L.tjamd_sample_distances_weighted(*args, w, n_rep) if weighted else L.tjamd_sample_distances(*args)
        err = L.tjamd_last_error().decode()
        assert err.startswith(names[weighted] + ": "), err
        return rc, err[len(names[weighted]):]

    shared = [({"null_out": True}, "null d_out"),
              ({"n_sites": -1}, "n_sites -1, n_alleles 4: a count below 0"), ({"n_alleles": -1}, "n_sites 3, n_alleles -1: a count below 0"),
              ({"sites": None}, "null site, allele or genotype buffer"), ({"alleles": None}, "null site, allele or genotype buffer"),
              ({"gt": None}, "null site, allele or genotype buffer"),
              ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"),
              ({"n_alleles": 2}, "2 alleles for 3 sites (a site has at least one)"),
              ({"n_alleles": 1 << 31}, "2147483648 alleles: 2^31 or more"),
              ({"n_sites": 1 << 19, "n_alleles": 1 << 19, "ns": 4096}, "524288 sites x 4096 samples: 2^31 cells or more")]
    own = [({"w": None}, "null d_weights"), ({"n_rep": 0}, "n_replicates 0 outside 1..4096"), ({"n_rep": 4097}, "n_replicates 4097 outside 1..4096"),
           ({"n_sites": 1 << 19, "n_alleles": 1 << 19, "n_rep": 4096}, "4096 replicates x 524288 sites: 2^31 weights or more")]
    for kw, msg in shared:
        plain, weighted = call(False, **kw), call(True, **kw)
        assert plain == weighted and plain == (-ERR_ARG, ": " + msg), (kw, plain, weighted)
        n_both = 0
        for more, _ in own:                        # a shared refusal is named before any of the weighted entry's own
            if set(more) & set(kw):                # (the two bad arguments are different ones)
                continue
            both = dict(more, **kw)
            assert call(True, **both) == weighted, (both, weighted)
            n_both += 1
        assert n_both >= 3, kw
    for kw, msg in own:                            # ... which come where the shared checks pass
        got = call(True, **kw)
        assert got == (-ERR_ARG, ": " + msg), (kw, got)
        if tj.device_count() == 0:                 # the same arguments pass every check of the plain entry: it asks for the device
            rc, err = call(False, **{k: v for k, v in kw.items() if k not in ("w", "n_rep")})
            assert rc == -ERR_NO_DEVICE and "TJAMD_ERR_NO_DEVICE" in err, (kw, rc, err)
    assert out.untouched()
    out.check("d_out")
