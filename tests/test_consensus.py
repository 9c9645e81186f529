"""tjamd_consensus_tree on the GPU, with no difference allowed anywhere: every result is compared with the restatement of
tests/test_consensus_cabi.py, and beside it with the entries that exist: d_rep_count with the loop the call replaces (a call of
tjamd_clade_support per replicate, that replicate as the base), the consensus nodes, cast, as the base of tjamd_clade_support
(d_support[j] == count) and as the nodes of tjamd_clade_sites.  Sample counts 2, 3, 5, 63, 64, 65, 130 and 257, and 1025 once;
replicate counts 1, 2, 3, 5 and 8; min_count at the majority, one above it and at n_replicates.  Replicates come from the
fabricated corpus (shown on the CPU to hold a multifurcation, rejected classes and a thinner strict consensus), from
tjamd_replicate_trees on the planted corpus of tests/test_bootstrap.py under all three linkages, from two caterpillars in
opposite directions, from one tree under different leaf orders, and from forests, empty replicates, duplicate nodes and nodes
out of order.  Counters under TATAJUBA_AMD_CONSENSUS_KEY_BITS = 0 and 3 must give the bytes of the default.  Outputs always sit
in guarded buffers (tests/guarded.py), every input is held frozen, and every call is made twice and must give the same bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, frozen, payload_pattern
from tests.test_bootstrap import PLANTED_NS, PLANTED_REPLICATES, PLANTED_SEED, PLANTED_SITES, dev_support, dev_weighted, dev_weights, planted_chain
from tests.test_clades import OUTPUTS, dev_clade_sites
from tests.test_consensus_cabi import (CNODE, CORPUS, CROSS, NODE, PERMUTATION, RANGE, as_rows, fabricate_replicates, majority, nodes_of, one_differing_replicate, pack,
                                       restate_consensus, three_children, two_roots)
from tests.test_bootstrap_cabi import restate_bootstrap_weights, restate_sample_distances_weighted
from tests.test_clades_cabi import restate_linkage_tree
from tests.test_depths_cabi import restate_site_depths
from tests.test_distances_cabi import restate_sample_distances
from tests.test_linkage_cabi import DIFFER, restate_sample_linkage
from tests.test_locate import _dev, _p
from tests.test_sites import pipeline  # noqa: F401  (the module-scoped fixture, built here as there)
from tests.test_sites_cabi import restate_merge_variants
from tests.test_replicate_trees import dev_rep_trees
from tests.test_replicate_trees_cabi import LINKAGES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 3
UNSET = -77


def _torch():
    return pytest.importorskip("torch")


def dev_consensus(counter, reps, ns, min_count, null=()):
    """two calls of tjamd_consensus_tree on reps [(intervals or NODE array, order)] -> {"nodes", "order", "rep_count", "n_classes"}
    as the restatement gives them; or, when the call is refused, (negative code, message, the guarded buffers).  Entries past
    the return value and past a replicate's count must hold what the buffers held before the call."""
    torch = _torch()
    L = tj.lib()
    rep_nodes, rep_orders, counts = pack(reps, ns)
    R = len(counts)
    pad = lambda a: _dev(a) if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")
    rnd, rod = pad(rep_nodes), _dev(rep_orders)
    runs = []
    for _ in range(2):
        bufs = {"nodes": GuardedDevice((ns - 1) * 16), "order": GuardedDevice(ns * 4), "rep_count": GuardedDevice(R * (ns - 1) * 4)}
        h_counts, n_classes = (C.c_int * R)(*counts), C.c_long(UNSET)
        torch.cuda.synchronize()
        with frozen(rnd, rod):
            rc = L.tjamd_consensus_tree(counter._h, _p(rnd) if sum(counts) else None, _p(rod), h_counts, ns, R, min_count, bufs["nodes"].c if ns > 1 else None, bufs["order"].c,
                                        None if "rep_count" in null else bufs["rep_count"].c, None if "classes" in null else C.byref(n_classes))
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        assert list(h_counts) == counts
        for k, b in bufs.items():
            b.check("d_" + k)
        if rc < 0:
            assert counter.last_consensus_tree_ms() == -1.0 and err.startswith("tjamd_consensus_tree")
            assert n_classes.value == UNSET and all(b.untouched() for b in bufs.values()), err     # a refused call leaves its outputs alone
            return rc, err, bufs
        assert 0 <= rc <= ns - 1 and (counter.last_consensus_tree_ms() > 0 if ns > 1 else counter.last_consensus_tree_ms() == -1.0)
        raw = {k: b.payload.cpu().numpy() for k, b in bufs.items()}
        assert (raw["nodes"][rc * 16:] == payload_pattern(bufs["nodes"].nbytes)[rc * 16:]).all()   # entries from the return value on are not written
        rep_count, pattern = [], payload_pattern(bufs["rep_count"].nbytes)
        for r in range(R):
            lo, hi = (r * (ns - 1) + (0 if "rep_count" in null else counts[r])) * 4, (r + 1) * (ns - 1) * 4
            assert (raw["rep_count"][lo:hi] == pattern[lo:hi]).all(), r
            rep_count.append(raw["rep_count"][r * (ns - 1) * 4: (r * (ns - 1) + counts[r]) * 4].copy().view(np.int32))
        runs.append({"nodes": raw["nodes"][: rc * 16].copy().view(CNODE), "order": raw["order"].copy().view(np.int32), "rep_count": rep_count,
                     "n_classes": None if "classes" in null else n_classes.value})
    a, b = runs
    assert a["nodes"].tobytes() == b["nodes"].tobytes() and a["order"].tobytes() == b["order"].tobytes() and a["n_classes"] == b["n_classes"]     # two runs: the same bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a["rep_count"], b["rep_count"]))
    return a


def same(got, want, what=""):
    assert isinstance(got, dict), (what, got[:2])
    assert as_rows(got["nodes"]) == as_rows(want["nodes"]) and got["nodes"].tobytes() == want["nodes"].tobytes(), (what, as_rows(got["nodes"])[:8], as_rows(want["nodes"])[:8])
    assert got["order"].tobytes() == want["order"].tobytes(), (what, got["order"][:16], want["order"][:16])
    assert got["n_classes"] == want["n_classes"], (what, got["n_classes"], want["n_classes"])
    assert len(got["rep_count"]) == len(want["rep_count"])
    for r, (g, w) in enumerate(zip(got["rep_count"], want["rep_count"])):
        assert g.tobytes() == w.tobytes(), (what, r, g[:8], w[:8])


def check(counter, reps, ns, min_count, what=""):
    got = dev_consensus(counter, reps, ns, min_count)
    same(got, restate_consensus(*pack(reps, ns), ns, min_count), what)
    return got


def as_arrays(reps):
    return [(rn if isinstance(rn, np.ndarray) else nodes_of(rn), np.asarray(ro, np.int32)) for rn, ro in reps]


def cross_check(counter, reps, ns, got, bases=5):
    """the entries that exist, on the device: the loop the call replaces, and the consensus as the base of tjamd_clade_support"""
    reps = as_arrays(reps)
    for r, (rn, ro) in enumerate(reps[:bases]):
        if len(rn) and len({(int(n["first"]), int(n["size"])) for n in rn}) == len(rn):     # (a replicate with a duplicate node: the loop's base would hold it twice)
            assert dev_support(counter, rn, ro, reps).tolist() == got["rep_count"][r].tolist(), r
    if len(got["nodes"]):
        assert dev_support(counter, got["nodes"].view(NODE), got["order"], reps).tolist() == got["nodes"]["count"].tolist()


def thresholds(R):
    return sorted({m for m in (majority(R), majority(R) + 1, R) if m <= R})


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
def hook_counters():
    """every clade of a size in one run; eight keys a size; and the keys as they are"""
    assert "TATAJUBA_AMD_CONSENSUS_KEY_BITS" not in os.environ
    cs = [_counter_under(TATAJUBA_AMD_CONSENSUS_KEY_BITS="0"), _counter_under(TATAJUBA_AMD_CONSENSUS_KEY_BITS="3"), tj.Counter(15)]
    yield cs
    for c in cs:
        c.close()


def test_hand_cases(counter):
    reps, ns = one_differing_replicate()
    got = check(counter, reps, ns, 2)
    assert as_rows(got["nodes"]) == [(1, 2, 0, 2), (2, 2, 0, 3), (3, 2, 0, 4), (-1, 3, 0, 5)] and got["n_classes"] == 7
    cross_check(counter, reps, ns, got)
    assert as_rows(check(counter, reps, ns, 3)["nodes"]) == [(-1, 3, 0, 5)]
    reps, ns = three_children()
    got = check(counter, reps, ns, 2)
    assert as_rows(got["nodes"]) == [(2, 3, 0, 2), (2, 2, 2, 2), (-1, 2, 0, 5)]
    cross_check(counter, reps, ns, got)
    check(counter, reps, ns, 3)
    reps, ns = two_roots()
    got = check(counter, reps, ns, 1)
    assert as_rows(got["nodes"]) == [(-1, 1, 0, 2), (-1, 1, 3, 2)] and got["order"].tolist() == [0, 3, 1, 2, 4]
    cross_check(counter, reps, ns, got)


@pytest.mark.parametrize("shape", sorted(CORPUS))
def test_the_fabricated_corpus(counter, shape):
    ns, R, k = shape
    reps = fabricate_replicates(ns, R, k, CORPUS[shape])
    for m in thresholds(R):
        got = check(counter, reps, ns, m, (shape, m))
        cross_check(counter, reps, ns, got, bases=R if m == majority(R) else 1)


@pytest.mark.parametrize("ns", [2, 3, 5, 63, 64, 65, 130, 257])
def test_sample_replicate_and_threshold_counts(counter, ns):
    reps = fabricate_replicates(ns, 8, 1 + ns // 64, 100 + ns)
    for R in (1, 2, 3, 5, 8):
        for m in thresholds(R):
            got = check(counter, reps[:R], ns, m, (ns, R, m))
        cross_check(counter, reps[:R], ns, got, bases=2)                # (at the strict threshold)


def test_more_than_a_sample_per_thread(counter):
    """1025 samples: a workgroup of 1024 no longer holds a sample, a node or a kept class per thread"""
    ns = 1025
    reps = fabricate_replicates(ns, 3, 5, 1025)
    got = check(counter, reps, ns, 2)
    assert len(got["nodes"]) > ns // 2
    cross_check(counter, reps, ns, got, bases=1)


def test_one_sample(counter):
    got = dev_consensus(counter, [([], [0]), ([], [0])], 1, 2)
    assert len(got["nodes"]) == 0 and got["order"].tolist() == [0] and got["n_classes"] == 0


def test_the_chain_on_the_planted_corpus(counter):
    """weights, weighted matrices, the trees of all replicates in one call, their consensus: N19, N20 and N21 on the device"""
    ns, n_sites, R = PLANTED_NS, PLANTED_SITES, PLANTED_REPLICATES
    x = planted_chain()
    w = dev_weights(counter, n_sites, R, PLANTED_SEED)
    rep_dist = dev_weighted(counter, x["sites"], x["alleles"], x["g"], ns, w)
    for linkage in LINKAGES:
        trees = dev_rep_trees(counter, rep_dist, tj.LINK_DIFFER, 1, linkage)
        reps = [(t["nodes"], t["order"]) for t in trees]
        for m in (majority(R), R):
            got = check(counter, reps, ns, m, (linkage, m))
        cross_check(counter, reps, ns, check(counter, reps, ns, majority(R)), bases=3)
    # the wrapper, on device pointers, behind tjamd_replicate_trees as it stands
    torch = _torch()
    dd = _dev(rep_dist)
    nodes, order, cn, co, rc_ = (torch.zeros(R * ns * 16, dtype=torch.uint8, device="cuda") for _ in range(5))
    counts, _ = counter.replicate_trees(_p(dd), ns, R, tj.LINK_DIFFER, 1, tj.TREE_SINGLE, None, _p(nodes), _p(order))
    n, n_classes = counter.consensus_tree(_p(nodes), _p(order), counts, ns, majority(R), _p(cn), _p(co), _p(rc_))
    want = restate_consensus(*pack([(t["nodes"], t["order"]) for t in dev_rep_trees(counter, rep_dist, tj.LINK_DIFFER, 1, tj.TREE_SINGLE)], ns), ns, majority(R))
    assert n == len(want["nodes"]) and n_classes == want["n_classes"] and counter.last_consensus_tree_ms() > 0
    assert cn.cpu().numpy()[: n * 16].tobytes() == want["nodes"].tobytes() and co.cpu().numpy()[: ns * 4].tobytes() == want["order"].tobytes()
    print(f"\n[consensus] {ns} samples, {R} replicates: {n} nodes of {n_classes} classes, {counter.last_consensus_tree_ms():.3f} ms in one call")


def caterpillar(ns, from_left):
    return [(0, s) if from_left else (ns - s, s) for s in range(2, ns + 1)]


@pytest.mark.parametrize("ns", [5, 65, 130])
def test_two_caterpillars_in_opposite_directions(counter, ns):
    order = np.random.RandomState(ns).permutation(ns)
    left, right = (caterpillar(ns, True), order), (caterpillar(ns, False), order)
    got = check(counter, [left, right], ns, 2)
    assert as_rows(got["nodes"]) == [(-1, 2, 0, ns)] and got["n_classes"] == 2 * (ns - 1) - 1     # they share the full set alone: a star
    got = check(counter, [left, right, left], ns, 2)
    assert len(got["nodes"]) == ns - 1 and got["nodes"]["parent"].tolist() == list(range(1, ns - 1)) + [-1]
    cross_check(counter, [left, right, left], ns, got)
    assert as_rows(check(counter, [left, right, left], ns, 3)["nodes"]) == [(-1, 3, 0, ns)]


def nested(samples, rng):
    if len(samples) == 1:
        return samples[0]
    cut = rng.randint(1, len(samples))
    return (nested(samples[:cut], rng), nested(samples[cut:], rng))


def laid_out(tree, rng):
    """-> (intervals, order) of the nested pairs with the two children of every node in a random order"""
    order, iv = [], []

    def walk(t):
        if not isinstance(t, tuple):
            order.append(t)
            return
        first = len(order)
        for child in (t if rng.randint(2) else t[::-1]):
            walk(child)
        iv.append((first, len(order) - first))

    walk(tree)
    return iv, order


@pytest.mark.parametrize("ns", [5, 65, 130])
def test_one_tree_under_different_leaf_orders(counter, ns):
    """the same sets at other (first, size) of other orders: every count is R, and the consensus is that tree"""
    rng = np.random.RandomState(7 * ns)
    tree = nested([int(x) for x in rng.permutation(ns)], rng)
    for R in (2, 3, 5):
        reps = [laid_out(tree, rng) for _ in range(R)]
        assert len({tuple(o) for _, o in reps}) > 1
        for m in thresholds(R):
            got = check(counter, reps, ns, m, (ns, R, m))
            assert len(got["nodes"]) == ns - 1 and got["n_classes"] == ns - 1 and (got["nodes"]["count"] == R).all()
            assert all((c == R).all() for c in got["rep_count"])
        cross_check(counter, reps, ns, got, bases=2)


@pytest.mark.parametrize("ns", [9, 70])
def test_forests_empty_replicates_duplicates_and_nodes_out_of_order(counter, ns):
    reps = fabricate_replicates(ns, 5, 1, 900 + ns)
    iv = reps[0][0]
    forest = [n for n in iv if n[1] <= ns // 2]                           # no root: several trees
    twice = (forest + iv[:3])[: ns - 1]                                   # three nodes a second time
    mixed = [(forest, reps[0][1]), (iv, reps[1][1]), ([], reps[2][1]), (twice, reps[3][1]), (iv[::-1], reps[4][1])]     # ... and parents before children
    assert 0 < len(forest) < len(iv) and len(set(twice)) < len(twice)
    for m in thresholds(5):
        got = check(counter, mixed, ns, m, (ns, m))
    cross_check(counter, mixed, ns, check(counter, mixed, ns, 3))
    got = check(counter, [([], reps[0][1]), ([], reps[1][1])], ns, 2)     # no replicate has a node: the identity
    assert len(got["nodes"]) == 0 and got["order"].tolist() == list(range(ns)) and got["n_classes"] == 0


@pytest.mark.parametrize("ns,R,k", [(5, 3, 1), (65, 8, 3), (130, 5, 3)])
def test_the_key_hook(hook_counters, ns, R, k):
    """with no bit of the hash every clade of a size shares a key and the comparison alone tells the sets apart: the same bytes"""
    reps = fabricate_replicates(ns, R, k, CORPUS[(ns, R, k)])
    for m in thresholds(R):
        want = restate_consensus(*pack(reps, ns), ns, m)
        got = [dev_consensus(c, reps, ns, m) for c in hook_counters]
        for g in got:
            same(g, want, (ns, R, m))
            assert g["nodes"].tobytes() == got[-1]["nodes"].tobytes() and g["order"].tobytes() == got[-1]["order"].tobytes()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(g["rep_count"], got[-1]["rep_count"]))


@pytest.mark.parametrize("ns", [9, 70])
def test_device_refusals(counter, ns):
    """each refusal planted in the last replicate: nothing is written, the timer reads -1.0 and the message names the replicate"""
    good = fabricate_replicates(ns, 3, 1, 600 + ns)
    iv, order = good[2]
    twice = order.copy()
    twice[ns - 1] = twice[0]
    crossing = [n for n in iv if n[1] < ns - 2][: ns - 3] + [(1, ns - 2), (2, ns - 2)]
    plants = [((iv, twice), PERMUTATION), ((iv, np.r_[order[:-1], ns].astype(np.int32)), PERMUTATION), ((iv, np.r_[order[:-1], -1].astype(np.int32)), PERMUTATION),
              ((iv[:-1] + [(ns - 1, 2)], order), RANGE), ((iv[:-1] + [(-1, 2)], order), RANGE), ((iv[:-1] + [(3, 1)], order), RANGE), ((iv[:-1] + [(0, ns + 1)], order), RANGE),
              (([(0, 3), (2, 3)], order), CROSS), ((crossing, order), CROSS)]
    for bad, why in plants:
        reps = good[:2] + [bad]
        with pytest.raises(ValueError) as e:
            restate_consensus(*pack(reps, ns), ns, 2)
        assert e.value.replicate == 2 and why in str(e.value)
        rc, err, bufs = dev_consensus(counter, reps, ns, 2)             # (dev_consensus: the buffers and *h_n_classes untouched, the timer at -1.0)
        assert rc == -ERR_ARG and why in err and "replicate 2" in err, (why, rc, err)
        same(dev_consensus(counter, good, ns, 2), restate_consensus(*pack(good, ns), ns, 2), "after a refused call")
    # two refused replicates: the smaller one is named, with its first broken rule
    reps = [good[0], ([(0, 3), (2, 3), (ns, 2)], good[1][1]), plants[0][0]]
    rc, err, _ = dev_consensus(counter, reps, ns, 2)
    assert rc == -ERR_ARG and RANGE in err and "replicate 1" in err, (rc, err)


def test_a_reused_counter_and_optional_outputs():
    shapes = [(130, 5, 3), (9, 5, 1), (257, 7, 4), (65, 8, 3)]
    fresh = []
    for shape in shapes:
        c = tj.Counter(15)
        fresh.append(dev_consensus(c, fabricate_replicates(*shape, CORPUS[shape]), shape[0], majority(shape[1])))
        c.close()
    c = tj.Counter(15)
    try:
        for _ in range(2):
            for shape, want in zip(shapes, fresh):
                reps = fabricate_replicates(*shape, CORPUS[shape])
                same(dev_consensus(c, reps, shape[0], majority(shape[1])), want, shape)
                got = dev_consensus(c, reps, shape[0], majority(shape[1]), null=("rep_count", "classes"))     # both may be NULL: the same tree
                assert got["nodes"].tobytes() == want["nodes"].tobytes() and got["order"].tobytes() == want["order"].tobytes() and got["n_classes"] is None
                cross_check(c, reps, shape[0], want, bases=1)             # tjamd_clade_support on the same scratch in between
    finally:
        c.close()


def test_the_consensus_is_a_tree_for_clade_sites(counter):
    """the consensus nodes and order, cast, are accepted by tjamd_clade_sites: the result of the same intervals as plain nodes"""
    ns, R, k = 65, 8, 3
    got = check(counter, fabricate_replicates(ns, R, k, CORPUS[(ns, R, k)]), ns, majority(R))
    rng = np.random.RandomState(65)
    n_sites = 40
    genotype = rng.randint(-1, 2, (n_sites, ns)).astype(np.int16)
    plain = nodes_of([(int(n["first"]), int(n["size"])) for n in got["nodes"]])
    a = dev_clade_sites(counter, [1] * n_sites, genotype, got["nodes"].view(NODE), got["order"], 1)
    b = dev_clade_sites(counter, [1] * n_sites, genotype, plain, got["order"], 1)
    assert isinstance(a, dict) and isinstance(b, dict) and a["rc"] == b["rc"] >= 0 and a["n_marks"] == b["n_marks"]
    for key in OUTPUTS:
        assert a[key].tobytes() == b[key].tobytes(), key


def consensus_newick(names, nodes, order):
    """the text of consensus_tree.nwk: a root per line, the children in the order of the leaves, an inner node's count as its label"""
    def clade(j):
        first, end = (0, len(order)) if j < 0 else (int(nodes[j]["first"]), int(nodes[j]["first"] + nodes[j]["size"]))
        parts, p = [], first
        while p < end:
            child = [i for i in range(len(nodes)) if nodes[i]["parent"] == j and nodes[i]["first"] == p]
            parts.append(clade(child[0]) if child else names[order[p]])
            p += int(nodes[child[0]]["size"]) if child else 1
        return "".join(x + ";\n" for x in parts) if j < 0 else "(%s)%d" % (",".join(parts), nodes[j]["count"])
    return clade(-1)


def consensus_clades_text(names, nodes, order, R):
    return "".join("%d\t%d\t%d\t%d\t%d\t%s\n" % (j, n["parent"], n["size"], n["count"], R, ",".join(names[s] for s in order[n["first"]: n["first"] + n["size"]]))
                   for j, n in enumerate(nodes))


def test_the_text_of_the_hand_cases():
    reps, ns = three_children()
    want = restate_consensus(*pack(reps, ns), ns, 2)
    names = ["s%d" % i for i in range(ns)]
    assert consensus_newick(names, want["nodes"], want["order"]) == "((s0,s1)3,(s2,s3)2,s4)2;\ns5;\n"
    assert consensus_clades_text(names, want["nodes"], want["order"], 3) == "0\t2\t2\t3\t3\ts0,s1\n1\t2\t2\t2\t3\ts2,s3\n2\t-1\t5\t2\t3\ts0,s1,s2,s3,s4\n"


def test_merged_vcf_c_example_with_the_consensus(pipeline, tmp_path):  # noqa: F811
    p = pipeline
    exe, libdir = str(tmp_path / "merged_vcf"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "merged_vcf.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", exe])
    genome = p["genome"]
    fasta = str(tmp_path / "ref.fa")
    with open(fasta, "w") as fh:
        fh.write(">genome some text\n%s\n" % "\n".join(genome[j: j + 70] for j in range(0, len(genome), 70)))
    files = []
    for smp, s in enumerate(p["streams"]):
        f = str(tmp_path / ("s%d.fq" % smp))
        with open(f, "wb") as fh:
            fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rd, b"I" * len(rd)) for i, rd in enumerate(s.split(b"\n")[:-1])))
        files.append(f)
    names = [os.path.basename(f) for f in files]
    ns, R = p["ns"], 16
    m = restate_merge_variants(p["recs"], ns, p["k"], n_tracts=p["nt"])
    d = restate_site_depths(p["u"].keys, p["u"].mat, p["u"].tracts, p["u"].tract_loc, p["ref"].download(), p["k"], m)
    links = restate_sample_linkage(restate_sample_distances(m["sites"], m["alleles"], d["genotype"]), DIFFER, 1)
    cut = int(links["key"][len(links) // 2])
    common = ["-x", "1", "-k", str(p["k"]), "-m", str(p["m"]), "-c", "5", "-d", "1", "-l", "2"]
    base = ("-D", "-C", str(cut), "-N", "-B", "%d:3" % R)
    written = {}
    for extra in ((), ("-K",), ("-K", "75")):
        out = tmp_path / ("out" + "".join(extra))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, *base, *extra, *common, "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        written[extra] = {name: (out / name).read_text() for name in sorted(os.listdir(out))}
    plain = written[()]
    reps = []
    for dist in restate_sample_distances_weighted(m["sites"], m["alleles"], d["genotype"], restate_bootstrap_weights(len(m["sites"]), R, 3)):
        t = restate_linkage_tree(restate_sample_linkage(dist, DIFFER, 1), ns)
        reps.append((t["nodes"], t["order"]))
    for extra, min_count in ((("-K",), R // 2 + 1), (("-K", "75"), 12)):
        got = written[extra]
        assert sorted(got) == sorted(list(plain) + ["consensus_tree.nwk", "consensus_clades.tsv"])
        for name in plain:
            assert got[name] == plain[name], name                                 # -K leaves the other files as they are, sample_tree.nwk among them
        want = restate_consensus(*pack(reps, ns), ns, min_count)
        assert got["consensus_tree.nwk"] == consensus_newick(names, want["nodes"], want["order"])
        assert got["consensus_clades.tsv"] == consensus_clades_text(names, want["nodes"], want["order"], R)
    for flags in (("-D", "-C", str(cut), "-N", "-K"), base + ("-K", "50"), base + ("-K", "100.5"), ("-D", "-C", str(cut), "-B", "16", "-K")):
        out = tmp_path / ("refused" + "".join(flags).replace(":", "_"))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, *flags, *common, "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stderr.startswith("usage:") and os.listdir(out) == [], flags     # -K without -B R, or a percentage outside (50, 100]
