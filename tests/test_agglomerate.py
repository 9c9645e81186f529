"""tjamd_sample_agglomerate on the GPU against the restatement of tests/test_agglomerate_cabi.py, with no difference allowed in
the links or in the number of rounds: the hand case; fabricated symmetric matrices at sample counts on both sides of every
tile edge of the key pass (32), of the single-workgroup path (64), of a wavefront's 128 cells a step and of the pair kernel's
1024 threads, with keys in 0..3 (ties decide the tree) and over the whole range, with and without missing edges, under both
linkages; all three metrics; equal keys everywhere, whose n_samples - 1 rounds cross a batch of rounds; cliques with no edge
or one missing pair between them; two pairs that merge in one round and whose unions merge in the next; the bound of 2^40
under AVERAGE; every refusal raised on the device; 4096 samples; the links fed to tjamd_linkage_tree and
tjamd_linkage_clusters; the eight-sample pipeline of tests/test_sites.py; and examples/merged_vcf.c -L.  Outputs always sit in
guarded buffers (tests/guarded.py), every input is held frozen, and every call is made twice and must give the same bytes.

The one switch is at 64 samples, up to which the call is one workgroup in one launch; TATAJUBA_AMD_LINKAGE_SMALL=0, read when
the counter is made, sends every call through the key pass, the rounds and the sort kernel, and the cases of 64 samples and
fewer run with a counter of either kind."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, frozen, payload_pattern
from tests.test_agglomerate_cabi import (AVERAGE, COMPLETE, HAND_LINKS, HAND_ROUNDS, KEY_MAX, LINKAGES, cap_for_average, hand_case, replay, restate_sample_agglomerate)
from tests.test_clades import check_tree, dev_tree
from tests.test_clades_cabi import clade_sites_text, newick_text, restate_clade_sites, restate_linkage_tree
from tests.test_depths import dev_depths
from tests.test_depths_cabi import restate_site_depths
from tests.test_distances import dev_distances
from tests.test_distances_cabi import restate_sample_distances
from tests.test_linkage import check_clusters, check_links, clusters_text, dev_clusters, linkage_text
from tests.test_linkage_cabi import DIFFER, DIFFER_RATE, LENGTH, METRICS, as_tuples, fabricate_small, fabricate_wide, restate_linkage_clusters, restate_sample_linkage, symmetric
from tests.test_locate import _dev, _p
from tests.test_sites import dev_merge, pipeline  # noqa: F401  (pipeline: the module-scoped fixture, built here as there)
from tests.test_sites_cabi import restate_merge_variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 3
DIST, LINK = tj.SAMPLE_DISTANCE_DTYPE, tj.LINK_DTYPE
ROUNDS_UNSET = -77


def _torch():
    return pytest.importorskip("torch")


def _rest_untouched(buf, written):
    return bool((buf.payload.cpu().numpy()[written:] == payload_pattern(buf.nbytes)[written:]).all())


def dev_agglomerate(counter, dist, metric, min_both, linkage, on_device=None):
    """two calls of tjamd_sample_agglomerate -> (the links as numpy LINK [n_links], n_rounds); or, when the call is refused,
    (negative code, message, the guarded buffer).  on_device: the matrix where it already is, dist then only gives the shape"""
    torch = _torch()
    L = tj.lib()
    ns = dist.shape[0]
    dd = _dev(dist) if on_device is None else on_device
    runs = []
    for _ in range(2):
        buf = GuardedDevice((ns - 1) * LINK.itemsize)
        rounds = C.c_int(ROUNDS_UNSET)
        torch.cuda.synchronize()
        with frozen(dd):
            rc = L.tjamd_sample_agglomerate(counter._h, _p(dd), ns, metric, min_both, linkage, buf.c, C.byref(rounds))
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        buf.check("d_links")
        if rc < 0:
            assert counter.last_sample_agglomerate_ms() == -1.0 and err.startswith("tjamd_sample_agglomerate") and rounds.value == ROUNDS_UNSET
            return rc, err, buf
        assert 0 <= rc <= ns - 1 and 0 <= rounds.value <= rc and (ns == 1 or counter.last_sample_agglomerate_ms() > 0)
        assert _rest_untouched(buf, rc * LINK.itemsize)                       # entries from n_links on are not written
        runs.append((buf.view(LINK)[:rc], rounds.value))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1] == runs[1][1]   # two runs: the same bytes
    return runs[0]


def check(got, want, what=""):
    assert isinstance(got[0], np.ndarray), (what, got[:2])
    check_links(got[0], want[0])
    assert got[1] == want[1], (what, got[1], want[1])


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(15)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rounds_counter():
    """a counter whose calls never take the single-workgroup path: the key pass, the rounds and the sort kernel at any size"""
    saved = os.environ.get("TATAJUBA_AMD_LINKAGE_SMALL")
    os.environ["TATAJUBA_AMD_LINKAGE_SMALL"] = "0"
    c = tj.Counter(15)
    if saved is None:
        del os.environ["TATAJUBA_AMD_LINKAGE_SMALL"]
    else:
        os.environ["TATAJUBA_AMD_LINKAGE_SMALL"] = saved
    yield c
    c.close()


@pytest.fixture(scope="module", params=["one workgroup up to 64 samples", "rounds at any size"])
def either_counter(request, counter, rounds_counter):
    return counter if request.param.startswith("one") else rounds_counter


def test_hand_case(either_counter):
    counter = either_counter
    d = hand_case()
    for linkage in LINKAGES:
        got = dev_agglomerate(counter, d, DIFFER, 1, linkage)
        assert as_tuples(got[0]) == HAND_LINKS[linkage] and got[1] == HAND_ROUNDS, linkage
        check(got, restate_sample_agglomerate(d, DIFFER, 1, linkage))
        assert dev_agglomerate(counter, d, DIFFER, 11, linkage)[1] == 0       # no pair has that much in common: no link, no round
    # the wrapper, on the same pointers
    torch = _torch()
    dd, out = _dev(d), torch.zeros(3 * LINK.itemsize, dtype=torch.uint8, device="cuda")
    assert counter.sample_agglomerate(_p(dd), 4, tj.LINK_DIFFER, 1, tj.AGGL_AVERAGE, _p(out)) == (3, 2) and counter.last_sample_agglomerate_ms() > 0
    assert as_tuples(out.cpu().numpy().view(LINK)) == HAND_LINKS[AVERAGE]


def four_matrices(ns, rng):
    """(name, matrix, metric, min_both): keys in 0..3 with and without missing edges; keys over the whole range (below 2^40: both
    linkages take them), with a tenth of the pairs missing and with none"""
    small = fabricate_small(ns, rng)
    full = fabricate_small(ns, rng)
    full["n_both"] += 1
    wide = cap_for_average(fabricate_wide(ns, rng))
    wide_full = cap_for_average(fabricate_wide(ns, rng))
    wide_full["n_both"] = np.maximum(wide_full["n_both"], 1)
    return (("small", small, DIFFER, 2), ("small, every pair", full, DIFFER, 1), ("wide", wide, LENGTH, 1), ("wide, every pair", wide_full, LENGTH, 1))


# One workgroup takes 64 samples and fewer where it may (65 is the other side).  The key pass walks tiles of 32 x 32 cells (31, 32,
# 33, 63, 64, 65); a wavefront of the row pass takes 128 cells a step (127, 128, 129) and a row of an odd count carries a padding
# cell; the pair kernel's 1024 threads take one sample each up to 1024 and two at 1025.
COUNTS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]


@pytest.mark.parametrize("ns,kind", [(ns, "default") for ns in COUNTS] + [(ns, "rounds") for ns in COUNTS if ns <= 64])
def test_sample_counts(counter, rounds_counter, ns, kind):
    c = counter if kind == "default" else rounds_counter
    rng = np.random.RandomState(ns)
    n_links = 0
    for name, d, metric, min_both in four_matrices(ns, rng):
        for linkage in LINKAGES:
            want = restate_sample_agglomerate(d, metric, min_both, linkage)
            check(dev_agglomerate(c, d, metric, min_both, linkage), want, (name, linkage))
            assert replay(want[0], ns) is not None
            n_links += len(want[0])
            assert "every pair" not in name or len(want[0]) == ns - 1
    assert n_links >= 4 * (ns - 1)
    if ns > 64:                                           # the whole range of COMPLETE, above the bound of AVERAGE
        d = fabricate_wide(ns, rng)
        check(dev_agglomerate(c, d, LENGTH, 1, COMPLETE), restate_sample_agglomerate(d, LENGTH, 1, COMPLETE))
    elif ns > 1:
        d = fabricate_wide(ns, rng)
        d["n_both"] = np.maximum(d["n_both"], 1)
        got = dev_agglomerate(c, d, LENGTH, 1, COMPLETE)
        check(got, restate_sample_agglomerate(d, LENGTH, 1, COMPLETE))
        assert ns < 31 or int(got[0]["key"].max()) > KEY_MAX


@pytest.mark.parametrize("ns", [33, 65])
def test_all_three_metrics(either_counter, ns):
    rng = np.random.RandomState(1000 + ns)
    for name, d, _, min_both in four_matrices(ns, rng):
        for metric in METRICS:
            for linkage in LINKAGES:
                check(dev_agglomerate(either_counter, d, metric, min_both, linkage), restate_sample_agglomerate(d, metric, min_both, linkage), (name, metric, linkage))


@pytest.mark.parametrize("ns", [33, 65, 257, 64, 66])
def test_equal_keys_take_a_round_per_link(either_counter, ns):
    """everyone's nearest neighbour is cluster 0 and one pair merges a round: n_samples - 1 rounds, more than one batch of them"""
    full = np.ones((ns, ns), np.int64)
    d = symmetric(ns, 3 * full, full - np.eye(ns, dtype=np.int64), 2 * (full - np.eye(ns, dtype=np.int64)))
    for metric, key in ((DIFFER, 1), (LENGTH, 2), (DIFFER_RATE, (1 << 32) // 3)):
        for linkage in LINKAGES:
            links, n_rounds = dev_agglomerate(either_counter, d, metric, 3, linkage)
            assert as_tuples(links) == [(0, b, key) for b in range(1, ns)] and n_rounds == ns - 1, (metric, linkage)
            check((links, n_rounds), restate_sample_agglomerate(d, metric, 3, linkage))


def test_cliques_and_a_missing_pair(either_counter):
    """samples 0..3 and 4..7 with 7 sites in common inside a clique; across the cliques none, then 7 for every pair but (2, 6): one
    missing pair keeps the two apart for good.  Sample 8 has nothing in common with anyone"""
    ns = 9
    rng = np.random.RandomState(9)
    nb = np.zeros((ns, ns), np.int64)
    nb[:4, :4] = 7
    nb[4:8, 4:8] = 7
    nd = rng.randint(1, 5, (ns, ns))
    np.fill_diagonal(nd, 0)
    apart = symmetric(ns, nb, np.minimum(nd, nb), 2 * np.minimum(nd, nb))
    nb[:4, 4:8] = 7
    nb[2, 6] = 0
    nearly = symmetric(ns, nb, np.minimum(nd, nb), 2 * np.minimum(nd, nb))
    nb[2, 6] = 7
    joined = symmetric(ns, nb, np.minimum(nd, nb), 2 * np.minimum(nd, nb))
    for metric in METRICS:
        for linkage in LINKAGES:
            for d, n_links in ((apart, 6), (nearly, 6), (joined, 7)):
                got = dev_agglomerate(either_counter, d, metric, 1, linkage)
                check(got, restate_sample_agglomerate(d, metric, 1, linkage), (metric, linkage, n_links))
                assert len(got[0]) == n_links and all(b < 8 for a, b, k in as_tuples(got[0]))
            roots = replay(dev_agglomerate(either_counter, apart, metric, 1, linkage)[0], ns)
            assert sorted(sorted(m) for m in roots.values()) == [[0, 1, 2, 3], [4, 5, 6, 7], [8]]          # two roots and a sample alone
            roots = replay(dev_agglomerate(either_counter, nearly, metric, 1, linkage)[0], ns)
            assert len(roots) == 3 and not any(2 in m and 6 in m for m in roots.values())


# (s0, s1), (s2, s3), then the four pairs across: the hand case's keys, whose sum over two of the four cells gives the same
# floor as over all four, and keys that rows alone (4 or 6 / 4), columns alone (3 or 5 / 4) and all four cells (50 or 59 / 4) tell apart
CROSS = {"hand case": (0, 1, 3, 2, 1, 1), "one large cell": (0, 0, 2, 3, 4, 50)}


@pytest.mark.parametrize("cross", sorted(CROSS))
@pytest.mark.parametrize("ns,at", [(66, (0, 65, 20, 40)), (66, (64, 65, 3, 33)), (40, (1, 39, 2, 38))])
def test_two_pairs_of_one_round_whose_unions_merge_in_the_next(either_counter, ns, at, cross):
    """four samples planted among samples that are far from everyone: (s0, s1) and (s2, s3) merge in round 0; in round 1 the cell
    of the two unions must hold all four of (s0, s2), (s0, s3), (s1, s2), (s1, s3) -- rows alone, or columns alone, give it two
    of them"""
    s0, s1, s2, s3 = at
    k01, k23, k02, k03, k12, k13 = CROSS[cross]
    rng = np.random.RandomState(ns)
    nd = 1000 + rng.randint(0, 100, (ns, ns))
    for (a, b), v in {(s0, s1): k01, (s2, s3): k23, (s0, s2): k02, (s0, s3): k03, (s1, s2): k12, (s1, s3): k13}.items():
        nd[min(a, b), max(a, b)] = v
    np.fill_diagonal(nd, 0)
    d = symmetric(ns, np.full((ns, ns), 5000), nd, nd)
    first = [(a, b, k) for k, a, b in sorted([(k01, min(s0, s1), max(s0, s1)), (k23, min(s2, s3), max(s2, s3))])]   # one round: by (key, a, b)
    union = tuple(sorted((min(s0, s1), min(s2, s3))))                          # the two unions keep their smaller ids
    for linkage, key in ((AVERAGE, (k02 + k03 + k12 + k13) // 4), (COMPLETE, max(k02, k03, k12, k13))):
        got = dev_agglomerate(either_counter, d, DIFFER, 1, linkage)
        assert as_tuples(got[0])[:3] == first + [(union[0], union[1], key)] and key < 1000, (linkage, as_tuples(got[0])[:4])
        check(got, restate_sample_agglomerate(d, DIFFER, 1, linkage))


def test_the_bound_of_average(either_counter):
    ns = 7
    rng = np.random.RandomState(7)
    ld = rng.randint(0, 1000, (ns, ns)).astype(np.int64)
    ld[2, 5] = KEY_MAX - 1
    d = symmetric(ns, np.full((ns, ns), 9), np.ones((ns, ns)) - np.eye(ns), ld)
    got = dev_agglomerate(either_counter, d, LENGTH, 1, AVERAGE)
    check(got, restate_sample_agglomerate(d, LENGTH, 1, AVERAGE))               # 2^40 - 1 is taken ...
    assert len(got[0]) == ns - 1
    ld[2, 5] = KEY_MAX
    d = symmetric(ns, np.full((ns, ns), 9), np.ones((ns, ns)) - np.eye(ns), ld)
    with pytest.raises(ValueError, match="key"):
        restate_sample_agglomerate(d, LENGTH, 1, AVERAGE)
    rc, err, buf = dev_agglomerate(either_counter, d, LENGTH, 1, AVERAGE)      # ... and 2^40 is not
    assert rc == -ERR_ARG and "a key of 2^40 or more under TJAMD_AGGL_AVERAGE" in err and buf.untouched()
    d["n_both"][2, 5] = d["n_both"][5, 2] = 1                                  # no edge at min_both 2: the cell has no key
    check(dev_agglomerate(either_counter, d, LENGTH, 2, AVERAGE), restate_sample_agglomerate(d, LENGTH, 2, AVERAGE))
    d["n_both"][2, 5] = d["n_both"][5, 2] = 9
    check(dev_agglomerate(either_counter, d, LENGTH, 1, COMPLETE), restate_sample_agglomerate(d, LENGTH, 1, COMPLETE))   # COMPLETE has no such bound
    check(dev_agglomerate(either_counter, d, DIFFER, 1, AVERAGE), restate_sample_agglomerate(d, DIFFER, 1, AVERAGE))     # nor a metric that does not read the cell


@pytest.mark.parametrize("ns", [70, 40])
def test_device_refusals(either_counter, ns):
    """everything tjamd_sample_linkage refuses, at the cells of tests/test_linkage.py: 70 samples are three tile rows of the key
    pass, the last of them ragged; 40 are two, or one workgroup"""
    counter = either_counter
    last = ns - 1
    d = fabricate_small(ns, np.random.RandomState(ns))
    d["n_both"] += 1                                                          # every cell has room under n_both
    want = restate_sample_agglomerate(d, DIFFER, 2, AVERAGE)
    check(dev_agglomerate(counter, d, DIFFER, 2, AVERAGE), want)
    cases = []

    def case(msg, changes):
        bad = d.copy()
        for field, at, value in changes:
            bad[field][at] = value
        cases.append((msg, bad))

    cell, mirror = "a cell has n_both < 0, n_differ < 0, n_differ > n_both or length_diff < 0", "differs from the cell (b, a)"
    for at in ((last, 3), (0, ns - 30), (33, 34)):                            # the last row of the ragged tile; the first row; beside the diagonal
        case(mirror, [("n_both", at, int(d["n_both"][at]) + 1)])
        case(mirror, [("n_differ", at, int(d["n_differ"][at]) + 1)])
        case(mirror, [("length_diff", at, int(d["length_diff"][at]) + 1)])
    for a, b in ((5, ns - 10), (last, last - 1)):                             # bad in the cell and in its mirror alike
        case(cell, [("n_differ", (a, b), int(d["n_both"][a, b]) + 1), ("n_differ", (b, a), int(d["n_both"][a, b]) + 1)])
        for field in DIST.names:
            case(cell, [(field, (a, b), -1), (field, (b, a), -1)])
    case(cell, [("n_both", (last, last), -3)])                                # the diagonal makes no edge and is checked all the same
    case(cell, [("n_differ", (0, 0), int(d["n_both"][0, 0]) + 1)])
    case(cell, [("length_diff", (31, 31), -(1 << 62))])
    for i, (msg, bad) in enumerate(cases):
        linkage = LINKAGES[i % 2]
        with pytest.raises(ValueError):
            restate_sample_agglomerate(bad, DIFFER, 2, linkage)
        rc, err, buf = dev_agglomerate(counter, bad, DIFFER, 2, linkage)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert buf.untouched(), msg                                            # nothing was written
    check(dev_agglomerate(counter, d, DIFFER, 2, AVERAGE), want)               # the counter serves the next good call
    # host refusals with real handles
    torch = _torch()
    L = tj.lib()
    dd, out = _dev(d), torch.zeros(ns * LINK.itemsize, dtype=torch.uint8, device="cuda")
    for args in ((_p(dd), ns, DIFFER, 2, COMPLETE, None), (None, ns, DIFFER, 2, COMPLETE, _p(out)), (_p(dd), ns, 3, 2, COMPLETE, _p(out)), (_p(dd), ns, DIFFER, 0, COMPLETE, _p(out)),
                 (_p(dd), 4097, DIFFER, 2, COMPLETE, _p(out)), (_p(dd), ns, DIFFER, 2, 0, _p(out)), (_p(dd), ns, DIFFER, 2, 3, _p(out))):
        assert L.tjamd_sample_agglomerate(counter._h, *args, None) == -ERR_ARG
    assert not out.any()
    assert L.tjamd_sample_agglomerate(counter._h, _p(dd), 1, DIFFER, 2, AVERAGE, None, None) == 0   # one sample: no link, d_links may be null


@pytest.mark.parametrize("ns", [40, 70])
def test_two_device_refusals_at_once(either_counter, ns):
    """a cell with n_differ > n_both and, elsewhere, a cell that differs from its mirror: the message of the lower error bit"""
    d = fabricate_small(ns, np.random.RandomState(ns))
    d["n_both"] += 1
    bad = d.copy()
    bad["n_differ"][5, ns - 10] = bad["n_differ"][ns - 10, 5] = int(d["n_both"][5, ns - 10]) + 1
    bad["n_both"][ns - 1, 3] += 1
    for linkage in LINKAGES:
        rc, err, buf = dev_agglomerate(either_counter, bad, DIFFER, 2, linkage)
        assert rc == -ERR_ARG and "a cell has n_both < 0, n_differ < 0, n_differ > n_both or length_diff < 0" in err, (linkage, rc, err)
        assert buf.untouched()
    check(dev_agglomerate(either_counter, d, DIFFER, 2, AVERAGE), restate_sample_agglomerate(d, DIFFER, 2, AVERAGE))   # the counter serves the next good call


def test_the_limit_of_samples(counter):
    """4096 samples, COMPLETE, keys over a wide range, once: 2^24 cells, 128 x 128 tiles, a few dozen rounds"""
    torch = _torch()
    ns = 4096
    rng = np.random.RandomState(4096)
    nd = np.triu(rng.randint(0, 1 << 30, (ns, ns), dtype=np.int32), 1)
    d = np.zeros((ns, ns), DIST)
    d["n_both"] = 1 << 30
    d["n_differ"] = nd + nd.T
    d["length_diff"] = d["n_differ"]
    del nd
    want = restate_sample_agglomerate(d, DIFFER, 1, COMPLETE)
    assert len(want[0]) == ns - 1 and 10 < want[1] < 200
    dd = _dev(d)
    got = dev_agglomerate(counter, d, DIFFER, 1, COMPLETE, on_device=dd)
    del dd
    torch.cuda.empty_cache()
    check(got, want)


@pytest.mark.parametrize("ns", [9, 65, 300])
def test_the_links_make_a_tree_and_clusters_on_the_device(counter, ns):
    """tjamd_linkage_tree and tjamd_linkage_clusters take the new links as they take single linkage's"""
    rng = np.random.RandomState(2000 + ns)
    for name, d, metric, min_both in four_matrices(ns, rng)[:2]:
        for linkage in LINKAGES:
            want, _ = restate_sample_agglomerate(d, metric, min_both, linkage)
            links, _ = dev_agglomerate(counter, d, metric, min_both, linkage)
            check_links(links, want)
            check_tree(dev_tree(counter, links, ns), restate_linkage_tree(want, ns), (name, linkage))
            for thr in range(-1, 4):
                labels = restate_linkage_clusters(want, ns, thr)
                check_clusters(dev_clusters(counter, links, ns, thr), labels)
                # the dendrogram cut at thr: the links up to thr are a prefix of the list, and replay as it
                cut = replay(want[want["key"] <= thr], ns)
                assert cut is not None and len(cut) == labels.max() + 1


# ---- the pipeline ----------------------------------------------------------------------------------------------------------

def test_eight_sample_pipeline(pipeline):  # noqa: F811
    p = pipeline
    merger, ref, u, k, ns = p["merger"], p["ref"], p["u"], p["k"], p["ns"]
    want_m = restate_merge_variants(p["recs"], ns, k, n_tracts=p["nt"])
    m = dev_merge(merger, k, p["recs"], ns, p["nt"], want=want_m)
    d = dev_depths(merger, ref, u, m["sites"], m["alleles"])
    dist = dev_distances(merger, m["sites"], m["alleles"], d["genotype"], ns)
    assert dist.tobytes() == restate_sample_distances(m["sites"], m["alleles"], d["genotype"]).tobytes()
    for metric in METRICS:
        for linkage in LINKAGES:
            got = dev_agglomerate(merger, dist, metric, 1, linkage)
            ms = merger.last_sample_agglomerate_ms()
            check(got, restate_sample_agglomerate(dist, metric, 1, linkage), (metric, linkage))
            assert len(got[0]) > 0
            check_tree(dev_tree(merger, got[0], ns), restate_linkage_tree(got[0], ns))
            print(f"\n[agglomerate] metric {metric} linkage {linkage}: {ns} samples, {len(got[0])} links in {got[1]} rounds; tjamd_last_sample_agglomerate_ms {ms:.3f} ms")


def test_merged_vcf_c_example_with_a_linkage(pipeline, tmp_path):  # noqa: F811
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
    ns = p["ns"]
    m = restate_merge_variants(p["recs"], ns, p["k"], n_tracts=p["nt"])
    d = restate_site_depths(p["u"].keys, p["u"].mat, p["u"].tracts, p["u"].tract_loc, p["ref"].download(), p["k"], m)
    dist = restate_sample_distances(m["sites"], m["alleles"], d["genotype"])
    single = restate_sample_linkage(dist, DIFFER, 1)
    cut = int(single["key"][len(single) // 2])
    common = ["-x", "1", "-k", str(p["k"]), "-m", str(p["m"]), "-c", "5", "-d", "1", "-l", "2"]
    written = {}
    for flags in (("-N",), ("-N", "-L", "single"), ("-N", "-L", "average"), ("-N", "-L", "complete"), ("-L", "average")):
        out = tmp_path / ("out" + "".join(flags))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, "-D", "-C", str(cut), *flags, *common, "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        written[flags] = {name: (out / name).read_text() for name in sorted(os.listdir(out))}

    def expected(links):
        tree = restate_linkage_tree(links, ns)
        marks = restate_clade_sites(m["sites"]["n_alleles"], d["genotype"], tree["nodes"], tree["order"], 1)
        return {"sample_linkage.tsv": linkage_text(names, links), "sample_clusters.tsv": clusters_text(names, restate_linkage_clusters(links, ns, cut)),
                "sample_tree.nwk": newick_text(names, links, tree, marks["node_marks"].tolist()), "clade_sites.tsv": clade_sites_text(["genome"], m, marks["marks"])}

    # without -L: what the example tests of N15 and N17 pin, byte for byte; -L single is the same run
    plain = written[("-N",)]
    assert sorted(plain) == ["clade_sites.tsv", "merged.vcf", "sample_clusters.tsv", "sample_distances.tsv", "sample_linkage.tsv", "sample_tree.nwk"]
    for name, text in expected(single).items():
        assert plain[name] == text, name
    assert written[("-N", "-L", "single")] == plain
    for word, linkage in (("average", AVERAGE), ("complete", COMPLETE)):
        links, _ = restate_sample_agglomerate(dist, DIFFER, 1, linkage)
        got = written[("-N", "-L", word)]
        assert sorted(got) == sorted(plain)
        for name, text in expected(links).items():
            assert got[name] == text, (word, name)
        for name in ("merged.vcf", "sample_distances.tsv"):
            assert got[name] == plain[name], (word, name)                         # -L leaves the other files as they are
    assert as_tuples(restate_sample_agglomerate(dist, DIFFER, 1, COMPLETE)[0]) != as_tuples(single)   # (another tree than single linkage's)
    assert written[("-L", "average")] == {n: t for n, t in written[("-N", "-L", "average")].items() if n not in ("sample_tree.nwk", "clade_sites.tsv")}
    for flags in (("-C", str(cut), "-L", "ward"), ("-M", "-L", "average"), ("-C", str(cut), "-L", "Average")):   # another word; -L without -C
        out = tmp_path / ("refused" + "".join(flags))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, "-D", *flags, *common, "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stderr.startswith("usage:") and os.listdir(out) == [], flags
