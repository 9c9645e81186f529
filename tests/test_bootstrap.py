"""tjamd_bootstrap_weights, tjamd_sample_distances_weighted and tjamd_clade_support on the GPU against the restatements of
tests/test_bootstrap_cabi.py, with no difference allowed: the weights at site counts on both sides of a workgroup and replicate
counts on both sides of a wavefront; the weighted distances at sample and site counts on both sides of every tile edge, chunk and
split of tests/test_distances.py, at replicate counts on both sides of the batch a workgroup serves per staged chunk, under
bootstrap weights and under hand weights, at the limits of the number formats and with every refusal raised on the device; the
support on fabricated intervals over random permutations; the whole chain on a planted corpus; and examples/merged_vcf.c -B.
Every output sits in a guarded buffer (tests/guarded.py), every input is held frozen, and every call is made twice and must give
the same bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, frozen
from tests.test_bootstrap_cabi import (SEEDS, clade_support_text, fabricate_support, hand_support_case, nodes_of, restate_bootstrap_weights, restate_clade_support,
                                       restate_sample_distances_weighted, HAND_SUPPORT, HAND_WEIGHTED, HAND_WEIGHTS, as_triples)
from tests.test_clades import check_tree, dev_tree
from tests.test_clades_cabi import clade_sites_text, newick_text, restate_clade_sites, restate_linkage_tree
from tests.test_depths_cabi import restate_site_depths
from tests.test_distances import _counter_aiming_at, check_distances, dev_distances
from tests.test_distances_cabi import fabricate, hand_case, restate_sample_distances
from tests.test_linkage import dev_linkage
from tests.test_linkage_cabi import DIFFER, restate_sample_linkage
from tests.test_locate import _dev, _p
from tests.test_sites import pipeline  # noqa: F401  (the module-scoped fixture, built here as there)
from tests.test_sites_cabi import restate_merge_variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 3
DIST, NODE, LINK = tj.SAMPLE_DISTANCE_DTYPE, tj.TREE_NODE_DTYPE, tj.LINK_DTYPE

with open(os.path.join(ROOT, "tatajuba_amd", "csrc", "hopo_device.hip")) as _src:
    _text = _src.read()
    BATCH = int(re.search(r"^#define SDISTW_BATCH (\d+)\s", _text, re.M).group(1))
    SDIST_CELLS = int(re.search(r"^#define SDIST_CELLS (\d+)\s", _text, re.M).group(1))
assert BATCH == 2                                        # the replicate counts below stand on both sides of it
REPLICATE_COUNTS = (1, BATCH, BATCH + 1, 2 * BATCH + 1)


def _torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(15)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_block_counter():
    """as in tests/test_distances.py: edge 64 beyond 16 samples, the sites never split"""
    c = _counter_aiming_at(1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twelve_block_counter():
    """as in tests/test_distances.py: twelve workgroups aimed at; tile pairs x batches of replicates x slices count against them"""
    c = _counter_aiming_at(12)
    yield c
    c.close()


# ---- the weights ------------------------------------------------------------------------------------------------------------

def dev_weights(counter, n_sites, n_rep, seed):
    torch = _torch()
    L = tj.lib()
    runs = []
    for _ in range(2):
        buf = GuardedDevice(n_rep * n_sites * 4)
        torch.cuda.synchronize()
        rc = L.tjamd_bootstrap_weights(counter._h, n_sites, n_rep, seed, buf.c)
        torch.cuda.synchronize()
        buf.check("d_weights")
        assert rc == n_rep and counter.last_bootstrap_weights_ms() > 0, (rc, L.tjamd_last_error())
        runs.append(buf.view(np.int32).reshape(n_rep, n_sites))
    assert runs[0].tobytes() == runs[1].tobytes()
    return runs[0]


@pytest.mark.parametrize("n_sites", [1, 2, 7, 255, 256, 257, 5000, 100_003])
def test_weights(counter, n_sites):
    for seed in SEEDS:
        want = restate_bootstrap_weights(n_sites, 65, seed)                   # (a shorter call is its prefix)
        for n_rep in (1, 3, 64, 65):
            got = dev_weights(counter, n_sites, n_rep, seed)
            assert got.tobytes() == want[:n_rep].tobytes(), (n_sites, n_rep, seed, np.argwhere(got != want[:n_rep])[:4])
    assert counter.bootstrap_weights(n_sites, 1, -1, GuardedDevice(n_sites * 4).c) == 1       # the wrapper takes any integer as the seed


# ---- the weighted distances -------------------------------------------------------------------------------------------------

def dev_weighted(counter, sites, alleles, genotype, ns, weights):
    """two calls of tjamd_sample_distances_weighted -> DIST [n_replicates, ns, ns]; or, when the call is refused, (negative code,
    message, the guarded buffer)"""
    torch = _torch()
    L = tj.lib()
    n_sites, n_alleles = len(sites), len(alleles)
    weights = np.ascontiguousarray(weights, np.int32)
    weights = weights.reshape(weights.shape[0] if weights.ndim == 2 else -1, n_sites)
    n_rep = len(weights)
    pad = lambda a: _dev(a) if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")
    sd, ad, gd, wd = pad(sites), pad(alleles), pad(np.ascontiguousarray(genotype, np.int16)), pad(weights)
    runs = []
    for _ in range(2):
        buf = GuardedDevice(n_rep * ns * ns * DIST.itemsize)
        torch.cuda.synchronize()
        with frozen(sd, ad, gd, wd):
            rc = L.tjamd_sample_distances_weighted(counter._h, _p(sd), n_sites, _p(ad), n_alleles, _p(gd), ns, buf.c, _p(wd), n_rep)
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        buf.check("d_out")
        if rc < 0:
            assert counter.last_sample_distances_weighted_ms() == -1.0 and err.startswith("tjamd_sample_distances_weighted")
            return rc, err, buf
        assert rc == n_sites and (n_sites == 0 or counter.last_sample_distances_weighted_ms() > 0)
        runs.append(buf.view(DIST).reshape(n_rep, ns, ns))
    assert runs[0].tobytes() == runs[1].tobytes()                             # two runs: the same bytes
    return runs[0]


def check_weighted(got, want, what=""):
    assert isinstance(got, np.ndarray), (what, got[:2])
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in DIST.names:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, (what, f, bad[:5], got[f][tuple(bad[0])], want[f][tuple(bad[0])])
    assert got.tobytes() == want.tobytes(), what


def hand_weights(n_sites, rng):
    """0, 1 and 65 535, every one of them present where there are three sites"""
    w = rng.choice([0, 1, 65535], n_sites)
    w[: min(3, n_sites)] = [0, 1, 65535][: min(3, n_sites)]
    return w


_CORPUS = {}


def corpus(ns, n_sites):
    """sites, alleles, genotypes, 2 * BATCH + 1 rows of weights (bootstrap rows with a hand row in the middle) and the restated
    matrices of all of them, made once per shape: a replicate does not depend on the others, so fewer are a prefix"""
    key = (ns, n_sites)
    if key not in _CORPUS:
        rng = np.random.RandomState(1000 * ns + n_sites)
        sites, alleles, g = fabricate(n_sites, ns, rng)
        w = restate_bootstrap_weights(n_sites, 2 * BATCH + 1, ns).astype(np.int64)
        w[1] = hand_weights(n_sites, rng)
        _CORPUS[key] = (sites, alleles, g, w, restate_sample_distances_weighted(sites, alleles, g, w))
        for x in _CORPUS[key]:
            x.setflags(write=False)
    return _CORPUS[key]


# sample and site counts: tests/test_distances.py says which tile edge, chunk and split each of them reaches
SHAPES = [(1, 1), (3, 256), (8, 257), (5, 5000), (16, 129), (17, 63), (33, 63), (64, 65), (65, 100), (130, 150)]


@pytest.mark.parametrize("n_rep", REPLICATE_COUNTS)
@pytest.mark.parametrize("ns,n_sites", SHAPES)
def test_sample_site_and_replicate_counts(counter, ns, n_sites, n_rep):
    sites, alleles, g, w, want = corpus(ns, n_sites)
    check_weighted(dev_weighted(counter, sites, alleles, g, ns, w[:n_rep]), want[:n_rep])


@pytest.mark.parametrize("n_rep", REPLICATE_COUNTS)
@pytest.mark.parametrize("ns,n_sites", [(17, 63), (65, 100), (130, 150)])
def test_unsplit_tiles_of_edge_64(one_block_counter, ns, n_sites, n_rep):
    sites, alleles, g, w, want = corpus(ns, n_sites)
    check_weighted(dev_weighted(one_block_counter, sites, alleles, g, ns, w[:n_rep]), want[:n_rep])


@pytest.mark.parametrize("n_rep", REPLICATE_COUNTS)
@pytest.mark.parametrize("ns,n_sites", [(130, 150), (33, 63), (5, 5000)])
def test_summed_slices(twelve_block_counter, ns, n_sites, n_rep):
    """twelve workgroups aimed at.  130 samples, 150 sites: up to one batch 6 tile pairs of edge 64 x 2 slices, summed from
    scratch; from two batches on the tile pairs x batches are the twelve and the tiles are stored at once.  33 samples, 63 sites:
    edge 32, one chunk, never split.  5 samples, 5000 sites: edge 8, one tile pair, split at every replicate count, every
    replicate's slices summed by its own row of the summing kernel's grid"""
    sites, alleles, g, w, want = corpus(ns, n_sites)
    check_weighted(dev_weighted(twelve_block_counter, sites, alleles, g, ns, w[:n_rep]), want[:n_rep])


@pytest.mark.parametrize("n_rep", (1, 3))
def test_slices_of_edge_32(twelve_block_counter, n_rep):
    """33 samples, 200 sites: 3 tile pairs of edge 32 x 4 slices for one replicate, x 2 batches x 2 slices for three"""
    sites, alleles, g = fabricate(200, 33, np.random.RandomState(33))
    w = restate_bootstrap_weights(200, n_rep, 5)
    check_weighted(dev_weighted(twelve_block_counter, sites, alleles, g, 33, w), restate_sample_distances_weighted(sites, alleles, g, w))


def test_hand_case(counter):
    sites, alleles, genotype = hand_case()
    got = dev_weighted(counter, sites, alleles, genotype, 3, [HAND_WEIGHTS, [1, 1, 1], [0, 0, 0]])
    assert as_triples(got[0]) == HAND_WEIGHTED and got[2].tobytes() == bytes(9 * DIST.itemsize)
    check_weighted(got, restate_sample_distances_weighted(sites, alleles, genotype, [HAND_WEIGHTS, [1, 1, 1], [0, 0, 0]]))


# one site, and one site more than a chunk (SDIST_CELLS / edge sites), at the edges 8, 16 and 32: the two entries share the
# decomposition, the cut of the scratch and the summing launch, by one slice and by two
EDGE_SHAPES = [(ns, n) for ns, edge in ((2, 8), (9, 16), (17, 32)) for n in (1, SDIST_CELLS // edge + 1)]
assert EDGE_SHAPES == [(2, 1), (2, 257), (9, 1), (9, 129), (17, 1), (17, 65)]


@pytest.mark.parametrize("ns,n_sites", [(3, 256), (17, 63), (65, 100), (130, 150)] + EDGE_SHAPES)
def test_one_replicate_of_ones_is_the_unweighted_matrix(counter, one_block_counter, twelve_block_counter, ns, n_sites):
    """the natural decomposition (a second chunk is a second slice), one workgroup aimed at (never split), and twelve (split
    wherever there are two chunks, 130 samples included)"""
    sites, alleles, g = corpus(ns, n_sites)[:3]
    want = restate_sample_distances(sites, alleles, g)
    for c in (counter, one_block_counter, twelve_block_counter):
        plain = dev_distances(c, sites, alleles, g, ns)
        check_distances(plain, want)
        got = dev_weighted(c, sites, alleles, g, ns, np.ones((1, n_sites), np.int32))
        assert isinstance(got, np.ndarray) and got[0].tobytes() == plain.tobytes()


def test_both_entries_report_the_shared_refusals_alike(counter):
    """each error bit of the check pass that the two entries share (16, 8, 32, 64, 128, 1), raised once on 3 sites x 2 samples
    through both: one code, one text behind the entry's name, nothing written"""
    ns, n_sites = 2, 3
    sites, alleles, g = fabricate(n_sites, ns, np.random.RandomState(5), n_alleles=[2] * n_sites, p_missing=0.0)
    ones = np.ones((1, n_sites), np.int32)
    plain = dev_distances(counter, sites, alleles, g, ns)
    check_distances(plain, restate_sample_distances(sites, alleles, g))
    assert dev_weighted(counter, sites, alleles, g, ns, ones)[0].tobytes() == plain.tobytes()
    cases = [("a site has n_alleles < 1", "sites", "n_alleles", 1, 0),
             ("first_allele and n_alleles of the sites do not chain from 0 to 6", "sites", "first_allele", 1, 3),
             ("an allele's site is not the site that holds it", "alleles", "site", 4, 1),
             ("an allele's alt_length is outside 0..1023", "alleles", "alt_length", 5, 1024),
             ("a site's ref_length is below 0", "sites", "ref_length", 2, -1),
             ("a genotype cell is below -1 or above its site's n_alleles", "genotype", None, (1, 1), -2)]
    for msg, which, field, idx, value in cases:
        s, a, gg = sites.copy(), alleles.copy(), g.copy()
        if which == "genotype":
            gg[idx] = value
        else:
            (s if which == "sites" else a)[field][idx] = value
        with pytest.raises(ValueError):
            restate_sample_distances(s, a, gg)
        texts = []
        for name, got in (("tjamd_sample_distances", dev_distances(counter, s, a, gg, ns)),
                          ("tjamd_sample_distances_weighted", dev_weighted(counter, s, a, gg, ns, ones))):
            rc, err, buf = got
            assert rc == -ERR_ARG and err.startswith(name + ": "), (msg, name, rc, err)
            assert buf.untouched(), (msg, name)                               # nothing was written
            texts.append(err[len(name):])
        assert texts[0] == texts[1] == ": " + msg, (msg, texts)
    assert dev_weighted(counter, sites, alleles, g, ns, ones)[0].tobytes() == plain.tobytes()     # the counter serves the next good call


@pytest.mark.parametrize("ns,n_sites", [(8, 257), (33, 63), (130, 150)])
def test_no_cross_talk_in_a_batch(counter, ns, n_sites):
    sites, alleles, g, w, want = corpus(ns, n_sites)
    together = dev_weighted(counter, sites, alleles, g, ns, w)
    for r in range(len(w)):
        alone = dev_weighted(counter, sites, alleles, g, ns, w[r: r + 1])
        assert alone[0].tobytes() == together[r].tobytes(), r


@pytest.mark.parametrize("ns", [4, 20, 70])
def test_the_largest_weight_on_the_largest_length(counter, one_block_counter, ns):
    """one site of weight 2^31 - 1 with ref_length 2^31 - 1 against an allele of length 0, all other weights 0: (2^31 - 1)^2 in
    length_diff, 2^31 - 1 in n_both and n_differ.  Neither factor fits the 24-bit multiplies: the call takes the exact form"""
    n_sites = 70
    sites, alleles, g = fabricate(n_sites, ns, np.random.RandomState(ns), n_alleles=[1] * n_sites, p_missing=0.1)
    sites["ref_length"][41] = 2 ** 31 - 1
    alleles["alt_length"][41] = 0
    g[41, 0], g[41, 1] = 0, 1
    w = np.zeros((3, n_sites), np.int64)
    w[1, 41] = 2 ** 31 - 1
    w[2] = 1
    want = restate_sample_distances_weighted(sites, alleles, g, w)
    assert tuple(int(v) for v in want[1][0, 1]) == (2 ** 31 - 1, 2 ** 31 - 1, (2 ** 31 - 1) ** 2) and want[0].tobytes() == bytes(ns * ns * DIST.itemsize)
    for c in (counter, one_block_counter):
        check_weighted(dev_weighted(c, sites, alleles, g, ns, w), want)


@pytest.mark.parametrize("ns,weight,top", [(70, 65535, 1800), (20, 65535, 1800), (4, 65535, 1800), (70, 4_000_000, 1023), (20, 4_000_000, 1023), (4, 4_000_000, 1000),
                                           (70, 4_198_404, 1000), (70, 4_198_405, 1000), (70, 1 << 24, 200), (70, 255, (1 << 24) - 1), (70, 255, 1 << 24)])
def test_products_that_fill_32_bits_inside_a_chunk(counter, one_block_counter, ns, weight, top):
    """sites of one large weight with lengths near `top` against alleles of length 0 or 1.  The kernel multiplies in 24 bits and
    sums in 32 between flushes while the call's largest weight and largest length (1023 at least) are below 2^24 and their product
    within 32 bits, and flushes when weight x the chunk's largest length no longer fits what the sums have left: 65 535 x 1 800
    fits 36 times (more than the 32, 16 or 4 sites a thread walks of a chunk: the flush is the one at the chunk's end, and the
    sums of a chunk pass 2^31); 4 000 000 x 1 023 fits once: a flush before every site.  4 198 404 x 1 023 is the last product
    within 32 bits and 4 198 405 x 1 023 the first beyond; 2^24 - 1 and 2^24 as the largest length stand on both sides of the
    24-bit form, and so does 2^24 as a weight."""
    n_sites = 120
    rng = np.random.RandomState(ns + weight % 1000 + top)
    sites, alleles, g = fabricate(n_sites, ns, rng, n_alleles=[2] * n_sites, p_missing=0.05, p_ref=0.5, ref_length=rng.randint(top - 20, top + 1, n_sites))
    alleles["alt_length"] = np.arange(len(alleles)) % 2
    w = np.zeros((3, n_sites), np.int64)
    w[0], w[2] = weight, restate_bootstrap_weights(n_sites, 1, 9)[0]
    w[1, ::3] = weight
    assert w.sum(1).max() < 2 ** 31
    want = restate_sample_distances_weighted(sites, alleles, g, w)
    assert int(want["length_diff"].max()) > 1 << 32
    for c in (counter, one_block_counter):
        check_weighted(dev_weighted(c, sites, alleles, g, ns, w), want)


def test_the_limit_of_a_replicates_sum(counter):
    ns, n_sites = 6, 300
    sites, alleles, g = fabricate(n_sites, ns, np.random.RandomState(2))
    w = np.ones((2, n_sites), np.int64)
    w[1, 7] = 2 ** 31 - 1 - (n_sites - 1)                                     # the sum is 2^31 - 1: accepted
    want = restate_sample_distances_weighted(sites, alleles, g, w)
    check_weighted(dev_weighted(counter, sites, alleles, g, ns, w), want)
    assert int(want["n_both"][1].max()) > 2 ** 31 - 1 - n_sites
    w[1, 299] += 1                                                            # 2^31: refused
    with pytest.raises(ValueError, match="weight sum"):
        restate_sample_distances_weighted(sites, alleles, g, w)
    rc, err, buf = dev_weighted(counter, sites, alleles, g, ns, w)
    assert rc == -ERR_ARG and "the weights of a replicate sum to 2^31 or more" in err and buf.untouched()
    w[1] = 0
    w[1, :2] = 2 ** 30                                                        # two weights that sum to it
    rc, err, buf = dev_weighted(counter, sites, alleles, g, ns, w)
    assert rc == -ERR_ARG and "the weights of a replicate sum to 2^31 or more" in err and buf.untouched()


def test_zero_sites(counter):
    for ns, n_rep in ((1, 1), (5, 3), (70, 2)):
        got = dev_weighted(counter, np.zeros(0, tj.SITE_DTYPE), np.zeros(0, tj.ALLELE_DTYPE), np.zeros((0, ns), np.int16), ns, np.zeros((n_rep, 0), np.int32))
        assert got.tobytes() == bytes(n_rep * ns * ns * DIST.itemsize)


def test_device_refusals(counter):
    ns, n_sites = 6, 40
    sites, alleles, g = fabricate(n_sites, ns, np.random.RandomState(11), n_alleles=[2] * n_sites)
    good = restate_bootstrap_weights(n_sites, 3, 4).astype(np.int64)
    want = restate_sample_distances_weighted(sites, alleles, g, good)
    check_weighted(dev_weighted(counter, sites, alleles, g, ns, good), want)
    cases = []

    def case(msg, cell=None, weight=None, **change):
        """every one of N14's refusals is raised in a site of weight 0 in all replicates"""
        s, a, gg, w = sites.copy(), alleles.copy(), g.copy(), good.copy()
        for name, (idx, value) in change.items():
            which, field = name.split("__")
            (s if which == "sites" else a)[field][idx] = value
            w[:, idx if which == "sites" else idx // 2] = 0
        if cell:
            gg[cell[0], cell[1]] = cell[2]
            w[:, cell[0]] = 0
        if weight:
            w[weight[0], weight[1]] = weight[2]
        cases.append((msg, s, a, gg, w))

    case("a genotype cell is below -1 or above its site's n_alleles", cell=(0, 0, -2))
    case("a genotype cell is below -1 or above its site's n_alleles", cell=(39, 5, 3))
    case("a genotype cell is below -1 or above its site's n_alleles", cell=(17, 2, 32767))
    case("do not chain from 0 to 80", sites__first_allele=(0, 1))
    case("do not chain from 0 to 80", sites__first_allele=(20, 41))
    case("do not chain from 0 to 80", sites__n_alleles=(39, 3))
    case("do not chain from 0 to 80", sites__n_alleles=(5, 1 << 30))
    case("a site has n_alleles < 1", sites__n_alleles=(0, 0))
    case("a site has n_alleles < 1", sites__n_alleles=(9, -2))
    case("an allele's site is not the site that holds it", alleles__site=(4, 1))
    case("an allele's site is not the site that holds it", alleles__site=(79, -1))
    case("an allele's site is not the site that holds it", alleles__site=(0, 1 << 30))
    case("an allele's alt_length is outside 0..1023", alleles__alt_length=(3, 1024))
    case("an allele's alt_length is outside 0..1023", alleles__alt_length=(60, -1))
    case("a site's ref_length is below 0", sites__ref_length=(7, -1))
    case("a weight is below 0", weight=(0, 0, -1))
    case("a weight is below 0", weight=(2, 39, -(2 ** 31)))
    case("a weight is below 0", weight=(1, 20, -5))
    case("the weights of a replicate sum to 2^31 or more", weight=(2, 13, 2 ** 31 - 1))
    for msg, s, a, gg, w in cases:
        with pytest.raises(ValueError):
            restate_sample_distances_weighted(s, a, gg, w)
        rc, err, buf = dev_weighted(counter, s, a, gg, ns, w)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert buf.untouched(), msg                                            # nothing was written
        check_weighted(dev_weighted(counter, sites, alleles, g, ns, good), want)   # the counter serves the next good call
    # the same with the sites split over workgroups: neither the tiles nor the summing kernel may run
    sites, alleles, g = fabricate(3000, ns, np.random.RandomState(12))
    w = restate_bootstrap_weights(3000, 3, 1).astype(np.int64)
    bad_w = w.copy()
    bad_w[2, 2999] = -1
    rc, err, buf = dev_weighted(counter, sites, alleles, g, ns, bad_w)
    assert rc == -ERR_ARG and "a weight is below 0" in err and buf.untouched()
    bad = g.copy()
    bad[2999, 5] = -5
    w0 = w.copy()
    w0[:, 2999] = 0
    rc, err, buf = dev_weighted(counter, sites, alleles, bad, ns, w0)
    assert rc == -ERR_ARG and "a genotype cell" in err and buf.untouched()
    check_weighted(dev_weighted(counter, sites, alleles, g, ns, w), restate_sample_distances_weighted(sites, alleles, g, w))
    # host refusals with real handles; the wrapper
    torch = _torch()
    L = tj.lib()
    sd, ad, gd, wd = _dev(sites), _dev(alleles), _dev(g), _dev(w.astype(np.int32))
    out = torch.zeros(3 * ns * ns * DIST.itemsize, dtype=torch.uint8, device="cuda")
    assert L.tjamd_sample_distances_weighted(counter._h, _p(sd), len(sites), _p(ad), len(alleles), _p(gd), ns, _p(out), None, 3) == -ERR_ARG
    assert L.tjamd_sample_distances_weighted(counter._h, _p(sd), len(sites), _p(ad), len(alleles), _p(gd), ns, _p(out), _p(wd), 0) == -ERR_ARG
    assert counter.sample_distances_weighted(_p(sd), len(sites), _p(ad), len(alleles), _p(gd), ns, _p(out), _p(wd), 3) == len(sites)
    assert counter.last_sample_distances_weighted_ms() > 0
    assert out.cpu().numpy().tobytes() == restate_sample_distances_weighted(sites, alleles, g, w).tobytes()


# ---- the support ------------------------------------------------------------------------------------------------------------

def pack_replicates(reps, ns):
    """-> rep_nodes NODE [R * (ns - 1)], rep_order int32 [R * ns], counts"""
    rep_nodes = np.zeros(len(reps) * max(ns - 1, 0), NODE)
    rep_nodes["first"], rep_nodes["size"] = -7, -7                            # beyond a replicate's count: never read
    rep_order = np.zeros(len(reps) * ns, np.int32)
    counts = []
    for r, (rn, ro) in enumerate(reps):
        rep_nodes[r * (ns - 1): r * (ns - 1) + len(rn)] = rn
        rep_order[r * ns: (r + 1) * ns] = ro
        counts.append(len(rn))
    return rep_nodes, rep_order, counts


def dev_support(counter, nodes, order, reps):
    """two calls of tjamd_clade_support -> int32 [n_nodes]; or, when the call is refused, (negative code, message, the buffer)"""
    torch = _torch()
    L = tj.lib()
    nodes, order = np.ascontiguousarray(nodes, NODE), np.ascontiguousarray(order, np.int32)
    ns = len(order)
    rep_nodes, rep_order, counts = pack_replicates(reps, ns)
    pad = lambda a: _dev(a) if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")
    nd, od = pad(nodes), _dev(order)
    rnd, rod = pad(rep_nodes), _dev(rep_order)
    h_counts = (C.c_int * len(counts))(*counts)
    runs = []
    for _ in range(2):
        buf = GuardedDevice(len(nodes) * 4)
        torch.cuda.synchronize()
        with frozen(nd, od, rnd, rod):
            rc = L.tjamd_clade_support(counter._h, _p(nd), len(nodes), _p(od), ns, _p(rnd), _p(rod), h_counts, len(reps), buf.c)
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        buf.check("d_support")
        if rc < 0:
            assert counter.last_clade_support_ms() == -1.0 and err.startswith("tjamd_clade_support")
            return rc, err, buf
        assert rc == len(nodes) and (len(nodes) == 0 or counter.last_clade_support_ms() > 0)
        runs.append(buf.view(np.int32))
    assert runs[0].tobytes() == runs[1].tobytes()
    return runs[0]


def test_support_on_the_hand_case(counter):
    nodes, order, reps = hand_support_case()
    got = dev_support(counter, nodes, order, reps)
    assert got.tolist() == HAND_SUPPORT
    assert dev_support(counter, nodes[:0], order, reps).tolist() == []        # no node: no kernel, nothing written
    assert dev_support(counter, nodes, order, [(nodes, order)] * 3).tolist() == [3] * 5


@pytest.mark.parametrize("n_rep", [1, 2, 33])
@pytest.mark.parametrize("ns", [2, 3, 64, 65, 130])
def test_support_on_fabricated_intervals(counter, ns, n_rep):
    nodes, order, reps = fabricate_support(ns, n_rep, np.random.RandomState(100 * ns + n_rep))
    want = restate_clade_support(nodes, order, reps)
    got = dev_support(counter, nodes, order, reps)
    assert isinstance(got, np.ndarray) and got.tolist() == want.tolist()
    assert ns < 64 or n_rep < 33 or (0 < want.max() and want.min() < want.max())


def test_support_refusals(counter):
    ns = 9
    nodes, order, reps = fabricate_support(ns, 5, np.random.RandomState(9))
    reps[3] = (nodes_of([(0, 2), (3, 4)]), reps[3][1])
    want = restate_clade_support(nodes, order, reps)
    assert dev_support(counter, nodes, order, reps).tolist() == want.tolist()
    perm, node = "is not a permutation of 0 .. n_samples - 1", "a node has size < 2, first < 0 or first + size above n_samples 9"
    cases = []
    for value in (-1, ns, int(order[0])):                                     # below, above, twice
        o = order.copy(); o[4] = value
        cases.append((perm, nodes, o, reps))
        ro = reps[3][1].copy(); ro[8] = value if value != int(order[0]) else int(ro[0])
        cases.append((perm, nodes, order, reps[:3] + [(reps[3][0], ro)] + reps[4:]))
    for first, size in ((0, 1), (-1, 3), (8, 2), (0, 10), (2, 0), (1 << 30, 1 << 30)):
        bad = nodes.copy(); bad[len(bad) // 2]["first"], bad[len(bad) // 2]["size"] = first, size
        cases.append((node, bad, order, reps))
        rn = reps[3][0].copy(); rn[1]["first"], rn[1]["size"] = first, size
        cases.append((node, nodes, order, reps[:3] + [(rn, reps[3][1])] + reps[4:]))
    for msg, n, o, rr in cases:
        with pytest.raises(ValueError):
            restate_clade_support(n, o, rr)
        rc, err, buf = dev_support(counter, n, o, rr)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert buf.untouched(), msg
        assert dev_support(counter, nodes, order, reps).tolist() == want.tolist()     # the counter serves the next good call
    # the wrapper
    torch = _torch()
    rep_nodes, rep_order, counts = pack_replicates(reps, ns)
    nd, od, rnd, rod = _dev(nodes), _dev(order), _dev(rep_nodes), _dev(rep_order)
    out = torch.zeros(len(nodes) * 4, dtype=torch.uint8, device="cuda")
    assert counter.clade_support(_p(nd), len(nodes), _p(od), ns, _p(rnd), _p(rod), counts, _p(out)) == len(nodes)
    assert counter.last_clade_support_ms() > 0 and out.cpu().numpy().view(np.int32).tolist() == want.tolist()


# ---- end to end -------------------------------------------------------------------------------------------------------------

PLANTED_NS, PLANTED_SITES, PLANTED_REPLICATES, PLANTED_SEED = 12, 120, 40, 1
FAMILY = ([list(range(0, 6)), list(range(6, 12))] + [list(range(0, 4)), list(range(4, 8)), list(range(8, 12))]
          + [[2 * i, 2 * i + 1] for i in range(6)] + [[i] for i in range(12)])   # halves, thirds, pairs, single samples


def nested_family(ns):
    """the halves of 0 .. ns - 1, their halves, and so on down to pairs: the clades of a balanced tree"""
    family = []

    def split(lo, hi):
        if hi - lo < ns:
            family.append(list(range(lo, hi)))
        if hi - lo > 2:
            split(lo, (lo + hi) // 2)
            split((lo + hi) // 2, hi)

    split(0, ns)
    return [f for f in family if len(f) >= 2]


def planted_corpus(ns=PLANTED_NS, n_sites=PLANTED_SITES, family=FAMILY, seed=19):
    """ns samples (12), n_sites sites (120) of one allele each, carried by one clade of the family; 15 % of the cells are missing"""
    rng = np.random.RandomState(seed)
    sites, alleles, g = fabricate(n_sites, ns, rng, n_alleles=[1] * n_sites, p_missing=0.0, p_ref=1.0)
    for i in range(n_sites):
        g[i, family[rng.randint(len(family))]] = 1
    g[rng.random_sample(g.shape) < 0.15] = -1
    return sites, alleles, g


def _single_linkage(dist):
    return restate_sample_linkage(dist, DIFFER, 1)


def planted_distances(ns=PLANTED_NS, n_sites=PLANTED_SITES, R=PLANTED_REPLICATES, seed=PLANTED_SEED, family=FAMILY, corpus_seed=19):
    """the restated chain on a planted corpus up to the replicates' matrices"""
    sites, alleles, g = planted_corpus(ns, n_sites, family, corpus_seed)
    x = {"sites": sites, "alleles": alleles, "g": g, "dist": restate_sample_distances(sites, alleles, g)}
    x["w"] = restate_bootstrap_weights(n_sites, R, seed)
    x["rep_dist"] = restate_sample_distances_weighted(sites, alleles, g, x["w"])
    return x


def planted_trees(x, build=_single_linkage, support=restate_clade_support):
    """the restated chain from the matrices on: the links that `build` makes of a matrix, their trees, and the support of the
    base's clades -> {"base_links", "base", "rep_links", "rep_trees", "support"}"""
    ns = x["dist"].shape[0]
    t = {"base_links": build(x["dist"]), "rep_links": [build(d) for d in x["rep_dist"]]}
    t["base"] = restate_linkage_tree(t["base_links"], ns)
    t["rep_trees"] = [restate_linkage_tree(l, ns) for l in t["rep_links"]]
    t["support"] = support(t["base"]["nodes"], t["base"]["order"], [(r["nodes"], r["order"]) for r in t["rep_trees"]])
    return t


def planted_chain(**corpus):
    """the chain of restatements on the planted corpus, single linkage"""
    x = planted_distances(**corpus)
    x.update(planted_trees(x))
    return x


def test_the_chain_on_a_planted_corpus(counter):
    ns, n_sites, R = PLANTED_NS, PLANTED_SITES, PLANTED_REPLICATES
    x = planted_chain()
    sites, alleles, g, want = x["sites"], x["alleles"], x["g"], x["support"]
    # no empty pass, on the restatement (PLANTED_SEED was picked by this line): a clade in every replicate, and one in some
    assert len(x["base"]["nodes"]) == ns - 1 and want.max() == R and ((want > 0) & (want < R)).any(), want
    got_w = dev_weights(counter, n_sites, R, PLANTED_SEED)
    assert got_w.tobytes() == x["w"].tobytes()
    got_dist = dev_weighted(counter, sites, alleles, g, ns, got_w)
    check_weighted(got_dist, x["rep_dist"])
    dist = dev_distances(counter, sites, alleles, g, ns)
    check_distances(dist, x["dist"])
    tree = dev_tree(counter, dev_linkage(counter, dist, DIFFER, 1), ns)
    check_tree(tree, x["base"])
    reps = []
    for r in range(R):
        links = dev_linkage(counter, got_dist[r], DIFFER, 1)
        assert links.tobytes() == x["rep_links"][r].tobytes(), r
        t = dev_tree(counter, links, ns)
        check_tree(t, x["rep_trees"][r], r)
        reps.append((t["nodes"], t["order"]))
    got = dev_support(counter, tree["nodes"], tree["order"], reps)
    assert got.tolist() == want.tolist()
    print(f"\n[bootstrap] {ns} samples, {n_sites} sites, {R} replicates: support {sorted(want.tolist())}; weighted distances "
          f"{counter.last_sample_distances_weighted_ms():.3f} ms, support {counter.last_clade_support_ms():.3f} ms")


def test_merged_vcf_c_example_with_bootstrap(pipeline, tmp_path):  # noqa: F811
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
    links = restate_sample_linkage(restate_sample_distances(m["sites"], m["alleles"], d["genotype"]), DIFFER, 1)
    cut = int(links["key"][len(links) // 2])
    common = ["-x", "1", "-k", str(p["k"]), "-m", str(p["m"]), "-c", "5", "-d", "1", "-l", "2"]
    written = {}
    for flags in (("-D", "-C", str(cut), "-N"), ("-D", "-C", str(cut), "-N", "-B", "16:3")):
        out = tmp_path / ("out" + "".join(flags).replace(":", "_"))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, *flags, *common, "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        written[flags[4:]] = {name: (out / name).read_text() for name in sorted(os.listdir(out))}
    plain, with_b = written[()], written[("-B", "16:3")]
    assert sorted(with_b) == sorted(list(plain) + ["clade_support.tsv"]) and "clade_support.tsv" not in plain
    for name in plain:
        assert with_b[name] == plain[name], name                                  # -B leaves the other files as they are
    tree = restate_linkage_tree(links, ns)
    marks = restate_clade_sites(m["sites"]["n_alleles"], d["genotype"], tree["nodes"], tree["order"], 1)
    assert with_b["sample_tree.nwk"] == newick_text(names, links, tree, marks["node_marks"].tolist())
    assert with_b["clade_sites.tsv"] == clade_sites_text(["genome"], m, marks["marks"])
    w = restate_bootstrap_weights(len(m["sites"]), 16, 3)
    reps = []
    for dist in restate_sample_distances_weighted(m["sites"], m["alleles"], d["genotype"], w):
        t = restate_linkage_tree(restate_sample_linkage(dist, DIFFER, 1), ns)
        reps.append((t["nodes"], t["order"]))
    support = restate_clade_support(tree["nodes"], tree["order"], reps)
    assert with_b["clade_support.tsv"] == clade_support_text(names, links, tree, marks["node_marks"].tolist(), support.tolist(), 16)
    assert len(with_b["clade_support.tsv"].splitlines()) == len(links) > 0
    for flags in (("-D", "-C", str(cut), "-B", "16:3"), ("-D", "-M", "-N", "-B", "16"), ("-D", "-C", str(cut), "-N", "-B", "0"), ("-D", "-C", str(cut), "-N", "-B", "4097")):
        out = tmp_path / ("refused" + "".join(flags).replace(":", "_"))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, *flags, *common, "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stderr.startswith("usage:") and os.listdir(out) == [], flags     # -B without -C T -N, or a count outside 1 .. 4096
