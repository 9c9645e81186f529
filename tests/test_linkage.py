"""tjamd_sample_linkage and tjamd_linkage_clusters on the GPU against the restatements of tests/test_linkage_cabi.py, with no
difference allowed: the hand case, fabricated symmetric matrices at sample counts on both sides of every tile edge of the key
pass (32), of a wavefront's 128 keys a step, of the merge kernel's 1024 threads, with keys in 0..3 (ties decide the tree) and over
the whole range, under all three metrics; the star of equal keys; paths whose components pair up round by round; cliques without
an edge between them; the limits of the number formats; 4096 samples; every refusal raised on the device; lists of links of any
shape; the eight-sample pipeline of tests/test_sites.py; and examples/merged_vcf.c -C.  Outputs always sit in guarded buffers
(tests/guarded.py), every input is held frozen, and every call is made twice and must give the same bytes.

Nothing in either entry depends on the device's size (the grid of every kernel follows from n_samples alone).  The one switch is
at 64 samples, up to which tjamd_sample_linkage runs as one workgroup in one launch; TATAJUBA_AMD_LINKAGE_SMALL=0, read when the
counter is made, sends every call through the key pass, the rounds and the sort kernel, and the cases of 64 samples and fewer
run with a counter of either kind."""
import os
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, frozen, payload_pattern
from tests.test_depths import dev_depths
from tests.test_depths_cabi import restate_site_depths
from tests.test_distances import dev_distances
from tests.test_distances_cabi import restate_sample_distances
from tests.test_linkage_cabi import (ANY_LIST_CLUSTERS, DIFFER, DIFFER_RATE, HAND_CLUSTERS, HAND_LINKS, HAND_LINKS_MIN_BOTH_1, HAND_MIN_BOTH, LENGTH, METRICS, NONE,
                                     _links, any_list, as_tuples, components_of_all_pairs, fabricate_small, fabricate_wide, hand_case, link_keys,
                                     planted_root_pairs, restate_linkage_clusters, restate_sample_linkage, restate_sample_linkage_prim, symmetric)
from tests.test_locate import _dev, _p
from tests.test_sites import dev_merge, pipeline  # noqa: F401  (pipeline: the module-scoped fixture, built here as there)
from tests.test_sites_cabi import restate_merge_variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 3
DIST, LINK = tj.SAMPLE_DISTANCE_DTYPE, tj.LINK_DTYPE


def _torch():
    return pytest.importorskip("torch")


def _rest_untouched(buf, written):
    return bool((buf.payload.cpu().numpy()[written:] == payload_pattern(buf.nbytes)[written:]).all())


def dev_linkage(counter, dist, metric, min_both, on_device=None):
    """two calls of tjamd_sample_linkage -> the links as numpy LINK [n_links]; or, when the call is refused, (negative code,
    message, the guarded buffer).  on_device: the matrix where it already is (a torch tensor), dist then only gives the shape"""
    torch = _torch()
    L = tj.lib()
    ns = dist.shape[0]
    dd = _dev(dist) if on_device is None else on_device
    runs = []
    for _ in range(2):
        buf = GuardedDevice((ns - 1) * LINK.itemsize)
        torch.cuda.synchronize()
        with frozen(dd):
            rc = L.tjamd_sample_linkage(counter._h, _p(dd), ns, metric, min_both, buf.c)
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        buf.check("d_links")
        if rc < 0:
            assert counter.last_sample_linkage_ms() == -1.0 and err.startswith("tjamd_sample_linkage")
            return rc, err, buf
        assert 0 <= rc <= ns - 1 and (ns == 1 or counter.last_sample_linkage_ms() > 0)
        assert _rest_untouched(buf, rc * LINK.itemsize)                       # entries from n_links on are not written
        runs.append(buf.view(LINK)[:rc])
    assert runs[0].tobytes() == runs[1].tobytes()                             # two runs: the same bytes
    return runs[0]


def dev_clusters(counter, links, ns, threshold, null_links=False):
    """two calls of tjamd_linkage_clusters -> (labels int32 [ns], n_clusters); or (negative code, message, the guarded buffer)"""
    torch = _torch()
    L = tj.lib()
    links = np.asarray(links, LINK)
    ld = _dev(links) if len(links) else torch.zeros(64, dtype=torch.uint8, device="cuda")
    runs = []
    for _ in range(2):
        buf = GuardedDevice(ns * 4)
        torch.cuda.synchronize()
        with frozen(ld):
            rc = L.tjamd_linkage_clusters(counter._h, None if null_links else _p(ld), len(links), ns, threshold, buf.c)
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        buf.check("d_cluster")
        if rc < 0:
            assert counter.last_linkage_clusters_ms() == -1.0 and err.startswith("tjamd_linkage_clusters")
            return rc, err, buf
        assert counter.last_linkage_clusters_ms() > 0
        runs.append((buf.view(np.int32), rc))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1] == runs[1][1]
    return runs[0]


def check_links(got, want):
    assert isinstance(got, np.ndarray), got[:2]
    assert len(got) == len(want), (len(got), len(want))
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (bad[:5], got[bad[0]], want[bad[0]])
    assert got.tobytes() == want.tobytes()


def check_clusters(got, want):
    assert isinstance(got[0], np.ndarray), got[:2]
    labels, n = got
    assert labels.tolist() == np.asarray(want).tolist() and n == int(np.max(want)) + 1 and labels[0] == 0


def check_cuts(counter, links, ns, thresholds, want_of):
    for thr in thresholds:
        check_clusters(dev_clusters(counter, links, ns, thr), want_of(thr))


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
    for metric in METRICS:
        got = dev_linkage(counter, d, metric, HAND_MIN_BOTH)
        assert as_tuples(got) == HAND_LINKS[metric], metric
        check_links(got, restate_sample_linkage(d, metric, HAND_MIN_BOTH))
    assert as_tuples(dev_linkage(counter, d, DIFFER, 1)) == HAND_LINKS_MIN_BOTH_1
    assert len(dev_linkage(counter, d, DIFFER, 11)) == 0
    links = dev_linkage(counter, d, DIFFER, HAND_MIN_BOTH)
    for thr, (want, n) in HAND_CLUSTERS.items():
        labels, got_n = dev_clusters(counter, links, 5, thr)
        assert labels.tolist() == want and got_n == n, thr
    # the wrappers, on the same pointers
    torch = _torch()
    dd, out, cl = _dev(d), torch.zeros(4 * LINK.itemsize, dtype=torch.uint8, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")
    assert counter.sample_linkage(_p(dd), 5, tj.LINK_DIFFER, HAND_MIN_BOTH, _p(out)) == 3 and counter.last_sample_linkage_ms() > 0
    assert counter.linkage_clusters(_p(out), 3, 5, 2, _p(cl)) == 3 and counter.last_linkage_clusters_ms() > 0
    assert cl.cpu().numpy().tolist() == HAND_CLUSTERS[2][0]


# One workgroup takes 64 samples and fewer where it may (1, 2, 3, 63, 64; 65 is the other side), a lane per sample, four rows a step.
# The key pass walks tiles of 32 x 32 cells (63, 64, 65: two and three tile rows, whole and ragged); a wavefront of the row pass
# takes 128 keys a step (255, 256, 257) and a row of an odd count carries a padding key (1, 3, 63, 65, 255, 257, 1025); the merge
# kernel's 1024 threads take one sample each up to 1024 and two at 1025.
@pytest.mark.parametrize("ns", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025])
def test_sample_counts(either_counter, ns):
    counter = either_counter
    rng = np.random.RandomState(ns)
    restate = restate_sample_linkage if ns <= 257 else restate_sample_linkage_prim
    small, wide = fabricate_small(ns, rng), fabricate_wide(ns, rng)
    for d, min_both in ((small, 2), (wide, 1)):
        for metric in METRICS:
            want = restate(d, metric, min_both)
            check_links(dev_linkage(counter, d, metric, min_both), want)
    assert ns < 63 or len(want) > ns // 2
    # the tree of the small keys cut either side of every key
    links = restate(small, DIFFER, 2)
    check_cuts(counter, links, ns, range(-1, 4), lambda thr: restate_linkage_clusters(links, ns, thr))
    if 2 < ns <= 65:
        for thr in range(-1, 4):                                               # ... is the cut of the graph of all pairs
            assert restate_linkage_clusters(links, ns, thr).tolist() == components_of_all_pairs(small, DIFFER, 2, thr).tolist()


@pytest.mark.parametrize("ns", [70, 33, 64, 65, 66])
def test_equal_keys_make_the_star(either_counter, ns):
    counter = either_counter
    full = np.ones((ns, ns), np.int64)
    d = symmetric(ns, 3 * full, full - np.eye(ns, dtype=np.int64), 2 * (full - np.eye(ns, dtype=np.int64)))
    for metric, key in ((DIFFER, 1), (LENGTH, 2), (DIFFER_RATE, (1 << 32) // 3)):
        got = dev_linkage(counter, d, metric, 3)
        assert as_tuples(got) == [(0, b, key) for b in range(1, ns)], metric   # the indices alone decide
        check_links(got, restate_sample_linkage(d, metric, 3))


def _path(ns, mirrored):
    """the edge (i, i + 1) has key ctz (i + 1), every other pair a larger one: components pair up once a round.  mirrored: the
    same from the other end, so that the sample left over by every round is the first and not the last"""
    nd = 100 + np.add.outer(np.arange(ns), np.arange(ns)) % 7
    for i in range(ns - 1):
        ctz = ((i + 1) & -(i + 1)).bit_length() - 1
        a, b = (i, i + 1) if not mirrored else (ns - 2 - i, ns - 1 - i)
        nd[a, b] = ctz
    np.fill_diagonal(nd, 0)
    return symmetric(ns, np.full((ns, ns), 1000), nd, 3 * nd)


@pytest.mark.parametrize("ns", [65, 257])
@pytest.mark.parametrize("mirrored", [False, True])
def test_paths_whose_components_pair_up(counter, ns, mirrored):
    """the slowest way to a tree: no round does much better than halve the components"""
    d = _path(ns, mirrored)
    for metric in (DIFFER, LENGTH):
        got = dev_linkage(counter, d, metric, 1)
        check_links(got, restate_sample_linkage(d, metric, 1))
        assert sorted((int(l["a"]), int(l["b"])) for l in got) == [(i, i + 1) for i in range(ns - 1)]   # the path itself


def test_cliques_and_an_isolated_sample(either_counter):
    """samples 0..3 and 4..7 with 7 sites in common inside a clique and none across; (0, 1), the nearest pair, has 5; sample 8 has
    nothing in common with anyone.  min_both 5 keeps (0, 1), 6 drops it, 8 drops every pair"""
    counter = either_counter
    ns = 9
    rng = np.random.RandomState(9)
    nb = np.zeros((ns, ns), np.int64)
    nb[:4, :4] = 7
    nb[4:8, 4:8] = 7
    nb[0, 1] = 5
    nd = np.minimum(rng.randint(1, 5, (ns, ns)), nb)
    nd[0, 1] = 0
    np.fill_diagonal(nd, 0)
    d = symmetric(ns, nb, nd, 2 * nd)
    for metric in METRICS:
        for min_both, n_links, has in ((5, 6, True), (6, 6, False), (7, 6, False), (8, 0, False)):
            got = dev_linkage(counter, d, metric, min_both)
            check_links(got, restate_sample_linkage(d, metric, min_both))
            assert len(got) == n_links and ((0, 1) in [(int(l["a"]), int(l["b"])) for l in got]) == has
            assert all((a < 4) == (b < 4) and b < 8 for a, b, k in as_tuples(got))
    links = dev_linkage(counter, d, DIFFER, 5)
    check_clusters(dev_clusters(counter, links, ns, 1 << 40), [0, 0, 0, 0, 1, 1, 1, 1, 2])


def test_number_limits(either_counter):
    counter = either_counter
    ns = 7
    big, most = (1 << 31) - 1, (1 << 63) - 1
    nb, nd, ld = np.zeros((ns, ns), np.int64), np.zeros((ns, ns), np.int64), np.zeros((ns, ns), np.int64)
    nb[0, 1], nd[0, 1], ld[0, 1] = big, big, most                             # everything at its largest: rate 2^32
    nb[1, 2], nd[1, 2], ld[1, 2] = 2, 1, most - 1                             # 1 of 2 ...
    nb[3, 4], nd[3, 4], ld[3, 4] = 4, 2, most - 1                             # ... beside 2 of 4: equal rates, the indices decide
    nb[2, 3], nd[2, 3], ld[2, 3] = big, big - 1, 0                            # 2^31 - 2 of 2^31 - 1: just under 2^32
    nb[4, 5], nd[4, 5], ld[4, 5] = big, 0, most
    nb[0, 6], nd[0, 6], ld[0, 6] = big - 1, big - 1, 1 << 62
    nb[5, 6], nd[5, 6], ld[5, 6] = big, big, most                             # a tie with (0, 1) at the top of every metric
    np.fill_diagonal(nb, big)
    d = symmetric(ns, nb, nd, ld)
    for metric in METRICS:
        check_links(dev_linkage(counter, d, metric, 1), restate_sample_linkage(d, metric, 1))
        check_links(dev_linkage(counter, d, metric, big), restate_sample_linkage(d, metric, big))
    rate = as_tuples(dev_linkage(counter, d, DIFFER_RATE, 1))
    assert rate[0] == (4, 5, 0) and rate[1:3] == [(1, 2, 1 << 31), (3, 4, 1 << 31)]
    assert (2, 3, ((big - 1) << 32) // big) in rate and rate[-2:] == [(0, 1, 1 << 32), (0, 6, 1 << 32)] and (5, 6, 1 << 32) not in rate   # three at the top: (5, 6), the last, would close the cycle
    length = as_tuples(dev_linkage(counter, d, LENGTH, 1))
    assert length[-2:] == [(0, 1, most), (4, 5, most)] and length[2:4] == [(1, 2, most - 1), (3, 4, most - 1)]
    check_clusters(dev_clusters(counter, _links([(most, 0, 1), (most - 1, 1, 2)]), 3, most - 1), [0, 1, 1])
    check_clusters(dev_clusters(counter, _links([(most, 0, 1), (most - 1, 1, 2)]), 3, most), [0, 0, 0])


def test_the_limit_of_samples(counter):
    """4096 samples: 2^24 cells, 128 x 128 tiles, twelve rounds launched; against Prim, and the tree cut at every key"""
    torch = _torch()
    ns = 4096
    rng = np.random.RandomState(4096)
    nd = rng.randint(0, 4, (ns, ns)).astype(np.int64)
    nd[rng.random_sample((ns, ns)) < 0.9995] = 3                               # few pairs under 3: the cuts at 0, 1 and 2 have many clusters
    np.fill_diagonal(nd, 0)
    d = symmetric(ns, nd + rng.randint(0, 3, (ns, ns)), nd, nd)
    want = restate_sample_linkage_prim(d, DIFFER, 2)
    dd = _dev(d)
    got = dev_linkage(counter, d, DIFFER, 2, on_device=dd)
    del dd
    torch.cuda.empty_cache()
    check_links(got, want)
    for thr in (0, 2, 3):
        labels = restate_linkage_clusters(want, ns, thr)
        check_clusters(dev_clusters(counter, got, ns, thr), labels)
    assert 1 < restate_linkage_clusters(want, ns, 2).max() + 1 < ns


@pytest.mark.parametrize("ns", [70, 40])
def test_device_refusals_of_the_linkage(either_counter, ns):
    """70 samples: three tile rows of the key pass, the last of them ragged (rows 64..69); 40: two, the second ragged, or one workgroup"""
    counter = either_counter
    last = ns - 1
    d = fabricate_small(ns, np.random.RandomState(ns))
    d["n_both"] += 1                                                          # every cell has room under n_both
    want = restate_sample_linkage(d, DIFFER, 2)
    check_links(dev_linkage(counter, d, DIFFER, 2), want)
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
    for a, b in ((5, ns - 10), (last, last - 1)):                                          # bad in the cell and in its mirror alike
        case(cell, [("n_differ", (a, b), int(d["n_both"][a, b]) + 1), ("n_differ", (b, a), int(d["n_both"][a, b]) + 1)])
        for field in DIST.names:
            case(cell, [(field, (a, b), -1), (field, (b, a), -1)])
    case(cell, [("n_both", (last, last), -3)])                                    # the diagonal makes no edge and is checked all the same
    case(cell, [("n_differ", (0, 0), int(d["n_both"][0, 0]) + 1)])
    case(cell, [("length_diff", (31, 31), -(1 << 62))])
    for msg, bad in cases:
        with pytest.raises(ValueError):
            restate_sample_linkage(bad, DIFFER, 2)
        rc, err, buf = dev_linkage(counter, bad, DIFFER, 2)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert buf.untouched(), msg                                            # nothing was written
    check_links(dev_linkage(counter, d, DIFFER, 2), want)                      # the counter serves the next good call
    # host refusals with real handles
    torch = _torch()
    L = tj.lib()
    dd, out = _dev(d), torch.zeros(ns * LINK.itemsize, dtype=torch.uint8, device="cuda")
    for args in ((_p(dd), ns, DIFFER, 2, None), (None, ns, DIFFER, 2, _p(out)), (_p(dd), ns, 3, 2, _p(out)), (_p(dd), ns, DIFFER, 0, _p(out)), (_p(dd), 4097, DIFFER, 2, _p(out))):
        assert L.tjamd_sample_linkage(counter._h, *args) == -ERR_ARG
    assert not out.any()
    assert L.tjamd_sample_linkage(counter._h, _p(dd), 1, DIFFER, 2, None) == 0   # one sample: no link, d_links may be null


@pytest.mark.parametrize("ns", [40, 70])
def test_two_device_refusals_of_the_linkage_at_once(either_counter, ns):
    """a cell with n_differ > n_both and, elsewhere, a cell that differs from its mirror: the message of the lower error bit"""
    d = fabricate_small(ns, np.random.RandomState(ns))
    d["n_both"] += 1
    bad = d.copy()
    bad["n_differ"][5, ns - 10] = bad["n_differ"][ns - 10, 5] = int(d["n_both"][5, ns - 10]) + 1
    bad["n_both"][ns - 1, 3] += 1
    rc, err, buf = dev_linkage(either_counter, bad, DIFFER, 2)
    assert rc == -ERR_ARG and "a cell has n_both < 0, n_differ < 0, n_differ > n_both or length_diff < 0" in err, (rc, err)
    assert buf.untouched()
    check_links(dev_linkage(either_counter, d, DIFFER, 2), restate_sample_linkage(d, DIFFER, 2))   # the counter serves the next good call


@pytest.mark.parametrize("ns", [1023, 1024, 1025, 4096])
def test_cuts_with_planted_roots(counter, ns):
    """the dense ids come from a scan over the roots, four consecutive samples a thread: threads with no root, one and four, and a
    wavefront without any (planted_root_pairs)"""
    links = _links([(1 + j % 2, a, b) for j, (a, b) in enumerate(planted_root_pairs(ns))])
    for thr in (2, 1, 0):
        want = restate_linkage_clusters(links, ns, thr)
        check_clusters(dev_clusters(counter, links, ns, thr), want)
    is_root = np.zeros(ns, bool)
    is_root[np.unique(restate_linkage_clusters(links, ns, 2), return_index=True)[1]] = True   # a component's first sample
    per_thread = np.add.reduceat(is_root, np.arange(0, ns, 4))
    assert {0, 1, 4} <= set(per_thread.tolist()) and not is_root[256:512].any()


def test_cuts_of_any_list_and_their_refusals(counter):
    # unsorted, cyclic, duplicated, longer than n - 1
    links = any_list()
    for thr, want in ANY_LIST_CLUSTERS.items():
        check_clusters(dev_clusters(counter, links, 8, thr), want)
    check_clusters(dev_clusters(counter, links[:0], 3, 7), [0, 1, 2])          # n_links == 0 ...
    check_clusters(dev_clusters(counter, links[:0], 3, 7, null_links=True), [0, 1, 2])   # ... with no list at all
    check_clusters(dev_clusters(counter, links[:0], 1, 0), [0])
    # every pair of a matrix as the list, shuffled: 2 080 links for 65 samples, and the labels follow the smallest member
    ns = 65
    rng = np.random.RandomState(65)
    for d, metric in ((fabricate_small(ns, rng), DIFFER), (fabricate_wide(ns, rng), LENGTH)):
        K = link_keys(d, metric, 1)
        a, b = np.triu_indices(ns, 1)
        every = _links([(int(K[x, y]), int(x), int(y)) for x, y in zip(a, b) if K[x, y] != NONE])
        every = every[rng.permutation(len(every))]
        assert len(every) > ns - 1
        tree = restate_sample_linkage(d, metric, 1)
        keys = sorted(set(int(k) for k in tree["key"]))
        keys = keys if len(keys) <= 6 else keys[:2] + keys[len(keys) // 2: len(keys) // 2 + 2] + keys[-2:]
        for thr in sorted(set([-1] + [k - 1 for k in keys] + keys)):           # either side of every key
            want = restate_linkage_clusters(every, ns, thr)
            check_clusters(dev_clusters(counter, every, ns, thr), want)
            check_clusters(dev_clusters(counter, tree[::-1], ns, thr), want)   # the tree, backwards, cuts to the same
    # a path handed over from its far end: labels have a long way to go
    ns = 300
    chain = _links([(1, i, i + 1) for i in range(ns - 2, -1, -1) if i != 150])
    check_clusters(dev_clusters(counter, chain, ns, 1), [0] * 151 + [1] * 149)
    # refusals: d_cluster untouched, whatever the threshold and wherever the link
    good = any_list()
    for at in (0, 8):
        for a, b, key in ((-1, 2, 0), (2, 2, 0), (3, 2, 0), (0, 8, 0), (0, 1, -1), (0, 1, -(1 << 63))):
            bad = good.copy()
            bad[at] = (a, b, key)
            with pytest.raises(ValueError):
                restate_linkage_clusters(bad, 8, 3)
            for thr in (3, -1):
                rc, err, buf = dev_clusters(counter, bad, 8, thr)
                assert rc == -ERR_ARG and "a link has a < 0, a >= b, b >= n_samples or key < 0" in err, (a, b, key, rc, err)
                assert buf.untouched()
    check_clusters(dev_clusters(counter, good, 8, 2), ANY_LIST_CLUSTERS[2])
    torch = _torch()
    L = tj.lib()
    ld, out = _dev(good), torch.zeros(8, dtype=torch.int32, device="cuda")
    for args in ((_p(ld), 9, 8, 2, None), (None, 9, 8, 2, _p(out)), (_p(ld), -1, 8, 2, _p(out)), (_p(ld), (1 << 24) + 1, 8, 2, _p(out)), (_p(ld), 9, 0, 2, _p(out))):
        assert L.tjamd_linkage_clusters(counter._h, *args) == -ERR_ARG
    assert not out.any()


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
        links = dev_linkage(merger, dist, metric, 1)
        ms = merger.last_sample_linkage_ms()
        check_links(links, restate_sample_linkage(dist, metric, 1))
        assert len(links) > 0
        keys = sorted(set(int(x) for x in links["key"]))
        for thr in sorted(set([-1] + [x - 1 for x in keys] + keys)):
            want = restate_linkage_clusters(links, ns, thr)
            check_clusters(dev_clusters(merger, links, ns, thr), want)
            assert want.tolist() == components_of_all_pairs(dist, metric, 1, thr).tolist()
        print(f"\n[linkage] metric {metric}: {ns} samples, keys {keys[0]} .. {keys[-1]}; tjamd_last_sample_linkage_ms {ms:.3f} ms, "
              f"tjamd_last_linkage_clusters_ms {merger.last_linkage_clusters_ms():.3f} ms")


def linkage_text(sample_names, links):
    return "".join("%s\t%s\t%d\n" % (sample_names[l["a"]], sample_names[l["b"]], l["key"]) for l in links)


def clusters_text(sample_names, labels):
    return "".join("%s\t%d\n" % (name, c) for name, c in zip(sample_names, labels))


def test_merged_vcf_c_example_with_clusters(pipeline, tmp_path):  # noqa: F811
    p = pipeline
    exe, libdir = str(tmp_path / "merged_vcf"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "merged_vcf.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", exe])
    genome = p["genome"]
    fasta = str(tmp_path / "ref.fa")
    with open(fasta, "w") as fh:
        fh.write(">genome some text\n%s\n" % "\n".join(genome[j: j + 70] for j in range(0, len(genome), 70)))
    files, samples = [], []
    for smp, s in enumerate(p["streams"]):
        f = str(tmp_path / ("s%d.fq" % smp))
        with open(f, "wb") as fh:
            fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rd, b"I" * len(rd)) for i, rd in enumerate(s.split(b"\n")[:-1])))
        files.append(f); samples.append("s%d.fq" % smp)
    m = restate_merge_variants(p["recs"], p["ns"], p["k"], n_tracts=p["nt"])
    d = restate_site_depths(p["u"].keys, p["u"].mat, p["u"].tracts, p["u"].tract_loc, p["ref"].download(), p["k"], m)
    dist = restate_sample_distances(m["sites"], m["alleles"], d["genotype"])
    links = restate_sample_linkage(dist, DIFFER, 1)
    cut = int(links["key"][len(links) // 2])                                   # a threshold inside the tree's keys
    written = {}
    for flags in (("-D", "-M"), ("-D", "-C", str(cut)), ("-D", "-M", "-C", "-1")):
        out = tmp_path / ("out" + "".join(flags))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, *flags, "-x", "1", "-k", str(p["k"]), "-m", str(p["m"]), "-c", "5", "-d", "1", "-l", "2", "-o", str(out)] + files,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        written[flags] = {name: (out / name).read_text() for name in sorted(os.listdir(out))}
    plain, with_cut, all_apart = written[("-D", "-M")], written[("-D", "-C", str(cut))], written[("-D", "-M", "-C", "-1")]
    assert sorted(plain) == ["merged.vcf", "sample_distances.tsv"]            # without -C: the files of before ...
    assert sorted(with_cut) == ["merged.vcf", "sample_clusters.tsv", "sample_distances.tsv", "sample_linkage.tsv"]   # (-C implies -M)
    for name in plain:
        assert with_cut[name] == plain[name] and all_apart[name] == plain[name], name   # ... and -C leaves them as they are
    assert with_cut["sample_linkage.tsv"] == linkage_text(samples, links) == all_apart["sample_linkage.tsv"]
    labels = restate_linkage_clusters(links, p["ns"], cut)
    assert with_cut["sample_clusters.tsv"] == clusters_text(samples, labels) and 1 <= labels.max() + 1 < p["ns"]
    assert all_apart["sample_clusters.tsv"] == clusters_text(samples, range(p["ns"]))
