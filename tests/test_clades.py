"""tjamd_linkage_tree and tjamd_clade_sites on the GPU against the restatements of tests/test_clades_cabi.py, with no difference
allowed: the hand case; chains, reverse chains, balanced trees, random forests with samples alone and no link at all at sample
counts on both sides of a wavefront's 64 lanes (CLD_SMALL), of a wavefront and of the 1024 threads of the workgroup form with
their four positions each, and once at 4096 samples; site counts of 0, 1, on both sides of the CLD_WAVE_SITES sites a workgroup
of the wavefront form is sized for, and one that leaves the last workgroup of the workgroup form a shorter run; every optional
output absent in turn; the capacity of the list at, one under and far under the marks; every refusal raised on the device; a
column of calls and its marks from tjamd_group_sites with the two-group labelling on the device; the eight-sample pipeline of
tests/test_sites.py; and examples/merged_vcf.c -N.  The outputs always sit in guarded buffers (tests/guarded.py), every input is
held frozen, and every call is made twice and must give the same bytes.

The one switch is at 64 samples, up to which a wavefront takes a site; TATAJUBA_AMD_CLADES_SMALL=0, read when the counter is
made, sends every call through the workgroup form with its LDS scans, and every case of 64 samples and fewer runs with a counter
of either kind."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, frozen, payload_pattern
from tests.test_clades_cabi import (HAND_CALLS_1, HAND_GENOTYPE, HAND_LINKS, HAND_MARKS, HAND_N_ALLELES, HAND_NODE_MARKS, HAND_NODES, HAND_ORDER, HAND_SITES, TREE_KINDS, clade_sites_text, links_of,
                                    newick_text, other_links_of, random_matrix, restate_clade_sites, restate_clade_sites_by_groups, restate_clade_sites_sets, restate_linkage_tree, tree_links)
from tests.test_depths import dev_depths
from tests.test_depths_cabi import restate_site_depths
from tests.test_distances import dev_distances
from tests.test_distances_cabi import restate_sample_distances
from tests.test_groups import dev_group_sites, sites_of
from tests.test_groups_cabi import as_tuples
from tests.test_linkage import dev_linkage
from tests.test_linkage_cabi import DIFFER, planted_root_pairs, restate_sample_linkage
from tests.test_locate import _dev, _p
from tests.test_sites import dev_merge, pipeline  # noqa: F401  (pipeline: the module-scoped fixture, built here as there)
from tests.test_sites_cabi import restate_merge_variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAPACITY = 3, 4
LINK, NODE, CALL, GSITE, MARK = tj.LINK_DTYPE, tj.TREE_NODE_DTYPE, tj.GROUP_CALL_DTYPE, tj.GROUP_SITE_DTYPE, tj.GROUP_MARK_DTYPE
OUTPUTS = ("calls", "sites", "node_marks", "marks")

with open(os.path.join(ROOT, "tatajuba_amd", "csrc", "hopo_device.hip")) as _src:
    _text = _src.read()
    CLD_SMALL, CLD_WAVE_SITES, CLD_THREADS = (int(re.search(r"^#define %s (\d+)\s" % name, _text, re.M).group(1)) for name in ("CLD_SMALL", "CLD_WAVE_SITES", "CLD_THREADS"))
assert (CLD_SMALL, CLD_WAVE_SITES, CLD_THREADS) == (64, 64, 1024)     # the sample and site counts below stand on both sides of these


def _torch():
    return pytest.importorskip("torch")


def dev_tree(counter, links, ns):
    """two calls of tjamd_linkage_tree -> {"nodes", "order"} as numpy; or, when the call is refused, (negative code, message, the
    guarded buffers)"""
    torch = _torch()
    L = tj.lib()
    links = np.asarray(links, LINK)
    ld = _dev(links) if len(links) else None
    runs = []
    for _ in range(2):
        bufs = {"nodes": GuardedDevice(len(links) * 16), "order": GuardedDevice(ns * 4)}
        torch.cuda.synchronize()
        with frozen(*([ld] if ld is not None else [])):
            rc = L.tjamd_linkage_tree(counter._h, _p(ld), len(links), ns, bufs["nodes"].c if len(links) else None, bufs["order"].c)
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        for k, b in bufs.items():
            b.check("d_" + k)
        if rc < 0:
            assert counter.last_linkage_tree_ms() == -1.0 and err.startswith("tjamd_linkage_tree")
            return rc, err, bufs
        assert rc == len(links) and counter.last_linkage_tree_ms() > 0
        runs.append({"nodes": bufs["nodes"].view(NODE), "order": bufs["order"].view(np.int32)})
    for k in ("nodes", "order"):
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k                   # two runs: the same bytes
    return runs[0]


def check_tree(got, want, what=""):
    assert isinstance(got, dict), (what, got[:2])
    for k in ("nodes", "order"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k][:8], want[k][:8])


def dev_clade_sites(counter, n_alleles, genotype, nodes, order, min_called, null=(), capacity=None, sites=None):
    """two calls of tjamd_clade_sites -> {"rc", "n_marks", "calls", "sites", "node_marks", "marks", "bufs"} with the outputs as numpy
    (None where the output was not asked for; marks: what lies below the capacity); or, when the call is refused for its
    arguments, (negative code, message, the guarded buffers, *h_n_marks)"""
    torch = _torch()
    L = tj.lib()
    nodes, order = np.ascontiguousarray(nodes, NODE), np.ascontiguousarray(order, np.int32)
    ns, n_sites, n_nodes = len(order), len(n_alleles), len(nodes)
    gt = np.ascontiguousarray(genotype, np.int16).reshape(n_sites, ns)
    sites = sites_of(n_alleles) if sites is None else sites
    pad = lambda a: _dev(a) if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")
    sd, gd, nd, od = pad(sites), pad(gt), pad(nodes), _dev(order)
    cap = n_sites * n_nodes if capacity is None else capacity
    cap_used = 0 if "marks" in null else cap
    runs = []
    for _ in range(2):
        bufs = {"calls": GuardedDevice(n_sites * n_nodes * 16), "sites": GuardedDevice(n_sites * 16), "node_marks": GuardedDevice(n_nodes * 4), "marks": GuardedDevice(cap * 16)}
        ptr = {k: (None if k in null else b.c) for k, b in bufs.items()}
        n_marks = C.c_long(-77)
        torch.cuda.synchronize()
        with frozen(sd, gd, nd, od):
            rc = L.tjamd_clade_sites(counter._h, _p(sd), n_sites, _p(gd), ns, _p(nd), n_nodes, _p(od), min_called, ptr["calls"], ptr["sites"], ptr["node_marks"], ptr["marks"],
                                     cap_used, None if "count" in null else C.byref(n_marks))
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        for k, b in bufs.items():
            b.check("d_" + k)
            assert k not in null or b.untouched(), k
        if rc < 0 and rc != -ERR_CAPACITY:
            assert counter.last_clade_sites_ms() == -1.0 and err.startswith("tjamd_clade_sites")
            return rc, err, bufs, n_marks.value
        assert rc >= 0 or (err.startswith("tjamd_clade_sites") and counter.last_clade_sites_ms() == -1.0)
        assert rc < 0 or n_sites == 0 or n_nodes == 0 or counter.last_clade_sites_ms() > 0
        found = n_marks.value if "count" not in null else rc
        assert "count" in null or (found >= 0 and (rc == found or (rc == -ERR_CAPACITY and found > cap_used)))
        written = min(found, cap_used) if found >= 0 else cap_used
        assert (bufs["marks"].payload.cpu().numpy()[written * 16:] == payload_pattern(bufs["marks"].nbytes)[written * 16:]).all()   # nothing at or beyond
        runs.append({"rc": rc, "n_marks": found, "bufs": bufs,
                     "calls": None if "calls" in null else bufs["calls"].view(CALL).reshape(n_sites, n_nodes),
                     "sites": None if "sites" in null else bufs["sites"].view(GSITE),
                     "node_marks": None if "node_marks" in null else bufs["node_marks"].view(np.int32),
                     "marks": None if "marks" in null else bufs["marks"].view(MARK)[:written]})
    for k in OUTPUTS:
        assert (runs[0][k] is None and runs[1][k] is None) or runs[0][k].tobytes() == runs[1][k].tobytes(), k     # two runs: the same bytes
    assert runs[0]["rc"] == runs[1]["rc"] and runs[0]["n_marks"] == runs[1]["n_marks"]
    return runs[0]


def check(got, want, what=""):
    assert isinstance(got, dict), (what, got[:2])
    assert got["rc"] == got["n_marks"] == len(want["marks"]), (what, got["rc"], got["n_marks"], len(want["marks"]))
    if want["calls"].shape[1] == 0:                                               # no node is no site: nothing is written
        assert got["rc"] == 0 and all(got["bufs"][k].untouched() for k in ("calls", "sites", "marks")), what
        return
    for k in OUTPUTS:
        if got[k] is None:
            continue
        g, w = got[k].reshape(-1), want[k].reshape(-1)
        assert len(g) == len(w), (what, k, len(g), len(w))
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, k, len(bad), int(bad[0]), g[bad[0]], w[bad[0]])
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(15)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scans_counter():
    """a counter whose calls never take the wavefront form: a workgroup and its LDS scans at any size"""
    saved = os.environ.get("TATAJUBA_AMD_CLADES_SMALL")
    os.environ["TATAJUBA_AMD_CLADES_SMALL"] = "0"
    c = tj.Counter(15)
    if saved is None:
        del os.environ["TATAJUBA_AMD_CLADES_SMALL"]
    else:
        os.environ["TATAJUBA_AMD_CLADES_SMALL"] = saved
    yield c
    c.close()


@pytest.fixture(scope="module", params=["a wavefront a site up to 64 samples", "a workgroup a run at any size"])
def either_counter(request, counter, scans_counter):
    return counter if request.param.startswith("a wavefront") else scans_counter


def partial_run_sites():
    """a site count that the workgroup form, two workgroups a compute unit, splits into runs of two with one left for the last"""
    torch = _torch()
    return 2 * 2 * torch.cuda.get_device_properties(0).multi_processor_count - 1


def test_hand_case(either_counter):
    counter = either_counter
    tree = dev_tree(counter, links_of(HAND_LINKS), 7)
    assert as_tuples(tree["nodes"]) == HAND_NODES and tree["order"].tolist() == HAND_ORDER
    four = dev_tree(counter, links_of(HAND_LINKS[:4]), 7)
    assert as_tuples(four["nodes"]) == HAND_NODES[:4] and four["order"].tolist() == HAND_ORDER
    for min_called in (1, 2, 3):
        got = dev_clade_sites(counter, HAND_N_ALLELES, HAND_GENOTYPE, tree["nodes"], tree["order"], min_called)
        assert as_tuples(got["marks"]) == HAND_MARKS[min_called] and got["node_marks"].tolist() == HAND_NODE_MARKS[min_called]
        assert min_called not in HAND_SITES or as_tuples(got["sites"]) == HAND_SITES[min_called]
        check(got, restate_clade_sites_sets(HAND_N_ALLELES, HAND_GENOTYPE, tree["nodes"], tree["order"], min_called), min_called)
    got = dev_clade_sites(counter, HAND_N_ALLELES, HAND_GENOTYPE, tree["nodes"], tree["order"], 1)
    assert [as_tuples(row) for row in got["calls"]] == HAND_CALLS_1
    # intervals that are no tree, over another permutation, more of them than samples
    loose = np.array([(77, -99, 1, 3), (0, 0, 1, 3), (5, 5, 0, 7)] + [(0, 0, f, n) for f in range(6) for n in range(2, 8 - f)] * 4, NODE)
    check(dev_clade_sites(counter, HAND_N_ALLELES, HAND_GENOTYPE, loose, [6, 5, 4, 3, 2, 1, 0], 1), restate_clade_sites_sets(HAND_N_ALLELES, HAND_GENOTYPE, loose, [6, 5, 4, 3, 2, 1, 0], 1))
    assert len(loose) > CLD_SMALL
    # the wrappers, on the same pointers
    torch = _torch()
    ld, sd, gd = _dev(links_of(HAND_LINKS)), _dev(sites_of(HAND_N_ALLELES)), _dev(np.array(HAND_GENOTYPE, np.int16))
    nd, od = torch.zeros(5 * 16, dtype=torch.uint8, device="cuda"), torch.zeros(7, dtype=torch.int32, device="cuda")
    assert counter.linkage_tree(_p(ld), 5, 7, _p(nd), _p(od)) == 5 and counter.last_linkage_tree_ms() > 0
    assert od.cpu().numpy().tolist() == HAND_ORDER and as_tuples(np.frombuffer(nd.cpu().numpy().tobytes(), NODE)) == HAND_NODES
    marks, nm = torch.zeros(4 * 16, dtype=torch.uint8, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")
    assert counter.clade_sites(_p(sd), 5, _p(gd), 7, _p(nd), 5, _p(od), 2, d_node_marks=_p(nm), d_marks=_p(marks), mark_capacity=4) == 3 and counter.last_clade_sites_ms() > 0
    assert nm.cpu().numpy().tolist() == HAND_NODE_MARKS[2]
    assert as_tuples(np.frombuffer(marks.cpu().numpy().tobytes(), MARK)[:3]) == HAND_MARKS[2]
    with pytest.raises(tj.capi.TatajubaAmdError) as e:
        counter.clade_sites(_p(sd), 5, _p(gd), 7, _p(nd), 5, _p(od), 1)          # sized with capacity 0
    assert e.value.n_marks == 4


# A wavefront takes 64 samples and fewer (CLD_SMALL; 1, 2, 3, 63, 64; 65 is the other side), a lane per leaf position.  A thread
# of the workgroup form takes four consecutive positions: 128, 129 are either side of half a wavefront's positions, 1023, 1024,
# 1025 either side of a quarter of the workgroup's, where the nodes (n_samples - 1 of them in a full tree) pass CLD_THREADS.
# The site counts: 63, 64, 65 either side of the CLD_WAVE_SITES sites of a workgroup of the wavefront form (sixteen a wavefront),
# partial_run_sites () for a last workgroup with a shorter run in the workgroup form.
@pytest.mark.parametrize("ns", [1, 2, 3, 63, 64, 65, 128, 129, 1023, 1024, 1025])
def test_trees_sample_and_site_counts(counter, scans_counter, ns):
    rng = np.random.RandomState(ns)
    counters = (counter, scans_counter) if ns <= CLD_SMALL else (counter,)
    site_counts = [40, 200] if ns >= 1023 else [1, 3, CLD_WAVE_SITES - 1, CLD_WAVE_SITES, CLD_WAVE_SITES + 1, partial_run_sites()]
    n_marks = 0
    for at, kind in enumerate(TREE_KINDS):
        want_tree = restate_linkage_tree(tree_links(kind, ns, rng), ns)
        check_tree(dev_tree(counter, tree_links(kind, ns, np.random.RandomState(ns)), ns), restate_linkage_tree(tree_links(kind, ns, np.random.RandomState(ns)), ns), kind)
        tree = dev_tree(counter, other_links_of(want_tree, rng), ns)             # the same tree from ends that the generator did not choose
        check_tree(tree, want_tree, kind)
        for n_sites in ([0] if kind == "none" else []) + site_counts[at % 2::2] + ([site_counts[0]] if ns < 1023 and at % 2 else []):
            na, gt = random_matrix(rng, n_sites, ns, want_tree, max_alleles=4)
            for min_called in (1, 2):
                want = restate_clade_sites(na, gt, want_tree["nodes"], want_tree["order"], min_called)
                n_marks += len(want["marks"])
                for c in counters:
                    check(dev_clade_sites(c, na, gt, tree["nodes"], tree["order"], min_called), want, (kind, n_sites, min_called))
    assert ns < 3 or n_marks > 0



def test_the_limit_of_samples(counter):
    """4096 samples: the chain, 4095 nodes deep, with 40 sites; the reverse chain and the balanced tree as trees"""
    ns = 4096
    rng = np.random.RandomState(ns)
    for kind in ("reverse chain", "balanced", "forest"):
        links = tree_links(kind, ns, rng)
        check_tree(dev_tree(counter, links, ns), restate_linkage_tree(links, ns), kind)
    links = tree_links("chain", ns)
    want_tree = restate_linkage_tree(links, ns)
    tree = dev_tree(counter, links, ns)
    check_tree(tree, want_tree, "chain")
    print(f"\n[clades] tjamd_linkage_tree, chain of {ns} samples: {counter.last_linkage_tree_ms():.3f} ms")
    na, gt = random_matrix(rng, 40, ns, want_tree, max_alleles=5)
    na[3] = 4096
    gt[3] = rng.randint(-1, 4096, ns)
    gt[3, ns - 2:] = 4096                                                         # the last allele a site may have, carried by the clade of the first link alone
    want = restate_clade_sites(na, gt, want_tree["nodes"], want_tree["order"], 2)
    assert len(want["marks"]) >= 3
    check(dev_clade_sites(counter, na, gt, tree["nodes"], tree["order"], 2), want, "chain")
    print(f"[clades] tjamd_clade_sites, 40 sites x {ns} samples x {ns - 1} nodes: {counter.last_clade_sites_ms():.3f} ms, {len(want['marks'])} marks")


@pytest.mark.parametrize("ns", [1023, 1024, 1025, 4096])
def test_trees_with_planted_roots(counter, ns):
    """the roots' places in the order come from a scan over their sizes, four consecutive samples a thread: threads with no root,
    one and four, and a wavefront without any (planted_root_pairs of tests/test_linkage_cabi.py)"""
    links = links_of(planted_root_pairs(ns))
    check_tree(dev_tree(counter, links, ns), restate_linkage_tree(links, ns))


@pytest.mark.parametrize("ns", [7, 130, 1500])
def test_tree_refusals(counter, ns):
    rng = np.random.RandomState(ns)
    good = tree_links("balanced", ns)
    want = restate_linkage_tree(good, ns)
    check_tree(dev_tree(counter, good, ns), want)
    link, cycle = "a link has a < 0, a >= b or b >= n_samples", "a cycle"
    cases = []
    chain = tree_links("chain", ns)
    for at in (1, len(chain) // 2, len(chain) - 1):                               # the earliest link that can close a cycle, one in the middle, the last
        bad = chain.copy()
        bad[at]["a"], bad[at]["b"] = (0, 1) if at == 1 else (0, at)               # both ends in the chain 0 .. at
        cases.append((cycle, "cycle", bad))
    for at in (0, len(good) // 2, len(good) - 1):
        for a, b in ((-1, 3), (2, 2), (3, 2), (0, ns), (ns, ns + 1), (-(1 << 31), 1), (1, (1 << 31) - 1)):
            bad = good.copy()
            bad[at]["a"], bad[at]["b"] = a, b
            cases.append((link, "link", bad))
    for msg, what, bad in cases:
        with pytest.raises(ValueError, match=what):
            restate_linkage_tree(bad, ns)
        rc, err, bufs = dev_tree(counter, bad, ns)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert all(b.untouched() for b in bufs.values()), msg                     # nothing was written
    keyed = good.copy()
    keyed["key"] = rng.randint(-5, 5, len(good))                                  # the key is not read
    check_tree(dev_tree(counter, keyed, ns), want)                                # ... and the counter serves the next good call
    L = tj.lib()
    torch = _torch()
    ld, out = _dev(good), torch.zeros(ns * 16, dtype=torch.uint8, device="cuda")
    for args in ((None, len(good), ns, _p(out), _p(out)), (_p(ld), len(good), ns, None, _p(out)), (_p(ld), len(good), ns, _p(out), None), (_p(ld), ns, ns, _p(out), _p(out)),
                 (_p(ld), -1, ns, _p(out), _p(out)), (_p(ld), 0, 0, _p(out), _p(out)), (_p(ld), 1, 4097, _p(out), _p(out))):
        assert L.tjamd_linkage_tree(counter._h, *args) == -ERR_ARG
    assert not out.any()


@pytest.mark.parametrize("ns", [6, 64, 70])
def test_clade_sites_refusals(either_counter, ns):
    counter = either_counter
    rng = np.random.RandomState(ns)
    n_sites = 37
    tree = restate_linkage_tree(tree_links("forest", ns, rng), ns)
    nodes, order = tree["nodes"], tree["order"]
    na, gt = random_matrix(rng, n_sites, ns, tree)
    na[:] = np.maximum(na, 2)
    want = restate_clade_sites(na, gt, nodes, order, 1)
    check(dev_clade_sites(counter, na, gt, nodes, order, 1), want)
    m_order, m_node = "d_order is not a permutation", "a node has size < 2, first < 0 or first + size above n_samples"
    m_alleles, m_cell = "a site has n_alleles < 1 or above n_samples", "a genotype cell is below -1 or above its site's n_alleles"
    cases = []
    for at, value in ((0, int(order[1])), (ns - 1, int(order[0])), (ns // 2, -1), (ns - 1, ns), (0, 1 << 30)):      # a sample twice (and so one left out); no sample at all
        bad = order.copy(); bad[at] = value
        cases.append((m_order, na, gt, nodes, bad))
    for at in (0, len(nodes) - 1):
        for first, size in ((ns - 1, 2), (0, ns + 1), (1, ns), (0, 1), (0, 0), (-1, 2), (2, -3), (1 << 30, 1 << 30), (1, (1 << 31) - 1)):   # past the end; size 1 and less; before the start
            bad = nodes.copy(); bad[at]["first"], bad[at]["size"] = first, size
            cases.append((m_node, na, gt, bad, order))
    for at in (0, n_sites - 1):
        for value in (0, ns + 1):
            bad = na.copy(); bad[at] = value
            bad_gt = gt.copy(); bad_gt[at] = np.minimum(bad_gt[at], 0)            # (the cells stay within any n_alleles)
            cases.append((m_alleles, bad, bad_gt, nodes, order))
    for at in ((0, 0), (n_sites - 1, ns - 1), (n_sites // 2, 0)):
        for value in (-2, int(na[at[0]]) + 1):
            bad = gt.copy(); bad[at] = value
            cases.append((m_cell, na, bad, nodes, order))
    for msg, a, g, nd, od in cases:
        with pytest.raises(ValueError):
            restate_clade_sites(a, g, nd, od, 1)
        rc, err, bufs, count = dev_clade_sites(counter, a, g, nd, od, 1)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert all(b.untouched() for b in bufs.values()) and count == -77, msg    # nothing was written, *h_n_marks is left alone
    check(dev_clade_sites(counter, na, gt, nodes, order, 1), want)                # the counter serves the next good call
    # host refusals with real handles
    torch = _torch()
    L = tj.lib()
    sd, gd, nd, od = _dev(sites_of(na)), _dev(gt.astype(np.int16)), _dev(nodes), _dev(order)
    out = torch.zeros(n_sites * len(nodes) * 16, dtype=torch.uint8, device="cuda")
    nn = len(nodes)
    for args in ((None, n_sites, _p(gd), ns, _p(nd), nn, _p(od), 1), (_p(sd), n_sites, None, ns, _p(nd), nn, _p(od), 1), (_p(sd), n_sites, _p(gd), ns, None, nn, _p(od), 1),
                 (_p(sd), n_sites, _p(gd), ns, _p(nd), nn, None, 1), (_p(sd), n_sites, _p(gd), 4097, _p(nd), nn, _p(od), 1), (_p(sd), n_sites, _p(gd), ns, _p(nd), -1, _p(od), 1),
                 (_p(sd), n_sites, _p(gd), ns, _p(nd), 4097, _p(od), 1), (_p(sd), n_sites, _p(gd), ns, _p(nd), nn, _p(od), 0), (_p(sd), -1, _p(gd), ns, _p(nd), nn, _p(od), 1)):
        assert L.tjamd_clade_sites(counter._h, *args, _p(out), _p(out), _p(out), _p(out), 1, None) == -ERR_ARG
    assert L.tjamd_clade_sites(counter._h, _p(sd), n_sites, _p(gd), ns, _p(nd), nn, _p(od), 1, None, None, None, None, 1, None) == -ERR_ARG   # a capacity without a list
    assert not out.any()


@pytest.mark.parametrize("ns", [6, 70])
def test_two_clade_sites_refusals_at_once(either_counter, ns):
    """two error bits raised in one call: the message is that of the lowest bit, and nothing is written"""
    rng = np.random.RandomState(ns)
    n_sites = 5
    tree = restate_linkage_tree(tree_links("forest", ns, rng), ns)
    nodes, order = tree["nodes"], tree["order"]
    na, gt = random_matrix(rng, n_sites, ns, tree)
    na[:] = np.maximum(na, 2)
    bad_order = order.copy(); bad_order[ns - 1] = order[0]
    bad_nodes = nodes.copy(); bad_nodes[len(nodes) - 1]["first"], bad_nodes[len(nodes) - 1]["size"] = ns - 1, 2
    bad_cell = gt.copy(); bad_cell[4, ns - 1] = -2
    for msg, g, nd, od in (("d_order is not a permutation", gt, bad_nodes, bad_order),
                           ("a node has size < 2, first < 0 or first + size above n_samples", bad_cell, bad_nodes, order)):
        rc, err, bufs, count = dev_clade_sites(either_counter, na, g, nd, od, 1)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert all(b.untouched() for b in bufs.values()) and count == -77, msg
    check(dev_clade_sites(either_counter, na, gt, nodes, order, 1), restate_clade_sites(na, gt, nodes, order, 1))   # the counter serves the next good call


@pytest.mark.parametrize("ns", [6, 130])
def test_optional_outputs_and_capacity(either_counter, ns):
    counter = either_counter
    rng = np.random.RandomState(ns)
    tree = restate_linkage_tree(tree_links("balanced", ns), ns)
    nodes, order = tree["nodes"], tree["order"]
    na, gt = random_matrix(rng, 40, ns, tree, planted=3)
    want = restate_clade_sites(na, gt, nodes, order, 1)
    n = len(want["marks"])
    assert n >= 3
    for null in (("calls",), ("sites",), ("node_marks",), ("count",), ("calls", "sites", "node_marks")):
        got = dev_clade_sites(counter, na, gt, nodes, order, 1, null=null)
        check(got, want, null)
        assert [k for k in OUTPUTS if got[k] is None] == [k for k in OUTPUTS if k in null]
    check(dev_clade_sites(counter, na, gt, nodes, order, 1, capacity=n), want, "exact fit")
    for cap, null in ((n - 1, ()), (1, ()), (0, ()), (0, ("marks",)), (0, ("calls", "sites", "node_marks", "marks"))):   # one short; a sizing call
        got = dev_clade_sites(counter, na, gt, nodes, order, 1, capacity=cap, null=null)
        assert got["rc"] == -ERR_CAPACITY and got["n_marks"] == n, (cap, null)    # *h_n_marks is the full count
        for k in OUTPUTS[:3]:
            assert got[k] is None or got[k].tobytes() == want[k].tobytes(), (cap, k)   # the other outputs are complete
        assert got["marks"] is None or got["marks"].tobytes() == want["marks"][:cap].tobytes()   # what lies below the capacity is in its place
    got = dev_clade_sites(counter, na, gt, nodes, order, 1, capacity=0, null=("marks", "count", "calls", "sites", "node_marks"))   # nothing but the return value
    assert got["rc"] == -ERR_CAPACITY
    # no mark at all fits a capacity of 0: nobody is called outside any clade
    none = np.full_like(gt, -1)
    got = dev_clade_sites(counter, na, none, nodes, order, 1, capacity=0, null=("marks",))
    assert got["rc"] == 0 and got["n_marks"] == 0
    assert dev_clade_sites(counter, na, none, nodes, order, 1, null=("marks", "count", "calls", "sites", "node_marks"))["rc"] == 0


def test_no_site_and_no_node(either_counter):
    counter = either_counter
    tree = restate_linkage_tree(links_of(HAND_LINKS), 7)
    got = dev_clade_sites(counter, np.zeros(0, np.int64), np.zeros((0, 7), np.int16), tree["nodes"], tree["order"], 1, capacity=4)
    assert got["rc"] == 0 and got["n_marks"] == 0 and got["node_marks"].tolist() == [0] * 5
    assert counter.last_clade_sites_ms() == -1.0                                  # no kernel ran
    for ns in (1, 7):                                                             # no node: a tree of one sample, or no link at all
        t = dev_tree(counter, links_of([]), ns)
        assert t["order"].tolist() == list(range(ns)) and len(t["nodes"]) == 0
        got = dev_clade_sites(counter, [1, 1, 1], np.zeros((3, ns), np.int16), t["nodes"], t["order"], 1, capacity=4)
        assert got["rc"] == 0 and got["n_marks"] == 0 and got["bufs"]["sites"].untouched() and got["bufs"]["marks"].untouched()
        assert counter.last_clade_sites_ms() == -1.0
    L = tj.lib()
    od = _dev(np.arange(7, dtype=np.int32))
    assert L.tjamd_clade_sites(counter._h, None, 0, None, 7, None, 0, _p(od), 1, None, None, None, None, 0, None) == 0


def test_a_node_is_a_group_on_the_device(counter):
    """three nodes of a random tree: tjamd_group_sites with the clade as group 0 and the rest as group 1 gives the node's column
    of d_calls and its marks"""
    ns, n_sites = 90, 120
    rng = np.random.RandomState(90)
    tree = dev_tree(counter, tree_links("forest", ns, rng), ns)
    nodes, order = tree["nodes"], tree["order"]
    na, gt = random_matrix(rng, n_sites, ns, tree, planted=2)
    got = dev_clade_sites(counter, na, gt, nodes, order, 1)
    marked = np.flatnonzero(got["node_marks"])
    assert len(marked) >= 3
    for j in (int(marked[0]), int(marked[len(marked) // 2]), int(marked[-1])):
        labels = np.ones(ns, np.int32)
        labels[order[int(nodes[j]["first"]): int(nodes[j]["first"]) + int(nodes[j]["size"])]] = 0
        by_group = dev_group_sites(counter, na, gt, labels, 2, 1)
        assert by_group["calls"][:, 0].tobytes() == got["calls"][:, j].tobytes(), j
        mine = got["marks"][got["marks"]["group"] == j]
        theirs = by_group["marks"][by_group["marks"]["group"] == 0]
        assert len(mine) == got["node_marks"][j] == by_group["group_marks"][0] > 0
        for k in ("site", "genotype", "n_called"):
            assert mine[k].tolist() == theirs[k].tolist(), (j, k)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------

def test_eight_sample_pipeline(pipeline, scans_counter):  # noqa: F811
    p = pipeline
    merger, ref, u, k, ns = p["merger"], p["ref"], p["u"], p["k"], p["ns"]
    want_m = restate_merge_variants(p["recs"], ns, k, n_tracts=p["nt"])
    m = dev_merge(merger, k, p["recs"], ns, p["nt"], want=want_m)
    d = dev_depths(merger, ref, u, m["sites"], m["alleles"])
    dist = dev_distances(merger, m["sites"], m["alleles"], d["genotype"], ns)
    links = dev_linkage(merger, dist, DIFFER, 1)
    want_tree = restate_linkage_tree(links, ns)
    tree = dev_tree(merger, links, ns)
    check_tree(tree, want_tree)
    for genotype, name in ((d["genotype"], "N13"), (m["genotype"], "N12")):
        for min_called in (1, 2):
            want = restate_clade_sites(m["sites"]["n_alleles"], genotype, want_tree["nodes"], want_tree["order"], min_called)
            assert name != "N13" or all(want[x].tobytes() == y[x].tobytes() for y in (restate_clade_sites_sets(m["sites"]["n_alleles"], genotype, want_tree["nodes"], want_tree["order"], min_called),
                                                                                   restate_clade_sites_by_groups(m["sites"]["n_alleles"], genotype, want_tree["nodes"], want_tree["order"], min_called))
                                        for x in OUTPUTS)
            for c in (merger, scans_counter):
                check(dev_clade_sites(c, m["sites"]["n_alleles"], genotype, tree["nodes"], tree["order"], min_called, sites=m["sites"]), want, (name, min_called))
        print(f"\n[clades] {len(links)} links of {ns} samples, {len(m['sites'])} sites, {len(want['marks'])} marks at min_called 2 ({name}'s genotypes); "
              f"tjamd_last_clade_sites_ms {merger.last_clade_sites_ms():.3f} ms")


def test_merged_vcf_c_example_with_the_tree(pipeline, tmp_path):  # noqa: F811
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
    m = restate_merge_variants(p["recs"], p["ns"], p["k"], n_tracts=p["nt"])
    d = restate_site_depths(p["u"].keys, p["u"].mat, p["u"].tracts, p["u"].tract_loc, p["ref"].download(), p["k"], m)
    links = restate_sample_linkage(restate_sample_distances(m["sites"], m["alleles"], d["genotype"]), DIFFER, 1)
    cut = int(links["key"][len(links) // 2])
    common = ["-x", "1", "-k", str(p["k"]), "-m", str(p["m"]), "-c", "5", "-d", "1", "-l", "2"]
    written = {}
    for flags in (("-D", "-C", str(cut)), ("-D", "-C", str(cut), "-N"), ("-D", "-C", str(cut), "-G", "-N"), ("-D", "-C", str(cut), "-G"), ("-N", "-C", str(cut))):
        out = tmp_path / ("out" + "".join(flags))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, *flags, *common, "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        written[flags] = {name: (out / name).read_text() for name in sorted(os.listdir(out))}
    plain, with_n = written[("-D", "-C", str(cut))], written[("-D", "-C", str(cut), "-N")]
    both, with_g, on_n12 = written[("-D", "-C", str(cut), "-G", "-N")], written[("-D", "-C", str(cut), "-G")], written[("-N", "-C", str(cut))]
    new = ["clade_sites.tsv", "sample_tree.nwk"]
    assert sorted(with_n) == sorted(list(plain) + new) and not set(new) & set(plain) and sorted(both) == sorted(list(with_g) + new)
    for name in plain:
        assert with_n[name] == plain[name], name                                  # -N leaves the other files as they are
    for name in with_g:
        assert both[name] == with_g[name], name
    tree = restate_linkage_tree(links, p["ns"])
    want = restate_clade_sites(m["sites"]["n_alleles"], d["genotype"], tree["nodes"], tree["order"], 1)
    assert len(want["marks"]) > 0
    for files_n in (with_n, both):
        assert files_n["sample_tree.nwk"] == newick_text(names, links, tree, want["node_marks"].tolist())
        assert files_n["clade_sites.tsv"] == clade_sites_text(["genome"], m, want["marks"])
    links12 = restate_sample_linkage(restate_sample_distances(m["sites"], m["alleles"], m["genotype"]), DIFFER, 1)   # without -D: N12's genotypes all the way
    tree12 = restate_linkage_tree(links12, p["ns"])
    want12 = restate_clade_sites(m["sites"]["n_alleles"], m["genotype"], tree12["nodes"], tree12["order"], 1)
    assert on_n12["sample_tree.nwk"] == newick_text(names, links12, tree12, want12["node_marks"].tolist())
    assert on_n12["clade_sites.tsv"] == clade_sites_text(["genome"], m, want12["marks"])
    out = tmp_path / "refused"
    out.mkdir()
    r = subprocess.run([exe, "-r", fasta, "-D", "-M", "-N", *common, "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.startswith("usage:") and os.listdir(out) == []   # -N without -C
