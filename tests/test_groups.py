"""tjamd_group_sites on the GPU against the restatements of tests/test_groups_cabi.py, with no difference allowed: the hand case;
random and planted matrices at sample counts on both sides of a wavefront's 64 lanes, of the 256 and 1024 samples a pass of the
workgroup form takes, and at 4096 samples with the last entry of every table in use; one group, everyone alone, a group without
members, nobody taking part; min_called at and one above a group's called members; every optional output absent in turn; the
capacity of the list at, one under and far under the marks; every refusal raised on the device; no site at all; the eight-sample
pipeline of tests/test_sites.py with the clusters of every cut of its tree; and examples/merged_vcf.c -G.  The four outputs
always sit in guarded buffers (tests/guarded.py), every input is held frozen, and every call is made twice and must give the
same bytes.

The one switch is at 64 samples, up to which a wavefront takes a site; TATAJUBA_AMD_GROUPS_SMALL=0, read when the counter is
made, sends every call through the workgroup form with its LDS tables, and every case of 64 samples and fewer runs with a
counter of either kind.  The workgroup form gives a workgroup a run of sites, two workgroups a compute unit: the site counts
include one that leaves the last workgroup a shorter run."""
import ctypes as C
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
from tests.test_groups_cabi import (HAND_CALL_3_0, HAND_CALLS_SITE_2, HAND_GENOTYPE, HAND_GROUP, HAND_GROUP_MARKS, HAND_MARKS, HAND_N_ALLELES, HAND_SITES_2, as_tuples,
                                    random_case, restate_group_sites, restate_group_sites_table, same_result)
from tests.test_linkage import dev_linkage
from tests.test_linkage_cabi import DIFFER, restate_linkage_clusters, restate_sample_linkage
from tests.test_locate import _dev, _p
from tests.test_sites import dev_merge, pipeline  # noqa: F401  (pipeline: the module-scoped fixture, built here as there)
from tests.test_sites_cabi import restate_merge_variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAPACITY = 3, 4
SITE, CALL, GSITE, MARK = tj.SITE_DTYPE, tj.GROUP_CALL_DTYPE, tj.GROUP_SITE_DTYPE, tj.GROUP_MARK_DTYPE
OUTPUTS = ("calls", "sites", "group_marks", "marks")


def _torch():
    return pytest.importorskip("torch")


def sites_of(n_alleles):
    """site records of which the entry reads n_alleles alone; the rest carries a pattern that no count could be"""
    s = np.zeros(len(n_alleles), SITE)
    for name in SITE.names:
        s[name] = 0x7ffffff9
    s["n_alleles"] = n_alleles
    return s


def dev_group_sites(counter, n_alleles, genotype, group, n_groups, min_called, null=(), capacity=None, sites=None):
    """two calls of tjamd_group_sites -> {"rc", "n_marks", "calls", "sites", "group_marks", "marks", "bufs"} with the outputs as numpy
    (None where the output was not asked for; marks: what lies below the capacity); or, when the call is refused for its
    arguments, (negative code, message, the guarded buffers, *h_n_marks).  capacity: that of d_marks, by default a site's
    largest possible count times the sites"""
    torch = _torch()
    L = tj.lib()
    group = np.ascontiguousarray(group, np.int32)
    ns, n_sites = len(group), len(n_alleles)
    gt = np.ascontiguousarray(genotype, np.int16).reshape(n_sites, ns)
    sites = sites_of(n_alleles) if sites is None else sites
    pad = lambda a: _dev(a) if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")
    sd, gd, ld = pad(sites), pad(gt), _dev(group)
    cap = n_sites * min(ns, n_groups) if capacity is None else capacity
    cap_used = 0 if "marks" in null else cap
    runs = []
    for _ in range(2):
        bufs = {"calls": GuardedDevice(n_sites * n_groups * 16), "sites": GuardedDevice(n_sites * 16), "group_marks": GuardedDevice(n_groups * 4),
                "marks": GuardedDevice(cap * 16)}
        ptr = {k: (None if k in null else b.c) for k, b in bufs.items()}
        n_marks = C.c_long(-77)
        torch.cuda.synchronize()
        with frozen(sd, gd, ld):
            rc = L.tjamd_group_sites(counter._h, _p(sd), n_sites, _p(gd), ns, _p(ld), n_groups, min_called, ptr["calls"], ptr["sites"], ptr["group_marks"], ptr["marks"],
                                     cap_used, None if "count" in null else C.byref(n_marks))
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        for k, b in bufs.items():
            b.check("d_" + k)
            assert k not in null or b.untouched(), k
        if rc < 0 and rc != -ERR_CAPACITY:
            assert counter.last_group_sites_ms() == -1.0 and err.startswith("tjamd_group_sites")
            return rc, err, bufs, n_marks.value
        assert rc >= 0 or (err.startswith("tjamd_group_sites") and counter.last_group_sites_ms() == -1.0)
        assert rc < 0 or n_sites == 0 or counter.last_group_sites_ms() > 0
        found = n_marks.value if "count" not in null else rc
        assert "count" in null or (found >= 0 and (rc == found or (rc == -ERR_CAPACITY and found > cap_used)))
        written = min(found, cap_used) if found >= 0 else cap_used
        assert (bufs["marks"].payload.cpu().numpy()[written * 16:] == payload_pattern(bufs["marks"].nbytes)[written * 16:]).all()   # nothing at or beyond
        out = {"rc": rc, "n_marks": found, "bufs": bufs,
               "calls": None if "calls" in null else bufs["calls"].view(CALL).reshape(n_sites, n_groups),
               "sites": None if "sites" in null else bufs["sites"].view(GSITE),
               "group_marks": None if "group_marks" in null else bufs["group_marks"].view(np.int32),
               "marks": None if "marks" in null else bufs["marks"].view(MARK)[:written]}
        runs.append(out)
    for k in OUTPUTS:
        assert (runs[0][k] is None and runs[1][k] is None) or runs[0][k].tobytes() == runs[1][k].tobytes(), k     # two runs: the same bytes
    assert runs[0]["rc"] == runs[1]["rc"] and runs[0]["n_marks"] == runs[1]["n_marks"]
    return runs[0]


def check(got, want, what=""):
    assert isinstance(got, dict), (what, got[:2])
    assert got["rc"] == got["n_marks"] == len(want["marks"]), (what, got["rc"], got["n_marks"], len(want["marks"]))
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
def tables_counter():
    """a counter whose calls never take the wavefront form: a workgroup and its LDS tables at any size"""
    saved = os.environ.get("TATAJUBA_AMD_GROUPS_SMALL")
    os.environ["TATAJUBA_AMD_GROUPS_SMALL"] = "0"
    c = tj.Counter(15)
    if saved is None:
        del os.environ["TATAJUBA_AMD_GROUPS_SMALL"]
    else:
        os.environ["TATAJUBA_AMD_GROUPS_SMALL"] = saved
    yield c
    c.close()


@pytest.fixture(scope="module", params=["a wavefront a site up to 64 samples", "a workgroup a run at any size"])
def either_counter(request, counter, tables_counter):
    return counter if request.param.startswith("a wavefront") else tables_counter


def partial_run_sites():
    """a site count that the workgroup form, two workgroups a compute unit, splits into runs of two with one left for the last"""
    torch = _torch()
    return 2 * 2 * torch.cuda.get_device_properties(0).multi_processor_count - 1


def plant(na, gt, group):
    """site 0: the group of the last sample carries the site's last allele and nobody else does (random cells mark nothing once
    the groups are large)"""
    if group[-1] >= 0:
        gt[0, gt[0] == na[0]] = 0
        gt[0, group == group[-1]] = na[0]


def test_hand_case(either_counter):
    counter = either_counter
    for min_called in (1, 2, 3):
        got = dev_group_sites(counter, HAND_N_ALLELES, HAND_GENOTYPE, HAND_GROUP, 3, min_called)
        assert as_tuples(got["marks"]) == HAND_MARKS[min_called] and got["group_marks"].tolist() == HAND_GROUP_MARKS[min_called]
        check(got, restate_group_sites(HAND_N_ALLELES, HAND_GENOTYPE, HAND_GROUP, 3, min_called), min_called)
    got = dev_group_sites(counter, HAND_N_ALLELES, HAND_GENOTYPE, HAND_GROUP, 3, 2)
    assert as_tuples(got["sites"]) == HAND_SITES_2 and as_tuples(got["calls"][2]) == HAND_CALLS_SITE_2 and as_tuples(got["calls"][3])[0] == HAND_CALL_3_0
    # the wrapper, on the same pointers
    torch = _torch()
    sd, gd, ld = _dev(sites_of(HAND_N_ALLELES)), _dev(np.array(HAND_GENOTYPE, np.int16)), _dev(np.array(HAND_GROUP, np.int32))
    marks, gm = torch.zeros(4 * 16, dtype=torch.uint8, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    assert counter.group_sites(_p(sd), 5, _p(gd), 6, _p(ld), 3, 2, d_group_marks=_p(gm), d_marks=_p(marks), mark_capacity=4) == 2 and counter.last_group_sites_ms() > 0
    assert gm.cpu().numpy().tolist() == HAND_GROUP_MARKS[2]
    assert as_tuples(np.frombuffer(marks.cpu().numpy().tobytes(), MARK)[:2]) == HAND_MARKS[2]
    with pytest.raises(tj.capi.TatajubaAmdError) as e:
        counter.group_sites(_p(sd), 5, _p(gd), 6, _p(ld), 3, 1)                  # sized with capacity 0
    assert e.value.n_marks == 3


# A wavefront takes 64 samples and fewer where it may (1, 2, 8, 63, 64; 65 is the other side), a lane per sample.  A thread of
# the workgroup form takes samples tid, tid + 1024, ...: 255, 256, 257 are either side of four wavefronts, 1000 leaves the last
# wavefront of the first pass ragged; the groups go the same way, so n_groups == n_samples walks the same edges there.
@pytest.mark.parametrize("ns", [1, 2, 8, 63, 64, 65, 255, 256, 257, 1000])
def test_sample_and_site_counts(counter, tables_counter, ns):
    rng = np.random.RandomState(ns)
    counters = (counter, tables_counter) if ns <= 64 else (counter,)
    n_marks = 0
    for n_sites in (1, 3, 257, partial_run_sites()):
        groupings = [("one group", 1, None), ("everyone alone", ns, rng.permutation(ns)), ("a group without members", min(ns, 5) + 1, None),
                     ("more groups than samples", 2 * ns + 3, None)]
        for what, n_groups, labels in groupings if n_sites <= 3 else groupings[1:3] if n_sites == 257 else groupings[:3]:
            na, gt, group = random_case(rng, n_sites, ns, n_groups, empty_group=what.startswith("a group without"), max_alleles=4)
            if labels is not None:
                group = labels
            plant(na, gt, group)
            if what.startswith("a group without") and ns > 1:
                assert not (group == n_groups // 2).any()
            for min_called in (1, 2):
                want = restate_group_sites_table(na, gt, group, n_groups, min_called)
                if n_sites <= 3 and ns <= 65:
                    assert same_result(want, restate_group_sites(na, gt, group, n_groups, min_called))
                n_marks += len(want["marks"])
                for c in counters:
                    check(dev_group_sites(c, na, gt, group, n_groups, min_called), want, (what, n_sites, min_called))
    assert ns < 8 or n_marks > 0
    # nobody takes part: every call empty, no mark
    na, gt, group = random_case(rng, 3, ns, 4)
    for c in counters:
        got = dev_group_sites(c, na, gt, np.full(ns, -1), 4, 1)
        check(got, restate_group_sites(na, gt, np.full(ns, -1), 4, 1), "all -1")
        assert got["rc"] == 0 and as_tuples(got["calls"].reshape(-1)) == [(0, -1, 0, 0)] * 12 and as_tuples(got["sites"]) == [(0, 0, 0, -1)] * 3


def test_the_limit_of_samples(counter):
    """4096 samples x 16 sites; a site with 4096 alleles and a cell that carries the 4096th, group 4095 marked: the last entry of
    the genotype table and of the group table"""
    ns, n_sites = 4096, 16
    rng = np.random.RandomState(4096)
    na, gt, _ = random_case(rng, n_sites, ns, 1, max_alleles=5)
    na[3] = 4096
    gt[3] = rng.randint(-1, 4096, ns)
    group = rng.permutation(ns)                                                   # everyone alone
    carrier = int(np.flatnonzero(group == 4095)[0])
    gt[3, carrier] = 4096                                                         # the only carrier of the last allele
    gt[3, (carrier + 1) % ns] = 7
    want = restate_group_sites_table(na, gt, group, ns, 1)
    assert (3, 4095, 4096, 1) in as_tuples(want["marks"])
    check(dev_group_sites(counter, na, gt, group, ns, 1), want, "alone")
    few = rng.randint(0, 7, ns)
    few[rng.random_sample(ns) < 0.1] = -1
    gt[5] = np.where(few == 4, 2, np.where(rng.random_sample(ns) < 0.5, 0, 1))    # group 4 fixed on an allele nobody else carries
    na[5] = 2
    want = restate_group_sites_table(na, gt, few, 7, 3)
    assert (5, 4) in [m[:2] for m in as_tuples(want["marks"])]
    check(dev_group_sites(counter, na, gt, few, 7, 3), want, "seven groups")


@pytest.mark.parametrize("ns", [8, 64, 70])
def test_planted_rows(either_counter, ns):
    """rows whose marks are known by construction.  Group 1 has three members (samples 1, 3, 5); sample 0 takes no part"""
    counter = either_counter
    group = np.arange(ns) % 2
    group[[1, 3, 5]], group[[2, 4, 6]] = 1, 0
    group[7:] = np.where(np.arange(7, ns) % 3 == 0, 2, 0)
    group[0] = -1
    n_groups = 4                                                                  # group 3 has no members
    members = np.array([1, 3, 5])
    base = np.where(np.arange(ns) % 5 == 0, -1, 0)                                # everyone else: the genome's length, or not called
    base[2] = 0                                                                   # (an outsider that is called)
    rows, marked = [], []

    def row(what, values, is_marked, outsider=None):
        r = base.copy()
        r[members] = values
        if outsider is not None:
            r[outsider[0]] = outsider[1]
        rows.append(r); marked.append((what, is_marked))

    row("a private fixed allele", [2, 2, 2], True)
    row("the same with one outside carrier", [2, 2, 2], False, (2, 2))
    row("the same carried by a sample that takes no part", [2, 2, 2], True, (0, 2))
    row("a mixed group", [2, 1, 2], False)
    row("one member not called: two called, min_called 3", [2, -1, 2], False)
    row("fixed on the genome's length, which others carry", [0, 0, 0], False)
    only = np.full(ns, -1)
    only[members] = 1
    rows.append(only); marked.append(("only one group is called", False))
    gt = np.array(rows)
    na = np.full(len(rows), 2)
    want = restate_group_sites_table(na, gt, group, n_groups, 3)
    assert same_result(want, restate_group_sites(na, gt, group, n_groups, 3))
    for i, (what, is_marked) in enumerate(marked):
        assert bool(want["calls"][i, 1]["mark"]) == is_marked, what
    assert as_tuples(want["calls"][6])[1] == (3, 1, 0, 0) and want["calls"][4, 1]["fixed"] == 2 and want["calls"][3, 1]["fixed"] == -2
    check(dev_group_sites(counter, na, gt, group, n_groups, 3), want)
    want2 = restate_group_sites_table(na, gt, group, n_groups, 2)                 # exactly min_called called members
    assert want2["calls"][4, 1]["mark"] == 1 and want2["calls"][4, 1]["n_called"] == 2
    check(dev_group_sites(counter, na, gt, group, n_groups, 2), want2)


@pytest.mark.parametrize("ns", [6, 130])
def test_optional_outputs_and_capacity(either_counter, ns):
    counter = either_counter
    rng = np.random.RandomState(ns)
    na, gt, group = random_case(rng, 40, ns, 5)
    for i in range(0, 40, 3):                                                     # marks by construction: group i % 5 alone carries the site's last allele
        gt[i, gt[i] == na[i]] = 0
        gt[i, group == i % 5] = na[i]
    want = restate_group_sites_table(na, gt, group, 5, 1)
    n = len(want["marks"])
    assert n >= 3
    for null in (("calls",), ("sites",), ("group_marks",), ("count",), ("calls", "sites", "group_marks")):
        got = dev_group_sites(counter, na, gt, group, 5, 1, null=null)
        check(got, want, null)
        assert [k for k in OUTPUTS if got[k] is None] == [k for k in OUTPUTS if k in null]
    check(dev_group_sites(counter, na, gt, group, 5, 1, capacity=n), want, "exact fit")
    for cap, null in ((n - 1, ()), (1, ()), (0, ()), (0, ("marks",)), (0, ("calls", "sites", "group_marks", "marks"))):   # one short; a sizing call
        got = dev_group_sites(counter, na, gt, group, 5, 1, capacity=cap, null=null)
        assert got["rc"] == -ERR_CAPACITY and got["n_marks"] == n, (cap, null)    # *h_n_marks is the full count
        for k in OUTPUTS[:3]:
            assert got[k] is None or got[k].tobytes() == want[k].tobytes(), (cap, k)   # the other outputs are complete
        assert got["marks"] is None or got["marks"].tobytes() == want["marks"][:cap].tobytes()   # what lies below the capacity is in its place
    got = dev_group_sites(counter, na, gt, group, 5, 1, capacity=0, null=("marks", "count", "calls", "sites", "group_marks"))   # nothing but the return value
    assert got["rc"] == -ERR_CAPACITY
    # no mark at all fits a capacity of 0
    got = dev_group_sites(counter, na, gt, np.full(ns, -1), 5, 1, capacity=0, null=("marks",))
    assert got["rc"] == 0 and got["n_marks"] == 0
    assert dev_group_sites(counter, na, gt, np.full(ns, -1), 5, 1, null=("marks", "count", "calls", "sites", "group_marks"))["rc"] == 0


@pytest.mark.parametrize("ns", [6, 64, 70])
def test_device_refusals(either_counter, ns):
    counter = either_counter
    rng = np.random.RandomState(ns)
    n_sites, n_groups = 37, 4
    na, gt, group = random_case(rng, n_sites, ns, n_groups, max_alleles=3)
    na[:] = np.maximum(na, 2)
    want = restate_group_sites_table(na, gt, group, n_groups, 1)
    check(dev_group_sites(counter, na, gt, group, n_groups, 1), want)
    label, alleles, cell = "a label is below -1 or not below n_groups", "a site has n_alleles < 1 or above n_samples", "a genotype cell is below -1 or above its site's n_alleles"
    cases = []
    for at in (0, ns - 1):
        for value in (-2, n_groups):
            bad = group.copy(); bad[at] = value
            cases.append((label, na, gt, bad))
    for at in (0, n_sites - 1):
        for value in (0, ns + 1):
            bad = na.copy(); bad[at] = value
            bad_gt = gt.copy(); bad_gt[at] = np.minimum(bad_gt[at], 0)            # (the cells stay within any n_alleles)
            cases.append((alleles, bad, bad_gt, group))
    for at in ((0, 0), (n_sites - 1, ns - 1), (n_sites // 2, 0)):
        for value in (-2, int(na[at[0]]) + 1):
            bad = gt.copy(); bad[at] = value
            cases.append((cell, na, bad, group))
    out_of_it = group.copy(); out_of_it[0] = -1
    bad = gt.copy(); bad[3, 0] = -2
    cases.append((cell, na, bad, out_of_it))                                      # the cell of a sample that takes no part is checked all the same
    for msg, a, g, l in cases:
        with pytest.raises(ValueError):
            restate_group_sites_table(a, g, l, n_groups, 1)
        rc, err, bufs, count = dev_group_sites(counter, a, g, l, n_groups, 1)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert all(b.untouched() for b in bufs.values()) and count == -77, msg    # nothing was written, *h_n_marks is left alone
    check(dev_group_sites(counter, na, gt, group, n_groups, 1), want)             # the counter serves the next good call
    # host refusals with real handles
    torch = _torch()
    L = tj.lib()
    sd, gd, ld, out = _dev(sites_of(na)), _dev(gt.astype(np.int16)), _dev(group.astype(np.int32)), torch.zeros(n_sites * n_groups * 16, dtype=torch.uint8, device="cuda")
    for args in ((None, n_sites, _p(gd), ns, _p(ld), n_groups, 1), (_p(sd), n_sites, None, ns, _p(ld), n_groups, 1), (_p(sd), n_sites, _p(gd), ns, None, n_groups, 1),
                 (_p(sd), n_sites, _p(gd), 4097, _p(ld), n_groups, 1), (_p(sd), n_sites, _p(gd), ns, _p(ld), 0, 1), (_p(sd), n_sites, _p(gd), ns, _p(ld), n_groups, 0),
                 (_p(sd), -1, _p(gd), ns, _p(ld), n_groups, 1)):
        assert L.tjamd_group_sites(counter._h, *args, _p(out), _p(out), _p(out), _p(out), 1, None) == -ERR_ARG
    assert L.tjamd_group_sites(counter._h, _p(sd), n_sites, _p(gd), ns, _p(ld), n_groups, 1, None, None, None, None, 1, None) == -ERR_ARG   # a capacity without a list
    assert not out.any()


@pytest.mark.parametrize("ns", [6, 70])
def test_two_device_refusals_at_once(either_counter, ns):
    """two error bits raised in one call: the message is that of the lowest bit, and nothing is written"""
    rng = np.random.RandomState(ns)
    n_sites, n_groups = 5, 3
    na, gt, group = random_case(rng, n_sites, ns, n_groups, max_alleles=3)
    na[:] = np.maximum(na, 2)
    bad_cell = gt.copy(); bad_cell[4, ns - 1] = -2
    bad_label = group.copy(); bad_label[1] = n_groups
    bad_alleles = na.copy(); bad_alleles[2] = 0
    bad_cell[2] = np.minimum(bad_cell[2], 0)                                      # (the cells of that site stay within any n_alleles)
    for msg, a, l in (("a label is below -1 or not below n_groups", na, bad_label), ("a site has n_alleles < 1 or above n_samples", bad_alleles, group)):
        rc, err, bufs, count = dev_group_sites(either_counter, a, bad_cell, l, n_groups, 1)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert all(b.untouched() for b in bufs.values()) and count == -77, msg
    gt[2] = np.minimum(gt[2], 0)
    check(dev_group_sites(either_counter, na, gt, group, n_groups, 1), restate_group_sites_table(na, gt, group, n_groups, 1))   # the counter serves the next good call


def test_no_site(either_counter):
    got = dev_group_sites(either_counter, np.zeros(0, np.int64), np.zeros((0, 5), np.int16), [0, 1, 1, -1, 2], 3, 1, capacity=4)
    assert got["rc"] == 0 and got["n_marks"] == 0 and got["group_marks"].tolist() == [0, 0, 0]
    assert either_counter.last_group_sites_ms() == -1.0                           # no kernel ran
    L = tj.lib()
    ld = _dev(np.array([0, 1, 1, -1, 2], np.int32))
    assert L.tjamd_group_sites(either_counter._h, None, 0, None, 5, _p(ld), 3, 1, None, None, None, None, 0, None) == 0


# ---- the pipeline ----------------------------------------------------------------------------------------------------------

def test_eight_sample_pipeline(pipeline, tables_counter):  # noqa: F811
    torch = _torch()
    p = pipeline
    merger, ref, u, k, ns = p["merger"], p["ref"], p["u"], p["k"], p["ns"]
    want_m = restate_merge_variants(p["recs"], ns, k, n_tracts=p["nt"])
    m = dev_merge(merger, k, p["recs"], ns, p["nt"], want=want_m)
    d = dev_depths(merger, ref, u, m["sites"], m["alleles"])
    dist = dev_distances(merger, m["sites"], m["alleles"], d["genotype"], ns)
    links = dev_linkage(merger, dist, DIFFER, 1)
    n_sites = len(m["sites"])
    sd, gd, ld = _dev(m["sites"]), _dev(np.ascontiguousarray(d["genotype"], np.int16)), _dev(links)
    cluster = torch.zeros(ns, dtype=torch.int32, device="cuda")
    keys = sorted(set(int(x) for x in links["key"]))
    for thr in [-1] + keys:
        n_clusters = merger.linkage_clusters(_p(ld), len(links), ns, thr, _p(cluster))   # d_cluster straight in as d_group
        labels = cluster.cpu().numpy()
        assert labels.tolist() == restate_linkage_clusters(links, ns, thr).tolist()
        for genotype, name in ((d["genotype"], "N13"), (m["genotype"], "N12")):
            want = restate_group_sites_table(m["sites"]["n_alleles"], genotype, labels, n_clusters, 1)
            if name == "N13" and thr == keys[len(keys) // 2]:
                assert same_result(want, restate_group_sites(m["sites"]["n_alleles"], genotype, labels, n_clusters, 1))
            for c in (merger, tables_counter):
                check(dev_group_sites(c, m["sites"]["n_alleles"], genotype, labels, n_clusters, 1, sites=m["sites"]), want, (thr, name))
        marks = torch.zeros(max(1, n_sites * ns) * 16, dtype=torch.uint8, device="cuda")
        n = merger.group_sites(_p(sd), n_sites, _p(gd), ns, _p(cluster), n_clusters, 1, d_marks=_p(marks), mark_capacity=n_sites * ns)
        print(f"\n[groups] cut at {thr}: {n_clusters} clusters of {ns} samples, {n_sites} sites, {n} marks (N13's genotypes); "
              f"tjamd_last_group_sites_ms {merger.last_group_sites_ms():.3f} ms")


def cluster_sites_text(contig_names, m, marks):
    """cluster_sites.tsv as examples/merged_vcf.c -G writes it, from a restate_merge_variants result and a list of marks"""
    out = ""
    for mk in marks:
        site = m["sites"][mk["site"]]
        ref, alts = m["text"][mk["site"]]
        out += "%d\t%s\t%d\t%s\t%s\t%d\n" % (mk["group"], contig_names[site["contig"]], site["pos"], ref, ref if mk["genotype"] == 0 else alts[mk["genotype"] - 1], mk["n_called"])
    return out


def test_merged_vcf_c_example_with_cluster_sites(pipeline, tmp_path):  # noqa: F811
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
    m = restate_merge_variants(p["recs"], p["ns"], p["k"], n_tracts=p["nt"])
    d = restate_site_depths(p["u"].keys, p["u"].mat, p["u"].tracts, p["u"].tract_loc, p["ref"].download(), p["k"], m)
    links = restate_sample_linkage(restate_sample_distances(m["sites"], m["alleles"], d["genotype"]), DIFFER, 1)
    cut = int(links["key"][len(links) // 2])                                   # a threshold inside the tree's keys
    labels = restate_linkage_clusters(links, p["ns"], cut)
    common = ["-x", "1", "-k", str(p["k"]), "-m", str(p["m"]), "-c", "5", "-d", "1", "-l", "2"]
    written = {}
    for flags in (("-D", "-C", str(cut)), ("-D", "-C", str(cut), "-G"), ("-G", "-C", str(cut))):
        out = tmp_path / ("out" + "".join(flags))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, *flags, *common, "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        written[flags] = {name: (out / name).read_text() for name in sorted(os.listdir(out))}
    plain, with_g, on_n12 = written[("-D", "-C", str(cut))], written[("-D", "-C", str(cut), "-G")], written[("-G", "-C", str(cut))]
    assert sorted(with_g) == sorted(list(plain) + ["cluster_sites.tsv"]) and "cluster_sites.tsv" not in plain
    for name in plain:
        assert with_g[name] == plain[name], name                                  # -G leaves the other files as they are
    want = restate_group_sites_table(m["sites"]["n_alleles"], d["genotype"], labels, int(labels.max()) + 1, 1)
    assert with_g["cluster_sites.tsv"] == cluster_sites_text(["genome"], m, want["marks"])
    links12 = restate_sample_linkage(restate_sample_distances(m["sites"], m["alleles"], m["genotype"]), DIFFER, 1)   # without -D: N12's genotypes all the way
    labels12 = restate_linkage_clusters(links12, p["ns"], cut)
    want12 = restate_group_sites_table(m["sites"]["n_alleles"], m["genotype"], labels12, int(labels12.max()) + 1, 1)
    assert on_n12["cluster_sites.tsv"] == cluster_sites_text(["genome"], m, want12["marks"])
    out = tmp_path / "refused"
    out.mkdir()
    r = subprocess.run([exe, "-r", fasta, "-D", "-M", "-G", *common, "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.startswith("usage:") and os.listdir(out) == []   # -G without -C
