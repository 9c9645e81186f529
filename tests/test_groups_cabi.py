"""The group step (include/tatajuba_groups.h: tjamd_group_sites) without a GPU: the entry is declared in its own header, exported
and prototyped and refuses bad arguments before any device call, the records match the header, and the restatement that the GPU
tests (tests/test_groups.py) compare against is pinned by the hand case of the header's rule, whose expected records are written
out here, by a second form of itself and by properties on random inputs.

restate_group_sites is written from the rule in the header in two independent forms that must agree byte for byte: one walks
the sites with sets of samples, one is vectorised over a table of counts per (site, group, genotype).  The device reads a site
with ballots of a wavefront or with LDS tables of a workgroup."""
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
NEW_ENTRIES = ["tjamd_group_sites", "tjamd_last_group_sites_ms"]
ERR_NO_DEVICE, ERR_ARG, ERR_CAPACITY = 1, 3, 4
CALL, GSITE, MARK = tj.GROUP_CALL_DTYPE, tj.GROUP_SITE_DTYPE, tj.GROUP_MARK_DTYPE


def _inputs(n_alleles, genotype, group, n_groups, min_called):
    """the arrays of a call, checked as the device checks them: ValueError names what is refused there"""
    na, group = np.asarray(n_alleles, np.int64), np.asarray(group, np.int64)
    ns = len(group)
    gt = np.asarray(genotype, np.int64).reshape(len(na), ns)
    assert 1 <= ns <= 4096 and 1 <= n_groups <= 4096 and min_called >= 1
    if (group < -1).any() or (group >= n_groups).any():
        raise ValueError("label")
    if (na < 1).any() or (na > ns).any():
        raise ValueError("n_alleles")
    if (gt < -1).any() or (gt > na[:, None]).any():
        raise ValueError("cell")
    return na, gt, group, ns


def _result(calls, sites, marks):
    marks = np.array(marks, MARK) if len(marks) else np.zeros(0, MARK)
    group_marks = np.bincount(marks["group"], minlength=calls.shape[1]).astype(np.int32)
    return {"calls": calls, "sites": sites, "group_marks": group_marks, "marks": marks}


def restate_group_sites(n_alleles, genotype, group, n_groups, min_called):
    """the rule, site by site with sets -> calls CALL [n_sites, n_groups], sites GSITE [n_sites], group_marks int32 [n_groups],
    marks MARK [n_marks] ascending in (site, group)"""
    na, gt, group, ns = _inputs(n_alleles, genotype, group, n_groups, min_called)
    calls, sites, marks = np.zeros((len(na), n_groups), CALL), np.zeros(len(na), GSITE), []
    members = [set(np.flatnonzero(group == G).tolist()) for G in range(n_groups)]
    taking = set(np.flatnonzero(group >= 0).tolist())
    for i in range(len(na)):
        called = {s for s in taking if gt[i, s] >= 0}
        marked = []
        for G in range(n_groups):
            mine, others = called & members[G], called - members[G]
            carried = {int(gt[i, s]) for s in mine}
            fixed = -1 if not mine else carried.pop() if len(carried) == 1 else -2
            n_outside = sum(1 for s in others if gt[i, s] == fixed) if fixed >= 0 else 0
            mark = int(fixed >= 0 and len(mine) >= min_called and n_outside == 0 and len(others) > 0)
            calls[i, G] = (len(mine), fixed, n_outside, mark)
            if mark:
                marked.append(G)
                marks.append((i, G, fixed, len(mine)))
        sites[i] = (len(called), len({int(gt[i, s]) for s in called}), len(marked), marked[0] if marked else -1)
    return _result(calls, sites, marks)


def restate_group_sites_table(n_alleles, genotype, group, n_groups, min_called):
    """the same from a table of counts per (site, group, genotype), kept as its occupied entries: no loop over sites or groups"""
    na, gt, group, ns = _inputs(n_alleles, genotype, group, n_groups, min_called)
    n_sites, X = len(na), 4097
    i, s = np.nonzero((gt >= 0) & (group >= 0)[None, :])
    x, G = gt[i, s], group[s]
    entry, count = np.unique((i * n_groups + G) * X + x, return_counts=True)     # the table: ascending in (site, group, genotype)
    cell, ex = entry // X, entry % X                                              # (site, group) of an entry, its genotype
    n_called = np.bincount(cell, weights=count, minlength=n_sites * n_groups).astype(np.int64)
    n_carried = np.bincount(cell, minlength=n_sites * n_groups)
    first_x = np.full(n_sites * n_groups, -1, np.int64)
    first_x[cell[::-1]] = ex[::-1]                                                # the smallest genotype of a cell: its only one where n_carried is 1
    fixed = np.where(n_carried == 0, -1, np.where(n_carried == 1, first_x, -2))
    carriers = np.bincount((entry // X // n_groups) * X + ex, weights=count, minlength=n_sites * X).astype(np.int64)   # per (site, genotype), over all groups
    site_of = np.repeat(np.arange(n_sites), n_groups)
    n_outside = np.where(fixed >= 0, carriers[site_of * X + np.maximum(fixed, 0)] - n_called, 0)
    site_called = n_called.reshape(n_sites, n_groups).sum(1)
    mark = (fixed >= 0) & (n_called >= min_called) & (n_outside == 0) & (site_called[site_of] > n_called)
    calls = np.zeros((n_sites, n_groups), CALL)
    for name, v in (("n_called", n_called), ("fixed", fixed), ("n_outside", n_outside), ("mark", mark)):
        calls[name] = v.reshape(n_sites, n_groups)
    m2 = mark.reshape(n_sites, n_groups)
    sites = np.zeros(n_sites, GSITE)
    sites["n_called"], sites["n_genotypes"], sites["n_marks"] = site_called, (carriers.reshape(n_sites, X) > 0).sum(1), m2.sum(1)
    sites["first_group"] = np.where(m2.any(1), m2.argmax(1), -1)
    at = np.flatnonzero(mark)
    marks = np.zeros(len(at), MARK)
    marks["site"], marks["group"], marks["genotype"], marks["n_called"] = at // n_groups, at % n_groups, fixed[at], n_called[at]
    return _result(calls, sites, marks)


def same_result(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in ("calls", "sites", "group_marks", "marks"))


def random_case(rng, n_sites, ns, n_groups, p_out=0.15, p_missing=0.25, max_alleles=3, empty_group=False):
    """labels with samples that take no part (and, on request, a group without members); few alleles, so that groups are often
    fixed and often private"""
    pool = [G for G in range(n_groups) if not (empty_group and n_groups > 1 and G == n_groups // 2)]
    group = rng.choice(pool, ns)
    group[rng.random_sample(ns) < p_out] = -1
    if ns >= 3:
        group[0] = -1
    na = rng.randint(1, min(max_alleles, ns) + 1, n_sites)
    gt = (rng.random_sample((n_sites, ns)) ** 2 * (na[:, None] + 1)).astype(np.int64)   # 0 most often
    gt[rng.random_sample((n_sites, ns)) < p_missing] = -1
    return na, gt, group


def as_tuples(a):
    return [tuple(int(v) for v in r) for r in a.tolist()]


# ---- the hand case of the header -------------------------------------------------------------------------------------------
HAND_GROUP = [0, 0, 1, 1, 2, -1]
HAND_N_ALLELES = [2, 1, 3, 1, 1]
HAND_GENOTYPE = [[1, 1, 0, 0, 0, 2], [1, -1, 1, 1, -1, -1], [1, 2, 3, 3, 0, 0], [1, 1, -1, -1, -1, 1], [-1] * 6]
HAND_MARKS = {1: [(0, 0, 1, 2), (2, 1, 3, 2), (2, 2, 0, 1)], 2: [(0, 0, 1, 2), (2, 1, 3, 2)], 3: []}
HAND_GROUP_MARKS = {1: [1, 1, 1], 2: [1, 1, 0], 3: [0, 0, 0]}
HAND_SITES_2 = [(5, 2, 1, 0), (3, 1, 0, -1), (5, 4, 1, 1), (2, 1, 0, -1), (0, 0, 0, -1)]
HAND_CALLS_SITE_2 = [(2, -2, 0, 0), (2, 3, 0, 1), (1, 0, 0, 0)]
HAND_CALL_3_0 = (2, 1, 0, 0)                      # fixed and private, but no outsider is called: sample 5 carries it and takes no part


@pytest.mark.parametrize("restate", [restate_group_sites, restate_group_sites_table])
def test_the_rule_on_the_hand_case(restate):
    for min_called in (1, 2, 3):
        r = restate(HAND_N_ALLELES, HAND_GENOTYPE, HAND_GROUP, 3, min_called)
        assert as_tuples(r["marks"]) == HAND_MARKS[min_called], min_called
        assert r["group_marks"].tolist() == HAND_GROUP_MARKS[min_called]
    r = restate(HAND_N_ALLELES, HAND_GENOTYPE, HAND_GROUP, 3, 2)
    assert as_tuples(r["sites"]) == HAND_SITES_2
    assert as_tuples(r["calls"][2]) == HAND_CALLS_SITE_2
    assert as_tuples(r["calls"][3])[0] == HAND_CALL_3_0
    assert as_tuples(r["calls"][4]) == [(0, -1, 0, 0)] * 3                       # nobody is called
    assert as_tuples(r["calls"][1]) == [(1, 1, 2, 0), (2, 1, 1, 0), (0, -1, 0, 0)]
    assert as_tuples(restate(HAND_N_ALLELES, HAND_GENOTYPE, HAND_GROUP, 3, 1)["calls"][2])[2] == (1, 0, 0, 1)
    # what is refused on the device
    for what, na, gt, group, ng in (("label", HAND_N_ALLELES, HAND_GENOTYPE, [0, 0, 1, 1, 2, -2], 3), ("label", HAND_N_ALLELES, HAND_GENOTYPE, [0, 0, 1, 3, 2, -1], 3),
                                    ("n_alleles", [2, 0, 3, 1, 1], HAND_GENOTYPE, HAND_GROUP, 3), ("n_alleles", [2, 1, 7, 1, 1], HAND_GENOTYPE, HAND_GROUP, 3),
                                    ("cell", HAND_N_ALLELES, [[1, 1, 0, 0, 0, -2]] + HAND_GENOTYPE[1:], HAND_GROUP, 3),
                                    ("cell", HAND_N_ALLELES, HAND_GENOTYPE[:3] + [[1, 1, -1, -1, -1, 2]] + HAND_GENOTYPE[4:], HAND_GROUP, 3)):
        with pytest.raises(ValueError, match=what):
            restate(na, gt, group, ng, 2)


@pytest.mark.parametrize("n_sites,ns,n_groups,seed", [(40, 6, 3, 1), (30, 13, 1, 2), (25, 9, 9, 3), (30, 70, 5, 4), (12, 130, 40, 5), (20, 5, 8, 6), (10, 1, 1, 7)])
def test_two_forms_agree_and_the_properties_hold(n_sites, ns, n_groups, seed):
    rng = np.random.RandomState(seed)
    na, gt, group = random_case(rng, n_sites, ns, n_groups, empty_group=seed % 2 == 0)
    if seed == 3:
        group = rng.permutation(ns)                                               # everyone alone
    assert ns < 3 or seed == 3 or (group == -1).any()
    assert seed != 4 or not (group == n_groups // 2).any()                        # a group without members
    n_marks_at = {}
    for min_called in (1, 2, 3):
        r = restate_group_sites(na, gt, group, n_groups, min_called)
        assert same_result(r, restate_group_sites_table(na, gt, group, n_groups, min_called)), min_called
        marks = as_tuples(r["marks"])
        assert marks == sorted(marks) and len(set(m[:2] for m in marks)) == len(marks)
        assert int(r["group_marks"].sum()) == len(marks) == int(r["sites"]["n_marks"].sum())
        for i, G, x, n in marks:
            mine = (group == G) & (gt[i] >= 0)
            others = (group != G) & (group >= 0) & (gt[i] >= 0)
            assert mine.sum() == n >= min_called and (gt[i][mine] == x).all()    # every called member carries it ...
            assert others.any() and not (gt[i][others] == x).any()               # ... and no called sample of another group
        n_marks_at[min_called] = set(m[:3] for m in marks)
    assert n_marks_at[3] <= n_marks_at[2] <= n_marks_at[1]                        # raising min_called only removes marks
    if ns > 1:
        # a non-member that leaves (label -1) never removes a mark of G, unless it was the last called outsider there
        r = restate_group_sites(na, gt, group, n_groups, 1)
        for s in rng.permutation(ns)[:4]:
            if group[s] < 0:
                continue
            fewer = group.copy()
            fewer[s] = -1
            q = restate_group_sites(na, gt, fewer, n_groups, 1)
            assert same_result(q, restate_group_sites_table(na, gt, fewer, n_groups, 1))
            kept = set(m[:3] for m in as_tuples(q["marks"]))
            for i, G, x, n in as_tuples(r["marks"]):
                if G == group[s]:
                    continue
                still_seen = ((fewer != G) & (fewer >= 0) & (gt[i] >= 0)).any()
                assert ((i, G, x) in kept) == bool(still_seen), (s, i, G)


def test_marks_exist_in_the_random_cases():
    """the properties above are about marks: the cases have some"""
    rng = np.random.RandomState(1)
    na, gt, group = random_case(rng, 40, 6, 3)
    assert len(restate_group_sites_table(na, gt, group, 3, 1)["marks"]) >= 3


# ---- declarations and argument checks --------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    own_path = os.path.join(ROOT, "include", "tatajuba_groups.h")
    own = strip(own_path)
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.GROUP_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_groups.h"]
    assert len(others) >= 11
    for s in NEW_ENTRIES:
        for path in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(path)), (s, path)   # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in (tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS + tj.EFFECT_EXPORTS + tj.SITE_EXPORTS
                         + tj.DEPTH_EXPORTS + tj.DISTANCE_EXPORTS + tj.LINKAGE_EXPORTS) and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert "tatajuba_groups.h" in open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read()
    assert '#include "tatajuba_linkage.h"' in own
    for name, dt in (("tjamd_group_call", CALL), ("tjamd_group_site", GSITE), ("tjamd_group_mark", MARK)):
        assert _fields(own, name) == list(dt.names), name
        assert dt.itemsize == 16 and [dt.fields[x][1] for x in dt.names] == [0, 4, 8, 12], name
    assert L.tjamd_last_group_sites_ms(None) == -1.0
    for name in ("group_sites", "last_group_sites_ms"):
        assert hasattr(tj.Counter, name)
    text = open(own_path).read()
    for what in ("Reference interface replaced: none", "N16 of DESIGN.md section 3.5", "Not built:", "test statistic or p-value per site", "groups that overlap", "weights",
                 "marks that allow a share of exceptions", "read depths", "marks of a tree's inner nodes without a cut"):
        assert what in text, what


def test_group_sites_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    outs = {"calls": GuardedHost(64 * 16), "site_out": GuardedHost(64 * 16), "group_marks": GuardedHost(64 * 4), "marks": GuardedHost(64 * 16)}
    n_marks = C.c_long(-77)

    def call(c=fake, sites=fake, n_sites=4, gt=fake, ns=6, group=fake, ng=3, min_called=1, cap=64, null=(), no_count=False):
        o = {k: (None if k in null else v.c) for k, v in outs.items()}
        rc = L.tjamd_group_sites(c, sites, n_sites, gt, ns, group, ng, min_called, o["calls"], o["site_out"], o["group_marks"], o["marks"], cap,
                                 None if no_count else C.byref(n_marks))
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"n_sites": -1}, "n_sites -1 below 0"),
                    ({"sites": None}, "null site or genotype buffer"), ({"gt": None}, "null site or genotype buffer"), ({"gt": None, "n_sites": 1}, "null site or genotype buffer"),
                    ({"group": None}, "null d_group"), ({"group": None, "n_sites": 0}, "null d_group"),
                    ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": -2}, "n_samples -2 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"),
                    ({"ng": 0}, "n_groups 0 outside 1..4096"), ({"ng": -1}, "n_groups -1 outside 1..4096"), ({"ng": 4097}, "n_groups 4097 outside 1..4096"),
                    ({"min_called": 0}, "min_called 0 below 1"), ({"min_called": -5}, "min_called -5 below 1"),
                    ({"cap": -1}, "mark_capacity -1 below 0"), ({"null": ("marks",), "cap": 1}, "null d_marks with a capacity of 1"),
                    ({"n_sites": 1 << 20, "ns": 2048}, "1048576 sites x 2048 samples: 2^31 cells or more"),
                    ({"n_sites": (1 << 31) // 6 + 1, "ns": 6}, "2^31 cells or more"), ({"n_sites": 1 << 62, "ns": 4}, "2^31 cells or more"),
                    ({"n_sites": 1 << 20, "ns": 6, "ng": 2048}, "1048576 sites x 2048 groups: 2^31 calls or more")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_group_sites") and msg in err, (kw, got, err)
    if tj.device_count() == 0:                     # good arguments, but nothing to run on: named, before the handles are read
        for kw in ({}, {"n_sites": 0, "sites": None, "gt": None}, {"null": ("calls", "site_out", "group_marks", "marks"), "cap": 0, "no_count": True},
                   {"n_sites": 1 << 20, "ns": 6, "ng": 2048, "null": ("calls",)},              # without d_calls the calls are not counted
                   {"n_sites": (1 << 31) // 4096 - 1, "ns": 4096, "ng": 1, "min_called": (1 << 31) - 1}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_group_sites") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    assert n_marks.value == -77                    # *h_n_marks is left alone by every refusal
    for name, buf in outs.items():
        assert buf.untouched(), name               # host memory handed in as an output stays as it was
        buf.check(name)


def test_group_sites_reports_the_first_of_two_broken_rules_without_a_gpu():
    """two rules broken in one call: the message is that of the rule that is checked first, for every pair of neighbours in the
    order of the checks (a pair that cannot be broken together, n_sites < 0 with a null site buffer for one, takes the next rule)"""
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    outs = {"calls": GuardedHost(64 * 16), "site_out": GuardedHost(64 * 16), "group_marks": GuardedHost(64 * 4), "marks": GuardedHost(64 * 16)}
    n_marks = C.c_long(-77)

    def call(c=fake, sites=fake, n_sites=4, gt=fake, ns=6, group=fake, ng=3, min_called=1, cap=64, null=()):
        o = {k: (None if k in null else v.c) for k, v in outs.items()}
        rc = L.tjamd_group_sites(c, sites, n_sites, gt, ns, group, ng, min_called, o["calls"], o["site_out"], o["group_marks"], o["marks"], cap, C.byref(n_marks))
        return rc, L.tjamd_last_error().decode()

    cells = {"n_sites": 1 << 20, "ns": 2048}
    for kw, msg in [({"c": None, "n_sites": -1}, "null counter"), ({"n_sites": -1, "group": None}, "n_sites -1 below 0"), ({"n_sites": -1, "ns": 0}, "n_sites -1 below 0"),
                    ({"sites": None, "group": None}, "null site or genotype buffer"), ({"gt": None, "ns": 0}, "null site or genotype buffer"),
                    ({"group": None, "ns": 0}, "null d_group"), ({"group": None, "ng": 0}, "null d_group"),
                    ({"ns": 0, "ng": 0}, "n_samples 0 outside 1..4096"), ({"ns": 4097, "min_called": 0}, "n_samples 4097 outside 1..4096"),
                    ({"ng": 4097, "min_called": 0}, "n_groups 4097 outside 1..4096"), ({"ng": 0, "cap": -1}, "n_groups 0 outside 1..4096"),
                    ({"min_called": 0, "cap": -1}, "min_called 0 below 1"), ({"min_called": 0, "null": ("marks",), "cap": 1}, "min_called 0 below 1"),
                    ({"cap": -1, **cells}, "mark_capacity -1 below 0"), ({"cap": -1, "null": ("marks",)}, "mark_capacity -1 below 0"),
                    ({"null": ("marks",), "cap": 1, **cells}, "null d_marks with a capacity of 1"),
                    ({"n_sites": 1 << 20, "ns": 2048, "ng": 2048}, "1048576 sites x 2048 samples: 2^31 cells or more")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_group_sites") and msg in err, (kw, got, err)
    assert n_marks.value == -77
    for name, buf in outs.items():
        assert buf.untouched(), name
        buf.check(name)
