"""tjamd_replicate_trees at the limits of what it admits, with no difference allowed anywhere: every result is compared with the
restatement of tests/test_replicate_trees_cabi.py and, where said, with the per-replicate loop of the existing entries on the
device.  tests/test_replicate_trees.py stops at 5 replicates and 1025 samples; here:

  many replicates   9 samples x 4096 replicates (the one-workgroup form: 4096 workgroups; and under TATAJUBA_AMD_LINKAGE_SMALL=0 the
                    replicate in the z of the check and key kernels' grids and in the y of every round kernel's), and 66 samples x 257
                    replicates in one group and in groups of 100, 100 and 57;
  stale scratch     groups of two in which a group of short replicates inherits the comp, size, rowbest, edges, pairs, links and
                    keys of a group that ran all its rounds, and the reverse, with batches of 32 and of 4 rounds;
  the natural group 1025 samples without TATAJUBA_AMD_TREES_GROUP: 1 GiB of scratch holds 126 replicates, the call has 129, and the last
                    replicate's matrix starts past byte 2^31 of d_dist;
  the sample limit  4095 and 4096 samples, a forest and a replicate in which every pair is an edge.

The shapes' conditions (forests of different sizes, G < R, the offset past 2^31) are asserted without a device.  Outputs always
sit in guarded buffers (tests/guarded.py), every input is held frozen, and every call is made twice and must give the same bytes
(tests/test_replicate_trees.py: dev_rep_trees)."""
import functools

import numpy as np
import pytest

import tatajuba_amd as tj
from tests import sample_calls as sc
from tests.test_agglomerate_cabi import AVERAGE, COMPLETE, cap_for_average
from tests.test_linkage_cabi import DIFFER, LENGTH, fabricate_wide
from tests.test_replicate_trees import _counter_under, _torch, check, dev_rep_trees, loop_on_device, mixed_replicates, same, stack_small
from tests.test_replicate_trees_cabi import LINKAGES, SINGLE, restate_replicate_trees

DIST = tj.SAMPLE_DISTANCE_DTYPE
MANY = [(9, 4096), (66, 257)]                              # samples, replicates
LOOPED = (0, 1, 2047, 4094, 4095)                          # the replicates of 4096 that the loop on the device takes
NATURAL_NS = 1025


def without_edges(d, samples):
    """the samples' pairs get an n_both of 1, below a min_both of 2, and an n_differ of 0: in place"""
    for s in samples:
        for f, v in (("n_both", 1), ("n_differ", 0)):
            keep = int(d[f][s, s])
            d[f][s, :] = d[f][:, s] = v
            d[f][s, s] = keep


@functools.lru_cache(maxsize=None)
def many_input(ns, R):
    """keys in 0..3; under min_both 2 a quarter of the pairs are no edge: ties, but at these sizes hardly ever a forest, so every
    fifth replicate has its last one, two or three samples without an edge"""
    dist = stack_small(ns, R, np.random.RandomState(9000 + ns))
    for r in range(3, R, 5):
        without_edges(dist[r], range(ns - 1 - (r // 5) % 3, ns))
    return dist


@functools.lru_cache(maxsize=None)
def many_want(ns, R, linkage):
    return restate_replicate_trees(many_input(ns, R), DIFFER, 2, linkage)


@pytest.mark.parametrize("ns,R", MANY)
def test_the_many_replicates_are_forests_of_different_sizes(ns, R):
    counts = [len(t["nodes"]) for t in many_want(ns, R, SINGLE)]
    assert len(set(counts)) > 1 and min(counts) < ns - 1, sorted(set(counts))
    rounds = [t["n_rounds"] for t in many_want(ns, R, COMPLETE)]
    assert len(set(rounds)) > 1                             # ... and the replicates of a call end at different rounds


def natural_shape():
    """-> (the replicates a group holds without the hook, the replicates of the call)"""
    per, G = sc.rep_group(NATURAL_NS, 4096)
    return G, max(G + 2, (1 << 31) // (NATURAL_NS * NATURAL_NS * DIST.itemsize) + 2)


def test_the_natural_group_is_smaller_than_the_call():
    ns = NATURAL_NS
    per, G = sc.rep_group(ns, 4096)
    ld, ldc = ns + 1, 1152
    assert per == ns * ld * 8 + 2 * ldc * 4 + 2 * ns * 16 + ns * 4 + (ns - 1) * 16 == 8475700 and G == (1 << 30) // per == 126
    G, R = natural_shape()
    assert R == 129 and G < R and R - G < G                 # a full group and a short one
    assert R * ns * ns * DIST.itemsize > 1 << 31 and (R - 1) * ns * ns * DIST.itemsize > 1 << 31      # the last replicate starts past 2^31
    assert sc.rep_group(ns, R) == (per, G) and sc.rep_group(ns, R, group=2) == (per, 2) and sc.rep_group(ns, 5) == (per, 5)


# ---- many replicates ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def _inputs_released():
    """the inputs are made once per shape and shared; half a gigabyte of them at 4096 samples, given back with the module"""
    yield
    for made in (many_input, many_want, natural_sources, limit_input):
        made.cache_clear()


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(15)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("kind", ["default", "rounds"])
def test_4096_replicates_of_9_samples(counter, kind, linkage):
    """default: a workgroup per replicate; rounds: 4096 in the z of rep_check_kernel and rep_keys_kernel and in the y of the rounds"""
    ns, R = MANY[0]
    c = counter if kind == "default" else _counter_under(TATAJUBA_AMD_LINKAGE_SMALL="0")
    try:
        dist = many_input(ns, R)
        got = dev_rep_trees(c, dist, DIFFER, 2, linkage)
        same(got, many_want(ns, R, linkage), (kind, linkage, "restatement"))
        at = list(LOOPED)
        same([got[r] for r in at], loop_on_device(c, dist[at], DIFFER, 2, linkage), (kind, linkage, "loop"))
    finally:
        if c is not counter:
            c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("group", [0, 100])
def test_257_replicates_of_66_samples(counter, group, linkage):
    """one group of 257, and groups of 100, 100 and 57"""
    ns, R = MANY[1]
    assert sc.rep_group(ns, R, group)[1] == (group or R)
    c = counter if not group else _counter_under(TATAJUBA_AMD_TREES_GROUP=str(group))
    try:
        dist = many_input(ns, R)
        got = dev_rep_trees(c, dist, DIFFER, 2, linkage)
        same(got, many_want(ns, R, linkage), (group, linkage, "restatement"))
        at = [0, 99, 100, 199, 200, 256]                    # the first and the last replicate of every group
        same([got[r] for r in at], loop_on_device(c, dist[at], DIFFER, 2, linkage), (group, linkage, "loop"))
    finally:
        if c is not counter:
            c.close()


# ---- stale group scratch --------------------------------------------------------------------------------------------------------

SEQUENCES = ["equal equal few none", "equal equal none few", "few none equal equal none"]


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [66, 129])
@pytest.mark.parametrize("batch", [None, "4"], ids=["batches of 32", "batches of 4"])
def test_a_group_inherits_the_scratch_of_the_group_before_it(ns, batch):
    """groups of two: the replicates of a group take over comp, size, rowbest, edges, pairs, links and keys as the group before
    left them, after all its ns - 1 rounds or after none"""
    env = {"TATAJUBA_AMD_TREES_GROUP": "2"}
    if batch:
        env["TATAJUBA_AMD_AGGL_BATCH"] = batch
    c = _counter_under(**env)
    try:
        kinds = dict(zip(("equal", "few", "none"), mixed_replicates(ns, np.random.RandomState(9500 + ns))))
        for linkage in LINKAGES:
            loops = {k: loop_on_device(c, d[None], DIFFER, 1, linkage)[0] for k, d in kinds.items()}
            wants = {k: restate_replicate_trees(d[None], DIFFER, 1, linkage)[0] for k, d in kinds.items()}
            assert linkage == SINGLE or (wants["equal"]["n_rounds"] == ns - 1 and 0 < wants["few"]["n_rounds"] < ns - 1)
            assert len(wants["none"]["links"]) == 0 and len(wants["equal"]["links"]) == ns - 1
            for seq in SEQUENCES:
                names = seq.split()
                check(c, np.stack([kinds[k] for k in names]), DIFFER, 1, linkage, (ns, linkage, seq), loop=[loops[k] for k in names], want=[wants[k] for k in names])
    finally:
        c.close()


# ---- the natural group boundary -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def natural_sources():
    """two matrices with keys over the full range and, between them, one with keys in 0..3 in which 1, 500, 1023 and 1024 have no edge"""
    rng = np.random.RandomState(9700)
    forest = stack_small(NATURAL_NS, 1, rng)[0]
    without_edges(forest, (1, 500, 1023, 1024))
    return [fabricate_wide(NATURAL_NS, rng), forest, fabricate_wide(NATURAL_NS, rng)]


@pytest.mark.gpu
@pytest.mark.parametrize("linkage", [SINGLE, COMPLETE])
def test_the_natural_group_boundary(counter, linkage):
    """129 replicates of 1025 samples with no hook: a group of 126 and a group of 3 that takes over its scratch, and the matrix
    of the last replicate starts past byte 2^31 of d_dist.  The input is laid out on the device from three matrices, replicate
    r holding matrix r % 3, and every replicate's links, nodes, order, count and rounds are those of its matrix."""
    torch = _torch()
    ns = NATURAL_NS
    G, R = natural_shape()
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("less than 8 GiB of device memory free: the call needs about 4")
    sources = natural_sources()
    three = np.stack(sources)
    want = restate_replicate_trees(three, DIFFER, 2, linkage)
    same(loop_on_device(counter, three, DIFFER, 2, linkage), want, "the loop on the three matrices")
    counts = [len(w["nodes"]) for w in want]                                  # the forest among them; complete linkage joins no two clusters with a pair that is no edge
    assert counts == [ns - 1, ns - 5, ns - 1] if linkage == SINGLE else counts[1] < min(counts[0], counts[2]) < ns - 1, counts
    per = ns * ns * DIST.itemsize
    dd = torch.empty(R * per, dtype=torch.uint8, device="cuda")
    for i, d in enumerate(sources):
        src = torch.from_numpy(np.ascontiguousarray(d).view(np.uint8).reshape(-1).copy()).cuda()
        for r in range(i, R, 3):
            dd[r * per: (r + 1) * per].copy_(src)
    got = dev_rep_trees(counter, (dd, R, ns), DIFFER, 2, linkage)         # (frozen by a copy on the device)
    same(got, [want[r % 3] for r in range(R)], (linkage, "restatement"))


# ---- the sample limit -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def limit_input(ns):
    """[a forest of two cliques, every pair an edge], keys over the full range; length_diff below 2^40: every linkage takes it"""
    whole = cap_for_average(fabricate_wide(ns, np.random.RandomState(9900 + ns)))
    whole["n_both"] = np.maximum(whole["n_both"], 1)
    halves = whole.copy()
    for f in DIST.names:
        halves[f][: ns // 2, ns // 2:] = 0
        halves[f][ns // 2:, : ns // 2] = 0
    return np.stack([halves, whole])


@pytest.mark.gpu
@pytest.mark.parametrize("ns,linkage", [(4095, SINGLE), (4095, COMPLETE), (4096, SINGLE), (4096, COMPLETE), (4096, AVERAGE)])
def test_the_sample_limit(counter, ns, linkage):
    dist = limit_input(ns)
    got = dev_rep_trees(counter, dist, LENGTH, 1, linkage)
    assert [len(g["nodes"]) for g in got] == [ns - 2, ns - 1]
    same(got, loop_on_device(counter, dist, LENGTH, 1, linkage), (ns, linkage, "loop"))


@pytest.mark.gpu
@pytest.mark.parametrize("r", [0, 1], ids=["the forest", "every pair an edge"])
@pytest.mark.parametrize("linkage", [SINGLE, COMPLETE])
def test_the_sample_limit_against_the_restatement(counter, linkage, r):
    """4096 samples; a replicate a case: the restatement of one takes four seconds"""
    dist = limit_input(4096)
    got = dev_rep_trees(counter, dist, LENGTH, 1, linkage)
    same(got[r: r + 1], restate_replicate_trees(dist[r: r + 1], LENGTH, 1, linkage), (linkage, r, "restatement"))
