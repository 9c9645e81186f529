"""Scratch carried between the calls of the sample-comparison layer (N14-N21).  Every one of its entries cuts its scratch from one
block of the counter, from offset 0, and the layouts differ: the two distance entries put their error words first, the entries of
the trees put their flag words last, where an earlier, larger call had its data; tjamd_replicate_trees (N20) cuts eight pieces
per group of replicates and keeps eight flag words per replicate in front of the call's, and tjamd_consensus_tree (N21) cuts
sixteen pieces, as many as a cut holds.  A kernel that read a word this call had not
written (a count that is added to, an error word, the round counters, the padding column of the key matrix) would pass every test
that takes a fresh counter.  tests/test_counter_reuse.py does this for the layers up to N12; here, on one counter per test:

  1. every entry on two small problems directly after every entry on a large one;
  2. every entry on the small problems after two calls that leave adversarial words over the start of the block;
  3. every entry on a small problem directly after every kind of call that is refused on the device, and the refused call again;
  4. step 1 among the entries that have a one-workgroup form, on a counter that never takes it.

Every result is bit for bit that of the same call on a fresh counter; on the small problems the fresh results are held to the
Python restatements of the per-entry tests, so that equal to fresh is right.  Every output sits in a guarded buffer and every
input is frozen (tests/sample_calls.py).

The problems.  large: 1025 samples (rows of 1026 keys: a padding column; a second trip of the 1024-thread kernels), 600 sites (tiles
of edge 32 over sliced sites: `partial` in use), 5 replicates (two full batches and one more).  small: 67 samples, 90 sites, 3
replicates (rows of 68; just past the 64 samples of the one-workgroup forms).  tiny: 9 samples, 40 sites (the one-workgroup forms:
no scratch but the flags; tiles of edge 16).  The replicates of tjamd_replicate_trees are the weighted matrices of the problem, under
all three linkages; those of tjamd_consensus_tree are one fabricated tree under 1 + samples / 64 transpositions a replicate
(tests/test_consensus_cabi.py), since the bootstrap trees of random sites share no clade: test_the_consensus_inputs_are_worth_a_consensus.

The poisons, both through the public API, their return codes alone checked:
  P1  tjamd_sample_distances on 16384 sites x 130 samples, every ref_length 2^31 - 1 and every genotype 0: `lens` is 0x7fffffff in
      every int from byte 256 to byte 256 + 4 x 16384 x 130 (8.5 MB).
  P2  tjamd_sample_linkage on the large problem's matrix with min_both 2^31 - 1: no pair has a key, so the key matrix is all ones
      from byte 37 888 (behind comp, rowbest and edges) for 1025 x 1026 x 8 bytes (8.4 MB).  No link.
Every counter here is made under TATAJUBA_AMD_DISTANCE_BLOCKS=4096.  At the 4 x 256 workgroups that a call aims at on the 256
compute units of an MI355X, the large problem's 561 tile pairs leave no room for a second slice of the sites; at 4096 its
unweighted call has 5 slices and its weighted call 2, `partial` is in use, and no cut depends on the device.  SMALL_CUTS lists
what every call on a small problem then cuts; test_the_poisons_cover_the_small_cuts holds the list to the formulas of
tests/sample_calls.py and the largest cut to half of what either poison covers."""
import functools
import os

import numpy as np
import pytest

import tatajuba_amd as tj
from tests import sample_calls as sc
from tests.bounds_calls import dev
from tests.test_agglomerate_cabi import AVERAGE, COMPLETE, restate_sample_agglomerate
from tests.test_bootstrap_cabi import restate_bootstrap_weights, restate_clade_support, restate_sample_distances_weighted
from tests.test_clades_cabi import restate_clade_sites, restate_linkage_tree
from tests.test_consensus_cabi import fabricate_replicates, majority, pack, restate_consensus
from tests.test_distances_cabi import fabricate, restate_sample_distances
from tests.test_groups_cabi import restate_group_sites
from tests.test_linkage_cabi import DIFFER, LENGTH, restate_linkage_clusters, restate_sample_linkage
from tests.test_replicate_trees_cabi import LINKAGES, SINGLE, restate_replicate_trees

ERR_ARG = 3
DIST, LINK, NODE = sc.DIST, sc.LINK, sc.NODE
UNSET = sc.UNSET
SHAPES = {"large": (1025, 600, 5), "small": (67, 90, 3), "tiny": (9, 40, 3)}       # samples, sites, replicates
SMALLS = ("small", "tiny")
POISON_SITES, POISON_SAMPLES = 16384, 130
BLOCKS = 4096                            # TATAJUBA_AMD_DISTANCE_BLOCKS of every counter here: the workgroups a distance call aims at

# bytes of the scratch block that a call on a small problem cuts (groups and nodes: at most as many as samples)
SMALL_CUTS = {
    ("tjamd_sample_distances", "small"): 221184,           # err 256, lens 24 320, partial 2 slices x 6 tile pairs x 32 x 32 x 16
    ("tjamd_sample_distances", "tiny"): 1792,              # err 256, lens 1 536, one slice
    ("tjamd_sample_distances_weighted", "small"): 614400,  # partial 3 replicates x 2 slices x 6 tile pairs x 32 x 32 x 16
    ("tjamd_sample_distances_weighted", "tiny"): 1792,
    ("tjamd_bootstrap_weights", "small"): 0,
    ("tjamd_bootstrap_weights", "tiny"): 0,
    ("tjamd_sample_linkage", "small"): 40192,              # comp 768, rowbest and edges 1 280 each, keys 67 x 68 x 8 = 36 448 -> 36 608, flags
    ("tjamd_sample_linkage", "tiny"): 256,
    ("tjamd_sample_linkage", "tiny", "rounds"): 2048,      # comp 512, rowbest and edges 256 each, keys 9 x 10 x 8 = 720 -> 768, flags
    ("tjamd_sample_agglomerate", "small"): 41472,          # size and comp 768 each, rowbest, edges 1 280, pairs 512, keys 36 608, flags
    ("tjamd_sample_agglomerate", "tiny"): 256,
    ("tjamd_sample_agglomerate", "tiny", "rounds"): 2816,
    ("tjamd_linkage_clusters", "small"): 256,
    ("tjamd_linkage_clusters", "tiny"): 256,
    ("tjamd_linkage_tree", "small"): 256,
    ("tjamd_linkage_tree", "tiny"): 256,
    ("tjamd_group_sites", "small"): 1280,                  # flags and marks 4 x (64 + 67) -> 768, cnt 360 -> 512
    ("tjamd_group_sites", "tiny"): 768,
    ("tjamd_clade_sites", "small"): 1280,
    ("tjamd_clade_sites", "tiny"): 768,
    ("tjamd_clade_support", "small"): 1024,                # cnt 264 -> 512, rep_n 256, flags
    ("tjamd_clade_support", "tiny"): 768,
    # three replicates: comp and size 3 x 192 ints each, rowbest and edges 3 x 67 x 16 -> 3 328 each, pairs 804 -> 1 024, links
    # 3 x 66 x 16 -> 3 328, keys 3 x 67 x 68 x 8 = 109 344 -> 109 568, the replicates' flags 3 x 8 ints -> 256, flags
    ("tjamd_replicate_trees", "small"): 125696,
    ("tjamd_replicate_trees", "tiny"): 512,                # the replicates' flags and the call's
    ("tjamd_replicate_trees", "tiny", "rounds"): 7680,     # comp and size 3 x 128 ints each, rowbest, edges 512, pairs, links 512, keys 2 160 -> 2 304, 256, 256
    # 198 records: two of keys 1 584 -> 1 792, seven of ints 792 -> 1 024, pos 402 -> 512, reps, rbad 256, kept 268 -> 512, kpar 536
    # -> 768, info 134 x 24 = 3 216 -> 3 328, flags
    ("tjamd_consensus_tree", "small"): 16640,
    ("tjamd_consensus_tree", "tiny"): 4352,                # 24 records: nine pieces of 256, pos, reps, rbad, kept, kpar 256 each, info 432 -> 512, flags
}


def small_cut_formulas():
    out = {}
    for name in SMALLS:
        ns, n_sites, n_rep = SHAPES[name]
        out["tjamd_sample_distances", name] = sc.cut_distances(ns, n_sites, dist_blocks=BLOCKS)
        out["tjamd_sample_distances_weighted", name] = sc.cut_distances(ns, n_sites, n_rep=n_rep, dist_blocks=BLOCKS)
        out["tjamd_bootstrap_weights", name] = []
        out["tjamd_sample_linkage", name] = sc.cut_linkage(ns)
        out["tjamd_sample_agglomerate", name] = sc.cut_agglomerate(ns)
        out["tjamd_linkage_clusters", name] = out["tjamd_linkage_tree", name] = sc.cut_flags_alone()
        out["tjamd_group_sites", name] = out["tjamd_clade_sites", name] = sc.cut_marks(ns, n_sites)
        out["tjamd_clade_support", name] = sc.cut_support(ns - 1, n_rep)
        out["tjamd_replicate_trees", name] = sc.cut_replicate_trees(ns, n_rep)
        out["tjamd_consensus_tree", name] = sc.cut_consensus(sum(consensus_input(name)[2]), ns, n_rep)
    out["tjamd_sample_linkage", "tiny", "rounds"] = sc.cut_linkage(9, small_form=False)
    out["tjamd_sample_agglomerate", "tiny", "rounds"] = sc.cut_agglomerate(9, small_form=False)
    out["tjamd_replicate_trees", "tiny", "rounds"] = sc.cut_replicate_trees(9, SHAPES["tiny"][2], small_form=False)
    return out


def test_the_poisons_cover_the_small_cuts():
    cuts = small_cut_formulas()
    assert {k: sc.cut_bytes(v) for k, v in cuts.items()} == SMALL_CUTS
    largest = max(SMALL_CUTS.values())
    assert largest == SMALL_CUTS["tjamd_sample_distances_weighted", "small"]
    # P1: lens, behind the 256 bytes of the error words
    p1 = sc.cut_distances(POISON_SAMPLES, POISON_SITES, dist_blocks=BLOCKS)
    first, last = sc.piece(p1, "lens")
    assert first == 256 and last == 256 + 4 * POISON_SITES * POISON_SAMPLES and 2 * largest <= last - first
    # P2: the key matrix of 1025 samples, behind comp (1026 + 64 ints), rowbest and edges (1025 x 16 bytes each)
    ns = SHAPES["large"][0]
    p2 = sc.cut_linkage(ns)
    first, last = sc.piece(p2, "keys")
    assert first == 4608 + 2 * 16640 == 37888 and last == first + ns * (ns + 1) * 8
    assert first <= 64 << 10 and last > largest and 2 * largest <= last - first
    # the flag words of the entries of the trees fall inside an earlier, larger call's data
    for entry in ("tjamd_sample_linkage", "tjamd_sample_agglomerate", "tjamd_clade_support", "tjamd_replicate_trees", "tjamd_consensus_tree"):
        at = sc.piece(cuts[entry, "small"], "flags")[0]
        assert 256 <= at < largest, entry
    # ... and so do the flag words that tjamd_replicate_trees keeps per replicate, and the words that tjamd_consensus_tree clears or
    # fills per call: the replicates' error words, their counts and offsets
    for entry, name in (("tjamd_replicate_trees", "rflags"), ("tjamd_consensus_tree", "rbad"), ("tjamd_consensus_tree", "reps")):
        at = sc.piece(cuts[entry, "small"], name)[0]
        assert 256 <= at < largest, (entry, name)
    assert sc.piece(cuts["tjamd_replicate_trees", "tiny", "rounds"], "rflags")[0] == 7168 and [n for n, _, _ in cuts["tjamd_consensus_tree", "small"]][-1] == "flags"
    assert len(cuts["tjamd_consensus_tree", "small"]) == sc.PIECES == 16 and len(cuts["tjamd_replicate_trees", "small"]) == 9
    # the groups of tjamd_replicate_trees: all replicates of these problems in one
    for name, (ns_, _, n_rep) in SHAPES.items():
        assert sc.rep_group(ns_, n_rep)[1] == n_rep, name
    # the shapes: a padding column, a second trip, sliced sites at edge 32; past the one-workgroup forms; inside them, edge 16
    assert ns % 2 == 1 and ns > 1024 and sc._tiles(ns, 600, 256, 0, BLOCKS) == (32, 561, 5) and sc._tiles(ns, 600, 256, 5, BLOCKS) == (32, 561, 2)
    assert sc._tiles(ns, 600, 256, 0)[2] == 1 == sc._tiles(ns, 600, 256, 5)[2]     # (without the switch: one slice, no `partial`)
    assert SHAPES["large"][2] == 2 * sc.SDISTW_BATCH + 1
    assert SHAPES["small"][0] % 2 == 1 and SHAPES["small"][0] > sc.SMALL and sc._tiles(67, 90, 256, 0, BLOCKS) == (32, 6, 2) and sc._tiles(9, 40, 256, 0, BLOCKS)[0] == 16
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tatajuba_amd", "csrc", "hopo_device.hip")) as src:
        text = src.read()
    for define in ("#define SDIST_CELLS %d " % sc.SDIST_CELLS, "#define SDISTW_BATCH %d " % sc.SDISTW_BATCH, "#define LINK_SMALL %d\n" % sc.SMALL,
                   "#define CLD_SMALL %d " % sc.SMALL, "used += (count * sizeof (T) + 255) & ~(size_t) 255;",
                   "#define REP_FLAGS %d\n" % sc.REP_FLAGS, "const size_t REP_SCRATCH_CAP = (size_t) 1 << 30;", "ldc = (ld + 64 + 63) & ~63;", "} piece[%d];" % sc.PIECES,
                   "const size_t per = small ? 0 : (size_t) ns * ld * 8 + 2 * (size_t) ldc * 4 + 2 * (size_t) ns * 16 + (size_t) ns * 4 + (size_t) (ns - 1) * 16;",
                   "std::min<size_t> ((size_t) R, REP_SCRATCH_CAP / per)", "const size_t n1 = (size_t) std::max (n, 1l);",
                   # the pieces in the order of the cut.take lines
                   "cut.take (A.comp, Gs * ldc); cut.take (A.size, Gs * ldc); cut.take (A.rowbest, Gs * ns); cut.take (A.edges, Gs * ns); cut.take (A.pairs, Gs * ns);\n"
                   "  cut.take (A.links, Gs * (ns - 1)); cut.take (A.keys, Gs * ns * ld); cut.take (A.rflags, (size_t) R * REP_FLAGS);\n",
                   "cut.take (key[0], n1); cut.take (key[1], n1); cut.take (val[0], n1); cut.take (val[1], n1); cut.take (head, n1); cut.take (hex, n1); cut.take (lead, n1);\n"
                   "  cut.take (cls, n1); cut.take (cnt, n1); cut.take (pos, (size_t) R * ns); cut.take (reps, (size_t) 2 * R + 1); cut.take (rbad, (size_t) R);\n"
                   "  cut.take (kept, (size_t) ns); cut.take (kpar, (size_t) 2 * ns); cut.take (info, (size_t) 2 * ns);\n",
                   "struct ConsKept { int size, minm, count, rep, first, pad; };", "const unsigned short *pos;"):
        assert define in text, define


# ---- the problems -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def consensus_input(name):
    """the replicates tjamd_consensus_tree is called on -> (rep_nodes, rep_orders, counts) as tests/test_consensus_cabi.py packs them"""
    ns, _, n_rep = SHAPES[name]
    return pack(fabricate_replicates(ns, n_rep, 1 + ns // 64, 100 + ns), ns)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_consensus_inputs_are_worth_a_consensus(name):
    ns, _, n_rep = SHAPES[name]
    want = restate_consensus(*consensus_input(name), ns, majority(n_rep))
    assert len(want["nodes"]) >= ns // 2 and want["n_classes"] > len(want["nodes"]), (len(want["nodes"]), want["n_classes"])


def new_counter(**switches):
    """a counter made under TATAJUBA_AMD_DISTANCE_BLOCKS=4096 and the switches given (read when the counter is made)"""
    env = dict({"TATAJUBA_AMD_DISTANCE_BLOCKS": str(BLOCKS)}, **switches)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return tj.Counter(15)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Problem:
    """a full set of inputs for all twelve entries; what one entry needs from another is made once, on a counter of its own"""

    def __init__(self, name):
        self.name = name
        self.ns, self.n_sites, self.n_rep = ns, n_sites, n_rep = SHAPES[name]
        self.seed = 100 + ns
        self.sites, self.alleles, self.g = fabricate(n_sites, ns, np.random.RandomState(self.seed))
        self.n_alleles = len(self.alleles)
        self.sd, self.ad, self.gd = dev(self.sites), dev(self.alleles), dev(self.g)
        prep = new_counter()
        try:
            self._prepare(prep)
        finally:
            prep.close()

    def _prepare(self, prep):
        ns, n_sites, n_rep = self.ns, self.n_sites, self.n_rep
        ok = lambda r: r if r.rc >= 0 else pytest.fail(r.err)
        keep = lambda g, nbytes=None: g.payload[: g.nbytes if nbytes is None else nbytes].clone()
        w = ok(sc.call_bootstrap_weights(prep, n_sites, n_rep, self.seed))
        self.wd, self.w = keep(w["d_weights"]), w["d_weights"].view(np.int32).reshape(n_rep, n_sites)
        d = ok(sc.call_sample_distances(prep, self.sd, n_sites, self.ad, self.n_alleles, self.gd, ns))
        self.dd, self.dist = keep(d["d_out"]), d["d_out"].view(DIST).reshape(ns, ns)
        l = ok(sc.call_sample_linkage(prep, self.dd, ns, DIFFER, 1))
        self.n_links = l.rc
        self.ld, self.links = keep(l["d_links"], l.rc * LINK.itemsize), l["d_links"].view(LINK, l.rc)
        assert self.n_links == ns - 1
        self.threshold = int(np.sort(self.links["key"])[self.n_links // 2]) - 1          # below the median key: ties leave one group at it
        cl = ok(sc.call_linkage_clusters(prep, self.ld, self.n_links, ns, self.threshold))
        self.n_groups, self.labels_d, self.labels = cl.rc, keep(cl["d_cluster"]), cl["d_cluster"].view(np.int32)
        assert 2 <= self.n_groups <= ns
        t = ok(sc.call_linkage_tree(prep, self.ld, self.n_links, ns))
        self.nd, self.od = keep(t["d_nodes"]), keep(t["d_order"])
        self.nodes, self.order = t["d_nodes"].view(NODE), t["d_order"].view(np.int32)
        # the sites that the groups and the clades are read from: random cells mark nothing among a thousand samples, so every second
        # site carries allele 1 in one clade, or in one group, and the genome's length elsewhere; a tenth of the cells are missing
        rng = np.random.RandomState(self.seed + 1)
        self.g_marks = self.g.copy()
        for i in range(0, n_sites, 2):
            if i % 4:
                members = np.flatnonzero(self.labels == rng.randint(self.n_groups))
            else:
                nd = self.nodes[rng.randint(self.n_links)]
                members = self.order[int(nd["first"]): int(nd["first"]) + int(nd["size"])]
            self.g_marks[i] = 0
            self.g_marks[i, members] = 1
            self.g_marks[i, rng.random_sample(ns) < 0.1] = -1
        self.gmd = dev(self.g_marks)
        gs = ok(sc.call_group_sites(prep, self.sd, n_sites, self.gmd, ns, self.labels_d, self.n_groups, 1, n_sites * min(ns, self.n_groups)))
        cs = ok(sc.call_clade_sites(prep, self.sd, n_sites, self.gmd, ns, self.nd, self.n_links, self.od, 1, n_sites * self.n_links))
        self.group_cap, self.clade_cap = gs.rc, cs.rc                       # the marks there are: the capacity from here on
        assert self.group_cap >= n_sites // 8 and self.clade_cap >= n_sites // 8
        wd = ok(sc.call_sample_distances_weighted(prep, self.sd, n_sites, self.ad, self.n_alleles, self.gd, ns, self.wd, n_rep))
        self.rep_dist = wd["d_out"].view(DIST).reshape(n_rep, ns, ns)
        rep_nodes = np.zeros(n_rep * (ns - 1), NODE)
        rep_nodes["first"], rep_nodes["size"] = -7, -7                            # beyond a replicate's count: never read
        rep_order, self.counts, self.reps = np.zeros(n_rep * ns, np.int32), [], []
        per = ns * ns * DIST.itemsize
        for r in range(n_rep):
            rl = ok(sc.call_sample_linkage(prep, wd["d_out"].payload[r * per: (r + 1) * per], ns, DIFFER, 1))
            rt = ok(sc.call_linkage_tree(prep, rl["d_links"].payload[: rl.rc * LINK.itemsize], rl.rc, ns))
            rn, ro = rt["d_nodes"].view(NODE, rl.rc), rt["d_order"].view(np.int32)
            rep_nodes[r * (ns - 1): r * (ns - 1) + rl.rc], rep_order[r * ns: (r + 1) * ns] = rn, ro
            self.counts.append(rl.rc)
            self.reps.append((rn, ro))
        self.rep_nodes, self.rnd, self.rod = rep_nodes, dev(rep_nodes), dev(rep_order)
        self.rep_dd = dev(self.rep_dist)
        self.cons_nodes, self.cons_orders, self.cons_counts = consensus_input(self.name)
        self.cnd, self.cod, self.min_count = dev(self.cons_nodes), dev(self.cons_orders), majority(n_rep)


def signature(r, *more):
    """a call's return value, its counts and every byte of its outputs"""
    assert r.rc >= 0 and r.ms >= 0, (r.rc, r.err, r.ms)
    return (r.rc, tuple(more), {name: g.view(np.uint8).tobytes() for name, g in r.outs.items()})


def run_agglomerate(c, p):
    both = [sc.call_sample_agglomerate(c, p.dd, p.ns, DIFFER, 1, linkage) for linkage in (COMPLETE, AVERAGE)]
    return tuple(signature(r, r.n_rounds) for r in both)


def run_replicate_trees(c, p):
    out = [sc.call_replicate_trees(c, p.rep_dd, p.ns, p.n_rep, DIFFER, 1, linkage) for linkage in LINKAGES]
    return tuple(signature(r, r.n_nodes, r.n_rounds) for r in out)


ENTRIES = {
    "tjamd_sample_distances": lambda c, p: signature(sc.call_sample_distances(c, p.sd, p.n_sites, p.ad, p.n_alleles, p.gd, p.ns)),
    "tjamd_bootstrap_weights": lambda c, p: signature(sc.call_bootstrap_weights(c, p.n_sites, p.n_rep, p.seed)),
    "tjamd_sample_distances_weighted": lambda c, p: signature(sc.call_sample_distances_weighted(c, p.sd, p.n_sites, p.ad, p.n_alleles, p.gd, p.ns, p.wd, p.n_rep)),
    "tjamd_sample_linkage": lambda c, p: signature(sc.call_sample_linkage(c, p.dd, p.ns, DIFFER, 1)),
    "tjamd_linkage_clusters": lambda c, p: signature(sc.call_linkage_clusters(c, p.ld, p.n_links, p.ns, p.threshold)),
    "tjamd_group_sites": lambda c, p: (lambda r: signature(r, r.n_marks))(sc.call_group_sites(c, p.sd, p.n_sites, p.gmd, p.ns, p.labels_d, p.n_groups, 1, p.group_cap)),
    "tjamd_linkage_tree": lambda c, p: signature(sc.call_linkage_tree(c, p.ld, p.n_links, p.ns)),
    "tjamd_clade_sites": lambda c, p: (lambda r: signature(r, r.n_marks))(sc.call_clade_sites(c, p.sd, p.n_sites, p.gmd, p.ns, p.nd, p.n_links, p.od, 1, p.clade_cap)),
    "tjamd_sample_agglomerate": run_agglomerate,
    "tjamd_clade_support": lambda c, p: signature(sc.call_clade_support(c, p.nd, p.n_links, p.od, p.ns, p.rnd, p.rod, p.counts)),
    "tjamd_replicate_trees": run_replicate_trees,
    "tjamd_consensus_tree": lambda c, p: (lambda r: signature(r, r.n_classes))(sc.call_consensus_tree(c, p.cnd, p.cod, p.cons_counts, p.ns, p.min_count)),
}
WITH_A_SMALL_FORM = ("tjamd_sample_linkage", "tjamd_sample_agglomerate", "tjamd_group_sites", "tjamd_clade_sites", "tjamd_replicate_trees")
assert {k[0] for k in SMALL_CUTS} == set(ENTRIES)


def check_against_the_restatements(p, fresh):
    """a small problem's fresh results are right, and what the preparation counter made is what the fresh counters make"""
    out = lambda entry, i=None: (fresh[entry, p.name] if i is None else fresh[entry, p.name][i])
    ns, na = p.ns, p.sites["n_alleles"]
    rc, _, o = out("tjamd_sample_distances")
    dist = restate_sample_distances(p.sites, p.alleles, p.g)
    assert rc == p.n_sites and o["d_out"] == dist.tobytes() == p.dist.tobytes()
    rc, _, o = out("tjamd_bootstrap_weights")
    assert rc == p.n_rep and o["d_weights"] == restate_bootstrap_weights(p.n_sites, p.n_rep, p.seed).tobytes() == p.w.tobytes()
    rc, _, o = out("tjamd_sample_distances_weighted")
    assert rc == p.n_sites and o["d_out"] == restate_sample_distances_weighted(p.sites, p.alleles, p.g, p.w).tobytes() == p.rep_dist.tobytes()
    rc, _, o = out("tjamd_sample_linkage")
    links = restate_sample_linkage(dist, DIFFER, 1)
    assert rc == len(links) == ns - 1 and o["d_links"] == links.tobytes() == p.links.tobytes()
    rc, _, o = out("tjamd_linkage_clusters")
    labels = restate_linkage_clusters(links, ns, p.threshold)
    assert rc == labels.max() + 1 == p.n_groups and o["d_cluster"] == labels.tobytes() == p.labels.tobytes()
    rc, (n_marks,), o = out("tjamd_group_sites")
    want = restate_group_sites(na, p.g_marks, labels, p.n_groups, 1)
    assert rc == n_marks == len(want["marks"]) == p.group_cap
    assert (o["d_calls"], o["d_site_out"], o["d_group_marks"], o["d_marks"]) == tuple(want[k].tobytes() for k in ("calls", "sites", "group_marks", "marks"))
    rc, _, o = out("tjamd_linkage_tree")
    tree = restate_linkage_tree(links, ns)
    assert rc == ns - 1 and o["d_nodes"] == tree["nodes"].tobytes() == p.nodes.tobytes() and o["d_order"] == tree["order"].tobytes() == p.order.tobytes()
    rc, (n_marks,), o = out("tjamd_clade_sites")
    want = restate_clade_sites(na, p.g_marks, tree["nodes"], tree["order"], 1)
    assert rc == n_marks == len(want["marks"]) == p.clade_cap
    assert (o["d_calls"], o["d_site_out"], o["d_node_marks"], o["d_marks"]) == tuple(want[k].tobytes() for k in ("calls", "sites", "node_marks", "marks"))
    for i, linkage in enumerate((COMPLETE, AVERAGE)):
        rc, (n_rounds,), o = out("tjamd_sample_agglomerate", i)
        want, rounds = restate_sample_agglomerate(dist, DIFFER, 1, linkage)
        assert rc == len(want) == ns - 1 and n_rounds == rounds and o["d_links"] == want.tobytes()
    reps = []
    for r in range(p.n_rep):
        t = restate_linkage_tree(restate_sample_linkage(p.rep_dist[r], DIFFER, 1), ns)
        assert (t["nodes"].tobytes(), t["order"].tobytes()) == (p.reps[r][0].tobytes(), p.reps[r][1].tobytes())
        reps.append((t["nodes"], t["order"]))
    rc, _, o = out("tjamd_clade_support")
    want = restate_clade_support(tree["nodes"], tree["order"], reps)
    assert rc == ns - 1 and o["d_support"] == want.tobytes() and 0 < want.max() and want.min() < want.max()
    for i, linkage in enumerate(LINKAGES):
        rc, (n_nodes, n_rounds), o = out("tjamd_replicate_trees", i)
        want = restate_replicate_trees(p.rep_dist, DIFFER, 1, linkage)
        assert rc == p.n_rep and n_nodes == tuple(len(t["nodes"]) for t in want) and n_rounds == tuple(t["n_rounds"] for t in want), linkage
        assert linkage == SINGLE or max(n_rounds) > 1
        for r, t in enumerate(want):                                          # (entries past a replicate's count: left as they were)
            at, n = r * (ns - 1) * 16, len(t["nodes"]) * 16
            assert o["d_rep_links"][at: at + n] == t["links"].tobytes() and o["d_rep_nodes"][at: at + n] == t["nodes"].tobytes(), (linkage, r)
            assert o["d_rep_order"][r * ns * 4: (r + 1) * ns * 4] == t["order"].tobytes(), (linkage, r)
            if linkage == SINGLE:                                             # what the preparation counter made replicate by replicate
                assert (t["nodes"].tobytes(), t["order"].tobytes()) == (p.reps[r][0].tobytes(), p.reps[r][1].tobytes())
    rc, (n_classes,), o = out("tjamd_consensus_tree")
    want = restate_consensus(p.cons_nodes, p.cons_orders, p.cons_counts, ns, p.min_count)
    assert rc == len(want["nodes"]) >= ns // 2 and n_classes == want["n_classes"] > rc
    assert o["d_nodes"][: rc * 16] == want["nodes"].tobytes() and o["d_order"] == want["order"].tobytes()
    for r, counts in enumerate(want["rep_count"]):
        assert o["d_rep_count"][r * (ns - 1) * 4: (r * (ns - 1) + len(counts)) * 4] == counts.tobytes(), r


class World:
    def __init__(self):
        self.p = {name: Problem(name) for name in SHAPES}
        self.fresh = {}
        for p in self.p.values():                                             # every entry on a counter of its own
            for name, entry in ENTRIES.items():
                f = new_counter()
                self.fresh[name, p.name] = entry(f, p)
                f.close()
        for name in SMALLS:
            check_against_the_restatements(self.p[name], self.fresh)
        self.poison = fabricate(POISON_SITES, POISON_SAMPLES, np.random.RandomState(1), n_alleles=[1] * POISON_SITES, p_missing=0.0, p_ref=1.0,
                                ref_length=2 ** 31 - 1)
        assert not self.poison[2].any() and (self.poison[0]["ref_length"] == 2 ** 31 - 1).all()
        self.poison_d = tuple(dev(x) for x in self.poison)


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture
def counter():
    c = new_counter()
    yield c
    c.close()


def small_equal_fresh(c, world, entry, what, names=SMALLS):
    for name in names:
        assert ENTRIES[entry](c, world.p[name]) == world.fresh[entry, name], (entry, name, what)


# ---- 1. after a large call --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("x", list(ENTRIES))
def test_small_calls_after_a_large_one(world, counter, x):
    large = world.p["large"]
    for y in ENTRIES:
        assert ENTRIES[x](counter, large) == world.fresh[x, "large"], (x, "large, before", y)
        small_equal_fresh(counter, world, y, "after " + x)
    assert ENTRIES[x](counter, large) == world.fresh[x, "large"], (x, "large again")


# ---- 2. after poison ----------------------------------------------------------------------------------------------------------

def poison_lens(c, world):
    sd, ad, gd = world.poison_d
    r = sc.call_sample_distances(c, sd, POISON_SITES, ad, POISON_SITES, gd, POISON_SAMPLES)
    assert r.rc == POISON_SITES, (r.rc, r.err)


def poison_keys(c, world):
    large = world.p["large"]
    r = sc.call_sample_linkage(c, large.dd, large.ns, DIFFER, 2 ** 31 - 1)
    assert r.rc == 0, (r.rc, r.err)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [poison_lens, poison_keys], ids=["P1: lens of 0x7fffffff", "P2: keys of all ones"])
def test_small_calls_after_poison(world, counter, poison):
    for y in ENTRIES:
        for name in SMALLS:
            poison(counter, world)
            small_equal_fresh(counter, world, y, poison.__name__, (name,))


# ---- 3. after a refusal -------------------------------------------------------------------------------------------------------
# A refusal is (the words of its message, make): make(p) builds the bad input once and gives the call.  Each bad input is the
# large problem's with one value changed; the places are those of the per-entry tests' device refusals.

CELL, MIRROR = "a cell has n_both < 0, n_differ < 0, n_differ > n_both or length_diff < 0", "differs from the cell (b, a)"
GENOTYPE = "a genotype cell is below -1 or above its site's n_alleles"
N_ALLELES, NODE_TEXT = "a site has n_alleles < 1 or above n_samples", "a node has size < 2, first < 0 or first + size above n_samples"


def _changed(a, field, at, value):
    b = a.copy()
    if field is None:
        b[at] = value
    else:
        b[field][at] = value
    return dev(b)


def _last_cell(p):
    return (p.n_sites - 1, p.ns - 1), -2


def _twice(p):
    return 4, int(p.order[0])


def distances(weighted, **bad):
    """bad: the one input that is replaced -> p -> (field,) place, value"""
    def make(p):
        sd = _changed(p.sites, *bad["sites"](p)) if "sites" in bad else p.sd
        ad = _changed(p.alleles, *bad["alleles"](p)) if "alleles" in bad else p.ad
        gd = _changed(p.g, None, *bad["g"](p)) if "g" in bad else p.gd
        wd = _changed(p.w, None, *bad["w"](p)) if "w" in bad else p.wd
        if weighted:
            return lambda c: sc.call_sample_distances_weighted(c, sd, p.n_sites, ad, p.n_alleles, gd, p.ns, wd, p.n_rep)
        return lambda c: sc.call_sample_distances(c, sd, p.n_sites, ad, p.n_alleles, gd, p.ns)
    return make


def matrix(call, changes):
    def make(p):
        d = p.dist.copy()
        for field, at, value in changes(p, d):
            d[field][at] = value
        dd = dev(d)
        return lambda c: call(c, p, dd)
    return make


def links(call, change):
    def make(p):
        l = p.links.copy()
        change(p, l)
        ld = dev(l)
        return lambda c: call(c, p, ld)
    return make


def marks(groups, **bad):
    def make(p):
        sd = _changed(p.sites, *bad["sites"](p)) if "sites" in bad else p.sd
        gd = _changed(p.g_marks, None, *bad["g"](p)) if "g" in bad else p.gmd
        labels = _changed(p.labels, None, *bad["labels"](p)) if "labels" in bad else p.labels_d
        nd = _changed(p.nodes, *bad["nodes"](p)) if "nodes" in bad else p.nd
        od = _changed(p.order, None, *bad["order"](p)) if "order" in bad else p.od
        if groups:
            return lambda c: sc.call_group_sites(c, sd, p.n_sites, gd, p.ns, labels, p.n_groups, 1, p.group_cap)
        return lambda c: sc.call_clade_sites(c, sd, p.n_sites, gd, p.ns, nd, p.n_links, od, 1, p.clade_cap)
    return make


def support(**bad):
    def make(p):
        od = _changed(p.order, None, *bad["order"](p)) if "order" in bad else p.od
        rnd = _changed(p.rep_nodes, None, *bad["rep_nodes"](p)) if "rep_nodes" in bad else p.rnd
        return lambda c: sc.call_clade_support(c, p.nd, p.n_links, od, p.ns, rnd, p.rod, p.counts)
    return make


def replicate_trees(metric, linkage, changes):
    """changes: p, the last replicate's matrix -> [(field, cell, value)]"""
    def make(p):
        d = p.rep_dist.copy()
        for field, at, value in changes(p, d[p.n_rep - 1]):
            d[field][p.n_rep - 1][at] = value
        dd = dev(d)

        def call(c):
            r = sc.call_replicate_trees(c, dd, p.ns, p.n_rep, metric, 1, linkage)
            assert r.rc >= 0 or (r["h_rep_n_nodes"].untouched() and r["h_rep_n_rounds"].untouched() and r.err.endswith("(replicate %d)" % (p.n_rep - 1))), r.err
            return r
        return call
    return make


def consensus(order=None, nodes=None):
    """order: p, the last replicate's order -> place, value; nodes: p, its nodes -> [(node, first, size)]"""
    def make(p):
        last = p.n_rep - 1
        cn, co = p.cons_nodes.copy(), p.cons_orders.copy()
        if order:
            at, value = order(p, co[last * p.ns: (last + 1) * p.ns])
            co[last * p.ns + at] = value
        for k, first, size in (nodes(p, cn[last * (p.ns - 1): last * (p.ns - 1) + p.cons_counts[last]]) if nodes else ()):
            cn[last * (p.ns - 1) + k]["first"], cn[last * (p.ns - 1) + k]["size"] = first, size
        cnd, cod = dev(cn), dev(co)

        def call(c):
            r = sc.call_consensus_tree(c, cnd, cod, p.cons_counts, p.ns, p.min_count)
            assert r.rc >= 0 or (r.n_classes == UNSET and "replicate %d" % last in r.err), r.err
            return r
        return call
    return make


def _a_key_of_2_40(p, d):
    """a pair that is an edge whatever the weights gave it, with a length_diff of 2^40"""
    both = max(int(d["n_both"][2, 5]), 1)
    return [(f, at, v) for f, v in (("length_diff", 1 << 40), ("n_both", both)) for at in ((2, 5), (5, 2))]


def _crossing(p, nodes):
    """two nodes of two samples each become (1, n_samples - 2) and (2, n_samples - 2): they overlap and neither holds the other"""
    two = [k for k in range(len(nodes)) if nodes[k]["size"] == 2][:2]
    assert len(two) == 2
    return [(two[0], 1, p.ns - 2), (two[1], 2, p.ns - 2)]


def _over(p, d):
    """a cell and its mirror with n_differ above n_both"""
    a, b = 5, p.ns - 10
    return [("n_differ", (a, b), int(d["n_both"][a, b]) + 1), ("n_differ", (b, a), int(d["n_both"][a, b]) + 1)]


def _cycle(p, l):
    l[len(l) - 1] = l[0]


def _set(field, at, value):
    def change(p, l):
        l[field][at(p)] = value(p)
    return change


_linkage = lambda c, p, dd: sc.call_sample_linkage(c, dd, p.ns, DIFFER, 1)
_complete = lambda c, p, dd: sc.call_sample_agglomerate(c, dd, p.ns, DIFFER, 1, COMPLETE)
_average_of_lengths = lambda c, p, dd: sc.call_sample_agglomerate(c, dd, p.ns, LENGTH, 1, AVERAGE)
_clusters = lambda c, p, ld: sc.call_linkage_clusters(c, ld, p.n_links, p.ns, p.threshold)
_tree = lambda c, p, ld: sc.call_linkage_tree(c, ld, p.n_links, p.ns)
_middle = lambda p: p.n_links // 2

REFUSALS = {}
for _w, _entry in ((False, "distances"), (True, "weighted")):
    REFUSALS.update({
        _entry + " 1: a genotype cell": (GENOTYPE, distances(_w, g=_last_cell)),
        _entry + " 8: the allele chain": ("do not chain from 0 to", distances(_w, sites=lambda p: ("first_allele", p.n_sites // 2, int(p.sites["first_allele"][p.n_sites // 2]) + 1))),
        _entry + " 16: n_alleles": ("a site has n_alleles < 1", distances(_w, sites=lambda p: ("n_alleles", 0, 0))),
        _entry + " 32: an allele's site": ("an allele's site is not the site that holds it", distances(_w, alleles=lambda p: ("site", p.n_alleles - 1, -1))),
        _entry + " 64: alt_length": ("an allele's alt_length is outside 0..1023", distances(_w, alleles=lambda p: ("alt_length", 5, 1024))),
        _entry + " 128: ref_length": ("a site's ref_length is below 0", distances(_w, sites=lambda p: ("ref_length", 7, -1))),
    })
REFUSALS.update({
    "weighted 256: a weight below 0": ("a weight is below 0", distances(True, w=lambda p: ((p.n_rep - 1, p.n_sites - 1), -1))),
    "weighted 512: a sum of 2^31": ("the weights of a replicate sum to 2^31 or more", distances(True, w=lambda p: ((2, 13), 2 ** 31 - 1))),
    "linkage 1: a cell": (CELL, matrix(_linkage, _over)),
    "linkage 2: a mirror": (MIRROR, matrix(_linkage, lambda p, d: [("n_both", (p.ns - 1, 3), int(d["n_both"][p.ns - 1, 3]) + 1)])),
    "agglomerate 1: a cell": (CELL, matrix(_complete, _over)),
    "agglomerate 2: a mirror": (MIRROR, matrix(_complete, lambda p, d: [("length_diff", (0, p.ns - 30), int(d["length_diff"][0, p.ns - 30]) + 1)])),
    "agglomerate 4: a key of 2^40": ("a key of 2^40 or more under TJAMD_AGGL_AVERAGE", matrix(_average_of_lengths, lambda p, d: [("length_diff", (2, 5), 1 << 40), ("length_diff", (5, 2), 1 << 40)])),
    "clusters: a bad link": ("a link has a < 0, a >= b, b >= n_samples or key < 0", links(_clusters, _set("b", _middle, lambda p: p.ns))),
    "tree: a bad end": ("a link has a < 0, a >= b or b >= n_samples", links(_tree, _set("a", _middle, lambda p: -1))),
    "tree: a cycle": ("a link joins two samples that the links before it have joined: a cycle", links(_tree, _cycle)),
    "groups: a label": ("a label is below -1 or not below n_groups", marks(True, labels=lambda p: (5, p.n_groups))),
    "groups: n_alleles": (N_ALLELES, marks(True, sites=lambda p: ("n_alleles", 3, 0))),
    "groups: a genotype cell": (GENOTYPE, marks(True, g=_last_cell)),
    "clades: the order": ("d_order is not a permutation of 0 .. n_samples - 1", marks(False, order=_twice)),
    "clades: a node": (NODE_TEXT, marks(False, nodes=lambda p: ("size", _middle(p), 1))),
    "clades: n_alleles": (N_ALLELES, marks(False, sites=lambda p: ("n_alleles", 3, 0))),
    "clades: a genotype cell": (GENOTYPE, marks(False, g=_last_cell)),
    "support 1: an order": ("is not a permutation of 0 .. n_samples - 1", support(order=_twice)),
    "support 2: a node": (NODE_TEXT, support(rep_nodes=lambda p: ((p.n_rep - 1) * (p.ns - 1) + 1, (0, 0, p.ns - 1, 2)))),
    "trees 1: a cell": (CELL, replicate_trees(DIFFER, COMPLETE, _over)),
    "trees 2: a mirror": (MIRROR, replicate_trees(DIFFER, SINGLE, lambda p, d: [("n_both", (p.ns - 1, 3), int(d["n_both"][p.ns - 1, 3]) + 1)])),
    "trees 4: a key of 2^40": ("a key of 2^40 or more under TJAMD_AGGL_AVERAGE", replicate_trees(LENGTH, AVERAGE, _a_key_of_2_40)),
    "consensus 1: an order": ("is not a permutation of 0 .. n_samples - 1", consensus(order=lambda p, o: (4, int(o[0])))),
    "consensus 2: a node": ("has size < 2, first < 0 or first + size above n_samples", consensus(nodes=lambda p, n: [(len(n) // 2, p.ns - 1, 2)])),
    "consensus 4: crossing nodes": ("cross (they overlap and neither contains the other)", consensus(nodes=_crossing)),
})
# distances and weighted: bits 1, 8, 16, 32, 64, 128, and 256 and 512; linkage 1, 2; agglomerate 1, 2, 4; a bad link; a bad end and
# a cycle; the three texts of the groups and the four of the clades; support 1, 2; the trees of the replicates 1, 2, 4; the consensus
# 1, 2, 4.  The last two entries' refusals lie in the last replicate, which their callers hold the message to.
assert len(REFUSALS) == 6 + 8 + 2 + 3 + 1 + 2 + 3 + 4 + 2 + 3 + 3


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(REFUSALS))
def test_small_calls_after_a_refusal(world, counter, kind):
    text, make = REFUSALS[kind]
    refuse = make(world.p["large"])

    def refused():
        r = refuse(counter)
        assert r.rc == -ERR_ARG and text in r.err, (kind, r.rc, r.err)
        assert r.ms == -1.0 and all(g.untouched() for g in r.outs.values()), kind     # nothing written, no timing left behind
        return r.rc, r.err

    first = refused()
    for i, y in enumerate(ENTRIES):
        assert i == 0 or refused() == first
        small_equal_fresh(counter, world, y, "after the refusal " + kind, ("small",))
    assert refused() == first                                                 # an error word is latched neither way


# ---- 4. the forms -------------------------------------------------------------------------------------------------------------

FORM_SWITCHES = ("TATAJUBA_AMD_LINKAGE_SMALL", "TATAJUBA_AMD_GROUPS_SMALL", "TATAJUBA_AMD_CLADES_SMALL")


@pytest.fixture
def large_forms_counter():
    """a counter whose calls never take a one-workgroup or wavefront-per-site form: the tiny problem goes through the scratch too"""
    c = new_counter(**{k: "0" for k in FORM_SWITCHES})
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("x", WITH_A_SMALL_FORM)
def test_small_calls_after_a_large_one_in_the_large_forms(world, large_forms_counter, x):
    c, large = large_forms_counter, world.p["large"]
    for y in WITH_A_SMALL_FORM:
        assert ENTRIES[x](c, large) == world.fresh[x, "large"], (x, "large, before", y)
        small_equal_fresh(c, world, y, "after " + x)
    assert ENTRIES[x](c, large) == world.fresh[x, "large"], (x, "large again")
