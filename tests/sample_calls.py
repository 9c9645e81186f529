"""One caller per entry of the sample-comparison layer (N14-N21: distances, bootstrap weights, weighted distances, linkage,
clusters, group sites, tree, clade sites, agglomerate, clade support, replicate trees, consensus tree), in the style of tests/bounds_calls.py: every output in a
guarded buffer of exactly the size the header asks for, every const input frozen, guards and inputs checked before the caller
returns; and the bytes that each of these entries cuts from the counter's scratch block, restated from hopo_device.hip.
tests/test_sample_reuse.py calls through these.  An entry of this layer that cuts scratch gets a caller and a line here.

The inputs are device tensors (tests/bounds_calls.py: dev), made once per problem by the caller's caller.  A Result carries the
return value, the message of a refused call, the guarded outputs, and .ms, the entry's timer read after the call."""
import ctypes as C

import tatajuba_amd as tj
import numpy as np

from tests.bounds_calls import Result, _buffers, _checked, _p
from tests.guarded import frozen

DIST, LINK, NODE = tj.SAMPLE_DISTANCE_DTYPE, tj.LINK_DTYPE, tj.TREE_NODE_DTYPE
CALL, GSITE, MARK = tj.GROUP_CALL_DTYPE, tj.GROUP_SITE_DTYPE, tj.GROUP_MARK_DTYPE
CNODE = tj.CONSENSUS_NODE_DTYPE
UNSET = -77                              # what a scalar output holds before the call

# entry -> the outputs it writes through caller pointers, each of which its caller below puts into a guarded buffer: this layer's
# part of the case table of tests/bounds_calls.py, read by tests/test_host_bounds.py.  An array on the host (h_rep_n_nodes) is an
# output like any other; a pointer to one scalar (h_n_rounds, h_n_marks, h_n_classes) has no row
OUTPUTS = {
    "tjamd_sample_distances": ("d_out",),
    "tjamd_bootstrap_weights": ("d_weights",),
    "tjamd_sample_distances_weighted": ("d_out",),
    "tjamd_sample_linkage": ("d_links",),
    "tjamd_sample_agglomerate": ("d_links",),
    "tjamd_linkage_clusters": ("d_cluster",),
    "tjamd_linkage_tree": ("d_nodes", "d_order"),
    "tjamd_group_sites": ("d_calls", "d_site_out", "d_group_marks", "d_marks"),
    "tjamd_clade_sites": ("d_calls", "d_site_out", "d_node_marks", "d_marks"),
    "tjamd_clade_support": ("d_support",),
    "tjamd_replicate_trees": ("d_rep_links", "d_rep_nodes", "d_rep_order", "h_rep_n_nodes", "h_rep_n_rounds"),
    "tjamd_consensus_tree": ("d_nodes", "d_order", "d_rep_count"),
}


def call_sample_distances(c, sd, n_sites, ad, n_alleles, gd, ns):
    """sd, ad, gd: device bytes of tjamd_site[n_sites], tjamd_allele[n_alleles] and int16 [n_sites, ns]"""
    outs = _buffers({"d_out": ns * ns * DIST.itemsize}, ())
    with frozen(sd, ad, gd):
        rc = tj.lib().tjamd_sample_distances(c._h, _p(sd), n_sites, _p(ad), n_alleles, _p(gd), ns, _p(outs["d_out"]))
        _checked(outs)
    return Result(rc, outs, ms=c.last_sample_distances_ms())


def call_bootstrap_weights(c, n_sites, n_rep, seed):
    outs = _buffers({"d_weights": n_rep * n_sites * 4}, ())
    rc = tj.lib().tjamd_bootstrap_weights(c._h, n_sites, n_rep, seed, _p(outs["d_weights"]))
    _checked(outs)
    return Result(rc, outs, ms=c.last_bootstrap_weights_ms())


def call_sample_distances_weighted(c, sd, n_sites, ad, n_alleles, gd, ns, wd, n_rep):
    """wd: device bytes of int32 [n_rep, n_sites]"""
    outs = _buffers({"d_out": n_rep * ns * ns * DIST.itemsize}, ())
    with frozen(sd, ad, gd, wd):
        rc = tj.lib().tjamd_sample_distances_weighted(c._h, _p(sd), n_sites, _p(ad), n_alleles, _p(gd), ns, _p(outs["d_out"]), _p(wd), n_rep)
        _checked(outs)
    return Result(rc, outs, ms=c.last_sample_distances_weighted_ms())


def call_sample_linkage(c, dd, ns, metric, min_both):
    """dd: device bytes of tjamd_sample_distance [ns, ns]"""
    outs = _buffers({"d_links": (ns - 1) * LINK.itemsize}, ())
    with frozen(dd):
        rc = tj.lib().tjamd_sample_linkage(c._h, _p(dd), ns, metric, min_both, _p(outs["d_links"]))
        _checked(outs)
    return Result(rc, outs, ms=c.last_sample_linkage_ms())


def call_sample_agglomerate(c, dd, ns, metric, min_both, linkage):
    outs = _buffers({"d_links": (ns - 1) * LINK.itemsize}, ())
    rounds = C.c_int(UNSET)
    with frozen(dd):
        rc = tj.lib().tjamd_sample_agglomerate(c._h, _p(dd), ns, metric, min_both, linkage, _p(outs["d_links"]), C.byref(rounds))
        _checked(outs)
    return Result(rc, outs, ms=c.last_sample_agglomerate_ms(), n_rounds=rounds.value)


def call_linkage_clusters(c, ld, n_links, ns, threshold):
    """ld: device bytes of tjamd_link[n_links]"""
    outs = _buffers({"d_cluster": ns * 4}, ())
    with frozen(ld):
        rc = tj.lib().tjamd_linkage_clusters(c._h, _p(ld), n_links, ns, threshold, _p(outs["d_cluster"]))
        _checked(outs)
    return Result(rc, outs, ms=c.last_linkage_clusters_ms())


def call_linkage_tree(c, ld, n_links, ns):
    outs = _buffers({"d_nodes": n_links * NODE.itemsize, "d_order": ns * 4}, ())
    with frozen(ld):
        rc = tj.lib().tjamd_linkage_tree(c._h, _p(ld), n_links, ns, _p(outs["d_nodes"]), _p(outs["d_order"]))
        _checked(outs)
    return Result(rc, outs, ms=c.last_linkage_tree_ms())


def call_group_sites(c, sd, n_sites, gd, ns, labels, n_groups, min_called, cap):
    """labels: device int32 [ns]; cap: the capacity of d_marks.  Every optional output is asked for"""
    outs = _buffers({"d_calls": n_sites * n_groups * CALL.itemsize, "d_site_out": n_sites * GSITE.itemsize, "d_group_marks": n_groups * 4, "d_marks": cap * MARK.itemsize}, ())
    n_marks = C.c_long(UNSET)
    with frozen(sd, gd, labels):
        rc = tj.lib().tjamd_group_sites(c._h, _p(sd), n_sites, _p(gd), ns, _p(labels), n_groups, min_called, _p(outs["d_calls"]), _p(outs["d_site_out"]),
                                        _p(outs["d_group_marks"]), _p(outs["d_marks"]), cap, C.byref(n_marks))
        _checked(outs)
    return Result(rc, outs, ms=c.last_group_sites_ms(), n_marks=n_marks.value)


def call_clade_sites(c, sd, n_sites, gd, ns, nd, n_nodes, od, min_called, cap):
    """nd, od: device bytes of tjamd_tree_node[n_nodes] and int32 [ns]"""
    outs = _buffers({"d_calls": n_sites * n_nodes * CALL.itemsize, "d_site_out": n_sites * GSITE.itemsize, "d_node_marks": n_nodes * 4, "d_marks": cap * MARK.itemsize}, ())
    n_marks = C.c_long(UNSET)
    with frozen(sd, gd, nd, od):
        rc = tj.lib().tjamd_clade_sites(c._h, _p(sd), n_sites, _p(gd), ns, _p(nd), n_nodes, _p(od), min_called, _p(outs["d_calls"]), _p(outs["d_site_out"]),
                                        _p(outs["d_node_marks"]), _p(outs["d_marks"]), cap, C.byref(n_marks))
        _checked(outs)
    return Result(rc, outs, ms=c.last_clade_sites_ms(), n_marks=n_marks.value)


def call_clade_support(c, nd, n_nodes, od, ns, rnd, rod, counts):
    """rnd, rod: device bytes of tjamd_tree_node [n_rep, ns - 1] and int32 [n_rep, ns]; counts: the nodes of every replicate"""
    outs = _buffers({"d_support": n_nodes * 4}, ())
    h_counts = (C.c_int * len(counts))(*counts)
    with frozen(nd, od, rnd, rod):
        rc = tj.lib().tjamd_clade_support(c._h, _p(nd), n_nodes, _p(od), ns, _p(rnd), _p(rod), h_counts, len(counts), _p(outs["d_support"]))
        _checked(outs)
    assert list(h_counts) == list(counts)
    return Result(rc, outs, ms=c.last_clade_support_ms())


def call_replicate_trees(c, dd, ns, n_rep, metric, min_both, linkage):
    """dd: device bytes of tjamd_sample_distance [n_rep, ns, ns].  The two host arrays are guarded like the device outputs: a call
    that leaves them alone leaves them untouched(); .n_nodes and .n_rounds are what they hold after the call"""
    outs = _buffers({"d_rep_links": n_rep * (ns - 1) * LINK.itemsize, "d_rep_nodes": n_rep * (ns - 1) * NODE.itemsize, "d_rep_order": n_rep * ns * 4,
                     "h_rep_n_nodes": n_rep * 4, "h_rep_n_rounds": n_rep * 4}, (), host=("h_rep_n_nodes", "h_rep_n_rounds"))
    with frozen(dd):
        rc = tj.lib().tjamd_replicate_trees(c._h, _p(dd), ns, n_rep, metric, min_both, linkage, _p(outs["d_rep_links"]), _p(outs["d_rep_nodes"]), _p(outs["d_rep_order"]),
                                            C.cast(outs["h_rep_n_nodes"].c, C.POINTER(C.c_int)), C.cast(outs["h_rep_n_rounds"].c, C.POINTER(C.c_int)))
        _checked(outs)
    return Result(rc, outs, ms=c.last_replicate_trees_ms(), n_nodes=tuple(outs["h_rep_n_nodes"].view(np.int32).tolist()),
                  n_rounds=tuple(outs["h_rep_n_rounds"].view(np.int32).tolist()))


def call_consensus_tree(c, rnd, rod, counts, ns, min_count):
    """rnd, rod: device bytes of tjamd_tree_node [n_rep, ns - 1] and int32 [n_rep, ns]; counts: the nodes of every replicate"""
    n_rep = len(counts)
    outs = _buffers({"d_nodes": (ns - 1) * CNODE.itemsize, "d_order": ns * 4, "d_rep_count": n_rep * (ns - 1) * 4}, ())
    h_counts, n_classes = (C.c_int * n_rep)(*counts), C.c_long(UNSET)
    with frozen(rnd, rod):
        rc = tj.lib().tjamd_consensus_tree(c._h, _p(rnd), _p(rod), h_counts, ns, n_rep, min_count, _p(outs["d_nodes"]), _p(outs["d_order"]), _p(outs["d_rep_count"]),
                                           C.byref(n_classes))
        _checked(outs)
    assert list(h_counts) == list(counts)
    return Result(rc, outs, ms=c.last_consensus_tree_ms(), n_classes=n_classes.value)


# ---- the scratch that each entry cuts ---------------------------------------------------------------------------------------
# ScratchCut of hopo_device.hip: the pieces of a call in the order they lie in the block, each on a 256-byte boundary, the first
# at offset 0.  n_cu: the device's compute units (256 on an MI355X): a distance call aims at 4 n_cu workgroups, or at dist_blocks
# where the counter was made under TATAJUBA_AMD_DISTANCE_BLOCKS, as every counter of tests/test_sample_reuse.py is.
# LINK_SMALL = CLD_SMALL = 64.  REP_FLAGS: the flag words tjamd_replicate_trees keeps per replicate of the call; REP_SCRATCH_CAP:
# the bytes its groups of replicates are sized for; PIECES: what one ScratchCut holds, the flag words included.

SDIST_CELLS, SDISTW_BATCH, SMALL = 2048, 2, 64
REP_FLAGS, REP_SCRATCH_CAP, PIECES = 8, 1 << 30, 16


def _r(nbytes):
    return (nbytes + 255) & ~255


def _tiles(ns, n_sites, n_cu, n_rep, dist_blocks=0):
    """the decomposition of both distance entries -> (tile edge, tile pairs, slices)"""
    want = dist_blocks or 4 * n_cu
    n_batches = (n_rep + SDISTW_BATCH - 1) // SDISTW_BATCH if n_rep else 1
    t64 = (ns + 63) // 64
    E = 8 if ns <= 8 else 16 if ns <= 16 else 64 if t64 * (t64 + 1) // 2 * n_batches >= (want + 1) // 2 else 32
    n_tiles = (ns + E - 1) // E
    n_pairs, chunk = n_tiles * (n_tiles + 1) // 2, SDIST_CELLS // E
    n_chunks = (n_sites + chunk - 1) // chunk
    n_slices = max(1, min(n_chunks, want // (n_pairs * n_batches)))
    per_slice = (n_chunks + n_slices - 1) // n_slices * chunk
    return E, n_pairs, (n_sites + per_slice - 1) // per_slice


def cut_distances(ns, n_sites, n_cu=256, n_rep=0, dist_blocks=0):
    """-> [(piece, offset, bytes)]: err, lens, partial.  n_rep 0: tjamd_sample_distances; otherwise the weighted entry"""
    E, n_pairs, n_slices = _tiles(ns, n_sites, n_cu, n_rep, dist_blocks)
    partial = (max(n_rep, 1) * n_slices * n_pairs * E * E * DIST.itemsize) if n_slices > 1 else 0
    return _layout([("err", 256), ("lens", 4 * n_sites * ns), ("partial", partial)])


def cut_linkage(ns, small_form=True):
    """comp, rowbest, edges, keys, flags: nothing but the flags in the one-workgroup form"""
    ld = (ns + 1) & ~1
    if ns <= SMALL and small_form:
        return _layout([("flags", 256)])
    return _layout([("comp", 4 * (ld + 64)), ("rowbest", 16 * ns), ("edges", 16 * ns), ("keys", 8 * ns * ld), ("flags", 256)])


def cut_agglomerate(ns, small_form=True):
    ld = (ns + 1) & ~1
    if ns <= SMALL and small_form:
        return _layout([("flags", 256)])
    return _layout([("size", 4 * (ld + 64)), ("comp", 4 * (ld + 64)), ("rowbest", 16 * ns), ("edges", 16 * ns), ("pairs", 4 * ns), ("keys", 8 * ns * ld), ("flags", 256)])


def cut_flags_alone():
    """tjamd_linkage_clusters and tjamd_linkage_tree"""
    return _layout([("flags", 256)])


def cut_marks(n_keys, n_sites):
    """tjamd_group_sites (n_keys: groups) and tjamd_clade_sites (nodes), in either form: the flags and every key's marks first"""
    return _layout([("flags", 4 * (64 + n_keys)), ("cnt", 4 * n_sites)])


def cut_support(n_nodes, n_rep):
    return _layout([("cnt", 4 * n_nodes), ("rep_n", 4 * n_rep), ("flags", 256)])


def rep_group(ns, n_rep, group=0, small_form=True):
    """-> (the bytes `per` of one replicate's pieces, the replicates G of a group); group: TATAJUBA_AMD_TREES_GROUP, 0 without it"""
    ld = (ns + 1) & ~1
    ldc = (ld + 64 + 63) & ~63
    if ns <= SMALL and small_form:
        return 0, min(n_rep, group) if group else n_rep
    per = ns * ld * 8 + 2 * ldc * 4 + 2 * ns * 16 + ns * 4 + (ns - 1) * 16
    return per, min(n_rep, group) if group else max(1, min(n_rep, REP_SCRATCH_CAP // per))


def cut_replicate_trees(ns, n_rep, group=0, small_form=True):
    """comp, size, rowbest, edges, pairs, links, keys of a group of replicates (comp and size ldc ints a replicate: ld + 64 rounded
    up to 64), the REP_FLAGS words of every replicate of the call, flags: nothing but the last two in the one-workgroup form"""
    ld = (ns + 1) & ~1
    ldc = (ld + 64 + 63) & ~63
    G = 0 if ns <= SMALL and small_form else rep_group(ns, n_rep, group, small_form)[1]
    return _layout([("comp", 4 * G * ldc), ("size", 4 * G * ldc), ("rowbest", 16 * G * ns), ("edges", 16 * G * ns), ("pairs", 4 * G * ns), ("links", 16 * G * (ns - 1)),
                    ("keys", 8 * G * ns * ld), ("rflags", 4 * n_rep * REP_FLAGS), ("flags", 256)])


def cut_consensus(n_clades, ns, n_rep):
    """the records (two buffers of keys and of values, head, hex, lead, cls, cnt: at least one record), the samples' positions,
    the counts and offsets of the replicates, their error words, the kept classes, flags: 16 pieces, as many as a cut holds"""
    n1 = max(n_clades, 1)
    return _layout([("key0", 8 * n1), ("key1", 8 * n1), ("val0", 4 * n1), ("val1", 4 * n1), ("head", 4 * n1), ("hex", 4 * n1), ("lead", 4 * n1), ("cls", 4 * n1), ("cnt", 4 * n1),
                    ("pos", 2 * n_rep * ns), ("reps", 4 * (2 * n_rep + 1)), ("rbad", 4 * n_rep), ("kept", 4 * ns), ("kpar", 4 * 2 * ns), ("info", 24 * 2 * ns), ("flags", 256)])


def _layout(pieces):
    assert len(pieces) <= PIECES
    out, at = [], 0
    for name, nbytes in pieces:
        out.append((name, at, nbytes))
        at += _r(nbytes)
    return out


def cut_bytes(layout):
    """the bytes of the block that a cut takes"""
    return sum(_r(nbytes) for _, _, nbytes in layout)


def piece(layout, name):
    """-> (first byte, one past the last byte written) of a piece"""
    (at, nbytes), = [(a, n) for p, a, n in layout if p == name]
    return at, at + nbytes
