"""Diagnostic: the figures of DESIGN 3.5 N17.  tjamd_linkage_tree and tjamd_clade_sites beside tjamd_group_sites, in one run.
1. 125 000 sites x 8 samples, the pipeline-sized input of tools/exp_group_sites.py: N8, N12, N13, N14, N15, then N16 on the
   clusters of the tree's cut at its median key and N17 on the tree itself, d_links handed over where they are.
2. fabricated matrices of 20 000 sites at 1024 and 4096 samples, made on the device: three alleles a site, a tenth of the cells
   not called, and at every 50th site the clade of one node alone carries the third allele (a mark by construction).  Each
   once with a chain tree (0,1),(1,2),..., n_samples - 1 nodes deep, and once with a balanced one, log2 n_samples deep; beside
   tjamd_group_sites on the same matrix with eight groups at random.  The first 40 sites are held to the restatement.
HIP-event timers of the library, twelve calls each, the median and range of the last ten.  The launches are computed: the
pass that checks and counts, the shared scan of the sites' counts (one launch up to 4096 sites, three up to 4096^2) and the
pass that writes; the tree is one launch.  The bytes are the matrix's, 2 a cell, read once by each pass.
   python tools/exp_clade_sites.py
   rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp_clade_sites.py"""
import ctypes as C, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p
from tests.test_clades_cabi import restate_clade_sites, restate_linkage_tree, tree_links
VAR, SITE, ALLELE, TR, LOC, DIST, LINK = tj.VARIANT_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE, tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE, tj.SAMPLE_DISTANCE_DTYPE, tj.LINK_DTYPE
CALL, GSITE, MARK, NODE = tj.GROUP_CALL_DTYPE, tj.GROUP_SITE_DTYPE, tj.GROUP_MARK_DTYPE, tj.TREE_NODE_DTYPE
L = tj.lib()

def last10(f):
    v = [f() for _ in range(12)][2:]
    return float(np.median(v)), f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})"

def tree_and_clades(tag, counter, links, n_links, ns, sites, n_sites, gt, min_called, check_first, h_na, h_gt):
    """the tree, then the list alone, then every output; the first check_first sites against the restatement"""
    nodes = torch.zeros(max(n_links, 1) * NODE.itemsize, dtype=torch.uint8, device="cuda"); order = torch.zeros(ns, dtype=torch.int32, device="cuda")
    def tree():
        assert counter.linkage_tree(_p(links), n_links, ns, _p(nodes), _p(order)) == n_links; return counter.last_linkage_tree_ms()
    _, text_tree = last10(tree)
    h_links = np.frombuffer(links.cpu().numpy().tobytes(), LINK)[:n_links]
    want_tree = restate_linkage_tree(h_links, ns)
    assert np.frombuffer(nodes.cpu().numpy().tobytes(), NODE)[:n_links].tobytes() == want_tree["nodes"].tobytes() and order.cpu().numpy().tobytes() == want_tree["order"].tobytes()
    try:
        counter.clade_sites(_p(sites), n_sites, _p(gt), ns, _p(nodes), n_links, _p(order), min_called)      # sized with capacity 0
        cap = 0
    except tj.capi.TatajubaAmdError as e:
        cap = e.n_marks
    marks = torch.zeros(max(cap, 1) * MARK.itemsize, dtype=torch.uint8, device="cuda"); nm = torch.zeros(max(n_links, 1), dtype=torch.int32, device="cuda")
    so = torch.zeros(n_sites * GSITE.itemsize, dtype=torch.uint8, device="cuda")
    with_calls = n_sites * n_links * CALL.itemsize <= 2 << 30
    calls = torch.zeros(n_sites * n_links * CALL.itemsize if with_calls else 16, dtype=torch.uint8, device="cuda")
    def listed():
        assert counter.clade_sites(_p(sites), n_sites, _p(gt), ns, _p(nodes), n_links, _p(order), min_called, d_node_marks=_p(nm), d_marks=_p(marks), mark_capacity=cap) == cap
        return counter.last_clade_sites_ms()
    def everything():
        assert counter.clade_sites(_p(sites), n_sites, _p(gt), ns, _p(nodes), n_links, _p(order), min_called, _p(calls) if with_calls else None, _p(so), _p(nm), _p(marks), cap) == cap
        return counter.last_clade_sites_ms()
    med, text = last10(listed)
    _, text_all = last10(everything)
    n_scan = 1 if n_sites <= 4096 else 3
    moved = 2 * 2 * n_sites * ns
    got = np.frombuffer(marks.cpu().numpy().tobytes(), MARK)[:cap]
    want = restate_clade_sites(h_na[:check_first], h_gt[:check_first], want_tree["nodes"], want_tree["order"], min_called)
    assert got[got["site"] < check_first].tobytes() == want["marks"].tobytes()
    assert np.frombuffer(so.cpu().numpy().tobytes(), GSITE)[:check_first].tobytes() == want["sites"].tobytes()
    assert not with_calls or np.frombuffer(calls[:check_first * n_links * 16].cpu().numpy().tobytes(), CALL).tobytes() == want["calls"].tobytes()
    assert int(nm.sum()) == cap
    print(f"[{tag}] linkage_tree {n_links} links of {ns} samples {text_tree} in 1 launch; clade_sites {n_sites} sites x {ns} samples x {n_links} nodes, min_called {min_called}: the list and "
          f"the nodes' counts {text} in {2 + n_scan} launches (computed), {cap} marks; {moved / 1e6:.1f} MB of matrix read by the two passes: {moved / med / 1e9:.3f} TB/s; with "
          f"{'d_calls (%.1f MB) and ' % (n_sites * n_links * 16 / 1e6) if with_calls else ''}d_site_out as well {text_all}", flush=True)
    return med

def group_sites(tag, counter, sites, n_sites, gt, ns, group, n_groups, min_called):
    cap = n_sites * min(ns, n_groups)
    marks = torch.zeros(max(cap, 1) * MARK.itemsize, dtype=torch.uint8, device="cuda"); gm = torch.zeros(n_groups, dtype=torch.int32, device="cuda")
    def listed():
        listed.n = counter.group_sites(_p(sites), n_sites, _p(gt), ns, _p(group), n_groups, min_called, d_group_marks=_p(gm), d_marks=_p(marks), mark_capacity=cap)
        return counter.last_group_sites_ms()
    med, text = last10(listed)
    print(f"[{tag}] group_sites, the yardstick: {n_sites} sites x {ns} samples, {n_groups} groups, min_called {min_called}: the list and the groups' counts {text}, {listed.n} marks", flush=True)
    return med

# 1. 125 000 tracts in eight samples on a random genome (the input of tools/exp_group_sites.py)
nrng = np.random.RandomState(9)
G, NT, ns, k, ROWS = 5_000_000, 125_000, 8, 15, 4
g = bytes(nrng.choice(np.frombuffer(b"ACGT", np.uint8), G)) + b"\n"
c = tj.Counter(k)
ref = tj.Reference(c, g)
entries = ref.download()
e = entries[np.arange(NT) * 25 + 7]
length = e["length"].astype(np.int64)[:, None] + np.arange(ROWS)[None, :]
keys = np.zeros((NT, ROWS, 3), np.uint64)
keys[:, :, 0], keys[:, :, 1] = e["ctx0"][:, None], e["ctx1"][:, None]
keys[:, :, 2] = (e["base"].astype(np.uint64)[:, None] & 3) | ((length.astype(np.uint64) & 0x3FF) << 2) | (1 << 12) | (0xffe << 32)
mat = np.zeros((NT, ROWS, ns), np.int32)
t_i, s_i = np.meshgrid(np.arange(NT), np.arange(ns), indexing="ij")
mat[t_i, nrng.randint(0, ROWS, (NT, ns)), s_i] = 9
mat[t_i, nrng.randint(0, ROWS, (NT, ns)), s_i] += 2
mat[nrng.randint(0, NT, NT // 10), :, nrng.randint(0, ns, NT // 10)] = 0
tracts = np.zeros(NT, TR); tracts["first"] = np.arange(NT) * ROWS; tracts["n_rows"] = ROWS; tracts["n_context"] = 1; tracts["mode"] = tracts["first"]
tloc = np.zeros(NT, LOC)
for f in ("flat", "contig", "pos"): tloc[f] = e[f]
tloc["ref_length"], tloc["neg_strand"], tloc["n_hits"] = e["length"], e["neg_strand"], 1
kd, md, td, ld_, nu = _dev(keys), torch.from_numpy(mat.reshape(NT * ROWS, ns)).cuda(), _dev(tracts), _dev(tloc), NT * ROWS
cap = NT * ns
d_var = torch.zeros(cap * VAR.itemsize, dtype=torch.uint8, device="cuda"); offs = (C.c_long * (ns + 1))()
n = L.tjamd_tract_variants(c._h, ref._h, _p(kd), _p(md), nu, ns, _p(td), NT, _p(ld_), None, NT, _p(d_var), cap, offs); assert n >= 0, L.tjamd_last_error()
sites = torch.zeros(n * SITE.itemsize, dtype=torch.uint8, device="cuda"); alleles = torch.zeros(n * ALLELE.itemsize, dtype=torch.uint8, device="cuda")
gt12 = torch.zeros(n * ns, dtype=torch.int16, device="cuda")
n_sites, n_alleles = c.merge_variants(k, _p(d_var), n, ns, NT, _p(sites), n, _p(alleles), n, _p(gt12))
gt = torch.zeros(n_sites * ns, dtype=torch.int16, device="cuda")
assert c.site_depths(ref, _p(kd), _p(md), nu, ns, _p(td), NT, _p(ld_), _p(sites), n_sites, _p(alleles), n_alleles, _p(gt)) == n_sites
dist = torch.zeros(ns * ns * DIST.itemsize, dtype=torch.uint8, device="cuda")
assert c.sample_distances(_p(sites), n_sites, _p(alleles), n_alleles, _p(gt), ns, _p(dist)) == n_sites
links = torch.zeros(ns * LINK.itemsize, dtype=torch.uint8, device="cuda"); cluster = torch.zeros(ns, dtype=torch.int32, device="cuda")
n_links = c.sample_linkage(_p(dist), ns, tj.LINK_DIFFER, 1, _p(links))
h_links = np.frombuffer(links.cpu().numpy().tobytes(), LINK)[:n_links]
n_clusters = c.linkage_clusters(_p(links), n_links, ns, int(np.median(h_links["key"])), _p(cluster))
h_sites = np.frombuffer(sites.cpu().numpy().tobytes(), SITE)[:n_sites]
h_gt = gt.cpu().numpy().reshape(n_sites, ns)
group_sites("125k sites", c, sites, n_sites, gt, ns, cluster, n_clusters, 1)
tree_and_clades("125k sites", c, links, n_links, ns, sites, n_sites, gt, 1, n_sites, h_sites["n_alleles"], h_gt)
ref.close()
del kd, md, td, ld_, d_var, sites, alleles, gt12, gt

# 2. fabricated matrices, made where they are used
T, NG, EVERY = 20_000, 8, 50
for S in (1024, 4096):
    gen = torch.Generator(device="cuda"); gen.manual_seed(S)
    label = torch.randint(0, NG, (S,), generator=gen, device="cuda", dtype=torch.int32)
    base = torch.randint(0, 3, (T, S), generator=gen, device="cuda", dtype=torch.int16)                 # the genome's length or one of two alleles
    base[torch.rand((T, S), generator=gen, device="cuda") < 0.1] = -1
    h_s = np.zeros(T, SITE); h_s["n_alleles"] = 3
    sd = _dev(h_s)
    ms = {}
    for kind in ("chain", "balanced"):
        h_links = tree_links(kind, S)
        t = restate_linkage_tree(h_links, S)
        m = base.clone()
        for i in range(0, T, EVERY):                                                                  # the clade of one node alone carries the third allele
            nd = t["nodes"][(i // EVERY * 37) % (len(h_links) - 1)]                                    # (never the last node: it covers every sample)
            m[i, torch.from_numpy(t["order"][int(nd["first"]): int(nd["first"]) + int(nd["size"])].astype(np.int64)).cuda()] = 3
        ms["group_sites, " + kind] = group_sites(f"fabricated, {kind}", c, sd, T, m.reshape(-1), S, label, NG, 2)
        ms[kind] = tree_and_clades(f"fabricated, {kind}", c, _dev(h_links), len(h_links), S, sd, T, m.reshape(-1), 2, 40, h_s["n_alleles"], m[:40].cpu().numpy())
        del m
    print(f"[fabricated] {S} samples: clade_sites on the chain {ms['chain']:.3f} ms, on the balanced tree {ms['balanced']:.3f} ms; group_sites with {NG} groups "
          f"{ms['group_sites, chain']:.3f} and {ms['group_sites, balanced']:.3f} ms", flush=True)
c.close()
