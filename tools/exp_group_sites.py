"""Diagnostic: the figures of DESIGN 3.5 N16.  tjamd_group_sites at three shapes.
1. 125 000 sites x 8 samples, the pipeline-sized input of tools/exp_sample_linkage.py: N8, N12, N13, N14, N15 and then the sites
   that set N15's clusters apart, d_cluster handed over as d_group where it is; the timers of N14, N15 and N16 side by side in
   one run.
2. fabricated matrices of 20 000 sites at 1024 and 4096 samples, made on the device: three alleles a site, a tenth of the cells
   not called, eight groups at random with a twentieth of the samples taking no part, and at every 50th site one group alone
   carries the third allele (a mark by construction).  The first 300 sites are held to the restatement.
HIP-event timers of the library, twelve calls each, the median and range of the last ten.  The launches are computed: the
pass that checks and counts, the shared scan of the sites' counts (one launch up to 4096 sites, three up to 4096^2) and the
pass that writes.  The bytes are the matrix's, 2 a cell, read once by each pass; the outputs are small beside them when
d_calls is not asked for.  The time of every kernel comes from a trace of this script:
   python tools/exp_group_sites.py
   rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp_group_sites.py"""
import ctypes as C, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p
from tests.test_groups_cabi import restate_group_sites_table
VAR, SITE, ALLELE, TR, LOC, DIST, LINK = tj.VARIANT_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE, tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE, tj.SAMPLE_DISTANCE_DTYPE, tj.LINK_DTYPE
CALL, GSITE, MARK = tj.GROUP_CALL_DTYPE, tj.GROUP_SITE_DTYPE, tj.GROUP_MARK_DTYPE
HBM_PEAK, COPY_RATE = 8.0e12, 4.9e12                                          # bytes a second, MI355X: the peak, and what a copy reaches
L = tj.lib()

def last10(f):
    v = [f() for _ in range(12)][2:]
    return float(np.median(v)), f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})"

def group_sites(tag, counter, sites, n_sites, gt, ns, group, n_groups, min_called, check_first, h_na, h_gt, h_group):
    """the list alone, then every output; the first check_first sites against the restatement"""
    cap = n_sites * min(ns, n_groups)
    marks = torch.zeros(max(cap, 1) * MARK.itemsize, dtype=torch.uint8, device="cuda"); gm = torch.zeros(n_groups, dtype=torch.int32, device="cuda")
    so = torch.zeros(n_sites * GSITE.itemsize, dtype=torch.uint8, device="cuda"); calls = torch.zeros(n_sites * n_groups * CALL.itemsize, dtype=torch.uint8, device="cuda")
    def listed():
        listed.n = counter.group_sites(_p(sites), n_sites, _p(gt), ns, _p(group), n_groups, min_called, d_group_marks=_p(gm), d_marks=_p(marks), mark_capacity=cap)
        return counter.last_group_sites_ms()
    def everything():
        assert counter.group_sites(_p(sites), n_sites, _p(gt), ns, _p(group), n_groups, min_called, _p(calls), _p(so), _p(gm), _p(marks), cap) == listed.n
        return counter.last_group_sites_ms()
    med, text = last10(listed)
    _, text_all = last10(everything)
    n_scan = 1 if n_sites <= 4096 else 3
    moved = 2 * 2 * n_sites * ns
    got = np.frombuffer(marks.cpu().numpy().tobytes(), MARK)[:listed.n]
    want = restate_group_sites_table(h_na[:check_first], h_gt[:check_first], h_group, n_groups, min_called)
    assert got[got["site"] < check_first].tobytes() == want["marks"].tobytes()
    assert np.frombuffer(so.cpu().numpy().tobytes(), GSITE)[:check_first].tobytes() == want["sites"].tobytes()
    assert np.frombuffer(calls.cpu().numpy().tobytes(), CALL)[:check_first * n_groups].tobytes() == want["calls"].tobytes()
    assert int(gm.sum()) == listed.n
    print(f"[{tag}] group_sites {n_sites} sites x {ns} samples, {n_groups} groups, min_called {min_called}: the list and the groups' counts {text} in {2 + n_scan} launches "
          f"(computed), {listed.n} marks; {moved / 1e6:.1f} MB of matrix read by the two passes: {moved / med / 1e9:.3f} TB/s beside a copy's {COPY_RATE / 1e12:.1f} TB/s and "
          f"the HBM peak of {HBM_PEAK / 1e12:.0f} TB/s; with d_calls ({n_sites * n_groups * 16 / 1e6:.1f} MB) and d_site_out as well {text_all}", flush=True)
    return listed.n

# 1. 125 000 tracts in eight samples on a random genome (the input of tools/exp_sample_linkage.py)
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
def distances():
    assert c.sample_distances(_p(sites), n_sites, _p(alleles), n_alleles, _p(gt), ns, _p(dist)) == n_sites; return c.last_sample_distances_ms()
_, ms_d = last10(distances)
links = torch.zeros(ns * LINK.itemsize, dtype=torch.uint8, device="cuda"); cluster = torch.zeros(ns, dtype=torch.int32, device="cuda")
def linkage():
    linkage.n = c.sample_linkage(_p(dist), ns, tj.LINK_DIFFER, 1, _p(links)); return c.last_sample_linkage_ms()
_, ms_l = last10(linkage)
h_links = np.frombuffer(links.cpu().numpy().tobytes(), LINK)[:linkage.n]
threshold = int(np.median(h_links["key"]))
def clusters():
    clusters.n = c.linkage_clusters(_p(links), linkage.n, ns, threshold, _p(cluster)); return c.last_linkage_clusters_ms()
_, ms_c = last10(clusters)
h_sites = np.frombuffer(sites.cpu().numpy().tobytes(), SITE)[:n_sites]
h_gt = gt.cpu().numpy().reshape(n_sites, ns)
group_sites("125k sites, N15's clusters", c, sites, n_sites, gt, ns, cluster, clusters.n, 1, n_sites, h_sites["n_alleles"], h_gt, cluster.cpu().numpy())
print(f"[125k sites] {n_sites} sites x {ns} samples, {clusters.n} clusters at {threshold}; beside sample_distances {ms_d}, sample_linkage {ms_l}, linkage_clusters {ms_c}", flush=True)
ref.close()
del kd, md, td, ld_, d_var, sites, alleles, gt12, gt

# 2. fabricated matrices, made where they are used
T, NG = 20_000, 8
for S in (1024, 4096):
    gen = torch.Generator(device="cuda"); gen.manual_seed(S)
    label = torch.randint(0, NG, (S,), generator=gen, device="cuda", dtype=torch.int32)
    label[torch.rand(S, generator=gen, device="cuda") < 0.05] = -1
    m = torch.randint(0, 3, (T, S), generator=gen, device="cuda", dtype=torch.int16)                  # the genome's length or one of two alleles
    m[torch.rand((T, S), generator=gen, device="cuda") < 0.1] = -1
    for i in range(0, T, 50):                                                                       # one group alone carries the third allele
        m[i, label == (i // 50) % NG] = 3
    h_s = np.zeros(T, SITE); h_s["n_alleles"] = 3
    found = group_sites("fabricated", c, _dev(h_s), T, m.reshape(-1), S, label, NG, 2, 300, h_s["n_alleles"], m[:300].cpu().numpy(), label.cpu().numpy())
    assert found >= T // 50
    del m
c.close()
