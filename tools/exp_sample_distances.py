"""Diagnostic: the figures of DESIGN 3.5 N14.  tjamd_sample_distances at two shapes.
1. 125 000 sites x 8 samples, the pipeline-sized input of tools/exp_site_depths.py (every 25th run of a random genome of 5 Mb as
   a tract of four rows): N8, N12, N13 and then N14 on N13's genotype matrix, the timers of N12, N13 and N14 side by side.
2. 20 000 sites x 1024 samples, fabricated: the time, the cell pairs a second, and beside it a plain torch formulation of n_both
   alone on the same device (called.T @ called on the 0/1 matrix in fp32), the one piece of the reduction a library does.
HIP-event timers of the library (torch events for the product), twelve calls each, the median and range of the last ten.
The launch count it prints is computed: launches() restates the entry's rule for the tile edge and the slices and does not
observe the device.  The observed count, and the time of every kernel, come from a trace of this script:
   python tools/exp_sample_distances.py
   rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp_sample_distances.py"""
import ctypes as C, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p
from tests.test_distances_cabi import fabricate
VAR, SITE, ALLELE, SD, TR, LOC, DIST = tj.VARIANT_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE, tj.SITE_DEPTH_DTYPE, tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE, tj.SAMPLE_DISTANCE_DTYPE
L = tj.lib()

def last10(f):
    v = [f() for _ in range(12)][2:]
    return float(np.median(v)), f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})"

def launches(counter, n_sites, ns):
    """the launches of a call as the entry's rule gives them (computed, not observed: see above): the check pass, the tiles, and
    the kernel that sums the slices where the sites are split"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t64 = -(-ns // 64)
    E = 8 if ns <= 8 else 16 if ns <= 16 else 64 if t64 * (t64 + 1) // 2 >= 2 * cus else 32
    tiles = -(-ns // E); pairs = tiles * (tiles + 1) // 2; chunks = -(-n_sites // (2048 // E))
    slices = max(1, min(chunks, 4 * cus // pairs))
    per = -(-chunks // slices); slices = -(-chunks // per)
    return (3 if slices > 1 else 2), E, pairs, slices

def distances(tag, counter, sites, n_sites, alleles, n_alleles, gt, ns):
    out = torch.zeros(ns * ns * DIST.itemsize, dtype=torch.uint8, device="cuda")
    def run():
        assert counter.sample_distances(_p(sites), n_sites, _p(alleles), n_alleles, _p(gt), ns, _p(out)) == n_sites
        return counter.last_sample_distances_ms()
    med, text = last10(run)
    n, E, pairs, slices = launches(counter, n_sites, ns)
    d = np.frombuffer(out.cpu().numpy().tobytes(), DIST).reshape(ns, ns)
    cell_pairs = ns * (ns + 1) // 2 * n_sites
    print(f"[{tag}] sample_distances {n_sites} sites x {ns} samples: {text} in {n} launches (computed from the entry's rule: tile edge {E}, {pairs} tile pairs x {slices} slices of the sites), "
          f"{cell_pairs / med / 1e6:.2f} G cell pairs/s over the {cell_pairs} pairs on or above the diagonal; n_both up to {d['n_both'].max()}, "
          f"n_differ up to {d['n_differ'].max()}, length_diff up to {d['length_diff'].max()}", flush=True)
    return d

# 1. 125 000 tracts in eight samples on a random genome (the input of tools/exp_site_depths.py)
nrng = np.random.RandomState(9)
G, NT, ns, k, ROWS = 5_000_000, 125_000, 8, 15, 4
g = bytes(nrng.choice(np.frombuffer(b"ACGT", np.uint8), G)) + b"\n"
c = tj.Counter(k)
ref = tj.Reference(c, g)
entries = ref.download()
e = entries[np.arange(NT) * 25 + 7]                                          # ascending flat: the tiling is in the order of the places
length = e["length"].astype(np.int64)[:, None] + np.arange(ROWS)[None, :]   # the genome's own length, then one, two and three bases more
keys = np.zeros((NT, ROWS, 3), np.uint64)
keys[:, :, 0], keys[:, :, 1] = e["ctx0"][:, None], e["ctx1"][:, None]
keys[:, :, 2] = (e["base"].astype(np.uint64)[:, None] & 3) | ((length.astype(np.uint64) & 0x3FF) << 2) | (1 << 12) | (0xffe << 32)
mat = np.zeros((NT, ROWS, ns), np.int32)
t_i, s_i = np.meshgrid(np.arange(NT), np.arange(ns), indexing="ij")
mat[t_i, nrng.randint(0, ROWS, (NT, ns)), s_i] = 9                            # a modal row ...
mat[t_i, nrng.randint(0, ROWS, (NT, ns)), s_i] += 2                           # ... and a lesser one
mat[nrng.randint(0, NT, NT // 10), :, nrng.randint(0, ns, NT // 10)] = 0      # some samples unseen on some tracts
tracts = np.zeros(NT, TR); tracts["first"] = np.arange(NT) * ROWS; tracts["n_rows"] = ROWS; tracts["n_context"] = 1; tracts["mode"] = tracts["first"]
tloc = np.zeros(NT, LOC)
for f in ("flat", "contig", "pos"): tloc[f] = e[f]
tloc["ref_length"], tloc["neg_strand"], tloc["n_hits"] = e["length"], e["neg_strand"], 1
kd, md, td, ld, nu = _dev(keys), torch.from_numpy(mat.reshape(NT * ROWS, ns)).cuda(), _dev(tracts), _dev(tloc), NT * ROWS
cap = NT * ns
d_var = torch.zeros(cap * VAR.itemsize, dtype=torch.uint8, device="cuda"); offs = (C.c_long * (ns + 1))()
n = L.tjamd_tract_variants(c._h, ref._h, _p(kd), _p(md), nu, ns, _p(td), NT, _p(ld), None, NT, _p(d_var), cap, offs); assert n >= 0, L.tjamd_last_error()
sites = torch.zeros(n * SITE.itemsize, dtype=torch.uint8, device="cuda"); alleles = torch.zeros(n * ALLELE.itemsize, dtype=torch.uint8, device="cuda")
gt12 = torch.zeros(n * ns, dtype=torch.int16, device="cuda")
def merge():
    merge.n_sites, merge.n_alleles = c.merge_variants(k, _p(d_var), n, ns, NT, _p(sites), n, _p(alleles), n, _p(gt12)); return c.last_merge_variants_ms()
_, ms_mg = last10(merge)
n_sites, n_alleles = merge.n_sites, merge.n_alleles
gt = torch.zeros(n_sites * ns, dtype=torch.int16, device="cuda")
def depths():
    assert c.site_depths(ref, _p(kd), _p(md), nu, ns, _p(td), NT, _p(ld), _p(sites), n_sites, _p(alleles), n_alleles, _p(gt)) == n_sites
    return c.last_site_depths_ms()
_, ms_sd = last10(depths)
distances("125k sites, N13's genotypes", c, sites, n_sites, alleles, n_alleles, gt, ns)
distances("125k sites, N12's genotypes", c, sites, n_sites, alleles, n_alleles, gt12, ns)
print(f"[125k sites] {n} records -> {n_sites} sites, {n_alleles} alleles; beside site_depths (genotypes only) {ms_sd} in 2 launches and merge_variants {ms_mg}", flush=True)
ref.close()

# 2. 20 000 sites x 1024 samples, fabricated
T, S = 20_000, 1024
h_sites, h_alleles, h_g = fabricate(T, S, np.random.RandomState(14))
d = distances("fabricated", c, _dev(h_sites), T, _dev(h_alleles), len(h_alleles), _dev(h_g), S)
called = (torch.from_numpy(h_g).cuda() >= 0).float()                          # [T, S]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
def gemm():
    e0.record(); gemm.out = called.T @ called; e1.record(); torch.cuda.synchronize(); return e0.elapsed_time(e1)
med, text = last10(gemm)
assert (gemm.out.cpu().numpy().astype(np.int64) == d["n_both"]).all()         # (counts up to 20 000 are exact in fp32)
print(f"[fabricated] torch called.T @ called ({S} x {T} x {S}, fp32), n_both alone, the full square: {text}, {S * S * T / med / 1e6:.2f} G cell pairs/s", flush=True)
c.close()
