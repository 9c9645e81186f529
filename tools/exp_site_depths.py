"""Diagnostic: the figures of DESIGN 3.5 N13.  tjamd_site_depths beside tjamd_tract_variants (the yardstick: the same segment
mapping, the same reads of the count matrix, two passes) and tjamd_merge_variants, on the eight-sample pipeline union of
tests/test_locate.py and on 125 000 tracts in eight samples: every 25th run of a random genome of 5 Mb as a tract of four rows
(the genome's length and three longer ones), each sample with a modal row and a lesser one.  HIP-event timers of the library,
twelve calls each, the median and range of the last ten.
   python tools/exp_site_depths.py"""
import ctypes as C, random, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p, dev_locate, dev_located_tracts, stats_on
from tests.test_union_tracts import DNA, device_union, make_genome, reads_of, sample_of
VAR, SITE, ALLELE, SD, TR, LOC = tj.VARIANT_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE, tj.SITE_DEPTH_DTYPE, tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE
L = tj.lib()

def rng10(f):
    v = [f() for _ in range(12)][2:]
    return f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})"

def scan_launches(n):
    """launches of the device-wide exclusive scan over n words (blocks of 4096)"""
    return 1 if n <= 4096 else 2 + scan_launches(-(-n // 4096))

def measure(tag, counter, ref, k, kd, md, nu, ns, td, nt, ld, d_lst, n_list):
    """N8 on the list, N12 on its records, N13 on its sites: the three timers in one run"""
    cap = n_list * ns
    d_var = torch.zeros(cap * VAR.itemsize, dtype=torch.uint8, device="cuda"); offs = (C.c_long * (ns + 1))()
    def variants():
        n = L.tjamd_tract_variants(counter._h, ref._h, _p(kd), _p(md), nu, ns, _p(td), nt, _p(ld), _p(d_lst), n_list, _p(d_var), cap, offs); assert n >= 0, L.tjamd_last_error()
        variants.n = n; return counter.last_tract_variants_ms()
    ms_var = rng10(variants)
    n = variants.n
    sites = torch.zeros(n * SITE.itemsize, dtype=torch.uint8, device="cuda"); alleles = torch.zeros(n * ALLELE.itemsize, dtype=torch.uint8, device="cuda")
    gt12 = torch.zeros(n * ns, dtype=torch.int16, device="cuda")
    def merge():
        merge.n_sites, merge.n_alleles = counter.merge_variants(k, _p(d_var), n, ns, nt, _p(sites), n, _p(alleles), n, _p(gt12)); return counter.last_merge_variants_ms()
    ms_mg = rng10(merge)
    n_sites, n_alleles = merge.n_sites, merge.n_alleles
    gt = torch.zeros(n_sites * ns, dtype=torch.int16, device="cuda"); dp = torch.zeros(n_sites * ns, dtype=torch.int32, device="cuda")
    ad = torch.zeros((n_sites + n_alleles) * ns, dtype=torch.int32, device="cuda"); sd = torch.zeros(n_sites * SD.itemsize, dtype=torch.uint8, device="cuda")
    def depths():
        assert counter.site_depths(ref, _p(kd), _p(md), nu, ns, _p(td), nt, _p(ld), _p(sites), n_sites, _p(alleles), n_alleles, _p(gt), _p(dp), _p(ad), _p(sd)) == n_sites
        return counter.last_site_depths_ms()
    ms_sd = rng10(depths)
    g, g12 = gt.cpu().numpy(), gt12[: n_sites * ns].cpu().numpy()
    assert (g[g12 >= 1] == g12[g12 >= 1]).all() and (g[g12 < 0] <= 0).all()   # N12's genotype where it has one
    print(f"[{tag}] union {nu} rows x {ns} samples, {nt} tracts, {n_list} listed: {n} records -> {n_sites} sites, {n_alleles} alleles, {(g == 0).sum()} reference cells, "
          f"{(g < 0).sum()} unseen; site_depths {ms_sd} in 2 launches beside tract_variants {ms_var} in {3 + scan_launches(n_list * ns)} launches and merge_variants {ms_mg}", flush=True)

# 1. the pipeline union
k, m, ns, maxd, lev, mm = 15, 4, 8, 1, 2, 1
rng = random.Random(2024)
pieces = make_genome(rng, n_tracts=2000)
genome = "".join(left + DNA[b] * length + right for left, b, length, right in pieces)
counters, ocov = [], []
for smp in range(ns):
    s = reads_of(sample_of(pieces, rng, smp), rng)
    c = tj.Counter(k); c.scan_host(s, m); assert c.finalise(1, 5) == 0; counters.append(c); ocov.append(c.coverage)
hs = (C.c_void_p * ns)(*[c._h for c in counters]); drec, counts = C.c_void_p(), (C.c_long * ns)()
merger = tj.Counter(k)
total = L.tjamd_gather_histograms(merger._h, hs, ns, C.byref(drec), counts)
keys = torch.empty(total * 24, dtype=torch.uint8, device="cuda"); mat = torch.empty((total, ns), dtype=torch.int32, device="cuda")
nu = L.tjamd_merge_samples(merger._h, drec, counts, ns, C.c_void_p(keys.data_ptr()), C.c_void_p(mat.data_ptr()), total)
keys, mat = keys[: nu * 24], mat[:nu]
nt0, grouped = device_union(merger, keys, mat, ocov, maxd, lev, on_device=True)
ref = tj.Reference(merger, (genome + "\n").encode())
n_located, loc = dev_locate(merger, ref, keys, mm, on_device=True)
nt, lt = dev_located_tracts(merger, keys, mat, grouped["tracts"], loc, on_device=True)
kd, md, td, ld = lt["d_keys"], lt["d_mat"], lt["d_tracts"], _dev(lt["tract_loc"])
var = stats_on(merger, lt, nt, ns, ocov)["variable"]
measure("pipeline", merger, ref, k, kd, md, nu, ns, td, nt, ld, torch.from_numpy(np.asarray(var, np.int32)).cuda(), len(var))
ref.close()
for c in counters + [merger]: c.close()

# 2. 125 000 tracts in eight samples on a random genome
nrng = np.random.RandomState(9)
G, NT, ns, k, ROWS = 5_000_000, 125_000, 8, 15, 4
g = bytes(nrng.choice(np.frombuffer(b"ACGT", np.uint8), G)) + b"\n"
c = tj.Counter(k)
ref = tj.Reference(c, g)
entries = ref.download()
e = entries[np.arange(NT) * 25 + 7]                                          # ascending flat: the tiling is in the order of the places
length = e["length"].astype(np.int64)[:, None] + np.arange(ROWS)[None, :]   # the genome's own length, then one, two and three bases more
keys = np.zeros((NT, ROWS, 3), np.uint64)
keys[:, :, 0], keys[:, :, 1] = e["ctx0"][:, None], e["ctx1"][:, None]      # an entry holds the genome's flanks in the packing of the union rows
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
measure("125k tracts", c, ref, k, _dev(keys), torch.from_numpy(mat.reshape(NT * ROWS, ns)).cuda(), NT * ROWS, ns, _dev(tracts), NT, _dev(tloc), None, NT)
ref.close(); c.close()
