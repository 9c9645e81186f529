"""Diagnostic: the figures of DESIGN 3.5 N12.  tjamd_merge_variants beside tjamd_tract_variants (the yardstick: a flag pass, a
scan and a write pass over the same records) on the eight-sample pipeline union of tests/test_locate.py; then 1 000 000
synthetic records -- the genome, the features and the edits of N11's experiment (tools/exp_variant_effects.py), as 125 000
tracts in eight samples -- with the number of launches of the call and tjamd_variant_effects on all records beside the same on
d_unique.  HIP-event timers of the library, twelve calls each, the median and range of the last ten.
   python tools/exp_merge_variants.py"""
import ctypes as C, random, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p, _raw, dev_locate, dev_located_tracts, stats_on
from tests.test_union_tracts import DNA, device_union, make_genome, reads_of, sample_of
VAR, EF, TF, FT, SITE, ALLELE = tj.VARIANT_DTYPE, tj.EFFECT_DTYPE, tj.TRACT_FEATURE_DTYPE, tj.FEATURE_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE
L = tj.lib()

def rng10(f):
    v = [f() for _ in range(12)][2:]
    return f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})", float(np.median(v))

def scan_launches(n):
    """launches of the device-wide exclusive scan over n words (blocks of 4096)"""
    return 1 if n <= 4096 else 2 + scan_launches(-(-n // 4096))

def launches(n, k, n_tracts, genotype=True):
    """kernel launches of one tjamd_merge_variants call (hopo_device.hip, N12): key, sort passes, heads, two scans, starts, sites, fill, write"""
    tbits = max(n_tracts - 1, 0).bit_length()
    nblk = -(-n // 1024)
    one_pass = 2 + scan_launches(256 * nblk)
    if tbits + 16 + 2 * k <= 64:
        sort = 1 + -(-(tbits + 16 + 2 * k) // 8) * one_pass
    else:
        sort = 2 + (-(-2 * k // 8) + -(-(tbits + 16) // 8)) * one_pass
    return sort + 1 + 2 * scan_launches(n) + 1 + 1 + (1 if genotype else 0) + 1

class Merge:
    def __init__(self, counter, k, d_records, n, ns, nt):
        self.c, self.k, self.d, self.n, self.ns, self.nt = counter, k, d_records, n, ns, nt
        self.sites = torch.zeros(n * SITE.itemsize, dtype=torch.uint8, device="cuda"); self.alleles = torch.zeros(n * ALLELE.itemsize, dtype=torch.uint8, device="cuda")
        self.gt = torch.zeros(n * ns, dtype=torch.int16, device="cuda"); self.aof = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.unique = torch.zeros(n * VAR.itemsize, dtype=torch.uint8, device="cuda")
    def __call__(self):
        self.n_sites, self.n_alleles = self.c.merge_variants(self.k, _p(self.d), self.n, self.ns, self.nt, _p(self.sites), self.n, _p(self.alleles), self.n,
                                                             _p(self.gt), _p(self.aof), _p(self.unique))
        return self.c.last_merge_variants_ms()

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
for name, lst in (("the variable tracts", stats_on(merger, lt, nt, ns, ocov)["variable"]), ("every tract", None)):
    n_list = nt if lst is None else len(lst)
    d_lst = None if lst is None else torch.from_numpy(np.asarray(lst, np.int32)).cuda()
    cap = n_list * ns
    d_var = torch.zeros(cap * VAR.itemsize, dtype=torch.uint8, device="cuda"); offs = (C.c_long * (ns + 1))()
    def variants():
        n = L.tjamd_tract_variants(merger._h, ref._h, _p(kd), _p(md), nu, ns, _p(td), nt, _p(ld), _p(d_lst), n_list, _p(d_var), cap, offs); assert n >= 0, L.tjamd_last_error()
        variants.n = n; return merger.last_tract_variants_ms()
    ms_var, _ = rng10(variants)
    mg = Merge(merger, k, d_var, variants.n, ns, nt)
    ms_mg, _ = rng10(mg)
    print(f"[pipeline] union {nu} rows x {ns} samples, {nt} tracts, {name} listed: {variants.n} records -> {mg.n_sites} sites, {mg.n_alleles} alleles; "
          f"merge_variants {ms_mg} in {launches(variants.n, k, nt)} launches beside tract_variants {ms_var}", flush=True)
ref.close()
for c in counters + [merger]: c.close()

# 2. N11's experiment input as 125 000 tracts in eight samples: 1 000 000 records
rng = random.Random(9); nrng = np.random.RandomState(9)
G = 5_000_000
g = (bytes(nrng.choice(np.frombuffer(b"ACGT", np.uint8), G)) + b"\n")
rows = [(0, 1, G, 0, 0)]
for _ in range(2500):
    length = rng.randint(300, 3000); start = rng.randint(1, G - length); strand = rng.randrange(2)
    rows += [(0, start, start + length - 1, 2, strand), (0, start, start + length - 1, 2, strand), (0, start + 30, start + length - 31, 1, strand)]
for _ in range(2489):
    start = rng.randint(1, G - 200); rows.append((0, start, start + rng.randint(1, 200), 2, rng.randrange(2)))
for _ in range(10):
    length = rng.randint(50_000, 500_000); start = rng.randint(1, G - length); rows.append((0, start, start + length - 1, 2, 0))
feats = np.zeros(len(rows), FT)
for i, (ct, s0, e0, cls, strand) in enumerate(rows): feats[i] = (ct, s0, e0, cls, strand, i + 1, 0, 0)
c = tj.Counter(15)
cod = tj.Coding(c, g, feats, None)
cds = np.flatnonzero(feats["cls"] == 1)
ns, NT = 8, 125_000
N = ns * NT
f = cds[nrng.randint(0, len(cds), NT)]                                       # per tract: its feature, reference length, base and place
lr = nrng.randint(4, 11, NT)
span = feats["end"][f] - feats["start"][f] + 1
pos0 = feats["start"][f] + 5 + (nrng.random_sample(NT) * (span - 20)).astype(np.int64)
base = nrng.randint(0, 4, NT)
var = np.zeros(N, VAR)
t = np.tile(np.arange(NT), ns)                                               # sample-major: every tract in every sample
shift = nrng.choice([-1, 1], N) * np.where(nrng.randint(0, 2, N) == 0, 1, 3)      # half frameshifts, half in frame: four alleles per tract at most
var["tract"], var["sample"], var["flat"], var["ref_length"], var["alt_length"], var["base"] = t, np.repeat(np.arange(ns), NT), pos0[t], lr[t], lr[t] + shift, base[t]
var["pos"] = pos0[t] + np.minimum(var["ref_length"], var["alt_length"])
tf = np.zeros(NT, TF); tf["feature"] = f
dv, dt = _dev(var), _dev(tf)
mg = Merge(c, 15, dv, N, ns, NT)
txt_mg, med = rng10(mg)
de = torch.zeros(N * EF.itemsize, dtype=torch.uint8, device="cuda")
def effects_all():
    assert c.variant_effects(cod, _p(dv), N, _p(de), _p(dt), NT) == N; return c.last_variant_effects_ms()
def effects_unique():
    assert c.variant_effects(cod, _p(mg.unique), mg.n_alleles, _p(de), _p(dt), NT) == mg.n_alleles; return c.last_variant_effects_ms()
txt_all, _ = rng10(effects_all)
all_e = _raw(de, EF, N).copy()
txt_uni, _ = rng10(effects_unique)
uni_e = _raw(de, EF, mg.n_alleles)
assert all_e.tobytes() == uni_e[mg.aof.cpu().numpy()].tobytes()               # a record's effect is its allele's
nblk = -(-N // 1024)
print(f"[1M records] {N} records of {ns} samples in {NT} tracts -> {mg.n_sites} sites, {mg.n_alleles} alleles: merge_variants {txt_mg} in {launches(N, 15, NT)} launches "
      f"({-(-(max(NT - 1, 0).bit_length() + 46) // 8)} sort passes; {N * 32 * -(-(max(NT - 1, 0).bit_length() + 46) // 8) / (med * 1e-3) / 1e9:.0f} GB/s if the passes' 32 bytes of key and value "
      f"traffic were all of it); variant_effects on all records {txt_all}, on d_unique {txt_uni}", flush=True)
cod.close(); c.close()
