"""Diagnostic: the entries that take a caller's tiling and that exp_site_depths.py does not time -- tjamd_union_tract_stats,
tjamd_located_tracts and tjamd_tract_features -- on the 125 000-tract union of that script (four rows a tract, eight samples,
10 000 random features).  HIP-event timers of the library, twelve calls each, the median and range of the last ten; the counts
behind each time are printed so that two library builds (TJ_DIAG_LIB) can be compared on their results as well.
   python tools/exp_tiled_entries.py"""
import ctypes as C, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p
TR, LOC, TF, FE = tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE, tj.TRACT_FEATURE_DTYPE, tj.FEATURE_DTYPE
L = tj.lib()

def rng10(f):
    v = [f() for _ in range(12)][2:]
    return f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})"

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
tracts = np.zeros(NT, TR); tracts["first"] = np.arange(NT) * ROWS; tracts["n_rows"] = ROWS; tracts["n_context"] = 1; tracts["mode"] = tracts["first"]
tloc = np.zeros(NT, LOC)
for f in ("flat", "contig", "pos"): tloc[f] = e[f]
tloc["ref_length"], tloc["neg_strand"], tloc["n_hits"] = e["length"], e["neg_strand"], 1
nu = NT * ROWS
kd, md, td, ld = _dev(keys), torch.from_numpy(mat.reshape(nu, ns)).cuda(), _dev(tracts), _dev(tloc)
rowloc = _dev(np.repeat(tloc, ROWS))

cov = (C.c_int * ns)(*([30] * ns))
summ = torch.zeros(NT * 64, dtype=torch.uint8, device="cuda")
var = torch.zeros(NT, dtype=torch.int32, device="cuda"); sel = torch.zeros(NT, dtype=torch.int32, device="cuda")
nv, nsel = C.c_long(), C.c_long()
def stats():
    assert L.tjamd_union_tract_stats(c._h, _p(kd), _p(md), nu, ns, _p(td), NT, cov, None, _p(summ), _p(var), C.byref(nv), _p(sel), C.byref(nsel)) == NT, L.tjamd_last_error()
    return c.last_union_tract_stats_ms()
ms_stats = rng10(stats)

perm = torch.zeros(nu, dtype=torch.int32, device="cuda"); ok, om = torch.zeros_like(kd), torch.zeros_like(md)
otr = torch.zeros(nu * 32, dtype=torch.uint8, device="cuda"); otl = torch.zeros(nu * 32, dtype=torch.uint8, device="cuda"); orl = torch.zeros(nu, dtype=torch.int32, device="cuda")
def located():
    located.n = L.tjamd_located_tracts(c._h, _p(kd), _p(md), nu, ns, _p(td), NT, _p(rowloc), _p(perm), _p(ok), _p(om), _p(otr), _p(otl), _p(orl), nu)
    assert located.n > 0, L.tjamd_last_error()
    return c.last_located_tracts_ms()
ms_lt = rng10(located)

feats = np.zeros(10_000, FE)
feats["start"] = 1 + np.sort(nrng.randint(0, G - 2000, 10_000)); feats["end"] = feats["start"] + nrng.randint(100, 1500, 10_000); feats["cls"] = nrng.randint(1, 3, 10_000)
ann = tj.Annotation(c, ref, feats)
d_tf = torch.zeros(NT * TF.itemsize, dtype=torch.uint8, device="cuda")
def features():
    assert L.tjamd_tract_features(c._h, ann._h, _p(kd), _p(md), nu, ns, _p(td), NT, _p(ld), _p(d_tf)) == NT, L.tjamd_last_error()
    return c.last_tract_features_ms()
ms_tf = rng10(features)
tf = np.frombuffer(d_tf.cpu().numpy().tobytes(), TF)
print(f"[125k tracts] union {nu} rows x {ns} samples, {NT} tracts: union_tract_stats {ms_stats} ({nv.value} variable, {nsel.value} selected); "
      f"located_tracts {ms_lt} ({located.n} tracts out); tract_features {ms_tf} ({(tf['feature'] >= 0).sum()} in a feature, max_length sum {tf['max_length'].sum()})", flush=True)
ann.close(); ref.close(); c.close()
