"""Diagnostic: the figures of DESIGN 3.5 N11.  tjamd_variant_effects beside tjamd_tract_variants (the yardstick: the same record
count, one flag pass and one write pass more) and tjamd_coding_create beside tjamd_annotation_create on the eight-sample
pipeline union of tests/test_locate.py with the GFF3 file of tests/test_features.py; then 1 000 000 synthetic records, half of
them frameshifts, on a 5 Mbase random genome with the 10 000 synthetic features of N9's experiment: codons walked per second
and the share of records that took the wavefront path.  HIP-event timers of the library, twelve calls each, the median and
range of the last ten.   python tools/exp_variant_effects.py"""
import ctypes as C, random, sys, os, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_features import gff3_of
from tests.test_locate import _dev, _p, _raw, dev_locate, dev_located_tracts
from tests.test_union_tracts import DNA, device_union, make_genome, reads_of, sample_of
VAR, EF, TF, FT = tj.VARIANT_DTYPE, tj.EFFECT_DTYPE, tj.TRACT_FEATURE_DTYPE, tj.FEATURE_DTYPE
L = tj.lib()

def rng10(f):
    v = [f() for _ in range(12)][2:]
    return f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})", float(np.median(v))

def walked(e, phase_of_feature):
    """codons the wavefronts translated per sequence: from the edit's codon to the alternative's stop or end"""
    w = e[e["cls"] >= 2]
    ph = np.maximum(phase_of_feature[w["feature"]], 0)
    first = np.maximum(w["cds_pos"].astype(np.int64) - 1 - ph, 0) // 3
    return int(np.maximum(w["alt_aa_len"].astype(np.int64) + ((w["flags"] & 2) >> 1) - first, 0).sum()), len(w)

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
stream = (genome + "\n").encode()
ref = tj.Reference(merger, stream)
n_located, loc = dev_locate(merger, ref, keys, mm, on_device=True)
nt, lt = dev_located_tracts(merger, keys, mat, grouped["tracts"], loc, on_device=True)
kd, md, td, ld = lt["d_keys"], lt["d_mat"], lt["d_tracts"], _dev(lt["tract_loc"])
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "genome.gff3")
    open(path, "w").write(gff3_of([pieces], ["genome"]))
    feats, strings = tj.read_gff3(path, ["genome"]); phase = tj.read_gff3_phase(path, ["genome"])
cap = nt * ns
d_var = torch.zeros(cap * VAR.itemsize, dtype=torch.uint8, device="cuda"); d_eff = torch.zeros(cap * EF.itemsize, dtype=torch.uint8, device="cuda")
d_tf = torch.zeros(nt * TF.itemsize, dtype=torch.uint8, device="cuda"); offs = (C.c_long * (ns + 1))()
def variants():
    n = L.tjamd_tract_variants(merger._h, ref._h, _p(kd), _p(md), nu, ns, _p(td), nt, _p(ld), None, 0, _p(d_var), cap, offs); assert n >= 0, L.tjamd_last_error()
    variants.n = n; return merger.last_tract_variants_ms()
def annotation():
    a = tj.Annotation(merger, ref, feats); t = merger.last_annotation_ms(); a.close(); return t
def coding():
    a = tj.Coding(merger, stream, feats, phase); t = merger.last_coding_ms(); a.close(); return t
ms_var, _ = rng10(variants); ms_ann, _ = rng10(annotation); ms_cod, _ = rng10(coding)
ann = tj.Annotation(merger, ref, feats); cod = tj.Coding(merger, stream, feats, phase)
assert L.tjamd_tract_features(merger._h, ann._h, _p(kd), _p(md), nu, ns, _p(td), nt, _p(ld), _p(d_tf)) == nt
def effects():
    assert merger.variant_effects(cod, _p(d_var), variants.n, _p(d_eff), _p(d_tf), nt) == variants.n; return merger.last_variant_effects_ms()
ms_eff, _ = rng10(effects)
e = _raw(d_eff, EF, variants.n)
print(f"[pipeline] union {nu} rows x {ns} samples, {nt} tracts, {len(feats)} features, {variants.n} records (every tract listed): "
      f"variant_effects {ms_eff} beside tract_variants {ms_var}; coding {ms_cod} beside annotation {ms_ann}; "
      f"classes {[int((e['cls'] == x).sum()) for x in range(5)]}; codons walked {walked(e, phase.astype(np.int64))}", flush=True)
cod.close(); ann.close(); ref.close()
for c in counters + [merger]: c.close()

# 2. a 5 Mbase random genome, the 10 000 synthetic features of N9's experiment, 1 000 000 synthetic records
rng = random.Random(9); nrng = np.random.RandomState(9)
G = 5_000_000
g = (bytes(nrng.choice(np.frombuffer(b"ACGT", np.uint8), G)) + b"\n")
rows = [(0, 1, G, 0, 0)]                                                      # one region
for _ in range(2500):                                                         # genes of 300 to 3 000 bases, each with an mRNA and a CDS
    length = rng.randint(300, 3000); start = rng.randint(1, G - length); strand = rng.randrange(2)
    rows += [(0, start, start + length - 1, 2, strand), (0, start, start + length - 1, 2, strand), (0, start + 30, start + length - 31, 1, strand)]
for _ in range(2489):                                                         # short features
    start = rng.randint(1, G - 200); rows.append((0, start, start + rng.randint(1, 200), 2, rng.randrange(2)))
for _ in range(10):                                                           # ten of 50 to 500 kbases
    length = rng.randint(50_000, 500_000); start = rng.randint(1, G - length); rows.append((0, start, start + length - 1, 2, 0))
feats = np.zeros(len(rows), FT)
for i, (ct, s0, e0, cls, strand) in enumerate(rows): feats[i] = (ct, s0, e0, cls, strand, i + 1, 0, 0)
assert len(feats) == 10_000
c = tj.Counter(15)
def coding5():
    a = tj.Coding(c, g, feats, None); t = c.last_coding_ms(); a.close(); return t
ms_cod5, _ = rng10(coding5)
cod = tj.Coding(c, g, feats, None)
cds = np.flatnonzero(feats["cls"] == 1)
N = 1_000_000
f = cds[nrng.randint(0, len(cds), N)]
lr = nrng.randint(4, 11, N); shift = nrng.choice([-1, 1], N) * np.where(np.arange(N) % 2 == 0, 1, 3)      # half frameshifts, half in frame
var = np.zeros(N, VAR)
var["tract"], var["ref_length"], var["alt_length"], var["base"] = f, lr, lr + shift, nrng.randint(0, 4, N)
span = feats["end"][f] - feats["start"][f] + 1
var["pos"] = feats["start"][f] + 5 + (nrng.random_sample(N) * (span - 20)).astype(np.int64)
tf = np.zeros(len(feats), TF); tf["feature"] = np.arange(len(feats))
dv, dt, de = _dev(var), _dev(tf), torch.zeros(N * EF.itemsize, dtype=torch.uint8, device="cuda")
def effects5():
    assert c.variant_effects(cod, _p(dv), N, _p(de), _p(dt), len(tf)) == N; return c.last_variant_effects_ms()
txt, med = rng10(effects5)
e = _raw(de, EF, N)
codons, n_walk = walked(e, np.zeros(len(feats), np.int64))
print(f"[5 Mbase] {len(feats)} features ({len(cds)} CDS), coding {ms_cod5}; {N} records: variant_effects {txt}; classes {[int((e['cls'] == x).sum()) for x in range(5)]}; "
      f"{n_walk} records ({100.0 * n_walk / N:.1f} %) took the wavefront path, {codons} alternative codons walked ({codons / n_walk:.1f} per record), "
      f"twice that translated: {2 * codons / (med * 1e-3) / 1e9:.2f} G codons/s; {N * (VAR.itemsize + EF.itemsize) / (med * 1e-3) / 1e9:.1f} GB/s of records", flush=True)
cod.close(); c.close()
