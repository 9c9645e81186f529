"""Diagnostic: the figures of DESIGN 3.5 N10.  tjamd_locate and tjamd_locate_gapped on the eight-sample pipeline union of
tests/test_locate.py and on 343 rows against a 5 Mbase random genome (k = 5: seed ranges of some 39 000 entries; k = 15),
with the seed order beside the index build and the located share before and after.  HIP-event timers of the library,
twelve calls each, the median and range of the last ten.   python tools/exp_locate_gapped.py"""
import ctypes as C, random, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p, _raw, dev_locate
from tests.test_locate_gapped import gapped_queries, dev_locate_gapped
from tests.test_union_tracts import DNA, make_genome, reads_of, sample_of
from oracle import orc
LOC = tj.LOCATION_DTYPE
L = tj.lib()

def rng10(f):
    v = [f() for _ in range(12)][2:]
    return f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})"

def time_calls(c, ref, kd, n, first_np, mm, me, ms):
    loc = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    def one_locate():
        L.tjamd_locate(c._h, ref._h, _p(kd), n, mm, _p(loc)); return c.last_locate_ms()
    a = rng10(one_locate)
    base = _dev(first_np)
    def one_gapped():
        loc.copy_(base); torch.cuda.synchronize()
        got = L.tjamd_locate_gapped(c._h, ref._h, _p(kd), n, me, ms, _p(loc), None); assert got >= 0
        return c.last_locate_gapped_ms()
    b = rng10(one_gapped)
    return a, b

# 1. the pipeline union
k, m, ns = 15, 4, 8
rng = random.Random(2024)
pieces = make_genome(rng, n_tracts=2000)
genome = "".join(left + DNA[b] * length + right for left, b, length, right in pieces)
counters = []
for smp in range(ns):
    s = reads_of(sample_of(pieces, rng, smp), rng)
    c = tj.Counter(k); c.scan_host(s, m); assert c.finalise(1, 5) == 0; counters.append(c)
hs = (C.c_void_p * ns)(*[c._h for c in counters]); drec, counts = C.c_void_p(), (C.c_long * ns)()
merger = tj.Counter(k)
total = L.tjamd_gather_histograms(merger._h, hs, ns, C.byref(drec), counts)
keys = torch.empty(total * 24, dtype=torch.uint8, device="cuda"); mat = torch.empty((total, ns), dtype=torch.int32, device="cuda")
nu = L.tjamd_merge_samples(merger._h, drec, counts, ns, C.c_void_p(keys.data_ptr()), C.c_void_p(mat.data_ptr()), total)
keys = keys[: nu * 24]
ref = tj.Reference(merger, (genome + "\n").encode())
ms_ref = merger.last_reference_ms()
ref.add_seeds(merger); ms_seed = merger.last_seed_order_ms()
n1, first = dev_locate(merger, ref, keys, 1, on_device=True)
keys_cpu = np.frombuffer(keys.cpu().numpy().tobytes(), np.uint64).reshape(-1, 3)
ctx_ids, _ = orc.tract_ids(keys_cpu); heads = np.flatnonzero(np.r_[True, ctx_ids[1:] != ctx_ids[:-1]])
for me, ms in ((3, 3), (2, 1), (1, 0)):
    rc, got, _ = dev_locate_gapped(merger, ref, keys, first, me, ms, with_how=False, on_device=True)
    a, b = time_calls(merger, ref, keys, nu, first, 1, me, ms)
    print(f"[pipeline] union {nu} rows, {ref.n_entries} entries: reference {ms_ref:.3f} ms, seed order {ms_seed:.3f} ms; locate(1) {a}; locate_gapped({me},{ms}) {b}; "
          f"rows {n1} -> {n1 + rc}; contexts {(first['flat'][heads] >= 0).sum()} -> {(got['flat'][heads] >= 0).sum()} of {len(heads)}", flush=True)
ref.close()
for c in counters + [merger]: c.close()

# 2. long ranges: a 5 Mbase random genome, k = 5 and k = 15
for k in (5, 15):
    rng = random.Random(k)
    g = ("".join(rng.choice("ACGT") for _ in range(5_000_000)) + "\n").encode()
    c = tj.Counter(k)
    def build():
        r = tj.Reference(c, g); t = c.last_reference_ms(); r.close(); return t
    ms_ref = rng10(build) if k == 15 else f"{build():.3f} ms"
    ref = tj.Reference(c, g)
    seeds = []
    for _ in range(4):
        r2 = tj.Reference(c, g); r2.add_seeds(c); seeds.append(c.last_seed_order_ms()); r2.close()
    ref.add_seeds(c)
    entries = ref.download()
    sub = entries[:: max(1, len(entries) // 20000)]
    keys_np = gapped_queries(rng, g[:200000], sub[sub["pos"] < 190000], k, n_each=75)[:343]
    kd = _dev(keys_np)
    n1, first = dev_locate(c, ref, kd, 1, on_device=True)
    rc, got, _ = dev_locate_gapped(c, ref, kd, first, 3, 3, with_how=False, on_device=True)
    a, b = time_calls(c, ref, kd, len(keys_np), first, 1, 3, 3)
    a3, b1 = time_calls(c, ref, kd, len(keys_np), first, 3, 2, 1)
    print(f"[5 Mbase] k = {k}, {ref.n_entries} entries: reference {ms_ref}, seed order {np.median(seeds):.3f} ms ({min(seeds):.3f}-{max(seeds):.3f}); {len(keys_np)} rows, "
          f"{n1} located by locate(1), {rc} more by locate_gapped(3,3): locate(1) {a}, locate(3) {a3}; locate_gapped(3,3) {b}, locate_gapped(2,1) {b1}", flush=True)
    ref.close(); c.close()
