"""Diagnostic: the figures of DESIGN 3.5 N21.  tjamd_consensus_tree beside the loop its d_rep_count replaces: n_replicates calls of
tjamd_clade_support, each with another replicate as the base, on the same replicates in the same run:
1. 64 samples x 1000 replicates, 256 x 1000, 1024 x 256 and 4096 x 64: one balanced tree (halves down to pairs) over a random
   order, each replicate with n_samples / 16 random transpositions of that order, so that the replicates disagree.
2. 4096 x 64 once more with a caterpillar and no transposition: every clade but the class's first is compared with its leader,
   n_samples * n_samples / 2 loads a replicate: the worst case of the exact comparison.
HIP-event timers of the library: nine calls of tjamd_consensus_tree, the median and range of the last seven; the loop is run
four times and its time is the sum of its calls' timers, the median and range of the last three (the waits between its calls
are left out, so the host's wall time of both is reported as well).  d_rep_count of the call is checked against the loop's
d_support, byte for byte, and the counts of the kept classes against tjamd_clade_support with the consensus as the base.
   python tools/exp_consensus.py [--resources]
--resources: compile tatajuba_amd/csrc/hopo_device.hip with -Rpass-analysis=kernel-resource-usage (no GPU needed) and print the
table of the kernels of N21."""
import ctypes, os, re, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

def resources():
    src = os.path.join(ROOT, "tatajuba_amd", "csrc", "hopo_device.hip")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void ", "")}
            rows.append(cur)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split()[0]] = int(m.group(2))
    print(f"{'kernel':42s} SGPRs VGPRs scratch waves/SIMD LDS")
    for row in rows:
        if re.match(r"cons_", row["name"]):
            print(f"{row['name']:42s} {row['TotalSGPRs']:5d} {row['VGPRs']:5d} {row['ScratchSize']:7d} {row['Occupancy']:10d} {row['LDS']:6d}")

if "--resources" in sys.argv:
    resources()
    sys.exit(0)

import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p
NODE, CNODE = tj.TREE_NODE_DTYPE, tj.CONSENSUS_NODE_DTYPE

def spread(rows, skip):
    v = np.array(rows[skip:])                                                  # rows of (timer ms, wall ms)
    return [f"{np.median(c):.3f} ms ({c.min():.3f}-{c.max():.3f})" for c in v.T], np.median(v, axis=0)

def balanced(ns):
    iv = []
    def split(lo, hi):
        if hi - lo >= 2:
            iv.append((lo, hi - lo))
            split(lo, (lo + hi) // 2); split((lo + hi) // 2, hi)
    split(0, ns)
    return sorted(iv, key=lambda n: (n[1], n[0]))

def caterpillar(ns):
    return [(0, s) for s in range(2, ns + 1)]

def at(t, offset):
    return ctypes.c_void_p(t.data_ptr() + offset)

def shape(tag, c, ns, R, iv, swaps, seed):
    rng = np.random.RandomState(seed)
    nodes = np.zeros(len(iv), NODE)
    nodes["left"], nodes["right"] = -9, -9
    nodes["first"], nodes["size"] = [n[0] for n in iv], [n[1] for n in iv]
    rep_nodes = np.zeros((R, ns - 1), NODE)
    rep_nodes[:, : len(iv)] = nodes
    base = rng.permutation(ns).astype(np.int32)
    rep_order = np.tile(base, (R, 1))
    for r in range(R):
        for _ in range(swaps):
            a, b = rng.randint(0, ns, 2)
            rep_order[r, a], rep_order[r, b] = rep_order[r, b], rep_order[r, a]
    counts = [len(iv)] * R
    rnd, rod = _dev(rep_nodes), _dev(rep_order)
    cn, co, rcount, support = (torch.zeros(n * 4, dtype=torch.uint8, device="cuda") for n in (4 * ns, ns, R * (ns - 1), R * (ns - 1)))
    m = R // 2 + 1
    def call():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        call.n, call.classes = c.consensus_tree(_p(rnd), _p(rod), counts, ns, m, _p(cn), _p(co), _p(rcount))
        return c.last_consensus_tree_ms(), (time.perf_counter() - t0) * 1e3
    def loop():
        torch.cuda.synchronize(); t0 = time.perf_counter(); ms = 0.0
        for r in range(R):
            c.clade_support(at(rnd, r * (ns - 1) * 16), counts[r], at(rod, r * ns * 4), ns, _p(rnd), _p(rod), counts, at(support, r * (ns - 1) * 4)); ms += c.last_clade_support_ms()
        return ms, (time.perf_counter() - t0) * 1e3
    (ct, cw), cm = spread([call() for _ in range(9)], 2)
    (lt, lw), lm = spread([loop() for _ in range(4)], 1)
    assert torch.equal(rcount, support), tag                                   # the all-against-all counts: the same bytes
    held = torch.zeros(4 * ns, dtype=torch.uint8, device="cuda")
    c.clade_support(_p(cn), call.n, _p(co), ns, _p(rnd), _p(rod), counts, _p(held))
    kept = cn.cpu().numpy().view(CNODE)[: call.n]
    assert held.cpu().numpy().view(np.int32)[: call.n].tolist() == kept["count"].tolist() and (kept["count"] >= m).all(), tag
    print(f"[{tag}] {ns} samples x {R} replicates, {sum(counts)} clades in {call.classes} classes, {call.n} kept at {m}: one call {ct}, wall {cw}; "
          f"the loop of {R} calls {lt} (sum of timers), wall {lw}; timers {lm[0] / cm[0]:.2f}x, wall {lm[1] / cm[1]:.2f}x", flush=True)

c = tj.Counter(15)
for ns, R in ((64, 1000), (256, 1000), (1024, 256), (4096, 64)):
    shape("balanced", c, ns, R, balanced(ns), ns // 16, ns + R)
shape("caterpillar", c, 4096, 64, caterpillar(4096), 0, 1)
c.close()
