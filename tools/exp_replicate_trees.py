"""Diagnostic: the figures of DESIGN 3.5 N20.  tjamd_replicate_trees under single, complete and average linkage beside the loop it
replaces (tjamd_sample_linkage or tjamd_sample_agglomerate, then tjamd_linkage_tree, per replicate) on the same matrices in the
same run:
1. 8 samples x 100 replicates, the pipeline's shape.
2. 1024 samples x 32 replicates, n_differ at random in 0 .. 999 of 1000 sites in common; and with all keys equal
   (n_samples - 1 rounds under the agglomerative linkages).
3. 4096 samples x 4 replicates (one fabricated matrix four times: 1 GB of matrices on the device).
HIP-event timers of the library, twelve calls each, the median and range of the last ten; the loop's time is the sum of its
calls' timers, which leaves out the waits between them, so the host's wall time of both is reported as well.  Every replicate's
links, nodes and order of the batched call are checked against the loop's, byte for byte.  The launches and waits are computed
from the entries' rules with the rounds that the entries report (one round more is enqueued where a replicate ends as a forest)
and were not observed.
   python tools/exp_replicate_trees.py [--resources]
--resources: compile tatajuba_amd/csrc/hopo_device.hip with -Rpass-analysis=kernel-resource-usage (no GPU needed) and print the
table of the kernels of N15, N17, N18 and N20."""
import os, re, subprocess, sys, time
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
        if re.match(r"(linkage_|aggl_|rep_)", row["name"]):
            print(f"{row['name']:42s} {row['TotalSGPRs']:5d} {row['VGPRs']:5d} {row['ScratchSize']:7d} {row['Occupancy']:10d} {row['LDS']:6d}")

if "--resources" in sys.argv:
    resources()
    sys.exit(0)

import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p
from tests.test_linkage_cabi import symmetric
DIST, LINK, NODE = tj.SAMPLE_DISTANCE_DTYPE, tj.LINK_DTYPE, tj.TREE_NODE_DTYPE
BATCH = 32                                                                     # AGGL_BATCH of the library
NAMES = {tj.TREE_SINGLE: "single", tj.AGGL_COMPLETE: "complete", tj.AGGL_AVERAGE: "average"}

def last10(f):
    v = np.array([f() for _ in range(12)][2:])                                 # rows of (timer ms, wall ms)
    return [f"{np.median(c):.3f} ms ({c.min():.3f}-{c.max():.3f})" for c in v.T], np.median(v, axis=0)

def counts(ns, R, G, linkage, links, rounds):
    """(launches, waits) of the batched call and of the loop, from the rules"""
    if ns <= 64:
        return (1 + (R + G - 1) // G, 1), (2 * R, 2 * R)
    n_rounds = int(np.ceil(np.log2(ns)))
    groups = [range(r0, min(r0 + G, R)) for r0 in range(0, R, G)]
    if linkage == tj.TREE_SINGLE:
        one = 1 + 2 * n_rounds + 1
        return (1 + len(groups) * (one + 1), 1), (R * (one + 1), 2 * R)
    reading = [rounds[r] + (0 if links[r] == ns - 1 else 1) for r in range(R)]
    batches = [max(1, -(-x // BATCH)) for x in reading]
    queued = [min(b * BATCH, ns - 1) for b in batches]
    loop = (sum(2 + 4 * q + b + 1 for q, b in zip(queued, batches)), sum(batches) + R)
    gb = [max(batches[r] for r in g) for g in groups]
    return (1 + sum(1 + 4 * min(b * BATCH, ns - 1) + b + 1 for b in gb), sum(gb) + 1), loop

def shape(tag, c, dd, ns, R):
    links, nodes = (torch.zeros(R * ns * 16, dtype=torch.uint8, device="cuda") for _ in range(2))
    order = torch.zeros(R * ns * 4, dtype=torch.uint8, device="cuda")
    l1, n1 = (torch.zeros(R * ns * 16, dtype=torch.uint8, device="cuda") for _ in range(2))
    o1 = torch.zeros(R * ns * 4, dtype=torch.uint8, device="cuda")
    per = ns * ((ns + 1) & ~1) * 8 + 2 * (((ns + 1) & ~1) + 64 + 63 & ~63) * 4 + 2 * ns * 16 + ns * 4 + (ns - 1) * 16
    G = R if ns <= 64 else max(1, min(R, (1 << 30) // per))
    for linkage in (tj.TREE_SINGLE, tj.AGGL_COMPLETE, tj.AGGL_AVERAGE):
        def batched():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            batched.counts, batched.rounds = c.replicate_trees(_p(dd), ns, R, tj.LINK_DIFFER, 1, linkage, _p(links), _p(nodes), _p(order))
            wall = (time.perf_counter() - t0) * 1e3
            return c.last_replicate_trees_ms(), wall
        def loop():
            torch.cuda.synchronize(); t0 = time.perf_counter(); ms = 0.0
            for r in range(R):
                d_one = C_void(dd, r * ns * ns * DIST.itemsize); lr = C_void(l1, r * (ns - 1) * 16)
                if linkage == tj.TREE_SINGLE:
                    n = c.sample_linkage(d_one, ns, tj.LINK_DIFFER, 1, lr); ms += c.last_sample_linkage_ms()
                else:
                    n, _ = c.sample_agglomerate(d_one, ns, tj.LINK_DIFFER, 1, linkage, lr); ms += c.last_sample_agglomerate_ms()
                c.linkage_tree(lr, n, ns, C_void(n1, r * (ns - 1) * 16), C_void(o1, r * ns * 4)); ms += c.last_linkage_tree_ms()
            return ms, (time.perf_counter() - t0) * 1e3
        (bt, bw), bm = last10(batched)
        (lt, lw), lm = last10(loop)
        for r in range(R):                                                     # the same bytes
            n = batched.counts[r] * 16
            for a, b, stride in ((links, l1, (ns - 1) * 16), (nodes, n1, (ns - 1) * 16)):
                assert torch.equal(a[r * stride: r * stride + n], b[r * stride: r * stride + n]), (tag, linkage, r)
        assert torch.equal(order, o1)
        (bl, bwt), (ll, lwt) = counts(ns, R, G, linkage, batched.counts, batched.rounds)
        print(f"[{tag}] {ns} samples x {R} replicates, {NAMES[linkage]}: one call {bt}, wall {bw}, {bl} launches and {bwt} waits (computed, groups of {G}); "
              f"the loop {lt} (sum of timers), wall {lw}, {ll} launches and {lwt} waits (computed); rounds {min(batched.rounds)}..{max(batched.rounds)}; "
              f"timers {lm[0] / bm[0]:.2f}x, wall {lm[1] / bm[1]:.2f}x", flush=True)

def C_void(t, offset):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + offset)

def random_matrix(ns, seed):
    rng = np.random.RandomState(seed)
    nd = rng.randint(0, 1000, (ns, ns)).astype(np.int64); np.fill_diagonal(nd, 0)
    return symmetric(ns, np.full((ns, ns), 1000), nd, 2 * nd)

c = tj.Counter(15)
shape("pipeline shape", c, _dev(np.stack([random_matrix(8, r) for r in range(100)])), 8, 100)
shape("random keys", c, _dev(np.stack([random_matrix(1024, r) for r in range(32)])), 1024, 32)
S = 1024
full = np.ones((S, S), np.int64)
h_eq = symmetric(S, 3 * full, full - np.eye(S, dtype=np.int64), full - np.eye(S, dtype=np.int64))
shape("all keys equal", c, _dev(h_eq).repeat(32), S, 32)
del h_eq
shape("random keys", c, _dev(random_matrix(4096, 4096)).repeat(4), 4096, 4)
c.close()
