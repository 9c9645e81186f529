"""Diagnostic: the figures of DESIGN 3.5 N19.  tjamd_sample_distances_weighted under the weights of tjamd_bootstrap_weights at two
shapes, each beside the yardstick: as many calls of the unchanged tjamd_sample_distances as there are replicates, in the same run.
1. 20 000 sites x 1024 samples x 32 replicates (fabricate, seed 14: the second shape of tools/exp_sample_distances.py).
2. 125 000 sites x 8 samples x 100 replicates (fabricate, seed 14).
Then tjamd_clade_support at 1024 samples: the tree of a chain (the worst case: the clades' sizes sum to n^2 / 2) against 32
replicates of itself.
HIP-event timers of the library, twelve calls each, the median and range of the last ten; the yardstick's time is the sum of the
timers of its calls.  The launch counts it prints are computed: launches() restates the entry's rule for the tile edge, the
batches and the slices and does not observe the device.  The observed count, and the time of every kernel, come from a trace:
   python tools/exp_bootstrap.py
   rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp_bootstrap.py"""
import sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p
from tests.test_distances_cabi import fabricate
from tests.test_clades_cabi import links_of, restate_linkage_tree
DIST, BATCH = tj.SAMPLE_DISTANCE_DTYPE, 2

def last10(f):
    v = [f() for _ in range(12)][2:]
    return float(np.median(v)), f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})"

def launches(n_sites, ns, n_rep):
    """the launches of a weighted call as the entry's rule gives them (computed, not observed): the two check passes, the two
    instances of the tile kernel (one of them returns at once), and the kernel that sums the slices where the sites are split"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batches, t64 = -(-n_rep // BATCH), -(-ns // 64)
    E = 8 if ns <= 8 else 16 if ns <= 16 else 64 if t64 * (t64 + 1) // 2 * batches >= 2 * cus else 32
    tiles = -(-ns // E); pairs = tiles * (tiles + 1) // 2; chunks = -(-n_sites // (2048 // E))
    slices = max(1, min(chunks, 4 * cus // (pairs * batches)))
    per = -(-chunks // slices); slices = -(-chunks // per)
    return (5 if slices > 1 else 4), E, pairs, batches, slices

def shape(tag, c, T, S, R):
    h_sites, h_alleles, h_g = fabricate(T, S, np.random.RandomState(14))
    sites, alleles, gt = _dev(h_sites), _dev(h_alleles), _dev(h_g)
    w = torch.zeros(R * T, dtype=torch.int32, device="cuda")
    def weights():
        assert c.bootstrap_weights(T, R, 1, _p(w)) == R
        return c.last_bootstrap_weights_ms()
    _, ms_w = last10(weights)
    out = torch.zeros(R * S * S * DIST.itemsize, dtype=torch.uint8, device="cuda")
    def weighted():
        assert c.sample_distances_weighted(_p(sites), T, _p(alleles), len(h_alleles), _p(gt), S, _p(out), _p(w), R) == T
        return c.last_sample_distances_weighted_ms()
    med, text = last10(weighted)
    one = torch.zeros(S * S * DIST.itemsize, dtype=torch.uint8, device="cuda")
    def loop():
        ms = 0.0
        for _ in range(R):
            assert c.sample_distances(_p(sites), T, _p(alleles), len(h_alleles), _p(gt), S, _p(one)) == T
            ms += c.last_sample_distances_ms()
        return ms
    med_l, text_l = last10(loop)
    n, E, pairs, batches, slices = launches(T, S, R)
    d = np.frombuffer(out.cpu().numpy().tobytes(), DIST).reshape(R, S, S)
    zero = float((w == 0).float().mean())
    print(f"[{tag}] sample_distances_weighted {T} sites x {S} samples x {R} replicates: {text}, {med / R:.3f} ms a replicate, in {n} launches (computed from the entry's "
          f"rule: tile edge {E}, {pairs} tile pairs x {batches} batches of {BATCH} x {slices} slices of the sites); beside it {R} calls of sample_distances: {text_l}, "
          f"{med_l / R:.3f} ms a call; weighted / loop = {med / med_l:.2f}; bootstrap_weights {ms_w} in 1 launch behind a memset, {100 * zero:.1f} % of the weights are 0; "
          f"n_both up to {d['n_both'].max()}, length_diff up to {d['length_diff'].max()}", flush=True)

c = tj.Counter(15)
shape("1024 samples", c, 20_000, 1024, 32)
shape("8 samples", c, 125_000, 8, 100)

# the support of a chain's clades at 1024 samples: node j is the first j + 2 leaves
S, R = 1024, 32
tree = restate_linkage_tree(links_of([(0, j) for j in range(1, S)]), S)
nodes, order = _dev(tree["nodes"]), _dev(tree["order"])
rep_nodes, rep_order = _dev(np.tile(tree["nodes"], R)), _dev(np.tile(tree["order"], R))
support = torch.zeros(S - 1, dtype=torch.int32, device="cuda")
def run():
    assert c.clade_support(_p(nodes), S - 1, _p(order), S, _p(rep_nodes), _p(rep_order), [S - 1] * R, _p(support)) == S - 1
    return c.last_clade_support_ms()
_, text = last10(run)
assert (support.cpu().numpy() == R).all()
print(f"[support] clade_support {S} samples, a chain of {S - 1} nodes, {R} replicates: {text} in 2 launches", flush=True)
c.close()
