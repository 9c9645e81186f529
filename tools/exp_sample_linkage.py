"""Diagnostic: the figures of DESIGN 3.5 N15.  tjamd_sample_linkage and tjamd_linkage_clusters at three shapes.
1. 125 000 sites x 8 samples, the pipeline-sized input of tools/exp_sample_distances.py: N8, N12, N13, N14 and then the tree of
   N14's matrix and its cut, the timers of N14 and N15 side by side in one run.
2. fabricated symmetric matrices at 1024 and 4096 samples (n_differ at random in 0 .. 999 of 1000 sites in common): the time, the
   launches, the rounds, and the bytes a call moves per second beside the HBM peak.
HIP-event timers of the library, twelve calls each, the median and range of the last ten.
The launch count is computed (one launch up to 64 samples; beyond, one key pass, two kernels a round for ceil (log2 n_samples)
rounds, one sort), and so are the rounds taken: rounds() restates the Boruvka rounds of the entry on the host and does not
observe the device.  The bytes are the key pass's (16 bytes read twice and 8 written per cell) plus 8 per cell for every round
that reads the key matrix: those that merge and the one that finds nothing left.  The observed launches, and the time of every kernel, come from a trace of this script:
   python tools/exp_sample_linkage.py
   rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp_sample_linkage.py"""
import ctypes as C, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p
from tests.test_linkage_cabi import NONE, link_keys, restate_linkage_clusters, restate_sample_linkage_prim, symmetric
VAR, SITE, ALLELE, TR, LOC, DIST, LINK = tj.VARIANT_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE, tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE, tj.SAMPLE_DISTANCE_DTYPE, tj.LINK_DTYPE
HBM_PEAK = 8.0e12                                                             # bytes a second, MI355X
L = tj.lib()

def last10(f):
    v = [f() for _ in range(12)][2:]
    return float(np.median(v)), f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})"

def rounds(K):
    """the rounds of the entry that merge something, restated: every component takes its smallest edge under (key, a, b)"""
    ns = K.shape[0]
    comp, idx, n = np.arange(ns), np.arange(ns), 0
    while True:
        M = np.where(comp[:, None] == comp[None, :], NONE, K)
        b = M.argmin(1)                                                       # (the first of equal keys: the smallest b)
        key = M[idx, b]
        rows = np.flatnonzero(key != NONE)
        if len(rows) == 0:
            return n
        n += 1
        pair = np.minimum(rows, b[rows]) * 4096 + np.maximum(rows, b[rows])
        order = np.lexsort((pair, key[rows], comp[rows]))
        first = order[np.r_[True, np.diff(comp[rows][order]) != 0]]           # a component's smallest (key, pair)
        parent = list(range(ns))
        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]; x = parent[x]
            return x
        for lo, hi in zip((pair[first] >> 12).tolist(), (pair[first] & 4095).tolist()):
            ra, rb = find(int(comp[lo])), find(int(comp[hi]))
            if ra != rb: parent[max(ra, rb)] = min(ra, rb)
        comp = np.array([find(int(x)) for x in comp])

def linkage(tag, counter, d_dist, ns, K, metric=tj.LINK_DIFFER, min_both=1, threshold=None):
    links = torch.zeros(ns * LINK.itemsize, dtype=torch.uint8, device="cuda"); cluster = torch.zeros(ns, dtype=torch.int32, device="cuda")
    def run():
        run.n = counter.sample_linkage(_p(d_dist), ns, metric, min_both, _p(links)); return counter.last_sample_linkage_ms()
    med, text = last10(run)
    got = np.frombuffer(links.cpu().numpy().tobytes(), LINK)[:run.n]
    n_rounds = max(1, int(np.ceil(np.log2(ns)))); taken = rounds(K); reading = min(taken + 1, n_rounds)
    ld = (ns + 1) & ~1
    moved = ns * ns * 32 + ns * ld * 8 * (1 + reading)
    threshold = int(np.median(got["key"])) if threshold is None else threshold
    def cut():
        cut.n = counter.linkage_clusters(_p(links), run.n, ns, threshold, _p(cluster)); return counter.last_linkage_clusters_ms()
    _, text_c = last10(cut)
    how = "1 launch (computed: one workgroup, the keys in LDS)" if ns <= 64 else f"{2 + 2 * n_rounds} launches (computed: 1 + 2 x {n_rounds} rounds + 1)"
    rate = "" if ns <= 64 else (f"; {moved / 1e6:.1f} MB moved by the key pass and {reading} reading rounds: {moved / med / 1e9:.3f} TB/s beside the HBM peak of "
                                 f"{HBM_PEAK / 1e12:.0f} TB/s, key matrix {ns * ld * 8 / 1e6:.1f} MB")
    print(f"[{tag}] sample_linkage {ns} samples: {text} in {how}, {taken} rounds merged (restated on the host), {run.n} links{rate}; "
          f"linkage_clusters at {threshold}: {text_c} in 1 launch, {cut.n} clusters", flush=True)
    return got, np.frombuffer(cluster.cpu().numpy().tobytes(), np.int32)

# 1. 125 000 tracts in eight samples on a random genome (the input of tools/exp_sample_distances.py)
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
h_dist = np.frombuffer(dist.cpu().numpy().tobytes(), DIST).reshape(ns, ns)
got, labels = linkage("125k sites, N14's matrix", c, dist, ns, link_keys(h_dist, tj.LINK_DIFFER, 1))
want = restate_sample_linkage_prim(h_dist, tj.LINK_DIFFER, 1)
assert got.tobytes() == want.tobytes() and labels.tolist() == restate_linkage_clusters(want, ns, int(np.median(want["key"]))).tolist()
print(f"[125k sites] {n_sites} sites x {ns} samples; beside sample_distances {ms_d}", flush=True)
ref.close()

# 2. fabricated matrices
for S in (1024, 4096):
    rng = np.random.RandomState(S)
    nd = rng.randint(0, 1000, (S, S)).astype(np.int64); np.fill_diagonal(nd, 0)
    h = symmetric(S, np.full((S, S), 1000), nd, 2 * nd)
    K = link_keys(h, tj.LINK_DIFFER, 1)
    dd = _dev(h)
    got, labels = linkage("fabricated", c, dd, S, K)
    want = restate_sample_linkage_prim(h, tj.LINK_DIFFER, 1)
    assert got.tobytes() == want.tobytes() and labels.tolist() == restate_linkage_clusters(want, S, int(np.median(want["key"]))).tolist()
    del dd
c.close()
