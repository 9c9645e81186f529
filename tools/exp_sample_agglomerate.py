"""Diagnostic: the figures of DESIGN 3.5 N18.  tjamd_sample_agglomerate under both linkages beside tjamd_sample_linkage on the same
matrix in the same run, at the shapes of tools/exp_sample_linkage.py and one more:
1. 125 000 sites x 8 samples, the pipeline-sized input: N8, N12, N13, N14 and then the three trees of N14's matrix.
2. fabricated symmetric matrices at 1024 and 4096 samples (n_differ at random in 0 .. 999 of 1000 sites in common).
3. 1024 samples with all keys equal: n_samples - 1 rounds, one pair a round, the shape that the batches of rounds are for.
4. the batch constant: shapes 2 (1024) and 3 again with counters made under TATAJUBA_AMD_AGGL_BATCH = 4 .. 1024.
HIP-event timers of the library, twelve calls each, the median and range of the last ten.  The rounds are the entry's own count
(*h_n_rounds), checked against the host restatement where that is affordable.  The launches are computed from the entry's rule
(one up to 64 samples; beyond, the key pass, the init pass, four kernels for every round enqueued and a sort kernel behind
every batch) and were not observed; so are the bytes: the key pass's 16 read twice and 8 written per cell, the init pass's
read of the keys under AVERAGE, and per round 8 bytes for every cell of a live row (the row minimum), 24 for every cell of
a merged row (two read, one written) and 24 for every (live row, pair).
   python tools/exp_sample_agglomerate.py"""
import ctypes as C, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tatajuba_amd as tj
from tests.test_locate import _dev, _p
from tests.test_linkage_cabi import NONE, link_keys, symmetric
from tests.test_agglomerate_cabi import _f, restate_sample_agglomerate
VAR, SITE, ALLELE, TR, LOC, DIST, LINK = tj.VARIANT_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE, tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE, tj.SAMPLE_DISTANCE_DTYPE, tj.LINK_DTYPE
L = tj.lib()
BATCH = 32                                                                     # AGGL_BATCH of the library
NAMES = {tj.AGGL_COMPLETE: "complete", tj.AGGL_AVERAGE: "average"}

def last10(f):
    v = [f() for _ in range(12)][2:]
    return float(np.median(v)), f"{np.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})"

def round_stats(K, linkage):
    """(live rows, pairs) of every round that reads the matrix, the last one, which finds nothing or is cut short, included"""
    K = K.copy(); ns = K.shape[0]; size = np.ones(ns, np.uint64); idx = np.arange(ns); out = []
    while True:
        D = K if linkage == tj.AGGL_COMPLETE else np.where(K != NONE, K // np.maximum(size[:, None] * size[None, :], np.uint64(1)), NONE)
        nn = D.argmin(1)
        X = np.flatnonzero((D[idx, nn] != NONE) & (nn[nn] == idx) & (idx < nn)); Y = nn[X]
        out.append((int((size > 0).sum()), len(X)))
        if len(X) == 0 or int((size > 0).sum()) - len(X) == 1:
            return out
        K[X, :] = _f(K[X, :], K[Y, :], linkage); K[:, X] = _f(K[:, X], K[:, Y], linkage); K[Y, :] = NONE; K[:, Y] = NONE
        size[X] += size[Y]; size[Y] = 0

def launches(ns, reading_rounds, batch):
    if ns <= 64:
        return 1, 1
    batches = max(1, -(-reading_rounds // batch))
    return 2 + 4 * min(batches * batch, ns - 1) + batches, batches

def moved(ns, linkage, stats):
    ld = (ns + 1) & ~1
    b = ns * ns * 32 + ns * ld * 8 + (ns * ld * 8 if linkage == tj.AGGL_AVERAGE else 0)
    return b + sum(live * ld * 8 + pairs * ld * 24 + (live - pairs) * pairs * 24 for live, pairs in stats)

def trees(tag, counter, d_dist, ns, h=None, stats_of=None, batch=BATCH, single=True):
    links = torch.zeros(ns * LINK.itemsize, dtype=torch.uint8, device="cuda")
    if single:
        def run_single():
            run_single.n = counter.sample_linkage(_p(d_dist), ns, tj.LINK_DIFFER, 1, _p(links)); return counter.last_sample_linkage_ms()
        _, text = last10(run_single)
        print(f"[{tag}] {ns} samples, sample_linkage (single) in the same run: {text}, {run_single.n} links", flush=True)
    for linkage in (tj.AGGL_COMPLETE, tj.AGGL_AVERAGE):
        def run():
            run.n, run.rounds = counter.sample_agglomerate(_p(d_dist), ns, tj.LINK_DIFFER, 1, linkage, _p(links)); return counter.last_sample_agglomerate_ms()
        med, text = last10(run)
        got = np.frombuffer(links.cpu().numpy().tobytes(), LINK)[:run.n]
        stats = stats_of(linkage) if stats_of else round_stats(link_keys(h, tj.LINK_DIFFER, 1), linkage)
        assert sum(1 for live, pairs in stats if pairs) == run.rounds, (len(stats), run.rounds)
        if h is not None:
            want, want_rounds = restate_sample_agglomerate(h, tj.LINK_DIFFER, 1, linkage)
            assert got.tobytes() == want.tobytes() and run.rounds == want_rounds
        n_launch, batches = launches(ns, len(stats), batch)
        b = moved(ns, linkage, stats)
        rate = "" if ns <= 64 else f"; {b / 1e6:.1f} MB moved (computed): {b / med / 1e9:.3f} TB/s"
        print(f"[{tag}] {ns} samples, sample_agglomerate {NAMES[linkage]}: {text}, {run.rounds} rounds merged, {run.n} links, {n_launch} launches and {batches} waits "
              f"(computed, batches of {batch}){rate}", flush=True)

def counter_with_batch(k, batch):
    saved = os.environ.get("TATAJUBA_AMD_AGGL_BATCH")
    os.environ["TATAJUBA_AMD_AGGL_BATCH"] = str(batch)
    c = tj.Counter(k)
    if saved is None: del os.environ["TATAJUBA_AMD_AGGL_BATCH"]
    else: os.environ["TATAJUBA_AMD_AGGL_BATCH"] = saved
    return c

# 1. 125 000 tracts in eight samples on a random genome (the input of tools/exp_sample_linkage.py)
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
assert c.sample_distances(_p(sites), n_sites, _p(alleles), n_alleles, _p(gt), ns, _p(dist)) == n_sites
h_dist = np.frombuffer(dist.cpu().numpy().tobytes(), DIST).reshape(ns, ns)
trees("125k sites, N14's matrix", c, dist, ns, h=h_dist)
ref.close()
del kd, md, td, ld_, d_var, sites, alleles, gt12, gt

# 2. fabricated matrices
fabricated = {}
for S in (1024, 4096):
    rng = np.random.RandomState(S)
    nd = rng.randint(0, 1000, (S, S)).astype(np.int64); np.fill_diagonal(nd, 0)
    h = symmetric(S, np.full((S, S), 1000), nd, 2 * nd)
    dd = _dev(h)
    if S == 1024: trees("fabricated", c, dd, S, h=h)
    else: trees("fabricated", c, dd, S, stats_of=lambda l: round_stats(link_keys(h, tj.LINK_DIFFER, 1), l))   # (4096: the restatement is tests/test_agglomerate.py's, once)
    if S == 1024: fabricated[S] = (h, dd)
    del dd, h

# 3. all keys equal: everyone's nearest neighbour is cluster 0, one pair merges a round
S = 1024
full = np.ones((S, S), np.int64)
h_eq = symmetric(S, 3 * full, full - np.eye(S, dtype=np.int64), full - np.eye(S, dtype=np.int64))
d_eq = _dev(h_eq)
equal_stats = lambda linkage: [(S - r, 1) for r in range(S - 1)]
trees("all keys equal", c, d_eq, S, stats_of=equal_stats)

# 4. the batch constant
h, dd = fabricated[1024]
stats = {l: round_stats(link_keys(h, tj.LINK_DIFFER, 1), l) for l in NAMES}
for batch in (4, 8, 16, 32, 64, 128, 1024):
    cb = counter_with_batch(k, batch)
    trees(f"batch {batch}, fabricated", cb, dd, 1024, stats_of=lambda l: stats[l], batch=batch, single=False)
    trees(f"batch {batch}, all keys equal", cb, d_eq, S, stats_of=equal_stats, batch=batch, single=False)
    cb.close()
c.close()
