"""Every scan / sink variant of scan_device_piece against the CPU oracle on the edge corpus (tests/edge_streams.py), in a
plain `pytest -m gpu` run: the variants are selected per counter through the creation-time hooks TATAJUBA_AMD_FAST,
TATAJUBA_AMD_SINK and TATAJUBA_AMD_SCAN_GRID, which monkeypatch sets in front of tj.Counter(k).

Checks and strictness are those of tests/test_gpu_parity.py (check_raw_multiset, check_finalise): raw records as multisets,
the undefined-run count, finalised arrays byte for byte, both index arrays, coverage, status.  Integer work: no
tolerances.  Every cell also proves that it ran the path it names (uses_log, tjamd_debug_slow_tiles, last_partition_ms).
Nothing in this file skips."""
import ctypes as C
import random

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests import edge_streams as E
from tests.pyref import scan_closed_form
from tests.test_gpu_parity import as_records, rec_sorted

pytestmark = pytest.mark.gpu

FILTERS = [(0, 0), (1, 3)]                                    # (remove_biased, min_coverage)
M_OF_K = {2: 1, 10: 3, 12: 32, 13: 5, 16: 2, 17: 8, 28: 3, 29: 32, 32: 5}      # minimum tract sizes 1 2 3 5 8 32 spread over k
VARIANTS = {                                                  # name -> (TATAJUBA_AMD_FAST, TATAJUBA_AMD_SINK); None: unset
    "default": (None, None), "fused": (None, "fused"), "log": (None, "log"), "fast2": ("2", None),
    "fast2+fused": ("2", "fused"), "fast2+log": ("2", "log"), "fast0": ("0", None)}
VARIANTS_OF_W = {1: ["default", "fused", "fast2", "fast2+fused", "fast0"],
                 2: ["default", "log", "fast2", "fast2+log", "fast0"],
                 4: ["default", "fast2", "fast0"]}
K_OF_W = {1: [2, 10, 12], 2: [13, 16, 17, 28], 4: [29, 32]}
CELLS = [(k, v) for w in (1, 2, 4) for k in K_OF_W[w] for v in VARIANTS_OF_W[w]]
W_CELLS = [(w, v) for w in (1, 2, 4) for v in VARIANTS_OF_W[w]]
FUZZ_SEEDS = [101, 202, 303, 404, 505, 606, 707, 808, 909, 1010, 1111, 1212]
FUZZ_MAX_BYTES = 12 << 20


# ---- variants: environment, expectations ---------------------------------------------------------------------------

def set_variant(monkeypatch, variant, grid=None):
    fast, sink = VARIANTS[variant]
    for name, val in (("TATAJUBA_AMD_FAST", fast), ("TATAJUBA_AMD_SINK", sink), ("TATAJUBA_AMD_SCAN_GRID", None if grid is None else str(grid))):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def expects_log(k, variant):
    fast, sink = VARIANTS[variant]
    widest = {None: 1, "fused": 0, "log": 2}[sink]            # widest record that goes through the record log
    return fast != "0" and E.record_width(k) <= widest


def slow_tiles(c):
    L = tj.lib()
    L.tjamd_debug_slow_tiles.restype = C.c_long
    L.tjamd_debug_slow_tiles.argtypes = [C.c_void_p]
    return int(L.tjamd_debug_slow_tiles(c._h))


def prove_path(c, k, variant, n_bytes, candidate_limit=False):
    """after a scan of n_bytes in one launch: the counter ran the kernels its cell names"""
    fast = VARIANTS[variant][0]
    log = expects_log(k, variant)
    n_fast_tiles = (n_bytes + E.FK_OWN - 1) // E.FK_OWN
    assert c.uses_log() == log, (variant, k)
    assert c.last_scan_launches() == 1
    assert (c.last_partition_ms() > 0) == log, (variant, k, c.last_partition_ms())
    n_slow = slow_tiles(c)
    if fast == "2":
        assert n_slow == n_fast_tiles, (n_slow, n_fast_tiles)         # the fast kernel handed every tile over
    elif fast == "0":
        assert n_slow == 0, n_slow                                     # no fast kernel: nothing is ever listed
    else:
        assert 0 <= n_slow <= n_fast_tiles
        if candidate_limit:
            assert 0 < n_slow < n_fast_tiles, (n_slow, n_fast_tiles)   # only the tiles over FK_MAXCAND (and the stream's ends)


# ---- the oracle, once per (stream, k, m) ------------------------------------------------------------------------------

_STREAMS, _ORACLE = {}, {}


def stream_of(key, make):
    if key not in _STREAMS:
        _STREAMS[key] = np.ascontiguousarray(make())
    return _STREAMS[key]


def two_batches(s):
    """the stream cut after the read delimiter nearest its middle; a stream of one read: the stream twice"""
    nl = np.nonzero(s[:-1] == E.NL)[0]
    if nl.size == 0:
        return [s, s]
    cut = int(nl[np.argmin(np.abs(nl - s.size // 2))]) + 1
    return [s[:cut], s[cut:]]


def oracle_of(key, s, k, m, filters=FILTERS):
    ck = (key, k, m)
    if ck not in _ORACLE:
        o = orc.Oracle(k)
        o.scan_stream(s, m)
        ref = {"raw": rec_sorted(as_records(o.elems())), "undef": int(o.c.n_undefined), "fin": {}}
        o.close()
        _ORACLE[ck] = ref
    ref = _ORACLE[ck]
    for f in filters:
        if f not in ref["fin"]:
            o = orc.Oracle(k)
            for p in two_batches(s):
                o.scan_stream(p, m)
            n_raw = int(o.c.n_elem)
            o.finalise(*f)
            st = int(o.c.status)
            ref["fin"][f] = {"n_raw": n_raw, "status": st, "n": int(o.c.n_elem), "kept": o.elems().tobytes() if st == 0 else b"",
                             "idx": o.idx() if st == 0 else None, "n_idx": int(o.c.n_idx), "coverage": int(o.c.coverage)}
            o.close()
    return ref


def check_raw(c, ref, what):
    got = c.download_raw()
    exp = ref["raw"]
    assert len(got) == len(exp), (what, len(got), len(exp))
    got = rec_sorted(got)
    if not (got == exp).all():
        bad = np.nonzero(got != exp)[0]
        raise AssertionError("%s: %d of %d sorted raw records differ from the oracle, first at %d: got %s, expected %s"
                             % (what, bad.size, len(exp), bad[0], got[bad[0]], exp[bad[0]]))
    assert c.undefined_runs() == ref["undef"], (what, c.undefined_runs(), ref["undef"])


def check_fin(c, f, st, what):
    assert st == f["status"], (what, st, f["status"])
    if st != 0:
        return
    assert c.n_kept == f["n"], (what, c.n_kept, f["n"])
    assert c.download_kept().tobytes() == f["kept"], what + ": kept records differ from the oracle"
    gi, gf = c.download_idx()
    ei, ef = f["idx"]
    assert c.n_idx == f["n_idx"] and (gi == ei).all() and (gf == ef).all(), what + ": index ranges"
    assert c.coverage == f["coverage"], (what, c.coverage, f["coverage"])


def check_stream(monkeypatch, variant, key, s, k, m, grid=None, candidate_limit=False, prove=True, filters=FILTERS):
    """one scan for the raw multiset, then for each filter: reset, the stream in two batches, finalise"""
    what = "%s k=%d m=%d %s grid=%s" % (key, k, m, variant, grid)
    ref = oracle_of(key, s, k, m, filters)
    set_variant(monkeypatch, variant, grid)
    c = tj.Counter(k)
    c.scan_host(s, m)
    check_raw(c, ref, what)
    if prove:
        prove_path(c, k, variant, s.size, candidate_limit)
    for f in filters:
        c.reset()
        for p in two_batches(s):
            c.scan_host(p, m)
        assert c.raw_count() == ref["fin"][f]["n_raw"], (what, f)
        check_fin(c, ref["fin"][f], c.finalise(*f), what + " filter=%s" % (f,))
    c.close()
    return len(ref["raw"])


# ---- the cells ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,variant", CELLS, ids=["k%d-%s" % c for c in CELLS])
def test_variant_cell_on_the_edge_corpus(monkeypatch, k, variant):
    m = M_OF_K[k]
    n_rec = 0
    # tracts on the seams of the fast kernel's, the generic kernel's and the located scan's tiles
    for tile in E.SEAM_TILES:
        for kind in E.SEAM_KINDS:
            s = stream_of(("seam", tile, k, m, kind), lambda: E.seam_stream(tile, k, m, kind))
            n_rec += check_stream(monkeypatch, variant, "seam-%d-%s" % (tile, kind), s, k, m)
    # the candidate limit (m = 2): whole grid, and one workgroup that walks every tile (ncand / bad rotation, many staging passes)
    s = stream_of("cand", E.candidate_limit_stream)
    for grid in (None, 1):
        n_rec += check_stream(monkeypatch, variant, "cand", s, k, 2, grid=grid, candidate_limit=True)
    # the record log's block ring (m = 2): j * RB - 1, j * RB, j * RB + 1 records through 1 and 8 workgroups
    for j in E.LOG_RING_J:
        for delta in (-1, 0, 1):
            s = stream_of(("ring", k, j, delta), lambda: E.log_ring_stream(k, j, delta))
            for grid in (1, 8):
                n = check_stream(monkeypatch, variant, "ring-%d%+d" % (j, delta), s, k, 2, grid=grid)
                assert n == j * E.log_block_records(k) + delta
    s = stream_of(("sparse", k), lambda: E.sparse_stream(k))
    for grid in (None, 1):
        assert check_stream(monkeypatch, variant, "sparse", s, k, 2, grid=grid) == 7
    s = stream_of("delims", E.delimiters_only_stream)
    for grid in (None, 1):
        assert check_stream(monkeypatch, variant, "delims", s, k, 2, grid=grid, prove=False) == 0
    # one hash bucket: one key (two keys) over more than three chunks
    for n_keys in (1, 2):
        s = stream_of(("bucket", k, n_keys), lambda: E.one_bucket_stream(k, n_keys))
        for grid in (None, 8):
            assert check_stream(monkeypatch, variant, "bucket-%d" % n_keys, s, k, m, grid=grid) > n_keys * 3 * E.MIN_CHUNK
    assert n_rec > 100000


# ---- the fix list ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,variant", W_CELLS, ids=["W%d-%s" % c for c in W_CELLS])
def test_fix_list_at_its_capacity(monkeypatch, w, variant):
    """TJ_FIX_CAP - 1 and TJ_FIX_CAP countable runs of 'N' in one batch equal the oracle; one more fails with
    TJAMD_ERR_CAPACITY when the counts are next fetched, returns no records, and leaves a counter that a reset makes good"""
    k, m = {1: 10, 2: 16, 4: 32}[w], 2
    L = tj.lib()
    for n in (E.TJ_FIX_CAP - 1, E.TJ_FIX_CAP):
        s = stream_of(("fix", n), lambda: E.fix_list_stream(n))
        assert check_stream(monkeypatch, variant, "fix-%d" % n, s, k, m, filters=[(0, 0)]) == 2 * n
    over = stream_of(("fix", E.TJ_FIX_CAP + 1), lambda: E.fix_list_stream(E.TJ_FIX_CAP + 1))
    clean = stream_of(("seam", E.FK_OWN, k, M_OF_K[k], "nocall"), lambda: E.seam_stream(E.FK_OWN, k, M_OF_K[k], "nocall"))
    ref = oracle_of("seam-%d-nocall" % E.FK_OWN, clean, k, M_OF_K[k])
    set_variant(monkeypatch, variant)
    for fetch in ("raw_count", "finalise"):
        c = tj.Counter(k)
        c.scan_host(over, m)
        if fetch == "raw_count":
            L.tjamd_raw_count.restype = C.c_long
            L.tjamd_raw_count.argtypes = [C.c_void_p]
            assert L.tjamd_raw_count(c._h) == -4                          # -TJAMD_ERR_CAPACITY
        else:
            st = C.c_int(-1)
            assert L.tjamd_finalise(c._h, 0, 0, C.byref(st)) == 4         # TJAMD_ERR_CAPACITY
        assert "non-ACGTU" in L.tjamd_last_error().decode(), L.tjamd_last_error()
        if fetch == "raw_count":                                          # the error stays until a reset: no records come out
            with pytest.raises(tj.TatajubaAmdError, match="non-ACGTU"):
                c.download_raw()
        else:                                                             # a failed finalise leaves nothing kept and nothing raw
            assert st.value == -1 and c.n_kept == 0 and c.raw_count() == 0
        # the same counter after a reset: a clean scan equals the oracle, no flag survives
        c.reset()
        c.scan_host(clean, M_OF_K[k])
        check_raw(c, ref, "after the fix-list overflow (%s)" % fetch)
        c.reset()
        for p in two_batches(clean):
            c.scan_host(p, M_OF_K[k])
        check_fin(c, ref["fin"][(1, 3)], c.finalise(1, 3), "after the fix-list overflow (%s)" % fetch)
        c.close()


# ---- the located scan on the seams of its 4096-byte tiles -----------------------------------------------------------------

@pytest.mark.parametrize("k", sorted(M_OF_K))
def test_located_scan_on_seam_streams(k):
    m = M_OF_K[k]
    for kind in E.SEAM_KINDS:
        s = stream_of(("seam", E.LOC_TILE, k, m, kind), lambda: E.seam_stream(E.LOC_TILE, k, m, kind))
        reads, starts = E.cut_reads(s)
        exp = []
        for r, st in zip(reads, starts):
            for (base, n, off, flag, c0, c1) in scan_closed_form(r.decode("latin-1"), k, m):
                exp.append((c0, c1, base | ((n & 0x3ff) << 2) | (1 << 12) | (0xffe << 32) | (flag << 49), int(st) + off + k))
        c = tj.Counter(k)
        loc = c.scan_host_located(s, m)
        got = list(zip(loc["ctx0"].tolist(), loc["ctx1"].tolist(), loc["meta"].tolist(), loc["pos"].tolist()))
        assert len(got) == len(exp) > 20, (k, kind, len(got), len(exp))
        assert got == exp, (k, kind)
        c.close()


# ---- seeded fuzz: the generator of tools/fuzz_gpu.py, a fixed list of seeds through every W x variant ------------------------

_FUZZ = {}


def fuzz_case(w, seed):
    if (w, seed) not in _FUZZ:
        rng = random.Random(seed * 10 + w)
        k = rng.choice({1: [2, 3, 5, 8, 10, 12], 2: [13, 15, 20, 25, 28], 4: [29, 31, 32]}[w])
        m = rng.choice([1, 2, 3, 4, 6])
        f = (rng.choice([0, 1]), rng.choice([0, 1, 3, 5, 50]))
        while True:                                               # (the tool's largest streams are left to the tool: time)
            parts = [E.random_stream(rng, tj.synth_stream)[0] for _ in range(rng.choice([1, 1, 2, 3]))]
            if sum(p.size for p in parts) <= FUZZ_MAX_BYTES:
                break
        parts = [np.ascontiguousarray(p) for p in parts]
        refs = []
        for use in (parts, parts[:1]):                            # the sample; then the counter again with its first part
            o = orc.Oracle(k)
            for p in use:
                o.scan_stream(p, m)
            n_raw = int(o.c.n_elem)
            o.finalise(*f)
            st = int(o.c.status)
            refs.append({"n_raw": n_raw, "status": st, "n": int(o.c.n_elem), "kept": o.elems().tobytes() if st == 0 else b"",
                         "idx": o.idx() if st == 0 else None, "n_idx": int(o.c.n_idx), "coverage": int(o.c.coverage)})
            o.close()
        _FUZZ[(w, seed)] = (k, m, f, parts, refs)
    return _FUZZ[(w, seed)]


@pytest.mark.parametrize("w,variant", W_CELLS, ids=["W%d-%s" % c for c in W_CELLS])
def test_seeded_fuzz_through_every_variant(monkeypatch, w, variant):
    for seed in FUZZ_SEEDS:
        k, m, f, parts, refs = fuzz_case(w, seed)
        what = "fuzz seed %d k=%d m=%d %s" % (seed, k, m, variant)
        set_variant(monkeypatch, variant)
        c = tj.Counter(k)
        assert c.uses_log() == expects_log(k, variant)
        for p in parts:
            c.scan_host(p, m)
        assert c.raw_count() == refs[0]["n_raw"], what
        check_fin(c, refs[0], c.finalise(*f), what)
        c.scan_host(parts[0], m)                                  # the counter again after a finalise, as the tool does
        assert c.raw_count() == refs[1]["n_raw"], what + " (reuse)"
        check_fin(c, refs[1], c.finalise(*f), what + " (reuse)")
        c.close()
