"""The ordering step of a begun finalise on the library's side stream, beside the next sample's scan.

A counter on which tjamd_counter_set_order_stream was never called queues the ordering step of tjamd_finalise_begin on a
side stream that the library owns (one per device), TATAJUBA_AMD_ORDER=main at its creation keeps the step on the counter's
stream, and the step's kernels are new: a workgroup scan of 256 threads, bin_sort_index_kernel for bins of at most 64 records
with bin_sort_full_kernel behind it for the fuller ones it lists.  Strictness as in tests/test_gpu_parity.py and
tests/test_finalise_edges.py: status, every byte of the kept elements, both index arrays, n_idx and the coverage equal the CPU
oracle's.  Every cell also proves the path it names through tjamd_debug_order_path (1: planned and queued on another stream,
2: run with the count in hand on the counter's stream, 4: planned and queued on the counter's stream).  Nothing here skips."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests import finalise_edges as F
from tests.test_finalise_edges import check_corpus, compare

pytestmark = pytest.mark.gpu

ASIDE, IN_HAND, PLANNED_MAIN = 1, 2, 4
MODES = {"default": ASIDE, "main": PLANNED_MAIN, "cap1": ASIDE | IN_HAND, "noplan": IN_HAND}
HOOKS = ("TATAJUBA_AMD_ORDER", "TATAJUBA_AMD_PLAN_CAP", "TATAJUBA_AMD_NO_PLAN", "TATAJUBA_AMD_NO_FUSED_BINS")


def order_path(c):
    f = tj.lib().tjamd_debug_order_path
    f.restype, f.argtypes = C.c_long, [C.c_void_p]
    return int(f(c._h))


def set_mode(monkeypatch, mode):
    """the environment of a mode: TATAJUBA_AMD_ORDER is read when a counter is made, the others when a finalise is queued"""
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    if mode == "main":
        monkeypatch.setenv("TATAJUBA_AMD_ORDER", "main")
    elif mode == "cap1":
        monkeypatch.setenv("TATAJUBA_AMD_PLAN_CAP", "1")
    elif mode == "noplan":
        monkeypatch.setenv("TATAJUBA_AMD_NO_PLAN", "1")


def outcome(c, st):
    out = {"status": st, "n": 0, "kept": b"", "idx": (np.zeros(0, np.int32), np.zeros(0, np.int32)), "n_idx": 0, "coverage": 0}
    if st == 0:
        out.update(n=c.n_kept, kept=c.download_kept().tobytes(), idx=c.download_idx(), n_idx=c.n_idx, coverage=c.coverage)
    return out


def oracle_outcome(o, f):
    o.finalise(*f)
    st = int(o.c.status)
    return {"status": st, "n": int(o.c.n_elem), "kept": o.elems().tobytes() if st == 0 else b"", "idx": o.idx() if st == 0 else None,
            "n_idx": int(o.c.n_idx) if st == 0 else 0, "coverage": int(o.c.coverage) if st == 0 else 0}


# ---- the bench's loop at small size ---------------------------------------------------------------------------------------

M_LOOP, F_LOOP = 3, (1, 3)
_SAMPLES, _LOOP_REF = {}, {}


def loop_samples():
    if not _SAMPLES:
        for i in range(4):
            _SAMPLES[i] = tj.synth_stream(2000 + 100 * i, 150, 20000, seed_reads=500 + i)      # ~300 KB, depth 15
    return _SAMPLES


def loop_reference(k, i):
    """the oracle on sample i at this k: computed once, shared by the modes"""
    if (k, i) not in _LOOP_REF:
        o = orc.Oracle(k)
        o.scan_stream(loop_samples()[i], M_LOOP)
        _LOOP_REF[(k, i)] = oracle_outcome(o, F_LOOP)
        o.close()
    return _LOOP_REF[(k, i)]


@pytest.mark.parametrize("k", [10, 16, 30])
def test_two_counters_take_turns_on_one_stream(monkeypatch, k):
    """bench.py's loop: sample i + 1 is scanned and its finalise begun before sample i's finalise is ended, two counters on
    one stream of torch's making.  Four samples, four modes; every sample equals the oracle, default equals main"""
    import torch
    samples = loop_samples()
    devs = [torch.from_numpy(samples[i].copy()).cuda() for i in range(4)]
    shared = torch.cuda.Stream()
    assert shared.cuda_stream != 0
    torch.cuda.synchronize()
    results = {}
    for mode, want_path in MODES.items():
        set_mode(monkeypatch, mode)
        ctr = [tj.Counter(k), tj.Counter(k)]
        for c in ctr:
            c.set_stream(shared.cuda_stream)
        got, begun = {}, None

        def end(i):
            c = ctr[i & 1]
            got[i] = outcome(c, c.finalise_end())
            assert order_path(c) == want_path, (k, mode, i, order_path(c))
            assert c.plan_mismatches() == 0

        for i in range(4):
            c = ctr[i & 1]
            c.reset()
            c.scan_device(devs[i].data_ptr(), samples[i].size, M_LOOP)
            c.finalise_begin(*F_LOOP)
            if begun is not None:
                end(begun)
            begun = i
        end(begun)
        for i in range(4):
            exp = loop_reference(k, i)
            assert exp["status"] == 0 and exp["n"] > 100, (k, i, exp["status"], exp["n"])
            compare(got[i], exp, "k=%d %s sample %d" % (k, mode, i))
        results[mode] = got
        for c in ctr:
            c.close()
    for i in range(4):
        a, b = results["default"][i], results["main"][i]
        assert (a["status"], a["kept"], a["n_idx"], a["coverage"]) == (b["status"], b["kept"], b["n_idx"], b["coverage"]), (k, i)
        assert (a["idx"][0] == b["idx"][0]).all() and (a["idx"][1] == b["idx"][1]).all(), (k, i)


def test_an_explicit_null_means_no_side_stream_and_a_handle_means_that_stream(monkeypatch):
    import torch
    set_mode(monkeypatch, "default")
    s = loop_samples()[0]
    exp = loop_reference(10, 0)
    other = torch.cuda.Stream()
    c = tj.Counter(10)
    for handle, want in ((None, PLANNED_MAIN), (other.cuda_stream, ASIDE), (None, PLANNED_MAIN)):
        c.set_order_stream(handle)
        c.reset()
        c.scan_host(s, M_LOOP)
        c.finalise_begin(*F_LOOP)
        compare(outcome(c, c.finalise_end()), exp, "order stream %s" % (handle,))
        assert order_path(c) == want, (handle, order_path(c))
    # tjamd_finalise (one call) never leaves the counter's stream
    c.reset()
    c.scan_host(s, M_LOOP)
    compare(outcome(c, c.finalise(*F_LOOP)), exp, "one call")
    assert order_path(c) == PLANNED_MAIN
    c.close()


# ---- the sort kernels' edges ---------------------------------------------------------------------------------------------------

# bins of exactly 1, 2, 63, 64, 65, 66, 128, 129, 255 and 256 records among 64 bins of which the others are empty (64: the last
# bin bin_sort_index_kernel sorts itself; 65 and 256: the first and last size it lists for bin_sort_full_kernel); a bin of 257:
# the radix fallback; under the corpus's min_coverage the bin of one record loses its only context.
STAIRS = ["bin_staircase-k%d-top%d-%s" % (k, top, lane63) for k in (10, 20, 31) for top, lane63 in ((256, "alone"), (256, "whole"), (257, "alone"))]


@pytest.mark.parametrize("mode", ["default", "main", "cap1"])
@pytest.mark.parametrize("name", STAIRS)
def test_bins_at_the_sort_kernels_limits(monkeypatch, name, mode):
    corpus = F.get(name)
    assert 64 in corpus.facts["bins"] and 65 in corpus.facts["bins"] and 1 in corpus.facts["bins"] and max(corpus.facts["bins"]) in (256, 257)
    set_mode(monkeypatch, mode)
    c = tj.Counter(corpus.k)
    for f in ((0, 0), (1, corpus.min_coverage)):
        # (check_corpus sets the plan hooks of its `path` itself: "cap-1" is one below the kept count, a second attempt as cap1's)
        assert check_corpus(monkeypatch, name, "cap-1" if mode == "cap1" else "default", [f], two_calls=True, counter=c) == 1
        assert order_path(c) == MODES[mode], (name, mode, f, order_path(c))
    c.close()


# ---- the workgroup scan's chunk boundary ---------------------------------------------------------------------------------------

def wgs_chunk():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tatajuba_amd", "csrc", "hopo_device.hip")).read()
    threads = int(re.search(r"^#define WGS_THREADS\s+(\d+)", src, re.M).group(1))
    per = int(re.search(r"^#define WGS_PER\s+(\d+)", src, re.M).group(1))
    return threads * per


@pytest.mark.parametrize("which", ["48chunk-1", "48chunk+1", "96chunk+1"])
def test_more_bins_than_one_chunk_of_the_workgroup_scan(monkeypatch, which):
    """bin_bits_for gives 2 x chunk bins once more than 48 x chunk records are kept, 4 x chunk above twice that: the scan of
    the bin counts (and of the bins' context counts) then carries from chunk to chunk.  The kept set is made without a large
    stream: every key is uploaded twice, once per strand, as raw records; a stream without a tract, scanned behind them,
    lifts the host's bound of the raw count so far that the ordering step is planned ahead and goes to the side stream."""
    import torch
    chunk = wgs_chunk()
    n1 = {"48chunk-1": 48 * chunk - 1, "48chunk+1": 48 * chunk + 1, "96chunk+1": 96 * chunk + 1}[which]
    k = 10
    nbins = 1 << F.bin_bits_for(n1, k)
    assert nbins == {"48chunk-1": chunk, "48chunk+1": 2 * chunk, "96chunk+1": 4 * chunk}[which], (n1, nbins, chunk)
    corpus = F.kept_exactly_full(k, 2 * n1)
    o = orc.Oracle(k)
    for p in corpus.parts():
        o.scan_stream(p, F.M)
    raw = o.elems()
    o.close()
    assert len(raw) == 2 * n1
    f = (1, 2)
    o = F.oracle_from_raw(k, raw)
    exp = oracle_outcome(o, f)
    o.close()
    assert exp["status"] == 0 and exp["n"] == n1
    blank = np.tile(np.frombuffer(b"ACGTACGTACGTACG\n", np.uint8), 2 * n1)          # 32 n1 bytes, no tract: bound + 16 n1
    dblank = torch.from_numpy(blank.copy()).cuda()
    torch.cuda.synchronize()
    for mode in ("default", "main"):
        set_mode(monkeypatch, mode)
        c = tj.Counter(k)
        c.upload_raw(raw)
        c.scan_device(dblank.data_ptr(), blank.size, F.M)
        c.finalise_begin(*f)
        got = outcome(c, c.finalise_end())
        compare(got, exp, "%s %s" % (which, mode))
        assert order_path(c) == MODES[mode], (which, mode, order_path(c))
        assert c.plan_mismatches() == 0
        c.close()


# ---- one counter alone, and the side stream's life ------------------------------------------------------------------------------

def test_begin_and_end_ten_times_with_counters_coming_and_going(monkeypatch):
    """begin, then end with nothing queued between, ten times on one counter; other counters are made, used and destroyed in
    between (the side stream is shared and outlives them), and half way every counter is destroyed, which releases the stream:
    the next counter makes it anew"""
    set_mode(monkeypatch, "default")
    samples = loop_samples()
    c = tj.Counter(10)
    for it in range(10):
        i = it % 4
        if it == 5:
            c.close()
            c = tj.Counter(10)
        guest = tj.Counter(10) if it % 3 == 1 else None
        c.reset()
        c.scan_host(samples[i], M_LOOP)
        c.finalise_begin(*F_LOOP)
        if guest is not None:
            guest.scan_host(samples[(i + 1) % 4], M_LOOP)
            guest.finalise_begin(*F_LOOP)
        st = c.finalise_end()
        compare(outcome(c, st), loop_reference(10, i), "turn %d" % it)
        assert st == 0 and order_path(c) == ASIDE and c.plan_mismatches() == 0, (it, st, order_path(c))
        if guest is not None:
            compare(outcome(guest, guest.finalise_end()), loop_reference(10, (i + 1) % 4), "guest of turn %d" % it)
            assert order_path(guest) == ASIDE
            guest.close()
    c.close()
