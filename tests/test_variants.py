"""tjamd_tract_variants on the GPU against the string restatement of tests/test_variants_cabi.py: the hand cases field for
field, planted corpora at the segment widths on both sides of a wavefront (every planted difference called with the planted
REF and ALT, nothing else), lists, refusals, capacity and buffer bounds, the eight-sample pipeline of tests/test_locate.py
with its reference genome, and examples/sample_vcfs.c.  d_out and h_offsets always sit in guarded buffers (tests/guarded.py)
and every const input is held frozen."""
import ctypes as C
import os
import random
import subprocess
import time

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests.guarded import GuardedDevice, GuardedHost, frozen, payload_pattern
from tests.test_locate import (BAD_SPANS_LOCATED, _dev, _p, dev_locate, dev_located_tracts, random_genome, same_entries, stats_on)
from tests.test_locate_cabi import NOWHERE, restate_locate, restate_located_tracts, restate_reference_index
from tests.test_union_tracts import DNA, _oracle_sample, device_union, make_genome, reads_of, sample_of
from tests.test_union_tracts_cabi import hand_union, oracle_union_grouping, restate_union_tract_stats
from tests.test_variants_cabi import (HAND_GENOME, HAND_NEAR, HAND_NEXT, HAND_PLAIN, K, NS, apply_it, calls_of, expected_calls, hand_case, planted_union,
                                      ref_alt_of, restate_tract_variants, vcf_text)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAP = 3, 4
VAR, TR, LOC = tj.VARIANT_DTYPE, tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE


def _torch():
    return pytest.importorskip("torch")


class Tiling:
    """a permuted union with its tiling and tract locations, on the host and on the device"""

    def __init__(self, keys, mat, tracts, tract_loc):
        torch = _torch()
        self.keys, self.mat = np.ascontiguousarray(np.asarray(keys, np.uint64).reshape(-1, 3)), np.ascontiguousarray(mat, np.int32)
        self.tracts, self.tract_loc = np.ascontiguousarray(tracts), np.ascontiguousarray(tract_loc)
        self.kd, self.md = _dev(self.keys), torch.from_numpy(self.mat.copy()).cuda()
        self.td, self.ld = _dev(self.tracts), _dev(self.tract_loc)
        self.nu, self.ns, self.nt = len(self.keys), self.mat.shape[1], len(self.tracts)


def dev_variants(counter, ref, u, lst="all", capacity="fit", want=None, nt=None):
    """-> (n, records, offsets), or (negative code, message, the guarded output) when the call is refused.  lst: 'all' (NULL),
    or tract ids; capacity: 'fit' = the number of records the restatement finds (want), or a number"""
    torch = _torch()
    L = tj.lib()
    cap = len(want) if capacity == "fit" else int(capacity)
    out = GuardedDevice(cap * VAR.itemsize)
    off = GuardedHost((u.ns + 1) * 8)
    ld = None if isinstance(lst, str) else torch.tensor(list(lst) + [0], dtype=torch.int32).cuda()      # (never empty: a NULL list means every tract)
    n_list = 0 if ld is None else ld.numel() - 1
    torch.cuda.synchronize()
    with frozen(u.kd, u.md, u.td, u.ld, ld):
        n = L.tjamd_tract_variants(counter._h, ref._h, _p(u.kd), _p(u.md), u.nu, u.ns, _p(u.td), u.nt if nt is None else nt, _p(u.ld), _p(ld), n_list,
                                   out.c, cap, off.c)
        err = L.tjamd_last_error().decode() if n < 0 else ""
        torch.cuda.synchronize()
    out.check("d_out")
    off.check("h_offsets")
    if n < 0:
        assert off.untouched()
        return n, err, out
    assert n <= cap
    got = out.view(VAR, n)
    assert (out.view(np.uint8)[n * VAR.itemsize:] == payload_pattern(out.nbytes)[n * VAR.itemsize:]).all()      # nothing behind the records
    return n, got, off.view(np.int64).tolist()


def check_same(got, want, offsets, want_offsets):
    assert len(got) == len(want) and offsets == want_offsets
    for f in VAR.names:
        assert (got[f] == want[f]).all(), (f, np.flatnonzero(got[f] != want[f])[:5])
    assert got.tobytes() == want.tobytes()


# ---- the hand cases ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hand():
    c = tj.Counter(K)
    ref = tj.Reference(c, HAND_GENOME)
    same_entries(ref.download(), restate_reference_index(HAND_GENOME, K)[0])
    yield c, ref
    ref.close()
    c.close()


@pytest.mark.parametrize("which,calls", [("plain", HAND_PLAIN), ("next", HAND_NEXT), ("near", HAND_NEAR)])
def test_hand_cases(hand, which, calls):
    c, ref = hand
    keys, mat, tracts, loc, entries = hand_case(which)
    u = Tiling(keys, mat, tracts, loc)
    want, want_off, text = restate_tract_variants(keys, mat, tracts, loc, entries, K)
    n, got, off = dev_variants(c, ref, u, want=want)
    assert n == len(calls) and c.last_tract_variants_ms() > 0
    check_same(got, want, off, want_off)
    assert calls_of(got, text) == calls


def test_lists_refusals_and_capacity(hand):
    c, ref = hand
    keys, mat, tracts, loc, entries = hand_case("plain")
    u = Tiling(keys, mat, tracts, loc)
    full, full_off, _ = restate_tract_variants(keys, mat, tracts, loc, entries, K)
    n, got, off = dev_variants(c, ref, u, want=full)
    # NULL against the explicit full list; two runs give the same bytes
    n2, got2, off2 = dev_variants(c, ref, u, lst=range(u.nt), want=full)
    assert n2 == n and got2.tobytes() == got.tobytes() == full.tobytes() and off2 == off == full_off
    # a list in descending order, a tract twice: the records follow the list
    for lst in ([3, 2, 1, 0], [1, 3, 1], [2]):
        want, want_off, _ = restate_tract_variants(keys, mat, tracts, loc, entries, K, lst=lst)
        n, got, off = dev_variants(c, ref, u, lst=lst, want=want)
        check_same(got, want, off, want_off)
    assert [int(x) for x in got["tract"]] == [2, 2, 2]
    # an empty list, and a list with no call in it (the unlocated tract), at capacity 0: nothing is written
    for lst in ([], [0]):
        n, got, off = dev_variants(c, ref, u, lst=lst, capacity=0)
        assert n == 0 and off == [0] * (NS + 1)
    # one short: refused, nothing behind the capacity, the offsets left alone
    rc, err, out = dev_variants(c, ref, u, capacity=len(full) - 1)
    assert rc == -ERR_CAP and err.startswith("tjamd_tract_variants") and f"{len(full)} records, caller capacity {len(full) - 1}" in err
    assert c.last_tract_variants_ms() == -1.0
    assert out.view(VAR).tobytes() == full[: len(full) - 1].tobytes()          # (what fits is in its place)
    # a list id out of range
    for lst in ([0, 4], [-1], [1, 2, 1 << 20]):
        rc, err, _ = dev_variants(c, ref, u, lst=lst, capacity=64)
        assert rc == -ERR_ARG and "a listed tract id is outside [0, 4)" in err, (lst, rc, err)
    # a reference of another k
    other = tj.Counter(K + 1)
    rc, err, _ = dev_variants(other, ref, u, capacity=64)
    assert rc == -ERR_ARG and f"built with k = {K}, the counter has k = {K + 1}" in err
    other.close()
    # tracts that do not tile the union (five rows, as the spans are written), listed or not
    k5, m5, _ = hand_union()
    for spans in BAD_SPANS_LOCATED:
        bad = np.zeros(len(spans), TR)
        bad["first"], bad["n_rows"] = [s[0] for s in spans], [s[1] for s in spans]
        b = Tiling(k5, m5, bad, np.array([NOWHERE] * len(spans), LOC))
        for lst in ("all", [0]):
            rc, err, _ = dev_variants(c, ref, b, lst=lst, capacity=16)
            assert rc == -ERR_ARG and "do not tile the union" in err, (spans, lst, rc, err)
    # n_samples is checked before anything else
    rc = tj.lib().tjamd_tract_variants(c._h, ref._h, _p(u.kd), _p(u.md), u.nu, 4097, _p(u.td), u.nt, _p(u.ld), None, 0, None, 0, (C.c_long * 2)())
    assert rc == -ERR_ARG and "n_samples 4097 outside 1..4096" in tj.lib().tjamd_last_error().decode()


# ---- planted corpora ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [1, 3, 8, 64, 65, 130])
@pytest.mark.parametrize("k", [2, 5, 15, 31, 32])
def test_planted_corpus(k, ns):
    """no reads and no noise: every planted (site, sample) with La != Lr comes back with the planted REF and ALT and nothing
    else does -- the share of planted cases that may be missing is zero"""
    rng = random.Random(1000 * k + ns)
    g = random_genome(rng, {2: 400, 5: 1500}.get(k, 3000), k)
    p = planted_union(g, k, ns, rng, max_sites=max(24, 2400 // ns))
    assert len(p["sites"]) >= 8 and p["tracts"]["n_rows"].max() > 64 and (p["tracts"]["n_rows"] == 1).any()
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    same_entries(ref.download(), p["entries"])
    n_loc, loc = dev_locate(c, ref, p["keys"], 1)
    assert n_loc == len(p["keys"])                                            # tjamd_locate's rule places every planted row
    nt, lt = dev_located_tracts(c, p["keys"], p["mat"], p["tracts"], loc)
    assert nt == len(p["sites"]) and (lt["tract_loc"]["flat"] >= 0).all()
    u = Tiling(lt["keys"], lt["mat"], lt["tracts"], lt["tract_loc"])
    want, want_off, text = restate_tract_variants(u.keys, u.mat, u.tracts, u.tract_loc, p["entries"], k)
    n, got, off = dev_variants(c, ref, u, want=want)
    check_same(got, want, off, want_off)
    planted = expected_calls(g, k, p)
    called = {(int(r["sample"]), int(r["flat"])): (int(r["contig"]), int(r["pos"])) + ref_alt_of(r) for r in got}
    assert len(called) == len(got) and called == planted and len(planted) > 0
    apply_it(g, k, got, text)
    if ns >= 3 and k >= 5:
        assert (got["n_flank"] > 0).any() and any(t["k_eff"] < k for t in text) and (got["base"] >= 2).any() and (got["base"] < 2).any()
    # the variable tracts as the list, as a caller has them
    var = stats_on(c, {"d_keys": u.kd, "d_mat": u.md, "d_tracts": u.td, "d_ref_length": _dev(lt["ref_length"].astype(np.int32), np.int32)}, nt, ns,
                   [50] * ns)["variable"]
    want, want_off, _ = restate_tract_variants(u.keys, u.mat, u.tracts, u.tract_loc, p["entries"], k, lst=var)
    n, got, off = dev_variants(c, ref, u, lst=var.tolist(), want=want)
    check_same(got, want, off, want_off)
    ref.close()
    c.close()


# ---- the pipeline ------------------------------------------------------------------------------------------------------

def test_eight_sample_pipeline_variants(monkeypatch):
    """the eight samples, the genome and the calls of tests/test_locate.py::test_eight_sample_pipeline_with_a_reference, then
    the variants of its variable tracts.  Measured on one MI355X: 1 143 variable tracts of 4 233, 749
    records (731 insertions, 18 deletions, 370 on the negative strand), 687 of 687 planted length variants called;
    tjamd_last_tract_variants_ms 0.049 ms (0.030 ms the second time); between two events on one stream 0.066 ms, beside 0.042 ms
    for tjamd_union_tract_sample_stats on the same union and list."""
    torch = _torch()
    monkeypatch.delenv("TATAJUBA_AMD_EDIT_DISTANCE", raising=False)
    k, m, ns, maxd, lev, mm = 15, 4, 8, 1, 2, 1
    rng = random.Random(2024)
    pieces = make_genome(rng, n_tracts=2000)
    genome = "".join(left + DNA[b] * length + right for left, b, length, right in pieces)
    counters, ocov = [], []
    for smp in range(ns):
        s = reads_of(sample_of(pieces, rng, smp), rng)
        c = tj.Counter(k)
        c.scan_host(s, m)
        assert c.finalise(1, 5) == 0
        counters.append(c); ocov.append(c.coverage)
    L = tj.lib()
    hs = (C.c_void_p * ns)(*[c._h for c in counters])
    drec, counts = C.c_void_p(), (C.c_long * ns)()
    merger = tj.Counter(k)
    total = L.tjamd_gather_histograms(merger._h, hs, ns, C.byref(drec), counts)
    keys = torch.empty(total * 24, dtype=torch.uint8, device="cuda")
    mat = torch.empty((total, ns), dtype=torch.int32, device="cuda")
    nu = L.tjamd_merge_samples(merger._h, drec, counts, ns, C.c_void_p(keys.data_ptr()), C.c_void_p(mat.data_ptr()), total)
    keys, mat = keys[: nu * 24], mat[:nu]
    nt0, grouped = device_union(merger, keys, mat, ocov, maxd, lev, on_device=True)
    stream = (genome + "\n").encode()
    ref = tj.Reference(merger, stream)
    entries = ref.download()
    n_located, loc = dev_locate(merger, ref, keys, mm, on_device=True)
    nt, lt = dev_located_tracts(merger, keys, mat, grouped["tracts"], loc, on_device=True)
    stats = stats_on(merger, lt, nt, ns, ocov)
    var = stats["variable"]
    u = Tiling(lt["keys"], lt["mat"], lt["tracts"], lt["tract_loc"])
    want, want_off, text = restate_tract_variants(u.keys, u.mat, u.tracts, u.tract_loc, entries, k, lst=var)
    n, got, off = dev_variants(merger, ref, u, lst=var.tolist(), want=want)
    ms_variants = merger.last_tract_variants_ms()
    check_same(got, want, off, want_off)
    apply_it(stream, k, got, text)
    ins, dele = int((got["alt_length"] > got["ref_length"]).sum()), int((got["alt_length"] < got["ref_length"]).sum())
    neg = int((got["base"] >= 2).sum())
    assert ins > 0 and dele > 0 and neg > 0, (ins, dele, neg)
    n2, again, off2 = dev_variants(merger, ref, u, lst=var.tolist(), want=want)
    assert n2 == n and again.tobytes() == got.tobytes() and off2 == off
    # the share of sample_of's planted length variants (every eighth piece, one base longer in the samples that carry it) that
    # come back as calls: printed, not asserted -- it depends on the read depth and on what tjamd_locate places
    starts, at = {}, 0
    for i, (left, b, length, right) in enumerate(pieces):
        starts[at + len(left)] = (i, length)
        at += len(left) + length + len(right)
    planted = {(smp, f) for f, (i, length) in starts.items() if i % 8 == 4 for smp in range(ns) if (smp + (i // 8) % 4) % 3 == 0}
    called = {(int(r["sample"]), int(r["flat"])) for r in got if int(r["alt_length"]) == int(r["ref_length"]) + 1}
    print(f"\n[variants] {len(var)} variable tracts of {nt}, {n} records ({ins} insertions, {dele} deletions, {neg} on the negative strand); "
          f"{len(planted & called)} of {len(planted)} planted length variants called ({100.0 * len(planted & called) / len(planted):.1f} %)")
    # the yardstick: tjamd_union_tract_sample_stats on the same permuted union and list, both calls between two events of one stream
    lst = torch.from_numpy(var.astype(np.int32)).cuda()
    cov = (C.c_int * ns)(*[int(x) for x in ocov])
    summ = _dev(stats["summary"])
    vals = torch.zeros((len(var), 5, ns), dtype=torch.float64, device="cuda")
    out = torch.zeros(max(len(want), 1) * VAR.itemsize, dtype=torch.uint8, device="cuda")
    offs = (C.c_long * (ns + 1))()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()                                                  # (the buffers above were filled on the default stream)
    merger.set_stream(side.cuda_stream)
    ms = {}
    with torch.cuda.stream(side):
        for name in ("sample_stats", "variants", "sample_stats", "variants"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(side)
            if name == "variants":
                rc = L.tjamd_tract_variants(merger._h, ref._h, _p(u.kd), _p(u.md), u.nu, ns, _p(u.td), u.nt, _p(u.ld), _p(lst), len(var), _p(out), len(want), offs)
            else:
                rc = L.tjamd_union_tract_sample_stats(merger._h, _p(u.kd), _p(u.md), u.nu, ns, cov, _p(summ), nt, _p(lst), len(var), _p(vals), None, None, None)
            e1.record(side)
            e1.synchronize()
            assert rc >= 0, L.tjamd_last_error()
            ms[name] = (e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0))
    print(f"[variants] union {nu} rows x {ns} samples, k = {k}, list of {len(var)}: tjamd_last_tract_variants_ms {ms_variants:.3f} ms "
          f"(second call {merger.last_tract_variants_ms():.3f} ms); between events on one stream, wait included: tjamd_tract_variants "
          f"{ms['variants'][0]:.3f} ms (host {ms['variants'][1]:.3f} ms), tjamd_union_tract_sample_stats {ms['sample_stats'][0]:.3f} ms (host {ms['sample_stats'][1]:.3f} ms)")
    assert ms_variants > 0
    merger.set_stream(0)
    ref.close()
    for c in counters + [merger]:
        c.close()


# ---- the example -------------------------------------------------------------------------------------------------------

def test_sample_vcfs_c_example(tmp_path):
    exe, libdir = str(tmp_path / "sample_vcfs"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sample_vcfs.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", exe])
    k, m, mm = 10, 3, 1
    rng = random.Random(7)
    pieces = make_genome(rng, n_tracts=200)
    contigs = ["".join(left + DNA[b] * length + right for left, b, length, right in part) for part in (pieces[:120], pieces[120:])]
    names = ["contig0", "chr|2"]
    fasta = str(tmp_path / "ref.fa")
    with open(fasta, "w") as fh:
        fh.write("".join(">%s some text\n%s\n" % (names[i], "\n".join(s[j: j + 70] for j in range(0, len(s), 70))) for i, s in enumerate(contigs)))
    files, recs, covs = [], [], []
    for smp, fname in enumerate(("s0.fq", "s 1'.fq")):
        s = reads_of(sample_of(pieces, rng, smp), rng)
        reads = bytes(s).split(b"\n")[:-1]
        f = str(tmp_path / fname)
        with open(f, "wb") as fh:
            fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rd, b"I" * len(rd)) for i, rd in enumerate(reads)))
        files.append(f)
        rec, cov = _oracle_sample(s, k, m)
        recs.append(rec); covs.append(cov)
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, "-r", fasta, "-x", str(mm), "-k", str(k), "-m", str(m), "-c", "5", "-d", "1", "-l", "-1", "-o", str(out)] + files,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # the same pipeline from the oracle and the restatements, as tests/test_locate.py does for located_tracts.c
    _, _, keys_o, mat_o = orc.merge_samples(np.frombuffer(np.concatenate(recs).tobytes(), np.uint64).reshape(-1, 3), [len(x) for x in recs])
    g = oracle_union_grouping(keys_o, mat_o, k, 1, 2)
    first = np.asarray(g["groups"]["first"], np.int64)
    tracts = np.zeros(len(first), TR)
    tracts["first"], tracts["n_rows"] = first, np.diff(np.r_[first, len(keys_o)])
    tracts["n_context"], tracts["indel"] = g["groups"]["n_context"], g["groups"]["indel"]
    tracts["mode"], tracts["lev_distance"], tracts["integral"] = g["mode"], g["lev_distance"], g["integral"]
    entries, n_contigs = restate_reference_index(("\n".join(contigs) + "\n").encode(), k)
    loc = restate_locate(entries, keys_o, mm)
    lt = restate_located_tracts(keys_o, mat_o, tracts, loc)
    perm = lt["perm"]
    ids = np.repeat(np.arange(len(lt["tracts"])), lt["tracts"]["n_rows"])
    st = restate_union_tract_stats(keys_o[perm], mat_o[perm], covs, ids, lt["tracts"]["lev_distance"], ref_length=lt["ref_length"])
    var = np.flatnonzero(st["variable"])
    want, off, _ = restate_tract_variants(keys_o[perm], mat_o[perm], lt["tracts"], lt["tract_loc"], entries, k, lst=var)
    assert len(want) > 0 and (want["contig"] == 1).any() and off[1] > 0 and off[2] > off[1]
    for smp, sample in enumerate(("s0.fq", "s_1_.fq")):
        text = (out / (sample + ".vcf")).read_text()
        assert text == vcf_text(names, [len(s) for s in contigs], sample, want[off[smp]: off[smp + 1]]), sample
    assert f"{len(var)} variable; {len(want)} variants in 2 samples" in r.stdout
