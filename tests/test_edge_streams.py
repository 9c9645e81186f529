"""The edge corpus (tests/edge_streams.py) is what it claims to be -- checked on the CPU, from the streams themselves, the
kernel source and the oracle.  tests/test_scan_variants.py judges the kernels on these streams; if a stream missed its
edge, those tests would prove nothing."""
import os
import re

import numpy as np
import pytest

from oracle import orc
from tests import edge_streams as E
from tests.pyref import scan_closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = E.NL


def _source():
    with open(os.path.join(ROOT, "tatajuba_amd", "csrc", "hopo_device.hip")) as fh:
        return fh.read()


def _define(src, name):
    m = re.findall(r"^\s*#define\s+%s\s+(.+?)\s*(?://.*)?$" % re.escape(name), src, re.M)
    assert len(m) == 1, (name, m)
    return m[0].strip()


def _value(text):
    text = text.strip()
    if text.startswith("(") and text.endswith(")"):
        text = text[1:-1]
    m = re.fullmatch(r"(\d+)u?\s*<<\s*(\d+)", text)
    if m:
        return int(m.group(1)) << int(m.group(2))
    return int(text.rstrip("u"))


def test_constants_are_those_of_the_kernel_source():
    src = _source()
    for name in ("FK_BLOCK", "FK_UNIT", "FK_HL", "FK_HR", "FK_MAXCAND", "TJ_HR", "TJ_SB_TILE", "TJ_LOGB_SHIFT", "TJ_CH0", "TJ_FIX_CAP"):
        assert _value(_define(src, name)) == getattr(E, name), name
    assert _define(src, "FK_WIN") == "(FK_BLOCK * FK_UNIT)" and _define(src, "FK_OWN") == "(FK_WIN - FK_HL - FK_HR)"
    assert E.FK_OWN == 16288 and _value(_define(src, "TJ_LIST_FOWN")) == E.FK_OWN
    # the located scan's tile: the template arguments of its kernel and the host's tile count
    assert "scan_tiles<256, %d, 1> (seq, n_bytes, n_tiles" % E.LOC_TILE in src
    assert "const long n_tiles = (long) ((n_bytes + %d) / %d);" % (E.LOC_TILE - 1, E.LOC_TILE) in src
    # a chunk is TJ_CH0 << shift with shift >= 3, a log block 2^TJ_LOGB_SHIFT words, the ring four slots
    assert re.search(r"int sft = 3;", src) and "static_assert ((TJ_CH0 << 3) > (int) TJ_LOGB" in src
    assert "alignas (16) u64 blk[4];" in src
    assert E.log_block_records(12) == 8192 and E.log_block_records(13) == 4096
    assert [E.record_width(k) for k in (2, 12, 13, 28, 29, 32)] == [1, 1, 2, 2, 4, 4]


SEAM_CASES = [(tile, k, m) for tile in E.SEAM_TILES for (k, m) in [(2, 1), (12, 3), (13, 5), (16, 8), (17, 2), (28, 32), (32, 3)]]


@pytest.mark.parametrize("tile,k,m", SEAM_CASES)
def test_seam_streams_hold_every_combination_where_it_was_meant(tile, k, m):
    for kind in E.SEAM_KINDS:
        s = E.seam_stream(tile, k, m, kind)
        plan, n_tiles = E.seam_plan(tile, k, m, kind)
        assert s.size == n_tiles * tile and s[-1] == NL
        assert 0.5e6 < s.size < 3.2e6
        want = {(d, n) for n in E.seam_lengths(m) for d in E.seam_offsets(tile, k, n)}
        assert {(d, n) for (_, d, n, _, _) in plan} == want and len(plan) == len(want)
        mp = E.mprime(m)
        assert {mp - 1, mp, mp + 1, 31, 32, 33, 63, 64, 65, 96, 97, 1023, 1024, 1025, 16288 + 5} - {0} == set(E.seam_lengths(m))
        hr = {16288: 64, 8192: 192, 4096: 192}[tile]
        seams = set()
        seen_extra = set()
        for (t, d, n, byte, extra) in plan:
            assert t not in seams
            seams.add(t)
            p = t * tile + d
            e = p + n - 1
            tract = s[p:e + 1]
            assert (tract == tract[0]).all() and s[p - 1] != tract[0] and s[e + 1] != tract[0], (t, d, n)
            assert s[p - 1] != NL or extra == "p-1"
            around = np.nonzero(s[p - k - 2:e + k + 3] == NL)[0] + (p - k - 2)
            if kind == "plain":
                assert around.size == 0 and tract[0] == byte and tract[0] in b"ACGT"
            elif kind == "delim":
                assert around.tolist() == [E.delim_pos(extra, p, e, k)], (t, d, n, extra)
                seen_extra.add((d if d in (-k - 1, -k, -1, 0, 1) else "edge", extra))
            else:
                b, where = extra
                assert around.size == 0
                if where == "tract":
                    assert tract[0] == b
                else:
                    q = p - 1 - k // 2 if where == "left" else e + 1 + k // 2
                    assert s[q] == b and (p - k <= q < p or e < q <= e + k) and tract[0] == byte
                seen_extra.add(extra)
        # the offsets that were asked for, in the kernel's terms
        for n in E.seam_lengths(m):
            ds = set(E.seam_offsets(tile, k, n))
            assert {-k - 1, -k, -1, 0, 1} <= ds
            assert -n in ds and -n - k in ds                               # the end / the right flank's end on the last own byte
            win = tile + (32 if tile == 16288 else 64) + hr                # window = left halo + own + right halo
            hl = win - tile - hr
            for target in (win - 1, win, win + 1):                         # e + k in window coordinates of the tile before the seam
                d = target - k - (n - 1) - hl - tile
                assert d in ds, (n, target)
        if kind == "delim":
            assert {x for (_, x) in seen_extra} == set(E.DELIM_OFFSETS)
            for d in (-k - 1, -k, -1, 0, 1):
                assert {x for (dd, x) in seen_extra if dd == d} == set(E.DELIM_OFFSETS)   # every fixed offset meets every delimiter place
        if kind == "nocall":
            assert seen_extra == {(b, w) for b in E.NOCALL_BYTES for w in ("tract", "left", "right")}


def test_generic_left_halo_is_what_the_seam_test_assumes():
    assert _value(_define(_source(), "TJ_HL")) == 64


def test_candidate_limit_stream_shows_every_count_in_the_range():
    s = E.candidate_limit_stream()
    assert E.CAND_RANGE == tuple(range(E.FK_MAXCAND - 12, E.FK_MAXCAND + 5))
    c = E.count_candidates(s, 2)
    n_tiles = len(E.CAND_RANGE) * 2
    assert len(c) == 2 * n_tiles + 1                                       # (then the reverse complement: a byte out of step)
    assert (abs(c[n_tiles:2 * n_tiles] - E.FK_MAXCAND) <= 30).all()
    assert sorted(set(c[:n_tiles].tolist())) == list(E.CAND_RANGE)
    assert c[:17].tolist() == list(E.CAND_RANGE)
    assert 0 < (c[:n_tiles] > E.FK_MAXCAND).sum() < n_tiles
    # the restatement itself, the slow way, on the first two tiles
    b = s[: 2 * E.FK_OWN + 8].tobytes()
    cnt = [0, 0]
    i = 0
    while i < 2 * E.FK_OWN:
        j = i
        while j + 1 < len(b) and b[j + 1] == b[i]:
            j += 1
        if j - i + 1 >= 2 and b[i] in b"ACGT":
            cnt[i // E.FK_OWN] += 1
        i = j + 1
    assert cnt == c[:2].tolist()
    o = orc.Oracle(15)
    o.scan_stream(s, 2)
    o.finalise(1, 3)
    assert o.c.status == 0 and o.c.n_elem > 3000                           # a finalise keeps most of it: the template repeats


@pytest.mark.parametrize("k", [2, 10, 12, 13, 16, 17, 28, 29, 32])
def test_log_ring_streams_have_exactly_the_record_counts(k):
    rb = {1: 8192, 2: 4096, 4: 4096}[E.record_width(k)]
    assert E.log_block_records(k) == rb and E.LOG_RING_J == (1, 2, 4, 5, 9)
    for j in E.LOG_RING_J:
        for delta in (-1, 0, 1):
            s = E.log_ring_stream(k, j, delta)
            o = orc.Oracle(k)
            o.scan_stream(s, 2)
            assert o.c.n_elem == j * rb + delta and o.c.n_undefined == 0, (k, j, delta)
            assert (s == NL).sum() == 1                                    # one read: one workgroup appends in stream order
    s = E.sparse_stream(k)
    o = orc.Oracle(k)
    o.scan_stream(s, 2)
    assert o.c.n_elem == 7 and s.size // E.FK_OWN == 60                    # fewer records than tiles, hence than workgroups
    o = orc.Oracle(k)
    o.scan_stream(E.delimiters_only_stream(), 2)
    assert o.c.n_elem == 0


@pytest.mark.parametrize("k", [2, 12, 13, 28, 32])
def test_one_bucket_streams_fill_more_than_three_chunks_with_one_key(k):
    for n_keys in (1, 2):
        s = E.one_bucket_stream(k, n_keys)
        for m in (1, 32):
            o = orc.Oracle(k)
            o.scan_stream(s, m)
            e = o.elems()
            assert len(e) == n_keys * (3 * E.MIN_CHUNK + 1200) and len(e) > n_keys * 3 * (E.TJ_CH0 << 3)
            keys, counts = np.unique(np.stack([e["ctx0"], e["ctx1"], e["meta"] & np.uint64(0xFFF)], 1), axis=0, return_counts=True)
            assert len(keys) == n_keys and (counts == 3 * E.MIN_CHUNK + 1200).all()
            o.finalise(1, 3)
            assert o.c.status == 0 and o.c.n_elem == n_keys                # both strands: the key survives remove_biased


def test_fix_list_streams_hold_exactly_the_three_counts_of_runs():
    for k, m in [(2, 1), (13, 2), (32, 2)]:
        for n in (E.TJ_FIX_CAP - 1, E.TJ_FIX_CAP, E.TJ_FIX_CAP + 1):
            tot = []
            for clean in (False, True):
                o = orc.Oracle(k)
                o.scan_stream(E.fix_list_stream(n, clean), m)
                tot.append(o.c.n_elem + o.c.n_undefined)
                if clean:
                    assert o.c.n_undefined == 0
            assert tot[0] - tot[1] == n, (k, n)                            # countable non-ACGTU runs, recorded plus undefined
    s = E.fix_list_stream(1000)
    assert (s == NL).sum() == 1 and s[-1] == NL                            # one read: both flanks of every run lie inside it
    body = s.tobytes()
    first, last = body.index(b"NN"), body.rindex(b"NN")
    assert first >= 32 and len(body) - 1 - (last + 2) >= 32
    assert 12.5e6 < E.fix_list_stream(E.TJ_FIX_CAP).size < 12.7e6


@pytest.mark.parametrize("k,m", [(12, 3), (17, 4), (32, 5)])
def test_second_reference_on_the_seam_streams(k, m):
    """the oracle == tests.pyref.scan_closed_form, record for record, on the seam streams cut into reads (one k per record width)"""
    for tile in E.SEAM_TILES:
        for kind in E.SEAM_KINDS:
            s = E.seam_stream(tile, k, m, kind)
            reads, _ = E.cut_reads(s)
            exp = []
            for r in reads:
                for (base, n, off, flag, c0, c1) in scan_closed_form(r.decode("latin-1"), k, m):
                    exp.append((c0, c1, base | ((n & 0x3ff) << 2) | (1 << 12) | (0xffe << 32) | (flag << 49), off))
            o = orc.Oracle(k)
            o.scan_stream(s, m)
            e = o.elems()
            got = list(zip(e["ctx0"].tolist(), e["ctx1"].tolist(), e["meta"].tolist(), e["read_offset"].tolist()))
            assert len(got) == len(exp) > 100 and got == exp, (tile, kind)


def test_random_stream_is_the_fuzz_tools_generator():
    import random
    calls = []

    def fake_synth(*a, **kw):
        calls.append((a, kw))
        return np.frombuffer(b"ACGT\n", np.uint8)

    kinds = set()
    rng = random.Random(12345)
    for _ in range(60):
        s, mode = E.random_stream(rng, fake_synth)
        assert s.dtype == np.uint8 and (s.size == 0 or s[-1] == NL)
        kinds.add(mode)
    assert kinds == {"synth", "synth_ragged", "alphabet", "lowcomplex"} and calls
    with open(os.path.join(ROOT, "tools", "fuzz_gpu.py")) as fh:
        tool = fh.read()
    assert "from tests.edge_streams import random_stream" in tool and "lowcomplex" not in tool     # (no second copy of the generator)
