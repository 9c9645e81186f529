"""FASTQ text parsed on the device (tjamd_fastq_*) against the rule restated in tests/test_fastq_device_cabi.py, which that file
pins against the host reader: consumed bytes, records, stop code and stream byte for byte, whatever way the text is cut into
pushes; and, where the session scans, the counter against tjamd_scan_host on the host reader's stream and against the oracle.
Byte and integer work: nothing is allowed to differ.  Shapes are aimed at T = tjamd_fastq_tile_bytes() (a workgroup's bytes)
and at the 1024 bytes of a wavefront."""
import ctypes as C
import functools
import gzip
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests import edge_streams as E
from tests.guarded import GuardedDevice
from tests.test_fastq_device_cabi import ERR_ARG, regular_record, restate_fastq_parse
from tests.test_gpu_parity import as_records, rec_sorted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = tj.lib().tjamd_fastq_tile_bytes()
WAVE = 1024


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(10)
    yield c
    c.close()


def record(i, n, head=None, qual="I"):
    head = ("r%d" % i) if head is None else head
    seq = "".join("ACGT"[(i + j * j) & 3] for j in range(n))
    return ("@%s\n%s\n+\n%s\n" % (head, seq, qual * n)).encode()


def check(c, text, cuts=(), what=""):
    """one parse-only session over text, cut at `cuts`: everything the restatement says"""
    want = restate_fastq_parse(text)
    got = c.fastq_parse(text, cuts)
    assert got[:3] == want[:3], (what, cuts, got[:3], want[:3])
    assert got[3] == want[3], (what, cuts, "the streams differ")
    return want


# ---- cuts --------------------------------------------------------------------------------------------------------------------

def test_two_pushes_cut_at_every_byte_and_one_byte_at_a_time(counter):
    text = record(0, 21) + record(1, 7, head="") + record(2, 12, qual="@")
    assert 90 <= len(text) <= 110
    want = restate_fastq_parse(text)
    assert want[:3] == (len(text), 3, 0)
    for cut in range(len(text) + 1):
        check(counter, text, (cut,), "cut")
    check(counter, text, tuple(range(1, len(text))), "byte by byte")
    # ... and without the last '\n', and with a last record that stays open
    check(counter, text[:-1], tuple(range(1, len(text) - 1)), "no last newline")
    for cut in (0, 5, len(text) - 9):
        w = check(counter, text[:-8], (cut,), "open record")
        assert w[1:3] == (2, 1)
    assert counter.last_fastq_ms() > 0


# ---- tile edges --------------------------------------------------------------------------------------------------------------

def test_a_line_end_on_every_side_of_a_tile_and_of_a_wavefront(counter):
    body = b"".join(record(i, 30) for i in range(1, 140))              # about 2.3 tiles of records of 70 bytes
    seen_tile, seen_wave = set(), set()
    for pad in range(0, 80):
        text = record(0, 30, head="h" * pad) + body
        nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
        seen_tile |= set((nl % T).tolist()) & {T - 1, 0}
        seen_wave |= set((nl % WAVE).tolist()) & {WAVE - 1, 0}
        check(counter, text, (), "pad %d" % pad)
    assert seen_tile == {T - 1, 0} and seen_wave == {WAVE - 1, 0}


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 3 * T + 5])
def test_a_sequence_line_as_long_as_a_tile_and_one_over_four_tiles(counter, n):
    text = record(0, 40) + record(1, n) + record(2, 150) + record(3, n, qual="@") + record(4, 1)
    w = check(counter, text, (), n)
    assert w[:3] == (len(text), 5, 0) and len(w[3]) == 2 * n + 40 + 150 + 1 + 5
    check(counter, text, (T, 2 * T + 1, len(text) - 3), n)


def test_4096_records_of_length_one(counter):
    text = b"".join(record(i, 1, head="") for i in range(4096))
    assert len(text) == 8 * 4096                                         # the shortest regular record: the bounds of the parse are tight
    w = check(counter, text)
    assert w[:3] == (len(text), 4096, 0)
    check(counter, text, (T - 3, T, 5 * T + 1))


def test_a_push_of_exactly_a_tile_and_of_one_byte_more(counter):
    for size in (T, T + 1):
        body = b"".join(record(i, 50) for i in range(1, 37))
        pad = size - len(body) - len(record(0, 50, head=""))
        text = record(0, 50, head="p" * pad) + body
        assert len(text) == size and text.endswith(b"\n")
        w = check(counter, text)
        assert w[:3] == (size, 37, 0)
        more = text + record(99, 33)
        check(counter, more, (size,))                                    # ... as the first of two pushes
        check(counter, more, (len(more) - size,))                        # ... and as the second


# ---- irregular records ---------------------------------------------------------------------------------------------------------

IRREGULAR = {
    "fasta": b">c1 x\nACGTACGT\n",
    "multiline": b"@m\nACGT\nACGT\n+\nIIII\nIIII\n",
    "crlf": b"@w\r\nACGT\r\n+\r\nIIII\r\n",
    "cr-in-quality": b"@w\nACGT\n+\nII\rI\n",
    "blank": b"\n",
    "short-quality": b"@s\nACGTA\n+\nIIII\n",
    "long-quality": b"@s\nACGTA\n+\nIIIIII\n",
    "no-plus": b"@s\nACGTA\n-\nIIIII\n",
    "sequence-starts-with-@": b"@s\n@CGTA\n+\nIIIII\n",
    "empty-sequence": b"@s\n\n+\n\n",
    "no-header": b"s\nACGTA\n+\nIIIII\n",
}


@pytest.mark.parametrize("kind", sorted(IRREGULAR))
def test_an_irregular_record_first_in_the_middle_and_last(counter, kind):
    regular = [record(i, 20 + (i * 7) % 90) for i in range(50)]
    clean = b"".join(regular)
    for at in (0, 25, 49):
        text = b"".join(regular[:at]) + IRREGULAR[kind] + b"".join(regular[at + 1:])
        w = check(counter, text, (), (kind, at))
        offset = len(b"".join(regular[:at]))
        assert w[:3] == (offset, at, 1) and w[3] == restate_fastq_parse(clean)[3][:len(w[3])], (kind, at)
        check(counter, text, (offset,), (kind, at))                        # the push boundary in front of it
        check(counter, text, (offset + 1, offset + 3), (kind, at))
        assert check(counter, clean)[:3] == (len(clean), 50, 0)               # a second session on the same counter is clean


def test_a_record_cut_short_by_the_end_of_the_text(counter):
    regular = [record(i, 30) for i in range(50)]
    text = b"".join(regular)
    for short in (1, 2, 31, 33, 34, 64):                                   # inside the quality line, the '+' line, the sequence, the header
        cut = text[:-short]
        w = check(counter, cut, (), short)
        assert w[:3] == ((len(text) - 1, 50, 0) if short == 1 else (len(b"".join(regular[:49])), 49, 1)), short
        check(counter, cut, (len(cut) // 2,), short)


def test_quality_lines_that_begin_like_a_header(counter):
    text = b"".join(record(i, 1 + i % 40, head="@%d" % i, qual="@") for i in range(300))
    assert b"\n@@@" in text and b"\n@@1" in text
    w = check(counter, text)
    assert w[:3] == (len(text), 300, 0)
    check(counter, text, (T, T + 1))


# ---- the carry, in child processes that shorten it ----------------------------------------------------------------------------

CARRY_CHILD = r"""
import json, sys
import tatajuba_amd as tj
from tests.test_fastq_device_cabi import restate_fastq_parse
from tests.test_fastq_device import record
c = tj.Counter(10)
front = record(0, 10) + record(1, 20)
out = {}
for name, total in (("outgrows", 300), ("fits", 200)):
    n = (total - 9) // 2                                    # "@big\n" + n + "\n+\n" + n + "\n"
    rec = record(7, n, head="big" + "x" * (total - 9 - 2 * n))
    assert len(rec) == total
    text = front + rec + record(8, 5)
    cut = len(front) + rec.index(b"\n") + 1                  # after its header
    got = c.fastq_parse(text, (cut,))
    whole = c.fastq_parse(text)                              # not cut by a push boundary: no carry is asked for
    out[name] = {"got": [got[0], got[1], got[2], got[3].decode()], "whole": [whole[0], whole[1], whole[2]], "front": len(front), "text": len(text),
                 "want": list(restate_fastq_parse(text)[:3]), "want_stream": restate_fastq_parse(text)[3].decode(), "front_stream": restate_fastq_parse(front)[3].decode()}
    # cut one byte at a time, the record reaches the carry's limit before it ends
    got = c.fastq_parse(text, tuple(range(1, len(text))))
    out[name]["bytewise"] = [got[0], got[1], got[2]]
print(json.dumps(out))
"""


def run_child(code, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_a_record_that_outgrows_a_carry_of_256_bytes_and_one_that_fits():
    out = run_child(CARRY_CHILD, {"TATAJUBA_AMD_FASTQ_CARRY": "256"})
    big, fits = out["outgrows"], out["fits"]
    assert big["got"] == [big["front"], 2, 2, big["front_stream"]]            # stop 2, at its start
    assert big["bytewise"] == [big["front"], 2, 2]
    assert big["whole"] == big["want"] == [big["text"], 4, 0]
    assert fits["got"] == fits["want"] + [fits["want_stream"]] and fits["want"] == [fits["text"], 4, 0]
    assert fits["bytewise"] == fits["want"] and fits["whole"] == fits["want"]


# ---- scan sessions -------------------------------------------------------------------------------------------------------------

def dress(stream):
    """a stream of reads as FASTQ text (empty reads have no regular record and are left out)"""
    reads = [r for r in bytes(stream).split(b"\n") if r]
    return b"".join(b"@s%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))


@functools.lru_cache(maxsize=None)
def scan_case(k, m):
    """the text of the scan sessions: seam, no-call and sparse streams of tests/edge_streams.py, built for this k and minimum tract size, dressed as FASTQ"""
    parts = [E.seam_stream(E.LOC_TILE, k, m, kind, seed=3) for kind in ("plain", "nocall")] + [E.sparse_stream(k, 7, 6)]
    text = dress(np.concatenate(parts).tobytes())
    return text


def finalised(c):
    st = c.finalise(0, 0)                                                  # (the corpus has its tracts on one strand: nothing is filtered)
    if st != 0:
        return (st,)
    gi, gf = c.download_idx()
    return (st, c.download_kept().tobytes(), gi.tobytes(), gf.tobytes(), c.coverage, c.n_kept, c.n_idx)


@pytest.mark.parametrize("k,m", [(10, 3), (15, 3), (25, 3)])
def test_scan_sessions_equal_scan_host_on_the_readers_stream_and_the_oracle(tmp_path, k, m):
    text = scan_case(k, m)
    path = tmp_path / "s.fq"
    path.write_bytes(text)
    stream, n_reads = tj.read_file_stream(str(path))
    want_parse = restate_fastq_parse(text)
    assert want_parse[:3] == (len(text), n_reads, 0) and want_parse[3] == stream.tobytes()
    # the sample is the text twice: a finalise drops what it has seen once, and keeps every tract of this corpus
    o = orc.Oracle(k)
    o.scan_stream(stream, m)
    o.scan_stream(stream, m)
    o_raw, o_undef = rec_sorted(as_records(o.elems())), int(o.c.n_undefined)
    o.finalise(0, 0)
    assert o.c.status == 0 and o.c.n_elem > 10000
    ei, ef = o.idx()
    o_fin = (0, o.elems().tobytes(), ei.tobytes(), ef.tobytes(), int(o.c.coverage), int(o.c.n_elem), int(o.c.n_idx))
    o.close()
    ref = tj.Counter(k)
    ref.scan_host(stream, m)
    ref.scan_host(stream, m)
    r_raw, r_undef = rec_sorted(ref.download_raw()), ref.undefined_runs()
    r_fin = finalised(ref)
    ref.close()
    assert r_fin == o_fin and r_undef == o_undef and (r_raw == o_raw).all()
    c = tj.Counter(k)
    for pieces in ((len(text), len(text)), (1024, len(text))):                # two sessions in one push each; the first in pushes of 1 KiB
        c.reset()
        for piece in pieces:
            c.fastq_begin(m)
            for at in range(0, len(text), piece):
                c.fastq_push_host(text[at: at + piece], final=(at + piece >= len(text)))
            consumed, reads, stop, n_stream = c.fastq_end()
            assert (consumed, reads, stop, n_stream) == (len(text), n_reads, 0, len(stream)), pieces
            assert tj.lib().tjamd_fastq_stream(c._h) is None                  # a session that scans keeps no stream
        raw = rec_sorted(c.download_raw())
        assert len(raw) == len(o_raw) and (raw == o_raw).all(), pieces
        assert c.undefined_runs() == o_undef, pieces                           # the delimiters that pad a push's stream count nothing
        assert finalised(c) == o_fin, pieces
    c.close()

def test_begin_takes_the_minimum_tract_sizes_of_scan_device():
    """tjamd_scan_device scans tracts of 1 ... 32 bases and more; 0 (all monomers) exists for located records only, and it
    refuses it: so does a session that would scan the same way.  A refused call leaves no time behind."""
    L = tj.lib()
    c = tj.Counter(10)
    one = record(0, 9)
    assert L.tjamd_last_fastq_ms(c._h) == -1.0                             # no session yet
    for m in (0, 33):
        assert L.tjamd_fastq_begin(c._h, m) == ERR_ARG == L.tjamd_scan_device(c._h, None, 0, m)
        assert L.tjamd_fastq_push_host(c._h, one, len(one), 1) == ERR_ARG   # no session was opened
        assert L.tjamd_last_fastq_ms(c._h) == -1.0
    assert check(c, one)[:3] == (len(one), 1, 0) and c.last_fastq_ms() > 0
    for refused in (lambda: L.tjamd_fastq_push_device(c._h, C.c_void_p(0x2001), 64, 0), lambda: L.tjamd_fastq_push_host(c._h, None, 5, 0),
                    lambda: L.tjamd_fastq_push_host(c._h, one, (1 << 30) + 1, 0), lambda: L.tjamd_fastq_begin(c._h, -2)):
        assert check(c, one)[:3] == (len(one), 1, 0) and c.last_fastq_ms() > 0
        assert refused() == ERR_ARG and L.tjamd_last_fastq_ms(c._h) == -1.0  # refused before the counter is read: the time is gone all the same
    c.fastq_begin(-1)
    c.fastq_push_host(one, final=True)
    assert L.tjamd_fastq_push_host(c._h, one, len(one), 0) == ERR_ARG        # behind the final push
    assert c.fastq_end()[:3] == (len(one), 1, 0)
    c.close()


def test_a_thousand_small_pushes_hold_on_to_no_more_than_the_text_asks_for():
    """3 MB in pushes of 1 KiB: the stream buffer is bounded by half the session's text, not by a share per push; the scratch
    of a push by what it can see (the carry's limit at most); the bound that sizes the record storage by the stream's"""
    L = tj.lib()
    L.tjamd_debug_fastq_footprint.restype = C.c_long
    L.tjamd_debug_fastq_footprint.argtypes = [C.c_void_p, C.c_int]
    text = scan_case(10, 3)
    want = restate_fastq_parse(text)
    assert 2 << 20 < len(text) < 8 << 20 and want[:3] == (len(text), text.count(b"\n") // 4, 0)
    cuts = tuple(range(1024, len(text), 1024))
    carry_limit = 1 << 20
    c = tj.Counter(10)
    assert c.fastq_parse(text, cuts) == want
    assert len(want[3]) <= L.tjamd_debug_fastq_footprint(c._h, 0) <= 3 * len(text) // 4 + 4096     # half the text, grown by halves
    assert L.tjamd_debug_fastq_footprint(c._h, 1) <= 5 * (carry_limit + 1024 + 4096)             # 3 bytes per byte in sight, grown by halves
    c.close()
    c = tj.Counter(10)
    c.fastq_begin(3)
    for at in range(0, len(text), 1024):
        c.fastq_push_host(text[at: at + 1024], final=(at + 1024 >= len(text)))
    assert c.fastq_end()[:3] == want[:3]
    assert L.tjamd_debug_fastq_footprint(c._h, 0) <= 3 * len(text) // 4 + 4096
    assert L.tjamd_debug_fastq_footprint(c._h, 1) <= 5 * (carry_limit + 1024 + 4096)
    # every hand-over to the scan adds a third of its bytes (m' = 3) to the bound; the bytes are half the text and 16 a hand-over
    assert 0 < L.tjamd_debug_fastq_footprint(c._h, 2) <= len(text) // 6 + 4096
    one = tj.Counter(10)
    one.scan_host(np.frombuffer(want[3], np.uint8), 3)
    assert (rec_sorted(c.download_raw()) == rec_sorted(one.download_raw())).all()
    one.close()
    c.close()


def test_the_golden_file_inflated(tmp_path, golden_dir):
    path = tmp_path / "err1750956.fastq"
    with gzip.open(os.path.join(golden_dir, "err1750956.fastq.gz"), "rb") as fh:
        path.write_bytes(fh.read())
    text = path.read_bytes()
    c = tj.Counter(10)
    c.fastq_begin(3)
    c.fastq_push_host(text, final=True)
    consumed, reads, stop, _ = c.fastq_end()
    assert (consumed, stop) == (len(text), 0) and reads == text.count(b"\n") // 4
    assert c.raw_count() == 22136
    assert c.finalise(1, 5) == 0 and (c.n_kept, c.n_idx, c.coverage) == (1035, 14, 8)
    c.close()


# ---- the drop-in, in child processes ---------------------------------------------------------------------------------------------

DROPIN_CHILD = r"""
import ctypes as C, hashlib, json, sys
import tatajuba_amd as tj
out = []
for path in sys.argv[1:]:
    h = tj.HopoCounter.new_or_append_from_file(None, path, tj.Options.defaults(10, 3, 2, True))
    n_raw = h.c.n_elem
    h.finalise()
    gi, gf = h.idx()
    out.append([n_raw, h.c.n_elem, h.c.n_idx, h.c.coverage, hashlib.sha256(h.elems().tobytes()).hexdigest(), hashlib.sha256(gi.tobytes() + gf.tobytes()).hexdigest()])
    h.delete()
L = tj.lib()
L.tjamd_debug_fastq_sessions.restype = C.c_long
print(json.dumps({"files": out, "sessions": L.tjamd_debug_fastq_sessions()}))
"""


def test_the_drop_in_under_device_equals_the_default(tmp_path):
    rng = random.Random(11)
    genome = "".join(rng.choice("ACGT") * rng.choice((1, 1, 1, 2, 4, 6)) for _ in range(3000))
    comp = str.maketrans("ACGT", "TGCA")
    both = lambda i, r: r if i % 2 == 0 else r.translate(comp)[::-1]        # every tract on both strands: a finalise keeps them
    reads = [both(i, genome[p: p + 100]) for i, p in enumerate(rng.randrange(len(genome) - 100) for _ in range(2000))]
    regular = [("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r))).encode() for i, r in enumerate(reads)]
    files = {"regular.fq": b"".join(regular),
             "irregular.fq": b"".join(regular[:1000]) + b"@w\r\n" + reads[5].encode() + b"\r\n+\r\n" + b"I" * 100 + b"\r\n" + b"".join(regular[1000:]),
             "contigs.fa": b"".join(b">c%d\n%s\n" % (i, both(i, genome[(i // 4) * 400: (i // 4) * 400 + 900]).encode()) for i in range(20))}
    paths = []
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    code = DROPIN_CHILD.replace("sys.argv[1:]", repr(paths))
    default = run_child(code, {"TATAJUBA_AMD_FASTQ_PARSE": "host", "TATAJUBA_AMD_FASTQ_PIECE": "4096"})
    device = run_child(code, {"TATAJUBA_AMD_FASTQ_PARSE": "device", "TATAJUBA_AMD_FASTQ_PIECE": "4096", "TATAJUBA_AMD_FEEDER_THREADS": "3"})
    assert default["sessions"] == 0 and device["sessions"] == 3                # which way each run went
    assert device["files"] == default["files"]
    for n_raw, n_kept, n_idx, cov, _, _ in default["files"]:
        assert n_raw > 0 and n_kept > 0 and n_idx > 0 and cov > 0


# ---- reuse, and the bytes a push may read ----------------------------------------------------------------------------------------

def test_sessions_around_a_reset_and_a_tree_entry_on_the_same_counter(counter):
    import torch
    text = b"".join(record(i, 1 + (i * 13) % 200) for i in range(400)) + IRREGULAR["fasta"] + record(1, 5)
    first = counter.fastq_parse(text, (T + 7,))
    assert first == restate_fastq_parse(text)
    counter.reset()
    assert counter.fastq_parse(text, (T + 7,)) == first
    weights = torch.zeros(8 * 1000, dtype=torch.int32, device="cuda")
    assert counter.bootstrap_weights(1000, 8, 5, weights.data_ptr()) == 8
    assert counter.fastq_parse(text, (T + 7,)) == first
    assert counter.fastq_parse(text) == first


@pytest.mark.parametrize("residue", [0, 1, 15])
def test_push_device_reads_no_byte_outside_a_buffer_of_exactly_the_text(counter, residue):
    import torch
    n_records = 60
    body = b"".join(record(i, 33 + i % 5) for i in range(1, n_records))
    pad = (residue - len(body) - len(record(0, 33, head=""))) % 16
    text = record(0, 33, head="p" * pad) + body
    assert len(text) % 16 == residue and text.endswith(b"\n")                # the last record ends on the buffer's last byte
    g = GuardedDevice(len(text))
    g.payload.copy_(torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(g.payload.device))
    torch.cuda.synchronize()
    for final in (True, False):
        counter.fastq_begin(-1)
        counter.fastq_push_device(g.ptr, len(text), final=final)
        if not final:
            counter.fastq_push_device(0, 0, final=True)                       # how a caller says `final` late
        consumed, reads, stop, n_stream = counter.fastq_end()
        want = restate_fastq_parse(text)
        assert (consumed, reads, stop) == want[:3] == (len(text), n_records, 0)
        assert counter.fastq_stream() == want[3] and n_stream == len(want[3])
    g.check("d_text")
    assert bytes(g.payload.cpu().numpy().tobytes()) == text                   # and the text is as it was
