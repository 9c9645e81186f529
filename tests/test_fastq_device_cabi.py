"""FASTQ text parsed on the device (tjamd_fastq_*), without a GPU: the declarations, the refusals that need no device, and the
rule of include/tatajuba_amd.h restated in Python and pinned against the project's host reader (tjamd_read_file_stream) on
seeded texts.  tests/test_fastq_device.py holds the device to the restatement."""
import ctypes as C
import fnmatch
import glob
import os
import random
import re

import tatajuba_amd as tj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NO_DEVICE, ERR_ARG = 1, 3
NEW_ENTRIES = ["tjamd_fastq_begin", "tjamd_fastq_push_device", "tjamd_fastq_push_host", "tjamd_fastq_end", "tjamd_fastq_reads", "tjamd_fastq_stop",
               "tjamd_fastq_stream", "tjamd_fastq_stream_bytes", "tjamd_fastq_tile_bytes", "tjamd_last_fastq_ms"]
HANDLES = ("tjamd_counter",)


# ---- the rule, restated ------------------------------------------------------------------------------------------------------

def restate_fastq_parse(text, final=True):
    """(consumed, reads, stop, stream) of the rule: the longest run of regular records from offset 0.  final: the end of the
    text ends a non-empty fourth line that has no '\\n'.  stop: 0 if all of the text was consumed, else 1."""
    text = bytes(text)
    n, p, reads, out = len(text), 0, 0, []
    while p < n:
        ends, q = [], p
        for line in range(4):
            e = text.find(b"\n", q)
            if e < 0:
                if not (final and line == 3 and q < n):
                    break
                e = n
            ends.append(e)
            q = e + 1
        if len(ends) < 4:
            break                                                         # a record cut short
        l0, l1, l2, l3 = text[p: ends[0]], text[ends[0] + 1: ends[1]], text[ends[1] + 1: ends[2]], text[ends[2] + 1: ends[3]]
        if not (l0[:1] == b"@" and len(l1) >= 1 and l1[:1] not in (b">", b"+", b"@") and l2[:1] == b"+" and len(l3) == len(l1)
                and b"\r" not in text[p: ends[3]]):
            break
        out.append(l1 + b"\n")
        reads += 1
        p = min(ends[3] + 1, n)
    return p, reads, (0 if p == n else 1), b"".join(out)


LENGTHS = (1, 2, 63, 64, 65, 150)
TAILS = ("nothing", "fasta", "multiline", "crlf", "blank", "short-quality", "open-complete", "open-incomplete")


def regular_record(rng, i, length=None):
    """a regular record: '@', '+' and '>' anywhere but in the first sequence byte, quality lines that may begin with '@'"""
    n = rng.choice(LENGTHS) if length is None else length
    seq = rng.choice("ACGTN") + "".join(rng.choice("ACGTNacgt@+>") for _ in range(n - 1))
    qual = "".join(rng.choice("@+>!I5F#") for _ in range(n))
    head = "@" + rng.choice(["r%d" % i, "r%d some text" % i, "", "@%d" % i, "r%d\t+>" % i])
    plus = "+" + rng.choice(["", "", "r%d" % i, "@x"])
    return ("%s\n%s\n%s\n%s\n" % (head, seq, plus, qual)).encode()


def irregular_tail(rng, kind):
    """the text behind the regular records: the first irregular record and what follows it"""
    seq = "".join(rng.choice("ACGT") for _ in range(rng.choice((5, 70))))
    more = regular_record(rng, 900) + regular_record(rng, 901)
    if kind == "nothing":
        return b""
    if kind == "fasta":
        return (">c1 x\n%s\n>c2\n%s\n" % (seq, seq[::-1])).encode() + more
    if kind == "multiline":
        return ("@m\n%s\n%s\n+\n%s\n%s\n" % (seq, seq, "I" * len(seq), "I" * len(seq))).encode() + more
    if kind == "crlf":
        return ("@w\r\n%s\r\n+\r\n%s\r\n" % (seq, "I" * len(seq))).encode() + more
    if kind == "blank":
        return b"\n" + more
    if kind == "short-quality":
        return ("@s\n%s\n+\n%s\n" % (seq, "I" * (len(seq) - 1))).encode() + more
    if kind == "open-complete":
        return ("@o\n%s\n+\n%s" % (seq, "I" * len(seq))).encode()
    assert kind == "open-incomplete"
    return ("@o\n%s\n+\n%s" % (seq, "I" * (len(seq) - 2))).encode() if rng.random() < 0.5 else ("@o\n%s" % seq).encode()


def seeded_text(seed):
    rng = random.Random(seed)
    body = b"".join(regular_record(rng, i) for i in range(rng.choice((0, 1, 2, 7, 30))))
    kind = TAILS[seed % len(TAILS)]
    return body + irregular_tail(rng, kind), kind, len(body)


def reader_stream(tmp_path, text, name="t.fq"):
    path = tmp_path / name
    path.write_bytes(text)
    s, n = tj.read_file_stream(str(path))
    return s.tobytes(), n


def test_the_restatement_on_texts_written_out_by_hand():
    r = restate_fastq_parse
    assert r(b"") == (0, 0, 0, b"")
    assert r(b"@a\nACG\n+\nIII\n") == (13, 1, 0, b"ACG\n")
    assert r(b"@a\nACG\n+\nIII") == (12, 1, 0, b"ACG\n")                   # the end of a final text ends the quality line
    assert r(b"@a\nACG\n+\nIII", final=False) == (0, 0, 1, b"")
    assert r(b"@a\nACG\n+\n") == (0, 0, 1, b"")                            # ... a non-empty one
    assert r(b"@a\nACG\n+\nII\n") == (0, 0, 1, b"")
    assert r(b"@a\nA\n+\n@\n@@b\nC\n+x\n@\n") == (20, 2, 0, b"A\nC\n")        # parity, not the byte, says what a header is
    assert r(b"@a\nA\n+\nI\n>c\nACGT\n") == (9, 1, 1, b"A\n")
    assert r(b"@a\nA\n+\nI\n\n@b\nC\n+\nI\n") == (9, 1, 1, b"A\n")
    assert r(b"@a\r\nA\r\n+\r\nI\r\n") == (0, 0, 1, b"")
    assert r(b"@a\n@A\n+\nII\n") == (0, 0, 1, b"") and r(b"@a\n\n+\n\n") == (0, 0, 1, b"")
    assert r(b"a\nA\n+\nI\n") == (0, 0, 1, b"") and r(b"@a\nA\n-\nI\n") == (0, 0, 1, b"")


def test_the_restatement_against_the_host_reader(tmp_path):
    kinds = {}
    for seed in range(320):
        text, kind, n_body = seeded_text(seed)
        consumed, reads, stop, stream = restate_fastq_parse(text)
        whole, n_whole = reader_stream(tmp_path, text)
        assert whole.startswith(stream), (seed, kind)
        assert stream.count(b"\n") == reads and consumed >= n_body, (seed, kind)
        if stop == 0:
            assert consumed == len(text) and whole == stream and n_whole == reads, (seed, kind)
        else:
            assert consumed < len(text), (seed, kind)
        rest, n_rest = reader_stream(tmp_path, text[consumed:], "rest.fq")   # the reader run on what is left supplies the rest
        assert stream + rest == whole and reads + n_rest == n_whole, (seed, kind)
        assert (stop == 0) == (kind in ("nothing", "open-complete")), (seed, kind)
        if kind not in ("nothing", "open-complete"):
            assert consumed == n_body, (seed, kind)
        kinds[kind] = kinds.get(kind, 0) + 1
    assert len(kinds) == len(TAILS) and min(kinds.values()) >= 40
    # every length of the list, alone and in a row
    rng = random.Random(1)
    for n in LENGTHS:
        text = b"".join(regular_record(rng, i, n) for i in range(5))
        consumed, reads, stop, stream = restate_fastq_parse(text)
        assert (consumed, reads, stop) == (len(text), 5, 0) and len(stream) == 5 * (n + 1)
        assert reader_stream(tmp_path, text) == (stream, 5)


# ---- declarations ---------------------------------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    own_path = os.path.join(ROOT, "include", "tatajuba_amd.h")
    own = strip(own_path)
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    declared = dict(re.findall(r"\b(tjamd_\w+)\s*\(([^;{}()]*)\)\s*;", own))
    for s in NEW_ENTRIES:
        assert s in declared, s
        for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
            if os.path.basename(path) != "tatajuba_amd.h":
                assert not re.search(r"\b%s\s*\(" % s, strip(path)), (s, path)
        assert s in tj.EXPORTS and any(fnmatch.fnmatchcase(s, pat) for pat in exported) and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
        # results leave through return values and accessors: no pointer that is neither const nor the counter
        for p in (x.strip() for x in declared[s].split(",")):
            assert "*" not in p or "const" in p or p.startswith(HANDLES), (s, p)
    assert len(glob.glob(os.path.join(ROOT, "include", "*.h"))) == 17     # and no header of their own
    assert re.search(r"enum \{ TJAMD_FASTQ_CARRY_MAX = 1 << 20 \};", own)
    assert L.tjamd_fastq_tile_bytes() == 4096 and L.tjamd_last_fastq_ms(None) == -1.0
    assert L.tjamd_fastq_reads(None) == -1 and L.tjamd_fastq_stop(None) == -1 and L.tjamd_fastq_stream(None) is None and L.tjamd_fastq_stream_bytes(None) == -1
    for name in ("fastq_begin", "fastq_push_host", "fastq_push_device", "fastq_end", "fastq_parse", "last_fastq_ms"):
        assert hasattr(tj.Counter, name)
    text = open(own_path).read()
    for what in ("L0[0] == '@'", "len (L1) >= 1 and L1[0] is none of '>' '+' '@'", "L2[0] == '+'", "len (L3) == len (L1)", "none of the record's bytes is '\\r'",
                 "Line parity decides", "a quality line may start with '@'", "ends a non-empty L3", "longest run of regular", "L1 + '\\n'",
                 "0: all text consumed", "1: irregular record at the consumed offset", "2: a record did not end within the carry",
                 "TJAMD_FASTQ_CARRY_MAX", "TATAJUBA_AMD_FASTQ_CARRY", "never through the host", "rounded up to 16", "the one wait of a session",
                 "Not built", "gzip or BGZF on the device", "FASTA or multi-line records on the device", "paired files", "read names"):
        assert what in text, what


# ---- refusals that need no device ------------------------------------------------------------------------------------------------

def test_host_refusals_with_a_counter_that_is_never_read():
    L = tj.lib()
    fake, text = C.c_void_p(0x1000), C.c_void_p(0x2000)       # never dereferenced: each call fails its argument checks first
    GIB = 1 << 30
    cases = [("tjamd_fastq_begin", lambda: L.tjamd_fastq_begin(None, 3), "null counter"),
             ("tjamd_fastq_begin", lambda: L.tjamd_fastq_begin(fake, -2), "min_tract_size -2 below -1"),
             ("tjamd_fastq_begin", lambda: L.tjamd_fastq_begin(fake, -100), "min_tract_size -100 below -1")]
    for fn in ("tjamd_fastq_push_device", "tjamd_fastq_push_host"):
        call = getattr(L, fn)
        cases += [(fn, lambda call=call: call(None, text, 16, 0), "null counter"),
                  (fn, lambda call=call: call(fake, None, 1, 0), "null text with n_bytes 1"),
                  (fn, lambda call=call: call(fake, None, GIB, 1), "null text"),
                  (fn, lambda call=call: call(fake, text, GIB + 1, 0), "above 1 GiB"),
                  (fn, lambda call=call: call(fake, text, 1 << 40, 1), "above 1 GiB")]
    for off in (1, 8, 15):
        cases.append(("tjamd_fastq_push_device", lambda off=off: L.tjamd_fastq_push_device(fake, C.c_void_p(0x2000 + off), 64, 0), "16-byte aligned"))
    cases.append(("tjamd_fastq_end", lambda: -L.tjamd_fastq_end(None), "null counter"))
    for fn, call, msg in cases:
        got, err = call(), L.tjamd_last_error().decode()
        assert got == ERR_ARG and err.startswith(fn) and "TJAMD_ERR_ARG" in err and msg in err, (fn, msg, got, err)
    if tj.device_count() == 0:                                 # good arguments, but nothing to run on: named, before the counter is read
        behind = [("tjamd_fastq_begin", lambda: L.tjamd_fastq_begin(fake, -1)), ("tjamd_fastq_begin", lambda: L.tjamd_fastq_begin(fake, 0)),
                  ("tjamd_fastq_begin", lambda: L.tjamd_fastq_begin(fake, 3)),
                  ("tjamd_fastq_push_device", lambda: L.tjamd_fastq_push_device(fake, text, 64, 0)),
                  ("tjamd_fastq_push_device", lambda: L.tjamd_fastq_push_device(fake, None, 0, 1)),
                  ("tjamd_fastq_push_device", lambda: L.tjamd_fastq_push_device(fake, text, GIB, 0)),
                  ("tjamd_fastq_push_host", lambda: L.tjamd_fastq_push_host(fake, C.c_void_p(0x2001), 7, 1)),
                  ("tjamd_fastq_push_host", lambda: L.tjamd_fastq_push_host(fake, None, 0, 0)),
                  ("tjamd_fastq_end", lambda: -L.tjamd_fastq_end(fake))]
        for fn, call in behind:
            got, err = call(), L.tjamd_last_error().decode()
            assert got == ERR_NO_DEVICE and err.startswith(fn) and "TJAMD_ERR_NO_DEVICE" in err, (fn, got, err)
