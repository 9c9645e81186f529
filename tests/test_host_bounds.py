"""The entries that write caller memory without a GPU, into guarded host buffers (tests/guarded.py) of exactly the size
their sizing call promised and of one byte less; and the case table of the bounds tests against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests import bounds_calls as bc
from tests.guarded import GuardedHost, payload_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLES = ("tjamd_counter", "tjamd_comm", "tjamd_reference")


def entries_with_an_output_pointer():
    """the functions of include/tatajuba_amd.h with a pointer parameter that is neither const nor one of the library's own
    handles"""
    text = open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = {}
    for name, params in re.findall(r"\b(tjamd_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        outs = [p.strip() for p in params.split(",") if "*" in p and "const" not in p and not p.strip().startswith(HANDLES)]
        if outs:
            found[name] = outs
    return found


def test_every_entry_with_an_output_pointer_is_in_the_table_or_allowed():
    declared = entries_with_an_output_pointer()
    assert len(declared) > 30 and "tjamd_located_tracts" in declared and "tjamd_counter_reset" not in declared
    tables = [bc.DEVICE, bc.HOST, bc.CPU, bc.ALLOW]
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names))                                      # each entry once
    for name in tj.EXPORTS:
        if name in declared:
            assert name in names, f"{name} writes through {declared[name]}: add it to tests/bounds_calls.py"
    for name in names:                                                        # and nothing stale
        assert name in tj.EXPORTS and name in declared, name
    for name, reason in bc.ALLOW.items():
        assert len(reason) > 20 and "\n" not in reason, name
    for table in (bc.DEVICE, bc.HOST, bc.CPU):                                # the outputs named are parameters of the entry
        for name, outs in table.items():
            assert all(any(re.search(r"\b%s$" % o, p) for p in declared[name]) for o in outs), (name, outs, declared[name])


def fastq_files(tmp_path, golden_dir):
    rng = np.random.default_rng(5)
    reads = ["".join(rng.choice(list("ACGTN"), int(rng.integers(1, 300)))) for _ in range(400)]
    plain = str(tmp_path / "small.fq")
    with open(plain, "w") as fh:
        fh.write("".join(f"@r{i} x\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)))
    return [os.path.join(golden_dir, "err1750956.fastq.gz"), plain]


@pytest.mark.parametrize("which", [0, 1], ids=["golden-gz", "plain"])
def test_file_readers_stay_inside_the_buffer(tmp_path, golden_dir, which):
    path = os.fsencode(fastq_files(tmp_path, golden_dir)[which])
    want, want_reads = orc.parse_file_to_stream(path)
    L = tj.lib()
    L.tjamd_read_file_stream_mt.restype = C.c_long
    L.tjamd_read_file_stream_mt.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.c_int, C.c_long]
    readers = [("single", lambda out, cap, n: L.tjamd_read_file_stream(path, out, cap, n))]
    for threads, window in ((1, 0), (3, 4096), (16, 65536)):
        readers.append((f"mt-{threads}-{window}", lambda out, cap, n, t=threads, w=window: L.tjamd_read_file_stream_mt(path, out, cap, n, t, w)))
    for name, read in readers:
        n = C.c_long(-1)
        need = read(None, 0, C.byref(n))                                      # the sizing call
        assert need == len(want) > 0 and n.value == want_reads, name
        out = GuardedHost(need)
        n = C.c_long(-1)
        assert read(out.c, need, C.byref(n)) == need and n.value == want_reads, name
        out.check(name)
        assert out.payload.tobytes() == want.tobytes(), name
        for cap in (need - 1, 1, 0):                                          # too small: the size again, nothing behind the capacity
            short = GuardedHost(cap)
            n = C.c_long(-1)
            assert read(short.c, cap, C.byref(n)) == need and n.value == want_reads, (name, cap)
            short.check(name)
            written = short.payload != payload_pattern(cap)                   # (the reads or batches that fit as a whole may have been copied)
            assert (short.payload[written] == want[:cap][written]).all(), (name, cap)


def test_synth_stream_stays_inside_the_buffer():
    L = tj.lib()
    args = (0x7A7A0001, 0x7A7A1000, 5, 50000, 3000, 100, 180)
    want = None
    for threads in (1, 3, 16):
        need = -L.tjamd_synth_stream(*args, None, 0, threads)
        assert need > 3000 * 101
        out = GuardedHost(need)
        assert L.tjamd_synth_stream(*args, out.c, need, threads) == need
        out.check(f"out, {threads} threads")
        want = out.payload.tobytes() if want is None else want
        assert out.payload.tobytes() == want and want.endswith(b"\n") and want.count(b"\n") == 3000   # the same stream whatever the threads
        for cap in (need - 1, 1, 0):
            short = GuardedHost(cap)
            assert L.tjamd_synth_stream(*args, short.c, cap, threads) == -need
            short.check(f"out, {threads} threads, capacity {cap}")
            assert short.untouched()


def test_peer_access_report_with_a_tiny_capacity():
    L = tj.lib()
    for cap in (0, 1, 2, 23, 24, 25, 64):
        out = GuardedHost(cap)
        staged = L.tjamd_peer_access_report(C.cast(out.c, C.c_char_p), cap)
        out.check(f"out, capacity {cap}")
        assert staged >= 0
        if cap:
            text = out.payload.tobytes()
            assert b"\0" in text                                              # a terminated string within the capacity
        else:
            assert out.untouched()
    assert L.tjamd_peer_access_report(None, 0) >= 0
