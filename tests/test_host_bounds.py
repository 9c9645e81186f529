"""The entries that write caller memory without a GPU, into guarded host buffers (tests/guarded.py) of exactly the size
their sizing call promised and of one byte less; and the case table of the bounds tests against the header."""
import ctypes as C
import fnmatch
import glob
import gzip
import inspect
import os
import random
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests import bounds_calls as bc
from tests import sample_calls as sc
from tests.guarded import GuardedHost, payload_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLES = ("tjamd_counter", "tjamd_comm", "tjamd_reference", "tjamd_annotation", "tjamd_coding")
N_WRITERS = 58                           # the entries of all headers that take a pointer that is neither const nor a handle


def declared_entries():
    """every tjamd_ function that a header under include/ declares -> {name: [its parameters]}, and the headers read"""
    found, headers = {}, sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))
    for header in headers:
        text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
        for name, params in re.findall(r"\b(tjamd_\w+)\s*\(([^;{}()]*)\)\s*;", text):
            assert name not in found, f"{name} is declared twice"
            found[name] = [p.strip() for p in params.split(",")]
    return found, headers


def entries_with_an_output_pointer():
    """the functions of the headers under include/ with a pointer parameter that is neither const nor one of the library's own
    handles"""
    found = {}
    for name, params in declared_entries()[0].items():
        outs = [p for p in params if "*" in p and "const" not in p and not p.startswith(HANDLES)]
        if outs:
            found[name] = outs
    return found


def exported_entries():
    """the tjamd_ names of every *_EXPORTS list of the package"""
    lists = [getattr(tj, x) for x in dir(tj) if x == "EXPORTS" or x.endswith("_EXPORTS")]
    assert len(lists) >= 15
    names = [n for lst in lists for n in lst if n.startswith("tjamd_")]
    assert len(names) == len(set(names))
    return set(names)


def check_the_table(declared, exported, tables, allow):
    """what the case table is held to; AssertionError names the entry"""
    names = [n for t in tables + [allow] for n in t]
    assert len(names) == len(set(names))                                      # each entry once
    for name in sorted(exported):
        if name in declared:
            assert name in names, f"{name} writes through {declared[name]}: add it to tests/bounds_calls.py"
    for name in names:                                                        # and nothing stale
        assert name in exported and name in declared, name
    for name, reason in allow.items():
        assert len(reason) > 20 and "\n" not in reason, name
    for table in tables:                                                      # the outputs named are parameters of the entry
        for name, outs in table.items():
            assert all(any(re.search(r"\b%s$" % o, p) for p in declared[name]) for o in outs), (name, outs, declared[name])


def test_every_entry_with_an_output_pointer_is_in_the_table_or_allowed():
    every, headers = declared_entries()
    declared = entries_with_an_output_pointer()
    assert len(headers) == 17 and len(declared) == N_WRITERS and "tjamd_located_tracts" in declared and "tjamd_counter_reset" not in declared
    exported = exported_entries()
    # the headers and the export lists name the same functions, and the linker's map lets each of them out
    assert sorted(exported - set(every)) == [], "exported, declared in no header"
    assert sorted(set(every) - exported) == [], "declared in a header, in no *_EXPORTS list"
    globs = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert any(g.startswith("tjamd_") for g in globs)
    for name in exported:
        assert any(fnmatch.fnmatchcase(name, g) for g in globs if g.startswith("tjamd_")), name
    tables = [bc.DEVICE, bc.HOST, bc.CPU, sc.OUTPUTS]
    check_the_table(declared, exported, tables, bc.ALLOW)
    # the 25 writers that headers of their own declare: each of them is missed when it leaves its table
    own = set(declared) - set(entries_of("tatajuba_amd.h"))
    assert len(own) == 25 and {"tjamd_locate_gapped", "tjamd_site_depths", "tjamd_translate", "tjamd_consensus_tree"} <= own
    for name in sorted(own):
        short = [{n: o for n, o in t.items() if n != name} for t in tables]
        with pytest.raises(AssertionError, match=name):
            check_the_table(declared, exported, short, bc.ALLOW)


def entries_of(header):
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(tjamd_\w+)\s*\([^;{}()]*\)\s*;", text)


def _guarded_names(fn):
    """the names a caller hands to _buffers(): the keys of the dict literal in its source"""
    src = inspect.getsource(fn)
    spec = src[src.index("_buffers({") + len("_buffers({"): src.index("}", src.index("_buffers({"))]
    return tuple(re.findall(r'"(\w+)":', spec))


def test_each_caller_guards_exactly_the_outputs_of_its_entry():
    for module, table in ((sc, sc.OUTPUTS), (bc, {n: o for n, o in {**bc.DEVICE, **bc.HOST}.items() if hasattr(bc, "call_" + n[len("tjamd_"):])})):
        assert len(table) >= 12
        for name, outs in table.items():
            fn = getattr(module, "call_" + name[len("tjamd_"):])
            assert _guarded_names(fn) == tuple(outs), (name, _guarded_names(fn), outs)
            assert name + "(" in inspect.getsource(fn)                        # and calls the entry it is named after


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


# ---- the host-only writers that headers of their own declare (N8-N12) ------------------------------------------------------

def test_translate_stays_inside_the_buffer():
    from tests.test_effects_cabi import restate_translate
    L = tj.lib()
    rng = random.Random(8)
    for n in (0, 1, 2, 3, 4, 5, 6, 7, 191, 192, 193, 3001):
        dna = "".join(rng.choice("ACGTacgtUuNn-") for _ in range(n))
        for reverse in (0, 1):
            want = restate_translate(dna, bool(reverse)).encode()
            need = L.tjamd_translate(dna.encode(), n, reverse, None, 0)       # the sizing call
            assert need == n // 3 == len(want), (n, reverse)
            out = GuardedHost(need)
            assert L.tjamd_translate(dna.encode(), n, reverse, out.c, need) == need
            out.check(f"out, n {n}")
            assert out.payload.tobytes() == want                              # no NUL: the last amino acid is the last byte
            for cap in sorted({need - 1, 1, 0} - {need, -1}):                 # too small: the size again, nothing written
                if cap < need:
                    short = GuardedHost(cap)
                    assert L.tjamd_translate(dna.encode(), n, reverse, short.c, cap) == need
                    short.check(f"out, n {n}, capacity {cap}")
                    assert short.untouched(), (n, reverse, cap)


def test_gff3_readers_stay_inside_their_buffers(tmp_path):
    from tests.test_effects_cabi import PHASE_LINES
    from tests.test_features_cabi import FT, GFF_LINES, N_SKIPPED, NAMES, WANT, check_features
    L = tj.lib()
    blob = "".join(n + "\n" for n in NAMES).encode()
    plain, gz = tmp_path / "a.gff3", tmp_path / "a.gff3.gz"
    plain.write_bytes("\n".join(GFF_LINES).encode())
    with gzip.open(gz, "wb") as fh:
        fh.write("\n".join(GFF_LINES).encode())
    n, need = len(WANT), sum(len(w[6]) + len(w[7]) + 2 for w in WANT)
    for path in (os.fsencode(str(plain)), os.fsencode(str(gz))):
        nb, sk = C.c_long(-1), C.c_long(-1)
        assert L.tjamd_gff3_read(path, blob, len(NAMES), None, 0, None, 0, C.byref(nb), C.byref(sk)) == n and (nb.value, sk.value) == (need, N_SKIPPED)
        out, strings = GuardedHost(n * FT.itemsize), GuardedHost(need)
        assert L.tjamd_gff3_read(path, blob, len(NAMES), out.c, n, strings.c, need, C.byref(nb), C.byref(sk)) == n and (nb.value, sk.value) == (need, N_SKIPPED)
        out.check("out"); strings.check("strings")
        check_features(out.view(FT), strings.payload.tobytes(), WANT)
        # the features short, the strings short, both: the sizes again, nothing written to either
        for cap, scap in [(c, need) for c in (n - 1, 1, 0)] + [(n, s) for s in (need - 1, 1, 0)] + [(n - 1, need - 1), (1, 1), (0, 0)]:
            o, s = GuardedHost(cap * FT.itemsize), GuardedHost(scap)
            nb.value = sk.value = -1
            assert L.tjamd_gff3_read(path, blob, len(NAMES), o.c, cap, s.c, scap, C.byref(nb), C.byref(sk)) == n and (nb.value, sk.value) == (need, N_SKIPPED)
            o.check(f"out, capacities {cap} and {scap}"); s.check(f"strings, capacities {cap} and {scap}")
            assert o.untouched() and s.untouched(), (cap, scap)
    # the phase column: the same lines through the same walker
    path = tmp_path / "p.gff3"
    path.write_bytes("\n".join(PHASE_LINES).encode())
    feats, _ = tj.read_gff3(str(path), NAMES)
    want = []
    for f in feats:
        col = PHASE_LINES[int(f["line"]) - 1].rstrip("\r").split("\t")[7]
        want.append(int(col) if col in ("0", "1", "2") else -1)
    n = L.tjamd_gff3_read_phase(os.fsencode(str(path)), blob, len(NAMES), None, 0)
    assert n == len(want) == 18
    out = GuardedHost(n)
    assert L.tjamd_gff3_read_phase(os.fsencode(str(path)), blob, len(NAMES), out.c, n) == n
    out.check("out")
    assert out.view(np.int8).tolist() == want
    for cap in (n - 1, 1, 0):
        short = GuardedHost(cap)
        assert L.tjamd_gff3_read_phase(os.fsencode(str(path)), blob, len(NAMES), short.c, cap) == n
        short.check(f"out, capacity {cap}")
        assert short.untouched(), cap


def test_read_file_names_stays_inside_the_buffer(tmp_path):
    from tests.test_variants_cabi import names_in_python
    L = tj.lib()
    rng = random.Random(3)
    fasta = b"".join(b">contig_%d some text\n%s\n" % (i, bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 200)))) for i in range(300)) + b">last\nACGT"
    fastq = b"".join(b"@read%d/1\tx\n%s\n+\n%s\n" % (i, b"ACGT" + b"A" * (i % 7), b"I" * (4 + i % 7)) for i in range(500))
    for name, data in (("ref.fa", fasta), ("reads.fq", fastq), ("one.fa", b">x\nA\n")):
        for zipped in (False, True):
            path = str(tmp_path / (name + (".gz" if zipped else "")))
            with (gzip.open(path, "wb") if zipped else open(path, "wb")) as fh:
                fh.write(data)
            want = b"".join(x + b"\n" for x in names_in_python(data))
            n = C.c_long(-1)
            need = L.tjamd_read_file_names(os.fsencode(path), None, 0, C.byref(n))
            assert need == len(want) > 0 and n.value == want.count(b"\n"), (name, zipped)
            out = GuardedHost(need)
            n.value = -1
            assert L.tjamd_read_file_names(os.fsencode(path), out.c, need, C.byref(n)) == need and n.value == want.count(b"\n")
            out.check("out")
            assert out.payload.tobytes() == want
            for cap in (need - 1, 1, 0):                                      # too small: the size again, nothing behind the capacity
                short = GuardedHost(cap)
                assert L.tjamd_read_file_names(os.fsencode(path), short.c, cap, None) == need
                short.check(f"out, capacity {cap}")
                written = short.payload != payload_pattern(cap)               # (the header promises the size, not that nothing is copied)
                assert (short.payload[written] == np.frombuffer(want, np.uint8)[:cap][written]).all(), (name, cap)


@pytest.mark.parametrize("k", [1, 4, 15, 32])
def test_site_ref_alt_stays_inside_the_buffer(k):
    from tests.test_sites_cabi import ALLELE, MAX_LENGTH, SITE, site_text
    L = tj.lib()
    rng = random.Random(500 + k)
    for trial in range(60):
        F = (0, k)[trial] if trial < 2 else rng.randint(0, k)
        ml = rng.randint(0, 40)
        site, al = np.zeros(1, SITE), np.zeros(1, ALLELE)
        site["base"], site["min_length"], site["n_flank"] = rng.randrange(4), ml, F
        site["ref_length"] = ml + rng.choice([0, 1, 5, MAX_LENGTH - ml])
        site["ref_flank"] = rng.getrandbits(2 * F) if F else 0
        al["alt_length"], al["n_flank"], al["alt_flank"] = rng.choice([ml, ml + 1, MAX_LENGTH]), rng.randint(0, F), (rng.getrandbits(2 * F) if F else 0)
        for ap, want in ((None, site_text(site[0])), (al.ctypes.data, site_text(site[0], al[0]))):
            length = L.tjamd_site_ref_alt(site.ctypes.data, ap, k, None, 0)   # the sizing call
            assert length == len(want) >= 1
            out = GuardedHost(length + 1)                                     # capacity > length: the text and a NUL, on the last byte
            assert L.tjamd_site_ref_alt(site.ctypes.data, ap, k, out.c, length + 1) == length
            out.check("out")
            assert out.payload.tobytes() == want.encode() + b"\0"
            for cap in (length, length - 1, 1, 0):                            # capacity = length has no room for the NUL: nothing
                if 0 <= cap <= length:
                    short = GuardedHost(cap)
                    assert L.tjamd_site_ref_alt(site.ctypes.data, ap, k, short.c, cap) == length
                    short.check(f"out, capacity {cap}")
                    assert short.untouched(), (trial, cap, length)
