"""Tracts located on a reference genome (tjamd_reference_*, tjamd_locate, tjamd_located_tracts) without a GPU: the entries
are declared, exported and refuse bad arguments before any device call, the structures match the header, and the brute-force
restatement that the GPU tests (tests/test_locate.py) compare against reproduces cases worked out by hand.

The restatement is written from the rules in include/tatajuba_amd.h, not from the device code:
  restate_reference_index   one entry per maximal run of one base whose k bytes on each side lie in the contig and are ACGTU
  restate_locate            one flank exact, the other within max_mismatches; fewest mismatches, then smallest flat
  restate_located_tracts    a tract sits where its located row with the highest total sits; tracts at one (flat, base) merge;
                            unlocated tracts first in input order, then ascending (flat, base)"""
import ctypes as C
import fnmatch
import os
import random
import re

import numpy as np

import tatajuba_amd as tj
from tests import pyref
from tests.test_union_tracts_cabi import hand_union, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_reference_create", "tjamd_reference_destroy", "tjamd_reference_entries", "tjamd_reference_contigs",
               "tjamd_reference_download", "tjamd_last_reference_ms", "tjamd_locate", "tjamd_last_locate_ms",
               "tjamd_located_tracts", "tjamd_last_located_tracts_ms"]
ERR_ARG, ERR_CAP = 3, 4
CODE = {ord(c): v for c, v in zip("ACGTUacgtu", [0, 1, 2, 3, 3] * 2)}
NOWHERE = (-1, -1, -1, 0, 0, 0, 0)                       # tjamd_location of a row or tract without a hit


def _pack(codes):
    return sum((c & 3) << (2 * i) for i, c in enumerate(codes))


def contigs_of(stream):
    """the contigs of a stream of reads: every contig is followed by a newline (a last one without it counts too)"""
    pieces = bytes(stream).split(b"\n")
    if pieces[-1] == b"":
        pieces.pop()
    return pieces


def restate_reference_index(stream, k):
    """-> (REF_ENTRY_DTYPE array in ascending flat, number of contigs)"""
    out = []
    offset = 0
    pieces = contigs_of(stream)
    for ci, s in enumerate(pieces):
        L = len(s)
        i = 0
        while i < L:
            b = CODE.get(s[i])
            if b is None:
                i += 1
                continue
            e = i
            while e + 1 < L and CODE.get(s[e + 1]) == b:
                e += 1
            left, right = s[max(i - k, 0):i], s[e + 1:e + 1 + k]
            if i >= k and e + k <= L - 1 and all(c in CODE for c in left + right):
                lc, rc = [CODE[c] for c in left], [CODE[c] for c in right]
                if b < 2:
                    rec = (_pack(lc), _pack(rc), offset + i, ci, i, e - i + 1, b, 0, 0)
                else:
                    rec = (_pack([3 - c for c in reversed(rc)]), _pack([3 - c for c in reversed(lc)]), offset + i, ci, i, e - i + 1, 3 - b, 1, 0)
                out.append(rec)
            i = e + 1
        offset += L
    return np.array(out, dtype=tj.REF_ENTRY_DTYPE), len(pieces)


def flank_distance(x, y):
    """positions at which packed flanks differ: popcount of (x ^ y | (x ^ y) >> 1) & 0x5555...; x an array, y a scalar"""
    v = np.asarray(x, dtype=np.uint64) ^ np.uint64(y)
    v = (v | (v >> np.uint64(1))) & np.uint64(0x5555555555555555)
    return np.unpackbits(np.ascontiguousarray(v).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def restate_locate(entries, keys, max_mismatches):
    """keys: uint64 [n, 3] records (only base, ctx0, ctx1 are read) -> LOCATION_DTYPE [n]"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    out = np.zeros(len(keys), dtype=tj.LOCATION_DTYPE)
    memo = {}
    for q, (c0, c1, meta) in enumerate(keys.tolist()):
        ctx = (c0, c1, meta & 3)
        if ctx not in memo:
            res = NOWHERE
            # every entry of the base with an exact flank, then the distance in its other flank
            cand = np.flatnonzero((entries["base"] == (meta & 3)) & ((entries["ctx0"] == c0) | (entries["ctx1"] == c1))) if len(entries) else []
            if len(cand):
                d = flank_distance(entries["ctx0"][cand], c0) + flank_distance(entries["ctx1"][cand], c1)    # (one of the two is 0)
                hit = cand[d <= max_mismatches]                               # (an entry exact in both flanks: once)
                if len(hit):
                    d = d[d <= max_mismatches]
                    best = np.lexsort((entries["flat"][hit], d))[0]          # fewest mismatches, then leftmost
                    e = entries[hit[best]]
                    res = (int(e["flat"]), int(e["contig"]), int(e["pos"]), int(e["length"]), int(d[best]), int(e["neg_strand"]), len(hit))
            memo[ctx] = res
        out[q] = memo[ctx]
    return out


def context_tracts(keys, mat):
    """the context-keyed tracts of tjamd_tract_ids as UNION_TRACT_DTYPE"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    totals = np.asarray(mat, dtype=np.int64).sum(axis=1)
    ctx = [(int(a), int(b), int(c) & 3) for a, b, c in keys]
    heads = [i for i in range(len(ctx)) if i == 0 or ctx[i] != ctx[i - 1]] + [len(ctx)]
    out = np.zeros(len(heads) - 1, dtype=tj.UNION_TRACT_DTYPE)
    for t, (lo, hi) in enumerate(zip(heads[:-1], heads[1:])):
        out[t] = (lo, hi - lo, 1, lo + int(np.argmax(totals[lo:hi])), 0, 0, int(totals[lo:hi].sum()))
    return out


def restate_located_tracts(keys, mat, tracts, loc):
    """-> dict of perm (int64 [n]), tracts (UNION_TRACT_DTYPE), tract_loc (LOCATION_DTYPE), ref_length; tracts None: the
    context-keyed ones"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    totals = np.asarray(mat, dtype=np.int64).sum(axis=1).tolist()
    if tracts is None:
        tracts = context_tracts(keys, mat)

    def place_of(rows):
        """the located row with the highest total, the first on a tie (None: no located row)"""
        best = None
        for r in rows:
            if loc["flat"][r] >= 0 and (best is None or totals[r] > totals[best]):
                best = r
        return best

    unlocated, located = [], {}
    for t in range(len(tracts)):
        first, n_rows = int(tracts["first"][t]), int(tracts["n_rows"][t])
        r = place_of(range(first, first + n_rows))
        if r is None:
            unlocated.append([t])                                             # alone, in input order
        else:
            located.setdefault((int(loc["flat"][r]), int(keys[first, 2]) & 3), []).append(t)
    merged = unlocated + [located[place] for place in sorted(located)]       # ascending (flat, base)
    perm, out_t, out_l = [], [], []
    for members in merged:
        start = len(perm)
        for t in members:
            perm.extend(range(int(tracts["first"][t]), int(tracts["first"][t]) + int(tracts["n_rows"][t])))
        rows = perm[start:]
        mode = start + max(range(len(rows)), key=lambda x: (totals[rows[x]], -x))
        out_t.append((start, len(rows), int(tracts["n_context"][members].sum()), mode, int(tracts["indel"][members].max() != 0),
                      int(tracts["lev_distance"][members].max()), int(tracts["integral"][members].sum())))
        r = place_of(rows)
        out_l.append(tuple(loc[r].tolist()) if r is not None else NOWHERE)
    out_l = np.array(out_l, dtype=tj.LOCATION_DTYPE)
    return {"perm": np.array(perm, dtype=np.int64), "tracts": np.array(out_t, dtype=tj.UNION_TRACT_DTYPE), "tract_loc": out_l,
            "ref_length": out_l["ref_length"].astype(np.int64)}


def location_line(t, loc):
    """one line of tract_locations.tsv (examples/located_tracts.c)"""
    return "tid_%06d\t%d\t%d\t%s\t%d\t%d\t%d\n" % (t, loc["contig"], loc["pos"], "." if loc["flat"] < 0 else "-" if loc["neg_strand"] else "+",
                                                    loc["ref_length"], loc["mismatches"], loc["n_hits"])


LOCATIONS_HEADER = "tract_id\tcontig\tposition\tstrand\treference_length\tmismatches\tn_hits\n"


# ---- declarations and argument checks ----------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    header = open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    for s in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % s, code), s
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s in tj.EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    for struct in ("tjamd_reference", "tjamd_ref_entry", "tjamd_location"):
        assert re.search(r"\}\s*%s\s*;|typedef struct %s %s;" % (struct, struct, struct), code), struct
    assert tj.REF_ENTRY_DTYPE.itemsize == 48 and tj.LOCATION_DTYPE.itemsize == 32
    f = tj.REF_ENTRY_DTYPE.fields
    assert [f[x][1] for x in ("ctx0", "ctx1", "flat", "contig", "pos", "length", "base", "neg_strand")] == [0, 8, 16, 24, 28, 32, 36, 40]
    f = tj.LOCATION_DTYPE.fields
    assert [f[x][1] for x in ("flat", "contig", "pos", "ref_length", "mismatches", "neg_strand", "n_hits")] == [0, 8, 12, 16, 20, 24, 28]
    assert L.tjamd_last_reference_ms(None) == -1.0 and L.tjamd_last_locate_ms(None) == -1.0 and L.tjamd_last_located_tracts_ms(None) == -1.0
    assert L.tjamd_reference_entries(None) == -1 and L.tjamd_reference_contigs(None) == -1
    L.tjamd_reference_destroy(None)


def test_reference_create_without_a_device_names_the_error():
    L = tj.lib()
    buf = C.create_string_buffer(b"ACGTACGTAAACGTACGT\n")
    ref = L.tjamd_reference_create(None, buf, 19)
    assert not ref
    err = L.tjamd_last_error().decode()
    assert err.startswith("tjamd_reference_create")
    if tj.device_count() == 0:
        assert "TJAMD_ERR_NO_DEVICE" in err, err
    else:
        assert "null counter" in err, err


def test_index_and_coding_table_refuse_a_stream_alike():
    """the two entries that take a genome stream from the host say one thing of it: a null stream with bytes, and a stream of
    2^31 bytes (through a pointer that is never read).  Each says it where its own order puts it: tjamd_reference_create refuses
    a missing device before it looks at anything else, tjamd_coding_create a null counter; so without a device the clause is
    heard from the coding table alone, and with one (a real counter then) from both, word for word behind the entry's name."""
    L = tj.lib()
    fake = C.c_void_p(0x1000)
    have_device = tj.device_count() > 0
    counter = tj.Counter(5) if have_device else None
    h = counter._h if have_device else fake      # (without a device no counter can exist, and neither entry reads the pointer)

    def said(name, handle):
        err = L.tjamd_last_error().decode()
        assert not handle and err.startswith(name + ": "), (name, err)
        return err[len(name) + 2:]

    for stream, n_bytes, code_clause in ((None, 5, "null stream"), (fake, 1 << 31, "a stream of 2147483648 bytes (positions are 32-bit)")):
        assert said("tjamd_coding_create", L.tjamd_coding_create(h, stream, n_bytes, None, 0, None)) == code_clause
        assert said("tjamd_coding_create", L.tjamd_coding_create(None, stream, n_bytes, None, 0, None)) == "null counter"
        of_index = said("tjamd_reference_create", L.tjamd_reference_create(h, stream, n_bytes))
        of_index_without_counter = said("tjamd_reference_create", L.tjamd_reference_create(None, stream, n_bytes))
        if have_device:
            assert of_index == code_clause and of_index_without_counter == "null counter"
            assert counter.last_reference_ms() == -1.0 and counter.last_coding_ms() == -1.0
        else:
            assert of_index.startswith("TJAMD_ERR_NO_DEVICE") and of_index_without_counter == of_index
    if have_device:
        counter.close()


def test_locate_entries_check_their_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    assert L.tjamd_locate(None, None, fake, 10, 1, fake) == -ERR_ARG and "null counter or reference" in L.tjamd_last_error().decode()

    def tracts(c=None, keys=fake, counts=fake, n=10, ns=2, tr=fake, nt=3, loc=fake, perm=fake, otr=fake, cap=10):
        rc = L.tjamd_located_tracts(c, keys, counts, n, ns, tr, nt, loc, perm, None, None, otr, None, None, cap)
        return rc, L.tjamd_last_error().decode()

    for kw, rc, msg in [({}, ERR_ARG, "null counter"), ({"ns": 0}, ERR_ARG, "n_samples 0 outside 1..4096"), ({"keys": None}, ERR_ARG, "null union buffers"),
                        ({"counts": None}, ERR_ARG, "null union buffers"), ({"n": -1}, ERR_ARG, "n_union -1 < 0"), ({"n": 1 << 31}, ERR_CAP, "union rows"),
                        ({"loc": None}, ERR_ARG, "null location, permutation or tract buffer"), ({"perm": None}, ERR_ARG, "null location, permutation or tract buffer"),
                        ({"otr": None}, ERR_ARG, "null location, permutation or tract buffer"), ({"nt": 0}, ERR_ARG, "n_tracts 0 for a union of 10 rows"),
                        ({"nt": 11}, ERR_ARG, "n_tracts 11 for a union of 10 rows"), ({"cap": 0}, ERR_CAP, "capacity 0 for a union of 10 rows")]:
        got, err = tracts(**kw)
        assert got == -rc and err.startswith("tjamd_located_tracts") and msg in err, (kw, got, err)


# ---- the index by hand: k = 4 ------------------------------------------------------------------------------------------
#   contig 0  ACGTAAAGCATNGCATccTGCAT   (23)  AAA at 4; G C A T at 7-10 have the N in their right flank, G C A T at 12-15 in
#                                             their left flank; the lowercase cc at 16 is a run of C; T at 18 is the last run
#                                             with 4 bases behind it; G at 19 is closer than k to the contig end
#   contig 1  ACGTACG                   (7)   shorter than 2k + 1: nothing
#   contig 2  TTGACGGGTCAAC             (13)  C at 4, GGG at 5 (a C tract on the other strand), T at 8; flat = pos + 30
K = 4
HAND_GENOME = b"ACGTAAAGCATNGCATccTGCAT\nACGTACG\nTTGACGGGTCAAC\n"
HAND_ENTRIES = [  # ctx0, ctx1, flat, contig, pos, length, base, neg_strand
    (pack("ACGT"), pack("GCAT"), 4, 0, 4, 3, 0, 0),
    (pack("GCAT"), pack("TGCA"), 16, 0, 16, 2, 1, 0),
    (pack("ATGC"), pack("GGAT"), 18, 0, 18, 1, 0, 1),     # T, flanks ATCC | GCAT: revcomp (GCAT) = ATGC, revcomp (ATCC) = GGAT
    (pack("TTGA"), pack("GGGT"), 34, 2, 4, 1, 1, 0),
    (pack("TTGA"), pack("GTCA"), 35, 2, 5, 3, 1, 1),      # GGG, flanks TGAC | TCAA: revcomp (TCAA) = TTGA, revcomp (TGAC) = GTCA
    (pack("GTTG"), pack("CCCG"), 38, 2, 8, 1, 0, 1),      # T, flanks CGGG | CAAC: revcomp (CAAC) = GTTG, revcomp (CGGG) = CCCG
]


def test_reference_index_of_the_hand_built_genome():
    entries, n_contigs = restate_reference_index(HAND_GENOME, K)
    assert n_contigs == 3
    got = [tuple(int(e[f]) for f in ("ctx0", "ctx1", "flat", "contig", "pos", "length", "base", "neg_strand")) for e in entries]
    assert got == HAND_ENTRIES
    assert restate_reference_index(b"", K)[1] == 0 and len(restate_reference_index(b"", K)[0]) == 0
    assert restate_reference_index(HAND_GENOME[:-1], K)[1] == 3          # a last contig without its newline still counts
    # U is T, and case does not split a run
    a = restate_reference_index(b"ACGTAAAGCAT\nGGCAtUtGGCA\n", K)[0]
    assert [(int(e["pos"]), int(e["length"]), int(e["neg_strand"])) for e in a] == [(4, 3, 0), (4, 3, 1)]


def test_reference_index_is_the_scan_of_the_genome_as_a_read():
    """on ACGT-only strings the entries are the tracts of the closed-form scan (m = 2) plus its monomers, at read_offset + k"""
    rng = random.Random(77)
    for k in (2, 4, 7, 13):
        for _ in range(20):
            s = "".join(rng.choice("ACGT") * rng.choice([1, 1, 1, 2, 3, 6]) for _ in range(rng.randint(1, 60)))
            want = sorted((off + k, base, n, flag - 1, c0, c1) for base, n, off, flag, c0, c1 in pyref.scan_closed_form(s, k, 2) + pyref.scan_all_monomers(s, k))
            e = restate_reference_index(s.encode() + b"\n", k)[0]
            got = [(int(x["pos"]), int(x["base"]), int(x["length"]), int(x["neg_strand"]), int(x["ctx0"]), int(x["ctx1"])) for x in e]
            assert got == want, (k, s)
            assert (e["flat"] == e["pos"]).all() and (e["contig"] == 0).all()


# ---- the lookup by hand ------------------------------------------------------------------------------------------------

def _key(base, left, right):
    return [pack(left), pack(right), base]


def test_locate_rule_on_hand_built_cases():
    entries = np.array([e + (0,) for e in HAND_ENTRIES], dtype=tj.REF_ENTRY_DTYPE)
    keys = [_key(0, "ACGT", "GCAT"),       # the AAA tract, exact
            _key(0, "ACGT", "GCAA"),       # one substitution in its right flank
            _key(0, "ACGA", "GCAA"),       # one in each flank: not matched
            _key(1, "ACGT", "GCAT"),       # another base
            _key(1, "TTGA", "GTCA"),       # the GGG run as the scan of a read would store it
            _key(0, "ATGC", "GGAT"),       # the T run
            _key(1, "TTGA", "GGGA")]       # left flank exact for two entries: GGGT at 1 mismatch, GTCA at 2
    r = restate_locate(entries, keys, 1)
    assert [tuple(x.tolist()) for x in r] == [(4, 0, 4, 3, 0, 0, 1), (4, 0, 4, 3, 1, 0, 1), NOWHERE, NOWHERE, (35, 2, 5, 3, 0, 1, 1), (18, 0, 18, 1, 0, 1, 1),
                                              (34, 2, 4, 1, 1, 0, 1)]
    assert [tuple(x.tolist()) for x in restate_locate(entries, keys, 0)][1] == NOWHERE
    assert tuple(restate_locate(entries, keys, 3)[6].tolist()) == (34, 2, 4, 1, 1, 0, 2)      # both now hit; the closer one wins
    # a repeat: two entries with one context -> n_hits 2, the leftmost is the location
    rep, _ = restate_reference_index(b"ACGTAAAGCATACGTAAAAGCAT\n", K)
    got = restate_locate(rep, [_key(0, "ACGT", "GCAT")], 0)[0]
    assert tuple(got.tolist()) == (4, 0, 4, 3, 0, 0, 2)
    # left flank exact at 1 mismatch (flat 10) against exact in both (flat 50): fewer mismatches beat leftmost, counted once;
    # without the exact one, right-exact at flat 5 and left-exact at flat 10 tie at 1 mismatch: the leftmost
    L_, R_ = pack("ACGT"), pack("GCAT")
    mk = lambda c0, c1, flat: (c0, c1, flat, 0, flat, 5, 0, 0, 0)
    three = np.array([mk(pack("ACGA"), R_, 5), mk(L_, pack("GCAA"), 10), mk(L_, R_, 50)], dtype=tj.REF_ENTRY_DTYPE)
    assert tuple(restate_locate(three, [[L_, R_, 0]], 1)[0].tolist()) == (50, 0, 50, 5, 0, 0, 3)
    assert tuple(restate_locate(three[:2], [[L_, R_, 0]], 1)[0].tolist()) == (5, 0, 5, 5, 1, 0, 2)
    assert tuple(restate_locate(three[1:2], [[L_, R_, 0]], 1)[0].tolist()) == (10, 0, 10, 5, 1, 0, 1)
    assert tuple(restate_locate(three[:0], [[L_, R_, 0]], 1)[0].tolist()) == NOWHERE
    assert flank_distance([pack("ACGT"), pack("TTTT")], pack("ACGA")).tolist() == [1, 4]


# ---- tracts by location on the hand union of tests/test_union_tracts_cabi.py -----------------------------------------------
#   rows 0, 1 (one context, totals 3 and 3) and row 2 (total 4, unlocated) are tract 0, row 3 (total 4) is tract 1, row 4
#   (base A, total 10) is tract 2; rows 0, 1 and 3 sit at flat 100, row 4 at flat 7

def hand_tracts_and_locations(row4_located=True):
    tracts = np.array([(0, 3, 2, 2, 0, 0, 10), (3, 1, 1, 3, 1, 2, 4), (4, 1, 1, 4, 0, 0, 10)], dtype=tj.UNION_TRACT_DTYPE)
    loc = np.array([(100, 1, 40, 6, 0, 0, 1), (100, 1, 40, 6, 0, 0, 1), NOWHERE, (100, 1, 40, 6, 1, 0, 1), (7, 0, 7, 8, 0, 1, 1) if row4_located else NOWHERE],
                   dtype=tj.LOCATION_DTYPE)
    return tracts, loc


def test_located_tracts_on_the_hand_built_union():
    keys, mat, _ = hand_union()
    for located in (True, False):                       # flat 7 sorts in front of flat 100; an unlocated tract comes first anyway
        tracts, loc = hand_tracts_and_locations(located)
        r = restate_located_tracts(keys, mat, tracts, loc)
        assert r["perm"].tolist() == [4, 0, 1, 2, 3]
        # the merged tract: contexts 2 + 1, mode = the first output row with total 4 (input row 2), indel and lev_distance from
        # tract 1, located where its highest located row (input row 3, total 4) is: 1 mismatch
        assert [tuple(t.tolist()) for t in r["tracts"]] == [(0, 1, 1, 0, 0, 0, 10), (1, 4, 3, 3, 1, 2, 14)]
        assert [tuple(x.tolist()) for x in r["tract_loc"]] == [(7, 0, 7, 8, 0, 1, 1) if located else NOWHERE, (100, 1, 40, 6, 1, 0, 1)]
        assert r["ref_length"].tolist() == [8 if located else 0, 6]
    # two unlocated tracts keep input order in front; different bases at one flat do not merge, and sort by base
    tracts, loc = hand_tracts_and_locations()
    loc[3] = NOWHERE
    loc[4] = (100, 1, 40, 8, 0, 0, 1)
    r = restate_located_tracts(keys, mat, tracts, loc)
    assert r["perm"].tolist() == [3, 4, 0, 1, 2] and r["tracts"]["first"].tolist() == [0, 1, 2] and r["tract_loc"]["flat"].tolist() == [-1, 100, 100]
    # no tracts given: one per context (rows 0-1, 2, 3, 4); rows 0-1 and row 3 merge at flat 100
    tracts, loc = hand_tracts_and_locations()
    assert [tuple(t.tolist()) for t in context_tracts(keys, mat)] == [(0, 2, 1, 0, 0, 0, 6), (2, 1, 1, 2, 0, 0, 4), (3, 1, 1, 3, 0, 0, 4), (4, 1, 1, 4, 0, 0, 10)]
    r = restate_located_tracts(keys, mat, None, loc)
    assert r["perm"].tolist() == [2, 4, 0, 1, 3] and [tuple(t.tolist()) for t in r["tracts"]] == [(0, 1, 1, 0, 0, 0, 4), (1, 1, 1, 1, 0, 0, 10), (2, 3, 2, 4, 0, 0, 10)]
    assert location_line(3, r["tract_loc"][0]) == "tid_000003\t-1\t-1\t.\t0\t0\t0\n" and location_line(0, loc[4]) == "tid_000000\t0\t7\t-\t8\t0\t1\n"
