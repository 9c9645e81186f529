"""Per-sample tract variants (tjamd_tract_variants) and contig names (tjamd_read_file_names) without a GPU: the entries are
declared, exported and refuse bad arguments before any device call, the record matches the header, the restatement that the
GPU tests (tests/test_variants.py) compare against reproduces cases worked out by hand, every call it makes on a random
genome spells the genome at its place and turns it into the sample's allele, and the names of a FASTA / FASTQ file are the
ones Python parses.

restate_tract_variants is written from the rule in include/tatajuba_variants.h with strings: the flank words are decoded to
forward text, the comparison is Python slicing.  The device does the same with two packed words, an XOR and a count of
leading zeros."""
import ctypes as C
import fnmatch
import gzip
import os
import random
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedHost
from tests.test_locate_cabi import NOWHERE, restate_locate, restate_reference_index
from tests.test_tract_stats_cabi import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_tract_variants", "tjamd_last_tract_variants_ms", "tjamd_read_file_names"]
ERR_NO_DEVICE, ERR_ARG, ERR_CAP = 1, 3, 4
VAR, TR, LOC = tj.VARIANT_DTYPE, tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE
DNA = "ACGT"
_COMP = str.maketrans("ACGT", "TGCA")
_FOLD = str.maketrans("acgtuU", "ACGTTT")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def pack(s):
    return sum(DNA.index(ch) << (2 * i) for i, ch in enumerate(s))


def unpack(word, n):
    return "".join(DNA[(int(word) >> (2 * i)) & 3] for i in range(n))


def signed_length(meta):
    v = (int(meta) >> 2) & 0x3FF
    return v - 0x400 if v & 0x200 else v


def forward_right(ctx0, ctx1, k, neg):
    """the k bases behind the run on the forward strand, the one next to the tract first"""
    return revcomp(unpack(ctx0, k)) if neg else unpack(ctx1, k)


def canonical_row(base_fwd, left_fwd, right_fwd, length):
    """a union row (ctx0, ctx1, meta) from forward text, as the scan stores it: A and C as read, G and T reverse-complemented"""
    b = DNA.index(base_fwd)
    if b < 2:
        return record(b, pack(left_fwd), pack(right_fwd), length)
    return record(3 - b, pack(revcomp(right_fwd)), pack(revcomp(left_fwd)), length)


def common_prefix_suffix(a, b):
    """the longest common prefix of two strings, then the longest common suffix of what the prefix leaves (the plain reading
    of common_prefix_suffix_lengths_from_strings)"""
    p = 0
    while p < min(len(a), len(b)) and a[p] == b[p]:
        p += 1
    a, b = a[p:], b[p:]
    s = 0
    while s < min(len(a), len(b)) and a[len(a) - 1 - s] == b[len(b) - 1 - s]:
        s += 1
    return p, s


def restate_tract_variants(keys, mat, tracts, tract_loc, entries, k, lst=None):
    """-> (VARIANT_DTYPE records in sample-major order, offsets [n_samples + 1], one dict per record: REF, ALT, k_eff, R_alt)"""
    keys = np.asarray(keys, np.uint64).reshape(-1, 3)
    mat = np.asarray(mat)
    ns = mat.shape[1]
    lst = range(len(tracts)) if lst is None else [int(t) for t in lst]
    flats = entries["flat"].tolist()
    at = {f: i for i, f in enumerate(flats)}
    recs, text, offsets = [], [], [0]
    for s in range(ns):
        for t in lst:
            loc = tract_loc[t]
            if loc["flat"] < 0 or int(loc["flat"]) not in at:
                continue
            e = entries[at[int(loc["flat"])]]
            first, n_rows = int(tracts["first"][t]), int(tracts["n_rows"][t])
            col = mat[first: first + n_rows, s]
            if col.max() <= 0:
                continue
            row = first + int(np.argmax(col))                                # the first of equal counts
            La, Lr, neg = signed_length(keys[row, 2]), int(e["length"]), int(e["neg_strand"])
            if La < 1 or La == Lr:
                continue
            B = DNA[3 - int(e["base"]) if neg else int(e["base"])]
            R_ref = forward_right(e["ctx0"], e["ctx1"], k, neg)
            R_alt = forward_right(keys[row, 0], keys[row, 1], k, neg)
            k_eff = k
            if t + 1 < len(tracts) and tract_loc["flat"][t + 1] >= 0 and tract_loc["contig"][t + 1] == loc["contig"]:
                overlap = int(loc["pos"]) + Lr + k - int(tract_loc["pos"][t + 1])
                if overlap > 0:
                    k_eff = max(k - overlap, 0)
            fr, fa = R_ref[:k_eff], R_alt[:k_eff]
            l1 = 0
            while l1 < k_eff and fr[k_eff - 1 - l1] == fa[k_eff - 1 - l1]:
                l1 += 1
            n_flank = k_eff - l1
            REF = B * (max(Lr - La, 0) + 1) + fr[:n_flank]
            ALT = B * (max(La - Lr, 0) + 1) + fa[:n_flank]
            recs.append((int(loc["flat"]), t, s, int(loc["contig"]), int(loc["pos"]) + min(Lr, La), row, DNA.index(B), Lr, La, n_flank, 0,
                         pack(fr[:n_flank]), pack(fa[:n_flank])))
            text.append({"REF": REF, "ALT": ALT, "k_eff": k_eff, "R_alt": R_alt, "R_ref": R_ref, "B": B})
        offsets.append(len(recs))
    return np.array(recs, dtype=VAR), offsets, text


def ref_alt_of(rec):
    """REF and ALT of a record, from its own fields alone"""
    B = DNA[int(rec["base"])]
    Lr, La, nf = int(rec["ref_length"]), int(rec["alt_length"]), int(rec["n_flank"])
    return B * (max(Lr - La, 0) + 1) + unpack(rec["ref_flank"], nf), B * (max(La - Lr, 0) + 1) + unpack(rec["alt_flank"], nf)


VCF_HEADER = ('##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
              '##INFO=<ID=TID,Number=A,Type=String,Description="tract ID">\n')


def vcf_text(names, lengths, sample_name, recs):
    """one sample's VCF as examples/sample_vcfs.c writes it"""
    out = VCF_HEADER + "".join("##contig=<ID=%s,length=%d>\n" % (n, l) for n, l in zip(names, lengths))
    out += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n" % sample_name
    for r in recs:
        REF, ALT = ref_alt_of(r)
        out += "%s\t%d\t.\t%s\t%s\t.\t.\tTID=tid_%06d\tGT\t1\n" % (names[int(r["contig"])], int(r["pos"]), REF, ALT, int(r["tract"]))
    return out


# ---- declarations and argument checks ----------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    code = "".join(re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in ("tatajuba_amd.h", "tatajuba_variants.h"))
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    for s in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % s, code), s
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s in tj.EXPORTS + tj.VARIANT_EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert re.search(r"\}\s*tjamd_variant\s*;", code)
    m = re.search(r"typedef struct \{([^}]*)\}\s*tjamd_variant\s*;", code)
    fields = [w for part in m.group(1).split(";") for w in re.sub(r"^\s*(long long|int|uint64_t)\s", "", part.strip()).replace(" ", "").split(",") if w]
    assert fields == list(VAR.names)                                         # the header's fields, in the header's order
    assert VAR.itemsize == 64
    f = VAR.fields
    assert [f[x][1] for x in VAR.names] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56]
    assert L.tjamd_last_tract_variants_ms(None) == -1.0
    assert hasattr(tj.Counter, "last_tract_variants_ms")


def test_tract_variants_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    off = (C.c_long * 8)()

    def call(c=None, ref=None, keys=fake, counts=fake, n=10, ns=2, tr=fake, nt=3, loc=fake, lst=fake, nl=3, out=fake, cap=10, offsets=off):
        rc = L.tjamd_tract_variants(c, ref, keys, counts, n, ns, tr, nt, loc, lst, nl, out, cap, offsets)
        return rc, L.tjamd_last_error().decode()

    for kw, rc, msg in [({}, ERR_ARG, "null counter or reference"), ({"c": fake}, ERR_ARG, "null counter or reference"), ({"ref": fake}, ERR_ARG, "null counter or reference"),
                        ({"ns": 0}, ERR_ARG, "n_samples 0 outside 1..4096"), ({"ns": 4097}, ERR_ARG, "n_samples 4097 outside 1..4096"),
                        ({"keys": None}, ERR_ARG, "null union buffers"), ({"counts": None}, ERR_ARG, "null union buffers"), ({"n": -1}, ERR_ARG, "n_union -1 < 0"),
                        ({"n": 1 << 31}, ERR_CAP, "union rows"), ({"tr": None}, ERR_ARG, "null tract or tract location buffer"),
                        ({"loc": None}, ERR_ARG, "null tract or tract location buffer"), ({"nt": 0}, ERR_ARG, "n_tracts 0 for a union of 10 rows"),
                        ({"nt": 11}, ERR_ARG, "n_tracts 11 for a union of 10 rows"), ({"nl": -1}, ERR_ARG, "n_list -1 < 0"),
                        ({"cap": -1}, ERR_ARG, "capacity -1"), ({"out": None}, ERR_ARG, "capacity 10 with a null record buffer"),
                        ({"offsets": None}, ERR_ARG, "null offsets"),
                        ({"c": fake, "ref": fake, "n": (1 << 31) - 1, "nt": 1 << 30, "lst": None, "ns": 2}, ERR_CAP, "listed tracts x 2 samples")]:
        got, err = call(**kw)
        assert got == -rc and err.startswith("tjamd_tract_variants") and msg in err, (kw, got, err)
    if tj.device_count() == 0:                     # good arguments, but nothing to run on: named, before the handles are read
        got, err = call(c=fake, ref=fake)
        assert got == -ERR_NO_DEVICE and err.startswith("tjamd_tract_variants") and "TJAMD_ERR_NO_DEVICE" in err, (got, err)


# ---- the rule by hand: k = 4 -------------------------------------------------------------------------------------------
#   contig 0  CAGTAAAGCAGTTTTTCAGCTGAC  (24)   AAA at 4 (left CAGT, right GCAG); TTTTT at 11 (left GCAG, right CAGC): an A
#                                              tract on the other strand, stored as GCTG | CTGC; G at 7 starts right after AAA;
#                                              G at 10 starts k - 1 = 3 bases after it
#   contig 1  GGCACCCCCTGAT             (13)   CCCCC at 4 (left GGCA, right TGAT), flat 28
K = 4
HAND_GENOME = b"CAGTAAAGCAGTTTTTCAGCTGAC\nGGCACCCCCTGAT\n"
#   The rows of the AAA tract (forward text; L = the reference length 3):
#     a0  len 3              a1  len 4              a2  len 2              a3  len 3, right GCAT (equal length: no call)
#     a4  len 4, right TCAG (differs next to the tract)      a5  len 4, right GCAT (differs at the far end)
#     a6  len 4, left GAGT (the left flank is ignored)
#   of the TTTTT tract:  t0 len 5    t1 len 6    t2 len 4, right CATC (differs at j = 2)
#   of the CCCCC tract:  c0 len 5    c1 len 7
#   of an unlocated tract: u0 (some context that is not in the genome)
#   Samples 0-8 pick their modal rows:
#     s0: a1 t1 c1   s1: a2 t2 c0   s2: a3 t0 c0   s3: a4 -- c0   s4: a5 t0 c0   s5: a6 t0 c0
#     s6: a1 and a2 with equal counts (a1 comes first), t0   s7: absent from AAA, t1   s8: a0 (the reference allele), t0
A_ROWS = [("A", "CAGT", "GCAG", 3), ("A", "CAGT", "GCAG", 4), ("A", "CAGT", "GCAG", 2), ("A", "CAGT", "GCAT", 3), ("A", "CAGT", "TCAG", 4),
          ("A", "CAGT", "GCAT", 4), ("A", "GAGT", "GCAG", 4)]
T_ROWS = [("T", "GCAG", "CAGC", 5), ("T", "GCAG", "CAGC", 6), ("T", "GCAG", "CATC", 4)]
C_ROWS = [("C", "GGCA", "TGAT", 5), ("C", "GGCA", "TGAT", 7)]
U_ROWS = [("A", "TTTT", "TTTT", 9)]
G7_ROWS = [("G", "TAAA", "CAGT", 2)]
G10_ROWS = [("G", "AGCA", "TTTT", 1)]
NS = 9
#                  s0 s1 s2 s3 s4 s5 s6 s7 s8
A_MAT = np.array([[1, 1, 1, 0, 0, 0, 1, 0, 9],     # a0
                  [7, 0, 0, 0, 0, 0, 5, 0, 0],     # a1
                  [0, 7, 0, 0, 0, 0, 5, 0, 1],     # a2
                  [0, 0, 7, 0, 0, 0, 0, 0, 0],     # a3
                  [0, 0, 0, 7, 2, 0, 0, 0, 0],     # a4
                  [0, 0, 0, 0, 7, 0, 0, 0, 0],     # a5
                  [0, 0, 0, 0, 0, 7, 0, 0, 0]], np.int32)
T_MAT = np.array([[1, 0, 4, 0, 4, 4, 4, 1, 4],     # t0
                  [6, 0, 0, 0, 0, 0, 0, 3, 0],     # t1
                  [0, 6, 0, 0, 0, 0, 0, 0, 0]], np.int32)
C_MAT = np.array([[2, 5, 5, 5, 5, 5, 0, 0, 0],     # c0
                  [3, 0, 0, 0, 0, 0, 0, 0, 0]], np.int32)
ONES = np.ones((1, NS), np.int32)


def hand_case(which):
    """-> keys, mat, tracts, tract_loc, entries of one of three tilings of the hand genome:
       'plain'  unlocated | AAA@4 | TTTTT@11 | CCCCC@28 (the next tract of AAA starts where its right flank ends; that of TTTTT
                is in another contig, and would cut it to nothing in the same one)
       'next'   AAA@4 | G@7     the next tract starts right after the run: k_eff = 0
       'near'   AAA@4 | G@10    the next tract starts k - 1 bases after the run: k_eff = k - 1 = 3"""
    entries, _ = restate_reference_index(HAND_GENOME, K)
    by_flat = {int(e["flat"]): e for e in entries}
    parts = {"plain": [(None, U_ROWS, ONES), (4, A_ROWS, A_MAT), (11, T_ROWS, T_MAT), (28, C_ROWS, C_MAT)],
             "next": [(4, A_ROWS, A_MAT), (7, G7_ROWS, ONES)], "near": [(4, A_ROWS, A_MAT), (10, G10_ROWS, ONES)]}[which]
    keys, mats, tracts, locs = [], [], [], []
    for flat, rows, m in parts:
        tracts.append((len(keys), len(rows), 1, len(keys), 0, 0, int(m.sum())))
        keys += [canonical_row(*r) for r in rows]
        mats.append(m)
        e = by_flat[flat] if flat is not None else None
        locs.append(NOWHERE if e is None else (int(e["flat"]), int(e["contig"]), int(e["pos"]), int(e["length"]), 0, int(e["neg_strand"]), 1))
    return np.array(keys, np.uint64), np.concatenate(mats), np.array(tracts, TR), np.array(locs, LOC), entries


def calls_of(recs, text):
    return [(int(r["sample"]), int(r["tract"]), int(r["pos"]), t["REF"], t["ALT"], int(r["n_flank"])) for r, t in zip(recs, text)]


# (sample, tract, POS, REF, ALT, n_flank), sample-major, by hand from the comment above
HAND_PLAIN = [
    (0, 1, 7, "A", "AA", 0),          # a1: one A more.  l0 = 3, POS = 4 + 3; flanks agree
    (0, 2, 16, "T", "TT", 0),         # t1: one T more.  POS = 11 + 5
    (0, 3, 9, "C", "CCC", 0),         # c1: two C more.  POS = 4 + 5 in contig 1
    (1, 1, 6, "AA", "A", 0),          # a2: one A less.  l0 = 2, POS = 4 + 2
    (1, 2, 15, "TTCAG", "TCAT", 3),   # t2: one T less and CAGC -> CATC: the difference at j = 2 and everything inside it
    (3, 1, 7, "AG", "AAT", 1),        # a4: GCAG -> TCAG next to the tract: n_flank = 1
    (4, 1, 7, "AGCAG", "AAGCAT", 4),  # a5: GCAG -> GCAT at the far end: n_flank = k
    (5, 1, 7, "A", "AA", 0),          # a6: the left flank differs: ignored
    (6, 1, 7, "A", "AA", 0),          # a1 and a2 tie at 5: the first in union order
    (7, 2, 16, "T", "TT", 0),         # absent from AAA; t1 in TTTTT
]                                     # s2: a3 has the reference length (no call whatever its flank); s8: a0 is the reference allele
HAND_NEXT = [(0, 0, 7, "A", "AA", 0), (0, 1, 8, "G", "GG", 0), (1, 0, 6, "AA", "A", 0), (1, 1, 8, "G", "GG", 0), (2, 1, 8, "G", "GG", 0),
             (3, 0, 7, "A", "AA", 0), (3, 1, 8, "G", "GG", 0), (4, 0, 7, "A", "AA", 0), (4, 1, 8, "G", "GG", 0), (5, 0, 7, "A", "AA", 0),
             (5, 1, 8, "G", "GG", 0), (6, 0, 7, "A", "AA", 0), (6, 1, 8, "G", "GG", 0), (7, 1, 8, "G", "GG", 0), (8, 1, 8, "G", "GG", 0)]
HAND_NEAR = [(0, 0, 7, "A", "AA", 0), (1, 0, 6, "AA", "A", 0), (3, 0, 7, "AG", "AAT", 1),      # k_eff = 3: a4 still differs at j = 0 ...
             (4, 0, 7, "A", "AA", 0), (5, 0, 7, "A", "AA", 0), (6, 0, 7, "A", "AA", 0)]         # ... a5's difference at j = 3 is cut off


def test_the_rule_on_hand_built_cases():
    for which, want in (("plain", HAND_PLAIN), ("next", HAND_NEXT), ("near", HAND_NEAR)):
        keys, mat, tracts, loc, entries = hand_case(which)
        recs, offsets, text = restate_tract_variants(keys, mat, tracts, loc, entries, K)
        assert calls_of(recs, text) == want, which
        assert offsets == [sum(1 for c in want if c[0] < s) for s in range(NS + 1)]
        assert [ref_alt_of(r) for r in recs] == [(t["REF"], t["ALT"]) for t in text]
        assert (recs["pad"] == 0).all()
    keys, mat, tracts, loc, entries = hand_case("plain")
    recs, offsets, text = restate_tract_variants(keys, mat, tracts, loc, entries, K)
    r = recs[4]                                                               # the T tract's deletion, field by field
    assert tuple(r.tolist()) == (11, 2, 1, 0, 15, 7 + 1 + 2, 3, 5, 4, 3, 0, pack("CAG"), pack("CAT"))
    assert [t["k_eff"] for t in text] == [4] * len(text)
    # a list: its order is the order inside a sample, a tract may come twice, the next tract is still the tiling's
    recs2, offsets2, _ = restate_tract_variants(keys, mat, tracts, loc, entries, K, lst=[3, 1, 1])
    assert [(int(x["sample"]), int(x["tract"])) for x in recs2[:3]] == [(0, 3), (0, 1), (0, 1)] and offsets2[1] == 3
    assert restate_tract_variants(keys, mat, tracts, loc, entries, K, lst=[])[1] == [0] * (NS + 1)
    assert [t["k_eff"] for t in restate_tract_variants(*hand_case("next")[:4], entries, K)[2]][:2] == [0, 4]
    # an entry that the location does not name: no call
    gone = entries[entries["flat"] != 4]
    assert all(int(x["tract"]) != 1 for x in restate_tract_variants(keys, mat, tracts, loc, gone, K)[0])
    assert common_prefix_suffix("AAAGCAG", "AAAAGCAT") == (3, 0) and common_prefix_suffix("TTTTTCAGC", "TTTTCATC") == (4, 1)
    assert common_prefix_suffix("AAA", "AAAA") == (3, 0) and common_prefix_suffix("AAAGC", "AAGC") == (2, 2)


# ---- planted corpora: a genome's own runs as tracts, each sample with a planted length and sometimes a planted mismatch ----

def fold(stream):
    return bytes(stream).decode("latin-1").translate(_FOLD)


def planted_union(stream, k, ns, rng, max_sites=400, big_site=True):
    """Sites = index entries whose context occurs once in the genome (so tjamd_locate's rule places their rows there),
    visited in a shuffled order; a site's rows are its own context with lengths Lr, Lr +- 1..3 (1..70 on the first site, one
    row in all on the second), some
    with one substitution in the right or in the left flank that keeps the run maximal and still lands on the site at one
    mismatch.  Each sample is absent from a site or has one modal row (count 9) and sometimes a lesser one (count 2).
    -> dict: keys, mat, tracts (one per site, input order), entries, sites [(entry index, {sample: (La, j or None, R_alt)})]"""
    entries, _ = restate_reference_index(stream, k)
    ctx = list(zip(entries["base"].tolist(), entries["ctx0"].tolist(), entries["ctx1"].tolist()))
    seen = {}
    for c in ctx:
        seen[c] = seen.get(c, 0) + 1
    unique = [i for i, c in enumerate(ctx) if seen[c] == 1 and entries["length"][i] < 400]
    rng.shuffle(unique)
    unique = unique[:max_sites]
    keys, cols, tracts, sites = [], [], [], []
    for n_site, i in enumerate(unique):
        e = entries[i]
        neg, Lr = int(e["neg_strand"]), int(e["length"])
        B = DNA[3 - int(e["base"]) if neg else int(e["base"])]
        R = forward_right(e["ctx0"], e["ctx1"], k, neg)
        Lf = revcomp(unpack(e["ctx1"], k)) if neg else unpack(e["ctx0"], k)
        rows, planted = {}, {}                                                # (La, left, right) -> {sample: count}

        def mutated(text, j):
            others = [x for x in DNA if x != text[j] and x != B]              # (never the tract's base: the run stays maximal)
            return text[:j] + rng.choice(others) + text[j + 1:]
        lengths = list(range(1, 71)) if (big_site and n_site == 0) else [Lr] * 3 + [max(1, Lr + d) for d in (-3, -2, -1, 1, 2, 3)]
        one_row = big_site and n_site == 1                                    # a tract of one row: every sample has the same allele
        for s in range(ns):
            if one_row:
                rows.setdefault((Lr + 1, Lf, R), {})[s] = 9
                planted[s] = (Lr + 1, None, R)
                continue
            if rng.random() < 0.15 and not (big_site and n_site == 0):
                continue                                                      # absent
            La = lengths[s % len(lengths)] if (big_site and n_site == 0) else rng.choice(lengths)
            left, right, j = Lf, R, None
            r = rng.random()
            if r < 0.3:
                j = rng.randrange(k)
                right = mutated(R, j)
            elif r < 0.4:
                left = mutated(Lf, rng.randrange(k))
            q = restate_locate(entries, [list(canonical_row(B, left, right, La))], 1)[0]
            if q["flat"] != e["flat"]:                                        # the mutated context sits better elsewhere: plant none
                left, right, j = Lf, R, None
            rows.setdefault((La, left, right), {})[s] = 9
            if rng.random() < 0.3:                                            # a lesser row beside the modal one
                rows.setdefault((max(1, La + 1), Lf, R), {}).setdefault(s, 2)
            planted[s] = (La, j, right)
        if big_site and n_site == 0:
            for La in lengths:                                                # more than 64 rows in this tract
                rows.setdefault((La, Lf, R), {})
        if not rows:
            rows[(Lr, Lf, R)] = {}
        order = sorted(rows, key=lambda x: (x[1], x[2], x[0]))                # rows of one context side by side
        tracts.append((len(keys), len(order), 1, len(keys), 0, 0, 0))
        for key in order:
            keys.append(canonical_row(B, key[1], key[2], key[0]))
            col = np.zeros(ns, np.int32)
            for s, n in rows[key].items():
                col[s] = n
            cols.append(col)
        sites.append((i, planted))
    return {"keys": np.array(keys, np.uint64).reshape(-1, 3), "mat": np.array(cols, np.int32).reshape(-1, ns), "tracts": np.array(tracts, TR),
            "entries": entries, "sites": sites}


def expected_calls(stream, k, p):
    """what was planted, from the genome's text: {(sample, flat): (contig, POS, REF, ALT)} for every (site, sample) with
    La != Lr.  The next tract is the next site of the contig."""
    text = [fold(c) for c in bytes(stream).split(b"\n")]
    entries = p["entries"]
    by_flat = sorted((int(entries["flat"][i]), i) for i, _ in p["sites"])
    nxt = {}
    for (f0, i0), (f1, i1) in zip(by_flat, by_flat[1:]):
        if entries["contig"][i0] == entries["contig"][i1]:
            nxt[i0] = int(entries["pos"][i1])
    want = {}
    for i, planted in p["sites"]:
        e = entries[i]
        g, pos, Lr = text[int(e["contig"])], int(e["pos"]), int(e["length"])
        B = g[pos]
        k_eff = k if i not in nxt else max(0, min(k, nxt[i] - pos - Lr))
        for s, (La, j, right) in planted.items():
            if La == Lr:
                continue
            nf = j + 1 if (j is not None and j < k_eff) else 0
            want[(s, int(e["flat"]))] = (int(e["contig"]), pos + min(La, Lr), B * (max(Lr - La, 0) + 1) + g[pos + Lr: pos + Lr + nf],
                                         B * (max(La - Lr, 0) + 1) + right[:nf])
    return want


def locate_and_tile(p):
    """the restatements of tjamd_locate (1 mismatch) and tjamd_located_tracts on a planted union -> permuted keys, mat, tiling, locations"""
    from tests.test_locate_cabi import restate_located_tracts
    loc = restate_locate(p["entries"], p["keys"], 1)
    lt = restate_located_tracts(p["keys"], p["mat"], p["tracts"], loc)
    return p["keys"][lt["perm"]], p["mat"][lt["perm"]], lt["tracts"], lt["tract_loc"]


def small_genome(rng, k, n_contigs=3, total=2400):
    """contigs of short random stretches and homopolymers, some lowercase: dense enough that neighbours cut each other's flank"""
    out = []
    for _ in range(n_contigs):
        s = []
        while sum(map(len, s)) < total // n_contigs:
            s.append(rng.choice(DNA) * rng.randrange(2, 9) if rng.random() < 0.2 else "".join(rng.choice(DNA) for _ in range(rng.randrange(1, 12))))
            if rng.random() < 0.1:
                s[-1] = s[-1].lower()
        out.append("".join(s))
    return ("\n".join(out) + "\n").encode()


def apply_it(stream, k, recs, text):
    """every call: the contig spells REF at POS - 1, and with ALT in its place the tract has La bases followed by R_alt[:k_eff]"""
    contigs = [fold(c) for c in bytes(stream).split(b"\n")]
    for r, t in zip(recs, text):
        g = contigs[int(r["contig"])]
        REF, ALT = ref_alt_of(r)
        at = int(r["pos"]) - 1
        assert g[at: at + len(REF)] == REF, (r, REF)
        new = g[:at] + ALT + g[at + len(REF):]
        start = int(r["pos"]) - min(int(r["ref_length"]), int(r["alt_length"]))      # the tract's first base
        La = int(r["alt_length"])
        assert new[start: start + La] == t["B"] * La and new[start - 1] != t["B"]
        assert new[start + La: start + La + t["k_eff"]] == t["R_alt"][: t["k_eff"]], (r, t)


@pytest.mark.parametrize("k,ns,seed", [(2, 3, 1), (5, 8, 2), (15, 5, 3), (32, 4, 4)])
def test_every_call_applied_to_the_genome_gives_the_samples_allele(k, ns, seed):
    rng = random.Random(seed)
    stream = small_genome(rng, k, total=500 if k == 2 else 2400)
    p = planted_union(stream, k, ns, rng)
    keys, mat, tracts, loc = locate_and_tile(p)
    recs, offsets, text = restate_tract_variants(keys, mat, tracts, loc, p["entries"], k)
    assert len(recs) > 20 and offsets[-1] == len(recs) and len(set(recs["contig"].tolist())) == 3
    apply_it(stream, k, recs, text)
    want = expected_calls(stream, k, p)
    got = {(int(r["sample"]), int(r["flat"])): (int(r["contig"]), int(r["pos"])) + ref_alt_of(r) for r in recs}
    assert got == want                                                        # every planted difference is called, and nothing else
    assert any(t["k_eff"] < k for t in text) and (recs["base"] >= 2).any() and (recs["base"] < 2).any()
    assert k == 2 or (recs["n_flank"] > 0).any()      # (at k = 2 nearly every mutated context occurs elsewhere in the genome and is not planted)
    assert (recs["alt_length"] > recs["ref_length"]).any() and (recs["alt_length"] < recs["ref_length"]).any()
    # the reference's own reading, on strings: prefix, then suffix of what it leaves, from the last common base on
    for r, t in zip(recs, text):
        ref_s = t["B"] * int(r["ref_length"]) + t["R_ref"][: t["k_eff"]]
        alt_s = t["B"] * int(r["alt_length"]) + t["R_alt"][: t["k_eff"]]
        l0, l1 = common_prefix_suffix(ref_s, alt_s)
        assert l0 == min(int(r["ref_length"]), int(r["alt_length"])) and l0 > 0
        assert (ref_s[l0 - 1: len(ref_s) - l1], alt_s[l0 - 1: len(alt_s) - l1]) == (t["REF"], t["ALT"])


# ---- contig names ------------------------------------------------------------------------------------------------------

def names_in_python(data):
    """record names of FASTA / FASTQ text whose sequences and qualities hold no '>' or '@': the header after the marker up
    to the first space or tab"""
    out = []
    for line in data.split(b"\n"):
        if line[:1] in (b">", b"@"):
            out.append(re.split(rb"[ \t]", line[1:].rstrip(b"\r"), maxsplit=1)[0])
    return out


def read_names(path):
    L = tj.lib()
    n = C.c_long(-1)
    need = L.tjamd_read_file_names(os.fsencode(path), None, 0, C.byref(n))
    if need < 0:
        return None, -1
    out = GuardedHost(need)
    n2 = C.c_long(-1)
    assert L.tjamd_read_file_names(os.fsencode(path), out.c, need, C.byref(n2)) == need and n2.value == n.value
    out.check("names")
    short = GuardedHost(max(need - 1, 0))
    if need:
        assert L.tjamd_read_file_names(os.fsencode(path), short.c, need - 1, None) == need      # one byte short: sized, not overrun
        short.check("names, one byte short")
    data = bytes(out.payload)
    assert data.count(b"\n") == n.value and (not data or data.endswith(b"\n"))
    return data.split(b"\n")[:-1], n.value


def test_read_file_names(tmp_path):
    fasta = (b">chr1 some text\nACGTACGT\nACGT\n>chr2\tand a tab\nGGGG\n>\nAC\n> only a comment\nTT\n>plain\nACGTNN\n>last_without_newline\nACGT")
    fastq = b"".join(b"@read%d/1 len=%d\n%s\n+\n%s\n" % (i, 4 + i, b"ACGT" + b"A" * i, b"I" * (4 + i)) for i in range(50)) + b"@tail\tx\nAC\n+\nII"
    cases = {"ref.fa": fasta, "reads.fq": fastq, "empty.fa": b"", "crlf.fa": b">a b\r\nAC\r\n>cc\r\nGT\r\n"}
    for name, data in cases.items():
        for gz in (False, True):
            path = str(tmp_path / (name + (".gz" if gz else "")))
            with (gzip.open(path, "wb") if gz else open(path, "wb")) as fh:
                fh.write(data)
            got, n = read_names(path)
            assert got == names_in_python(data) and n == len(got), (name, gz, got)
            _, n_reads = tj.read_file_stream(path)
            assert n == n_reads, (name, gz)
    assert names_in_python(fasta) == [b"chr1", b"chr2", b"", b"", b"plain", b"last_without_newline"]
    # it stops where tjamd_read_file_stream stops: a FASTQ record whose quality string is short ends the file
    path = str(tmp_path / "cut.fq")
    with open(path, "wb") as fh:
        fh.write(b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\nII\n@c\nACGT\n+\nIIII\n")
    got, n = read_names(path)
    assert n == tj.read_file_stream(path)[1] and got == [b"a", b"b", b"c"][:n]
    assert read_names(str(tmp_path / "missing.fa")) == (None, -1)
