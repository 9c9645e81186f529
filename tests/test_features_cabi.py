"""The annotation step (include/tatajuba_features.h) without a GPU: the entries are declared, exported and prototyped and
refuse bad arguments before any device call, the records match the header, tjamd_gff3_read parses files written here, and
the restatements that the GPU tests (tests/test_features.py) compare against agree with each other: the elementary-interval
table as it is built, read by one binary search, gives the brute-force rule on random feature sets with no difference.

restate_winner is the rule of the header as a loop in file order; restate_table builds the points and the winner of every
index the way the header says the device does; restate_tract_features joins both with the longest modal length."""
import bisect
import ctypes as C
import fnmatch
import gzip
import os
import random
import re

import numpy as np

import tatajuba_amd as tj
from tests.guarded import GuardedHost
from tests.test_variants_cabi import signed_length

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_gff3_read", "tjamd_annotation_create", "tjamd_annotation_destroy", "tjamd_annotation_features", "tjamd_annotation_download",
               "tjamd_tract_features", "tjamd_last_annotation_ms", "tjamd_last_tract_features_ms"]
ERR_NO_DEVICE, ERR_ARG, ERR_CAP = 1, 3, 4
FT, TF = tj.FEATURE_DTYPE, tj.TRACT_FEATURE_DTYPE
REGION, CDS, OTHER = 0, 1, 2


def features_of(rows):
    """(contig, start, end, cls) tuples -> a FEATURE_DTYPE array (line = file index + 1, no strings)"""
    f = np.zeros(len(rows), FT)
    for i, (contig, start, end, cls) in enumerate(rows):
        f[i] = (contig, start, end, cls, 2, i + 1, 0, 0)
    return f


# ---- the restatements --------------------------------------------------------------------------------------------------

def restate_winner(features, contig, pos):
    """the rule: the first CDS that contains 1-based pos + 1 of the contig, else the last feature that is not a region"""
    last = -1
    for i, f in enumerate(features):
        if int(f["cls"]) == REGION or int(f["contig"]) != contig or not int(f["start"]) <= pos + 1 <= int(f["end"]):
            continue
        if int(f["cls"]) == CDS:
            return i
        last = i
    return last


def restate_winners(features, places):
    """restate_winner for many (contig, pos) places: numpy over the features, the same rule (checked against the loop below)"""
    f, idx, out = features, np.arange(len(features)), []
    for contig, pos in places:
        m = (f["cls"] != REGION) & (f["contig"] == contig) & (f["start"].astype(np.int64) <= pos + 1) & (pos + 1 <= f["end"].astype(np.int64))
        cds, other = idx[m & (f["cls"] == CDS)], idx[m]
        out.append(int(cds[0]) if len(cds) else int(other[-1]) if len(other) else -1)
    return np.array(out, np.int32)


def restate_table(features):
    """-> (points ascending with duplicates, winner per index): every feature that is not a region takes, on the indices
    [lower_bound (start point), lower_bound (end + 1 point)), the maximum of its priority"""
    pts = []
    for f in features:
        if int(f["cls"]) != REGION:
            pts += [(int(f["contig"]) << 32) | int(f["start"]), (int(f["contig"]) << 32) | (int(f["end"]) + 1)]
    pts.sort()
    prio = [0] * len(pts)
    for i, f in enumerate(features):
        if int(f["cls"]) == REGION:
            continue
        lo = bisect.bisect_left(pts, (int(f["contig"]) << 32) | int(f["start"]))
        hi = bisect.bisect_left(pts, (int(f["contig"]) << 32) | (int(f["end"]) + 1))
        p = (1 << 31) | (0x7fffffff - i) if int(f["cls"]) == CDS else i + 1
        for e in range(lo, hi):
            prio[e] = max(prio[e], p)
    winner = [-1 if not p else 0x7fffffff - (p & 0x7fffffff) if p >> 31 else p - 1 for p in prio]
    return np.array(pts, np.uint64), np.array(winner, np.int32)


def table_lookup(points, winner, contig, pos):
    e = bisect.bisect_right(points, (contig << 32) | (pos + 1)) - 1
    return -1 if e < 0 else int(winner[e])


def restate_tract_features(features, keys, mat, tracts, tract_loc):
    """-> TRACT_FEATURE_DTYPE per tract; keys / mat None: max_length 0"""
    out = np.zeros(len(tract_loc), TF)
    if keys is not None:
        keys = np.asarray(keys, np.uint64).reshape(-1, 3)
    out["feature"] = restate_winners(features, [(int(l["contig"]), int(l["pos"])) for l in tract_loc])
    out["feature"][np.asarray(tract_loc["flat"]) < 0] = -1
    for t in range(len(tract_loc)):
        if keys is None or mat is None:
            continue
        first, n_rows = int(tracts["first"][t]), int(tracts["n_rows"][t])
        lengths = []
        for s in range(mat.shape[1]):
            col = mat[first: first + n_rows, s]
            if col.max() > 0:
                lengths.append(signed_length(keys[first + int(np.argmax(col)), 2]))      # the first of equal counts
        out["max_length"][t] = max(lengths) if lengths else 0
    return out


def name_of_tract(ctx0, ctx1, base, k, neg_strand):
    """generate_name_from_flanking_contexts: left.B.right, the whole reverse-complemented for a tract on the negative strand"""
    dna = "ACGT"
    left = "".join(dna[(int(ctx0) >> (2 * i)) & 3] for i in range(k))
    right = "".join(dna[(int(ctx1) >> (2 * i)) & 3] for i in range(k))
    if not neg_strand:
        return f"{left}.{dna[int(base)]}.{right}"
    rc = lambda x: x.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    return f"{rc(right)}.{dna[3 - int(base)]}.{rc(left)}"


def random_features(rng, n, n_contigs, contig_len):
    """lengths log-uniform from 1 to the contig's length, a quarter regions, a quarter CDS"""
    rows = []
    for _ in range(n):
        length = min(contig_len, int(round(contig_len ** rng.random())))
        start = rng.randint(1, contig_len - length + 1)
        rows.append((rng.randrange(n_contigs), start, start + length - 1, rng.choice([REGION, CDS, OTHER, OTHER])))
    return features_of(rows)


def places_for(rng, features, n_contigs, contig_len, n_random):
    """(contig, 0-based pos): every endpoint and its two neighbours, and random places"""
    places = set()
    for f in features:
        for x in (int(f["start"]), int(f["end"])):
            places.update((int(f["contig"]), x - 1 + d) for d in (-1, 0, 1) if 0 <= x - 1 + d)
    places.update((rng.randrange(n_contigs), rng.randrange(contig_len)) for _ in range(n_random))
    return sorted(places)


def test_the_table_is_the_rule_on_random_feature_sets():
    rng = random.Random(9)
    queries = differences = 0
    for trial in range(200):
        n_contigs, contig_len = (1, 40) if trial % 2 else (3, 3000)
        feats = random_features(rng, rng.choice([0, 1, 2, 5, 20, 80, 300]), n_contigs, contig_len)
        points, winner = restate_table(feats)
        pts = [int(x) for x in points]
        assert pts == sorted(pts) and len(pts) == 2 * int((feats["cls"] != REGION).sum())
        places = [(c, p) for c in range(n_contigs) for p in range(contig_len + 2)] if contig_len <= 40 else places_for(rng, feats, n_contigs, contig_len, 400)
        many = restate_winners(feats, places)
        for (c, p), w in zip(places, many):
            queries += 1
            differences += table_lookup(pts, winner, c, p) != restate_winner(feats, c, p) or int(w) != restate_winner(feats, c, p)
    assert queries > 50000 and differences == 0, (queries, differences)


def test_the_rule_on_hand_cases():
    gene, mrna, exon, cds = (0, 10, 50, OTHER), (0, 10, 50, OTHER), (0, 20, 30, OTHER), (0, 22, 28, CDS)
    for rows in ([gene, mrna, exon, cds], [cds, exon, mrna, gene]):
        f = features_of(rows)
        assert restate_winner(f, 0, 24) == rows.index(cds)                   # the CDS wins in either order
        assert restate_winner(f, 0, 20) == (2 if rows[0] == gene else 3)     # exon last / gene last
        assert restate_winner(f, 0, 50) == -1 and restate_winner(f, 0, 49) in (1, 3) and restate_winner(f, 1, 24) == -1
    two = features_of([(0, 5, 20, CDS), (0, 10, 30, CDS), (0, 1, 60, REGION)])
    assert [restate_winner(two, 0, p) for p in (3, 4, 12, 19, 20, 29, 30)] == [-1, 0, 0, 0, 1, 1, -1]
    pts, win = restate_table(two)
    assert pts.tolist() == [5, 10, 21, 31] and win.tolist() == [0, 0, 1, -1]


def test_the_name_restatement_is_the_library_function():
    L, rng = tj.lib(), random.Random(3)
    for k in (2, 5, 15, 32):
        for _ in range(20):
            ctx = (C.c_uint64 * 2)(rng.getrandbits(2 * k), rng.getrandbits(2 * k))
            base, neg = rng.randrange(4), rng.random() < 0.5
            p = L.generate_name_from_flanking_contexts(ctx, base, k, neg)
            assert C.string_at(p).decode() == name_of_tract(ctx[0], ctx[1], base, k, neg)
            C.CDLL(None).free(C.c_void_p(p))


# ---- declarations and argument checks ----------------------------------------------------------------------------------

def _fields(code, name):
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s\s*;" % name, code)
    return [w for part in m.group(1).split(";") for w in re.sub(r"^\s*(long long|int|uint64_t)\s", "", part.strip()).replace(" ", "").split(",") if w]


def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    own = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tatajuba_features.h")).read(), flags=re.S)
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read(), flags=re.S)
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.FEATURE_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    for s in NEW_ENTRIES:
        assert not re.search(r"\b%s\s*\(" % s, base), s                      # ... and tatajuba_amd.h none of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in tj.EXPORTS and s not in tj.VARIANT_EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert "tatajuba_features.h" in open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read()
    assert _fields(own, "tjamd_feature") == list(FT.names) and _fields(own, "tjamd_tract_feature") == list(TF.names)
    assert FT.itemsize == 32 and [FT.fields[x][1] for x in FT.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert TF.itemsize == 8 and [TF.fields[x][1] for x in TF.names] == [0, 4]
    assert re.search(r"TJAMD_FEATURE_REGION = 0, TJAMD_FEATURE_CDS = 1, TJAMD_FEATURE_OTHER = 2", own)
    assert L.tjamd_last_annotation_ms(None) == -1.0 and L.tjamd_last_tract_features_ms(None) == -1.0
    assert L.tjamd_annotation_features(None) == -1
    L.tjamd_annotation_destroy(None)
    for name in ("last_annotation_ms", "last_tract_features_ms"):
        assert hasattr(tj.Counter, name)
    assert all(hasattr(tj.Annotation, x) for x in ("download", "close", "n_features"))


def test_entries_check_their_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first

    def call(c=None, a=None, keys=fake, counts=fake, n=10, ns=2, tr=fake, nt=3, loc=fake, out=fake):
        rc = L.tjamd_tract_features(c, a, keys, counts, n, ns, tr, nt, loc, out)
        return rc, L.tjamd_last_error().decode()

    for kw, rc, msg in [({}, ERR_ARG, "null counter or annotation"), ({"a": fake}, ERR_ARG, "null counter or annotation"),
                        ({"ns": 0}, ERR_ARG, "n_samples 0 outside 1..4096"), ({"ns": 4097}, ERR_ARG, "n_samples 4097 outside 1..4096"),
                        ({"n": -1}, ERR_ARG, "n_union -1 < 0"), ({"n": 1 << 31}, ERR_CAP, "union rows"),
                        ({"tr": None}, ERR_ARG, "null tract buffer"), ({"loc": None}, ERR_ARG, "null tract location or output buffer"),
                        ({"out": None}, ERR_ARG, "null tract location or output buffer"),
                        ({"nt": 0}, ERR_ARG, "n_tracts 0 for a union of 10 rows"), ({"nt": 11}, ERR_ARG, "n_tracts 11 for a union of 10 rows"),
                        # without a union n_union, n_samples and d_tracts are not looked at
                        ({"keys": None, "ns": 0, "n": -1, "tr": None}, ERR_ARG, "null counter or annotation"),
                        ({"counts": None, "ns": 9999, "nt": 100}, ERR_ARG, "null counter or annotation"),
                        ({"keys": None, "nt": -1}, ERR_ARG, "n_tracts -1 < 0"), ({"keys": None, "nt": 1 << 31}, ERR_CAP, "tracts")]:
        got, err = call(**kw)
        assert got == -rc and err.startswith("tjamd_tract_features") and msg in err, (kw, got, err)
    one = features_of([(0, 1, 2, OTHER)])
    for c, ref, f, n, msg in [(None, fake, one, 1, "null counter or reference"), (None, fake, None, 1, "null counter or reference")]:
        h = L.tjamd_annotation_create(c, ref, f.ctypes.data if f is not None else None, n)
        err = L.tjamd_last_error().decode()
        assert not h and err.startswith("tjamd_annotation_create") and msg in err, (n, err)
    assert L.tjamd_annotation_download(None, None, None, 0) == -ERR_ARG and L.tjamd_last_error().decode().startswith("tjamd_annotation_download")
    if tj.device_count() == 0:                     # a counter cannot exist: the pointers below stand for one and are never read
        got, err = call(c=fake)
        assert got == -ERR_ARG and "null counter or annotation" in err
        for c, ref, f, n, msg in [(fake, None, one, 1, "null counter or reference"), (fake, fake, None, 1, "1 features with a null buffer"),
                                  (fake, fake, one, -1, "-1 features"), (fake, fake, one, (1 << 30) + 1, "more than 2^30")]:
            h = L.tjamd_annotation_create(c, ref, f.ctypes.data if f is not None else None, n)
            err = L.tjamd_last_error().decode()
            assert not h and err.startswith("tjamd_annotation_create") and msg in err, (n, err)
        # good arguments, but nothing to run on: named, before the handles are read
        got, err = call(c=fake, a=fake)
        assert got == -ERR_NO_DEVICE and err.startswith("tjamd_tract_features") and "TJAMD_ERR_NO_DEVICE" in err, (got, err)
        h = L.tjamd_annotation_create(fake, fake, one.ctypes.data, 1)
        err = L.tjamd_last_error().decode()
        assert not h and err.startswith("tjamd_annotation_create") and "TJAMD_ERR_NO_DEVICE" in err


# ---- tjamd_gff3_read ---------------------------------------------------------------------------------------------------

NAMES = ["chr1", "chr10", "ctg|2 x"]


def gff_line(seqid="chr1", typ="gene", start=1, end=9, strand="+", attr="ID=a", cols=9):
    return "\t".join([seqid, "src", typ, str(start), str(end), ".", strand, ".", attr][:cols])


GFF_LINES = [
    "##gff-version 3",                                                       # 1
    "#a comment",                                                            # 2
    gff_line("chr1", "region", 1, 5000, "+", "ID=chr1:1..5000;Dbxref=taxon:1"),        # 3   feature 0
    "",                                                                      # 4
    gff_line("chr1", "gene", 10, 500, "+", "ID=gene-A;Name=thrA"),           # 5   feature 1: ID first
    gff_line("chr1", "CDS", 10, 500, "-", "Parent=gene-A;ID=cds-A;product=x%3By") + "\r",     # 6   feature 2: ID in the middle, CRLF, escapes kept
    gff_line("chr10", "cds", 7, 7, ".", "Parent=gene-B;Note=n;ID=cds-B"),    # 7   feature 3: ID last, lower case, the longer name
    gff_line("chr1", "Region", 1, 2, "?", "Name=noid"),                      # 8   feature 4: no ID, a region in another case
    gff_line("chr2", "gene", 1, 2),                                          # 9   skipped: not among the names
    gff_line("chr", "gene", 1, 2),                                           # 10  skipped: a prefix of a name is not the name
    gff_line("chr1", "gene", 1, 2, cols=8),                                  # 11  skipped: eight columns
    gff_line("chr1", "gene", 0, 2),                                          # 12  skipped: start 0
    gff_line("chr1", "gene", 5, 4),                                          # 13  skipped: end < start
    gff_line("chr1", "gene", "1e3", 2000),                                   # 14  skipped: not a number
    gff_line("chr1", "gene", 5, "9x"),                                       # 15  skipped
    gff_line("chr1", "gene", 5, ""),                                         # 16  skipped
    gff_line("ctg|2 x", "mRNA", 3, 2147483647, "+", "Parent=xID=no;Note=ID=no"),       # 17  feature 5: ID= inside other values does not count
    gff_line("chr1", "exon", 5, 6, "+-", "Note=a;ID=;Name=b"),               # 18  feature 6: an empty ID, a strand of two bytes
    gff_line("chr1", "CDS_part", 5, 6, "+", "Parent=p;ID=last-one"),         # 19  feature 7: not a CDS by name
]
WANT = [  # contig, start, end, cls, strand, line, type, id
    (0, 1, 5000, REGION, 0, 3, "region", "chr1:1..5000"), (0, 10, 500, OTHER, 0, 5, "gene", "gene-A"), (0, 10, 500, CDS, 1, 6, "CDS", "cds-A"),
    (1, 7, 7, CDS, 2, 7, "cds", "cds-B"), (0, 1, 2, REGION, 2, 8, "Region", ""), (2, 3, 2147483647, OTHER, 0, 17, "mRNA", ""),
    (0, 5, 6, OTHER, 2, 18, "exon", ""), (0, 5, 6, OTHER, 0, 19, "CDS_part", "last-one")]
N_SKIPPED = 8


def check_features(feats, strings, want):
    assert len(feats) == len(want)
    at = 0
    for f, w in zip(feats, want):
        assert tuple(int(f[x]) for x in ("contig", "start", "end", "cls", "strand", "line")) == w[:6], (f, w)
        assert tj.gff3_string(strings, int(f["type_off"])) == w[6] and tj.gff3_string(strings, int(f["id_off"])) == w[7], (f, w)
        assert int(f["type_off"]) == at and int(f["id_off"]) == at + len(w[6]) + 1      # the strings lie back to back, in file order
        at += len(w[6]) + len(w[7]) + 2
    assert len(strings) == at


def test_gff3_read_plain_gzip_and_line_rules(tmp_path):
    text = "\n".join(GFF_LINES)                                               # (the last line has no newline)
    plain, gz, multi = tmp_path / "a.gff3", tmp_path / "a.gff3.gz", tmp_path / "m.gff3.gz"
    plain.write_bytes(text.encode())
    with gzip.open(gz, "wb") as fh:
        fh.write(text.encode())
    half = text.index("\n", len(text) // 2) + 1
    multi.write_bytes(gzip.compress(text[:half].encode()) + gzip.compress(b"") + gzip.compress(text[half:].encode(), 1))      # members, as BGZF has them
    got = [tj.read_gff3(str(p), NAMES) + (tj.read_gff3.last_skipped,) for p in (plain, gz, multi)]
    for feats, strings, skipped in got:
        check_features(feats, strings, WANT)
        assert skipped == N_SKIPPED
        assert feats.tobytes() == got[0][0].tobytes() and strings == got[0][1]
    # with a newline at the end: the same
    plain.write_bytes((text + "\n").encode())
    feats, strings = tj.read_gff3(str(plain), NAMES)
    assert feats.tobytes() == got[0][0].tobytes() and strings == got[0][1]
    # ##FASTA and a bare '>' both end the features; what follows is not read, not even counted as skipped
    for stop in ("##FASTA\n>chr1\nACGT\n", ">chr1\nACGT\n"):
        plain.write_bytes(("\n".join(GFF_LINES[:6]) + "\n" + stop + "\n".join(GFF_LINES[6:]) + "\n").encode())
        feats, strings = tj.read_gff3(str(plain), NAMES)
        check_features(feats, strings, WANT[:3])
        assert tj.read_gff3.last_skipped == 0
    # no names: everything is skipped; an empty file: nothing
    plain.write_bytes(text.encode())
    feats, strings = tj.read_gff3(str(plain), [])
    assert len(feats) == 0 and strings == b"" and tj.read_gff3.last_skipped == len(WANT) + N_SKIPPED
    plain.write_bytes(b"")
    feats, strings = tj.read_gff3(str(plain), NAMES)
    assert len(feats) == 0 and strings == b"" and tj.read_gff3.last_skipped == 0
    # a damaged gzip file is refused like a missing one
    z = bytearray(gz.read_bytes())
    z[-6] ^= 0x40                                                            # (in the CRC-32)
    (tmp_path / "bad.gz").write_bytes(bytes(z))
    assert tj.lib().tjamd_gff3_read(os.fsencode(str(tmp_path / "bad.gz")), b"chr1\n", 1, None, 0, None, 0, None, None) == -1


def test_gff3_read_sizing_and_capacities(tmp_path):
    L = tj.lib()
    path = tmp_path / "a.gff3"
    path.write_bytes("\n".join(GFF_LINES).encode())
    blob = "".join(n + "\n" for n in NAMES).encode()
    n, need = len(WANT), sum(len(w[6]) + len(w[7]) + 2 for w in WANT)
    nb, sk = C.c_long(-1), C.c_long(-1)

    def call(out, cap, strings, scap):
        nb.value = sk.value = -1
        return L.tjamd_gff3_read(os.fsencode(str(path)), blob, len(NAMES), out.c if out else None, cap, strings.c if strings else None, scap, C.byref(nb), C.byref(sk))

    out, strings = GuardedHost(n * FT.itemsize), GuardedHost(need)
    # sizing: no records buffer, no strings buffer, neither
    for o, s in ((None, None), (out, None), (None, strings)):
        assert call(o, n, s, need) == n and (nb.value, sk.value) == (need, N_SKIPPED)
        assert out.untouched() and strings.untouched()
    # one short on either side: the sizes come back and nothing is written
    for cap, scap in ((n - 1, need), (n, need - 1), (0, 0)):
        assert call(out, cap, strings, scap) == n and (nb.value, sk.value) == (need, N_SKIPPED)
        assert out.untouched() and strings.untouched()
    assert call(out, n, strings, need) == n
    out.check("out"); strings.check("strings")
    check_features(out.view(FT), strings.view(np.uint8).tobytes(), WANT)
    # the counters may be NULL; a missing file
    assert L.tjamd_gff3_read(os.fsencode(str(path)), blob, len(NAMES), None, 0, None, 0, None, None) == n
    assert L.tjamd_gff3_read(os.fsencode(str(tmp_path / "none.gff3")), blob, len(NAMES), None, 0, None, 0, C.byref(nb), C.byref(sk)) == -1
    try:
        tj.read_gff3(str(tmp_path / "none.gff3"), NAMES)
        assert False
    except FileNotFoundError:
        pass
