"""tjamd_coding_create / tjamd_coding_download / tjamd_variant_effects on the GPU against the string restatement of
tests/test_effects_cabi.py: a hand genome, the wavefront-step edges of the CDS scan, edits of every kind on both strands, record
counts around the wavefront and the block, device refusals, repeatability, the eight-sample pipeline of tests/test_locate.py
with the features of tests/test_features.py, and examples/variant_effects.c.  Outputs always sit in guarded buffers
(tests/guarded.py), const inputs are held frozen, every call is made twice and must give the same bytes; records are compared
with the restatement field by field, then byte for byte."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests.guarded import GuardedDevice, GuardedHost, frozen
from tests.test_effects_cabi import (ALT_STOP, BAD_FEATURES, BOUNDARY, CDS, CODON_AA, DNA, EF, EFFECTS_HEADER, FRAMESHIFT, FT, IDENTICAL, INFRAME, NONE, OTHER,
                                     REF_STOP, REGION, TF, VAR, CD, effects_tsv_line, one_feature, restate_cds, restate_effects, revcomp, unpack8, variant_of)
from tests.test_features import dev_tract_features, gff3_of
from tests.test_locate import _dev, _p, dev_locate, dev_located_tracts
from tests.test_locate_cabi import contigs_of, restate_locate, restate_located_tracts, restate_reference_index
from tests.test_features_cabi import restate_tract_features
from tests.test_union_tracts import _oracle_sample, device_union, make_genome, reads_of, sample_of
from tests.test_union_tracts_cabi import oracle_union_grouping, restate_union_tract_stats
from tests.test_variants import Tiling, dev_variants
from tests.test_variants_cabi import restate_tract_variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 3
TR = tj.UNION_TRACT_DTYPE
SENSE = [c for c, a in sorted(CODON_AA.items()) if a != "*"]


def _torch():
    return pytest.importorskip("torch")


def features_of(rows):
    """(contig, start, end, cls, strand) tuples -> a FEATURE_DTYPE array"""
    f = np.zeros(len(rows), FT)
    for i, (contig, start, end, cls, strand) in enumerate(rows):
        f[i] = (contig, start, end, cls, strand, i + 1, 0, 0)
    return f


def same_records(got, want, dt):
    assert len(got) == len(want)
    for f in dt.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, (f, bad[:5], got[bad[:3]], want[bad[:3]])
    assert got.tobytes() == want.tobytes()


def build(counter, stream, feats, phase=None):
    """the coding table, built twice: the same rows both times, the inputs left alone, the rows those of the restatement"""
    ph = None if phase is None else np.asarray(phase, np.int8)
    with frozen(feats, ph):
        a, b = tj.Coding(counter, stream, feats, ph), tj.Coding(counter, stream, feats, ph)
    assert counter.last_coding_ms() > 0
    ra, rb = a.download(), b.download()
    assert ra.tobytes() == rb.tobytes() and a.n_features == len(feats)
    b.close()
    same_records(ra, restate_cds(stream, feats, ph), CD)
    return a, ra


def dev_effects(counter, cod, variants, tf=None, n=None, n_tracts=None):
    """-> EFFECT_DTYPE per record, or (negative code, message) when the call is refused.  tf: TRACT_FEATURE_DTYPE or None"""
    torch = _torch()
    L = tj.lib()
    n = len(variants) if n is None else n
    vd = _dev(variants) if len(variants) else torch.zeros(64, dtype=torch.uint8, device="cuda")
    td = _dev(tf) if tf is not None else None
    nt = (len(tf) if tf is not None else -5) if n_tracts is None else n_tracts
    runs = []
    for _ in range(2):
        out = GuardedDevice(n * EF.itemsize)
        torch.cuda.synchronize()
        with frozen(vd, td):
            rc = L.tjamd_variant_effects(counter._h, cod._h, _p(vd), n, _p(td), nt, out.c)
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        out.check("d_out")
        if rc < 0:
            assert counter.last_variant_effects_ms() == -1.0 and err.startswith("tjamd_variant_effects")
            assert out.untouched()                                  # (the records are checked by a launch of its own, in front of the walk)
            return rc, err
        assert rc == n and (n == 0 or counter.last_variant_effects_ms() > 0)
        runs.append(out.view(EF, n))
    assert runs[0].tobytes() == runs[1].tobytes()
    return runs[0]


def check_effects(counter, cod, stream, feats, phase, variants, tf):
    got = dev_effects(counter, cod, variants, tf)
    same_records(got, restate_effects(stream, feats, phase, variants, tf), EF)
    return got


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(5)
    yield c
    c.close()


def sense(rng, n):
    return "".join(rng.choice(SENSE) for _ in range(n))


# ---- the hand genome ---------------------------------------------------------------------------------------------------

def hand_genome():
    rng = random.Random(41)
    c1 = list("".join(rng.choice(DNA) for _ in range(400)))
    c1[123] = "N"; c1[151] = "n"; c1[20] = "a"; c1[21] = "u"
    c2 = "".join(rng.choice(DNA) for _ in range(250))
    stream = ("\n" + "".join(c1) + "\n" + c2).encode()                       # contig 0 is empty; the last has no delimiter
    rows = [(1, 1, 400, REGION, 0), (1, 10, 99, CDS, 0), (1, 10, 99, CDS, 1), (1, 11, 100, CDS, 0), (1, 30, 130, CDS, 1),          # 101 bases: no multiple of three
            (1, 120, 200, CDS, 0), (1, 120, 200, CDS, 1), (1, 5, 300, OTHER, 0), (2, 200, 400, CDS, 0), (2, 200, 2147483647, CDS, 1),
            (2, 1, 250, CDS, 2), (2, 250, 250, CDS, 0), (2, 249, 250, CDS, 1), (2, 1, 250, CDS, 0), (2, 251, 260, CDS, 0), (2, 300, 310, CDS, 1),
            (0, 1, 5, CDS, 0), (0, 1, 5, CDS, 1), (1, 398, 400, CDS, 0), (1, 1, 3, CDS, 1)]
    phase = [-1, 0, 1, 2, 2, 1, 0, 0, 1, 2, 0, 2, 1, 0, 1, 2, 0, 1, 0, 3]
    return stream, features_of(rows), np.array(phase, np.int8)


def test_hand_genome(counter):
    stream, feats, phase = hand_genome()
    cod, rows = build(counter, stream, feats, phase)
    assert rows[0].tolist() == (-1, -1, -1, -1) and rows[7].tolist() == (-1, -1, -1, -1) and rows[10].tolist() == (-1, -1, -1, -1)
    assert rows["phase"].tolist() == [-1, 0, 1, 2, 2, 1, 0, -1, 1, 2, -1, 2, 1, 0, 1, 2, 0, 1, 0, 0]
    assert rows["n_codons"][4] == 33 and rows["n_codons"][8] == 16 and rows["n_codons"][9] == 16      # (101 - 2) / 3; 51 bases are left of the contig
    assert rows["n_codons"][11] == 0 and rows["n_codons"][14] == 0 and rows["n_codons"][15] == 0 and rows["n_codons"][16] == 0      # spans shorter than a codon, beyond the contig, in the empty one
    assert rows["n_codons"][18] == 1 and rows["n_codons"][19] == 1
    assert tj.translate(stream[121: 201].decode("latin-1"))[1] == "X" and rows["aa_len"][5] > 1      # feature 5 from its phase on: the N at 123 of contig 1 is in its second codon
    without, rows0 = build(counter, stream, feats, None)
    assert set(rows0["phase"].tolist()) == {-1, 0}
    # records against the hand genome: everywhere in contig 1's first CDSs, both strands, all three phases
    tf = np.zeros(len(feats) + 1, TF)
    tf["feature"] = list(range(len(feats))) + [-1]
    var = []
    for f in (1, 2, 3, 4, 5, 6, 7, 0, 20, 10):
        for pos in (10, 11, 12, 13, 57, 58, 97, 98, 99, 100, 121, 149, 150, 152, 199, 200):
            for lr, la, rf, af in ((3, 4, "", ""), (4, 3, "", ""), (2, 5, "G", "T"), (5, 2, "CA", "TA")):
                if pos + max(lr - la, 0) + len(rf) <= 400:
                    var.append(variant_of(1, pos, DNA[(pos + f) % 4], lr, la, rf, af, tract=f))
    var = np.array(var, VAR)
    got = check_effects(counter, cod, stream, feats, phase, var, tf)
    assert set(got["cls"].tolist()) == {NONE, BOUNDARY, IDENTICAL, INFRAME, FRAMESHIFT}
    cod.close(); without.close()
    # nothing at all
    empty, rows = build(counter, b"", features_of([]))
    assert len(rows) == 0 and empty.n_features == 0
    empty.close()


# ---- the wavefront-step edges of the CDS scan --------------------------------------------------------------------------

def test_cds_scan_step_edges(counter):
    rng = random.Random(43)
    cases = [[s] for s in (0, 62, 63, 64, 65, 127, 128, 129)] + [[70, 100], [3, 130], [64, 65], []]
    genes = []
    for stops in cases:
        codons = [rng.choice(SENSE) for _ in range(140)]
        for s in stops:
            codons[s] = rng.choice(["TAA", "TAG", "TGA"])
        genes.append("".join(codons))
    genes.append("GCTAAC" * 70)                                              # a stop only in another frame (GC TAA C)
    contig, rows, want = "", [], []
    for g, stops in zip(genes, cases + [[]]):
        for strand in (0, 1):
            rows.append((0, len(contig) + 1, len(contig) + len(g), CDS, strand))
            contig += (g if strand == 0 else revcomp(g)) + "ACGT"[strand:]
            want.append((min(stops) if stops else 140, 1 if stops else 0, 140, 0))
    feats = features_of(rows)
    stream = (contig + "\n").encode()
    cod, got = build(counter, stream, feats)
    assert [tuple(r) for r in got.tolist()] == want
    # the other frames of the last gene: phase 2 reads TAA at once, phase 1 never
    ph = np.array([0] * (len(rows) - 2) + [2, 1], np.int8)
    cod2, got2 = build(counter, stream, feats, ph)
    assert got2[-2].tolist() == (0, 1, 139, 2) and got2[-1].tolist() == (139, 0, 139, 1)
    cod.close(); cod2.close()


# ---- edits -------------------------------------------------------------------------------------------------------------

RUN, LR = 40 * 3, 8                                                          # the run's CDS-oriented start and length in the main gene


def edit_world(strand):
    """one contig (behind an empty one) with the genes the edit cases need, all on `strand`; -> stream, features, phases and
    {case name: (record, expected class)}.  Genes are written CDS-oriented and laid down reverse-complemented for strand 1."""
    rng = random.Random(47 + strand)
    contig, rows, phases, cases, tracts = "GATTACA", [], [], {}, {}

    def lay(cds, phase=0, cls=CDS, strand_=strand):
        nonlocal contig
        S = len(contig)
        contig += (cds if strand == 0 else revcomp(cds)) + "GCATGC"
        rows.append((1, S + 1, S + len(cds), cls, strand_))
        phases.append(phase)
        return len(rows) - 1, S, S + len(cds) - 1

    def record(f, S, E, at, base, lr, la):
        """the record (no flank bases) of a run of lr `base` at CDS-oriented `at` that is la long in the sample"""
        if strand == 0:
            return variant_of(1, S + at + min(lr, la), base, lr, la, tract=f)
        return variant_of(1, (E - at - lr + 1) + min(lr, la), revcomp(base), lr, la, tract=f)      # the run's forward start is E - at - lr + 1

    # the main gene: 40 codons, G A^8 C, then codons to a stop, and a tail behind the stop with a run of its own
    head, mid = sense(rng, 40), sense(rng, 300)
    main = head + "G" + "A" * LR + "C" + "GT" + mid + "TAA" + "GCGTCCCCCCGTTGCA" + sense(rng, 4)
    f, S, E = lay(main)
    for d in (-6, -3, -2, -1, 1, 2, 3, 6, 200, 600):
        cases["length %+d" % d] = (record(f, S, E, RUN + 1, "A", LR, LR + d), INFRAME if d % 3 == 0 else FRAMESHIFT)
    # flanks that differ: forward, the 32 bases behind the run
    fwd = contig[S: E + 1]
    r0 = RUN + 1 if strand == 0 else (E - S) - (RUN + 1) - LR + 1          # the run's forward start in the span
    behind = fwd[r0 + LR: r0 + LR + 32]
    assert len(behind) == 32 and fwd[r0: r0 + LR] in ("A" * LR, "T" * LR) and fwd[r0 - 1] != fwd[r0] != behind[0]
    swap = lambda s: s[:-1] + DNA[(DNA.index(s[-1]) + 1) % 4]                # the outermost base differs
    for nfl in (0, 1, 32):
        for d in (-1, 3):
            v = variant_of(1, S + r0 + min(LR, LR + d), fwd[r0], LR, LR + d, behind[:nfl], swap(behind[:nfl]) if nfl else "", tract=f)
            cases["n_flank %d, length %+d" % (nfl, d)] = (v, None)
    # wholly behind the reference's stop
    tail = len(head) + 12 + len(mid) + 3 + 4                                 # behind TAA GCGT
    assert main[tail - 1: tail + 7] == "TCCCCCCG"
    cases["behind the stop"] = (record(f, S, E, tail, "C", 6, 7), IDENTICAL)
    # REF crossing either end of the span
    cases["REF from in front of the span"] = (variant_of(1, S, "A", 2, 1, tract=f), BOUNDARY)                    # p = S - 1
    cases["REF beyond the span"] = (variant_of(1, E, "A", 3, 1, tract=f), BOUNDARY)                             # p = E - 1, q = E + 1
    cases["REF up to the span's last base"] = (variant_of(1, E, "A", 2, 1, tract=f), None)
    # an edit at codon 0, and the same span read with phases 1 and 2: the edit lies in the skipped bases
    first = "AAAAAG" + sense(rng, 30) + "TGA"
    f0, S0, E0 = lay(first)
    cases["codon 0"] = (record(f0, S0, E0, 0, "A", 5, 6), FRAMESHIFT)
    cases["codon 0, in frame"] = (record(f0, S0, E0, 0, "A", 5, 2), INFRAME)
    for ph in (1, 2):
        rows.append(rows[f0]); phases.append(ph)
        cases["inside the %d skipped bases" % ph] = (record(len(rows) - 1, S0, E0, 0, "A", 1, 2), None)
        cases["phase %d, behind the skipped bases" % ph] = (record(len(rows) - 1, S0, E0, 0, "A", 5, 7), None)
    # an edit that destroys the stop: TAA C -> TAC, then GTC and one base over; with two bases over
    for over in (1, 2):
        fs, Ss, Es = lay(sense(rng, 20) + "TAACGTC" + "CA"[:over])
        cases["the stop destroyed, %d over" % over] = (record(fs, Ss, Es, 61, "A", 2, 1), FRAMESHIFT)
    # an edit that creates a stop at its own codon: TGG A -> TGA
    fc, Sc, Ec = lay(sense(rng, 12) + "TGGATC" + sense(rng, 12) + "TAG")
    cases["a stop created"] = (record(fc, Sc, Ec, 37, "G", 2, 1), FRAMESHIFT)
    # no feature, a gene, a CDS without a strand
    fg, Sg, Eg = lay(sense(rng, 30), cls=OTHER)
    fu, Su, Eu = lay(sense(rng, 30), strand_=2)
    cases["no feature"] = (variant_of(1, S + 50, "A", 3, 4, tract=len(rows)), NONE)
    cases["a gene"] = (variant_of(1, Sg + 10, "A", 3, 4, tract=fg), NONE)
    cases["a CDS of strand 2"] = (variant_of(1, Su + 10, "A", 3, 4, tract=fu), NONE)
    tf = np.zeros(len(rows) + 1, TF)
    tf["feature"] = list(range(len(rows))) + [-1]
    tf["max_length"] = 7
    return ("\n" + contig + "\n").encode(), features_of(rows), np.array(phases, np.int8), cases, tf


@pytest.mark.parametrize("strand", [0, 1])
def test_edits(counter, strand):
    stream, feats, phase, cases, tf = edit_world(strand)
    cod, rows = build(counter, stream, feats, phase)
    assert rows[0].tolist() == (40 + 3 + 1 + 300, 1, (len("G" + "A" * LR + "CGT") + 3 * 340 + 3 + 16 + 12) // 3, 0)
    names = sorted(cases)
    var = np.array([cases[x][0] for x in names], VAR)
    got = check_effects(counter, cod, stream, feats, phase, var, tf)
    e = dict(zip(names, got))
    for x in names:
        assert cases[x][1] is None or int(e[x]["cls"]) == cases[x][1], (x, e[x])
    assert e["length +200"]["alt_aa_len"] - e["length +200"]["first_diff"] > 64 and e["length +600"]["alt_aa_len"] - e["length +600"]["first_diff"] > 192
    assert unpack8(e["length +3"]["alt_aa"])[0] == "K" and e["length +3"]["alt_aa_len"] == e["length +3"]["ref_aa_len"] + 1
    assert e["length -6"]["alt_aa_len"] == e["length -6"]["ref_aa_len"] - 2 and e["length -6"]["flags"] == REF_STOP | ALT_STOP
    assert e["behind the stop"]["first_diff"] == -1 and e["behind the stop"]["ref_aa"] == 0 and e["behind the stop"]["flags"] == REF_STOP | ALT_STOP
    for over in (1, 2):
        x = e["the stop destroyed, %d over" % over]
        assert x["flags"] == REF_STOP and x["first_diff"] == 20 and unpack8(x["ref_aa"]) == "*" and unpack8(x["alt_aa"]) == "YV" and x["alt_aa_len"] == 22
    x = e["a stop created"]
    assert x["flags"] == REF_STOP | ALT_STOP and x["first_diff"] == 12 and unpack8(x["alt_aa"]) == "*" and x["alt_aa_len"] == 12 and x["ref_aa_len"] == 26
    assert e["codon 0"]["cds_pos"] == (5 if strand == 0 else 0) and e["codon 0, in frame"]["alt_aa_len"] == e["codon 0, in frame"]["ref_aa_len"] - 1
    assert e["REF up to the span's last base"]["cls"] != BOUNDARY and e["REF beyond the span"]["ref_aa_len"] == rows[0]["aa_len"]
    for x in ("no feature", "a gene", "a CDS of strand 2"):
        assert e[x].tolist()[1:] == (NONE, 0, -1, 0, 0, 0, 0, 0, 0)
    # the walk's cost does not show in the result: the same records in another order and among others give the same answers
    order = np.random.RandomState(3).permutation(len(var))
    again = check_effects(counter, cod, stream, feats, phase, var[order], tf)
    assert again.tobytes() == got[order].tobytes()
    cod.close()


# ---- record counts -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(counter):
    stream, feats, phase, cases, tf = edit_world(0)
    cod, _ = build(counter, stream, feats, phase)
    yield stream, feats, phase, cases, tf, cod
    cod.close()


def test_record_counts(counter, world):
    stream, feats, phase, cases, tf, cod = world
    walk = [cases[x][0] for x in sorted(cases) if cases[x][1] in (INFRAME, FRAMESHIFT, IDENTICAL)]
    none = cases["a gene"][0]
    rng = random.Random(53)
    for n in (1, 2, 63, 64, 65, 255, 256, 257):
        mixed = np.array([rng.choice(walk) if rng.random() < 0.5 else none for _ in range(n)], VAR)
        last = np.array([none] * (n - 1) + [walk[n % len(walk)]], VAR)       # the only walk record in the last (partial) wavefront
        for var in (mixed, last):
            got = check_effects(counter, cod, stream, feats, phase, var, tf)
            assert (got["cls"] >= IDENTICAL).sum() == sum(int(v["tract"]) != int(none["tract"]) for v in var)
    owners = np.array([walk[i % len(walk)] for i in range(64)], VAR)          # all 64 lanes of one wavefront are owners
    got = check_effects(counter, cod, stream, feats, phase, owners, tf)
    assert (got["cls"] >= IDENTICAL).all()
    # d_tract_feat = NULL: nothing has a feature, the tract ids are not read
    wild = owners.copy()
    wild["tract"] = -99
    got = dev_effects(counter, cod, wild, None)
    same_records(got, restate_effects(stream, feats, phase, wild, None), EF)
    assert (got["cls"] == NONE).all() and (got["feature"] == -1).all()
    # n = 0 writes nothing
    assert len(dev_effects(counter, cod, owners, tf, n=0)) == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_device_refusals(counter, world):
    torch = _torch()
    stream, feats, phase, cases, tf, cod = world
    good = np.array([cases[x][0] for x in sorted(cases)] * 12, VAR)[:300]
    want = restate_effects(stream, feats, phase, good, tf)
    same_records(dev_effects(counter, cod, good, tf), want, EF)
    clen = len(stream) - 2
    plant = [("contig", -1, "contig is outside [0, 2)"), ("contig", 2, "contig is outside [0, 2)"), ("pos", 0, "pos < 1"), ("pos", -5, "pos < 1"),
             ("pos", clen + 1, "ends beyond its contig"), ("n_flank", -1, "n_flank is outside 0..32"), ("n_flank", 33, "n_flank is outside 0..32"),
             ("ref_length", 0, "ref_length or alt_length < 1"), ("alt_length", 0, "ref_length or alt_length < 1"), ("alt_length", -3, "ref_length or alt_length < 1"),
             ("ref_length", 1 << 30, "ends beyond its contig"), ("tract", -1, "tract is outside [0, %d)" % len(tf)), ("tract", len(tf), "tract is outside [0, %d)" % len(tf))]
    for at, (field, value, msg) in zip((0, 63, 64, 150, 299, 7, 255, 256, 100, 101, 102, 103, 104), plant):
        bad = good.copy()
        bad[field][at] = value
        rc, err = dev_effects(counter, cod, bad, tf)
        assert rc == -ERR_ARG and msg in err, (field, value, rc, err)
        same_records(dev_effects(counter, cod, good, tf), want, EF)           # the same table serves the next good call
    # a contig that exists but is too short for the record: contig 0 is empty
    bad = good.copy()
    bad["contig"][5] = 0
    rc, err = dev_effects(counter, cod, bad, tf)
    assert rc == -ERR_ARG and "ends beyond its contig" in err
    # a feature index outside [-1, n_features)
    for value in (-2, len(feats), 1 << 30):
        tfb = tf.copy()
        tfb["feature"][int(good["tract"][17])] = value
        rc, err = dev_effects(counter, cod, good, tfb)
        assert rc == -ERR_ARG and "feature index is outside [-1, %d)" % len(feats) in err, (value, err)
    # the tract ids are checked against n_tracts, not against the buffer
    rc, err = dev_effects(counter, cod, good, tf, n_tracts=int(good["tract"].max()))
    assert rc == -ERR_ARG and "tract is outside" in err
    same_records(dev_effects(counter, cod, good, tf), want, EF)
    # the host's checks with real handles; the table of another device where there is one
    L = tj.lib()
    for s, f, msg in BAD_FEATURES:
        h = L.tjamd_coding_create(counter._h, s, len(s), f.ctypes.data, 1, None)
        err = L.tjamd_last_error().decode()
        assert not h and err.startswith("tjamd_coding_create") and msg in err and counter.last_coding_ms() == -1.0, (msg, err)
    with pytest.raises(tj.TatajubaAmdError):
        tj.Coding(counter, b"ACGT", features_of([(1, 1, 2, CDS, 0)]))
    assert L.tjamd_variant_effects(counter._h, cod._h, None, 5, None, 0, None) == -ERR_ARG and counter.last_variant_effects_ms() == -1.0
    assert L.tjamd_variant_effects(counter._h, cod._h, None, -1, None, 0, None) == -ERR_ARG
    h = GuardedHost(len(feats) * CD.itemsize)
    assert L.tjamd_coding_download(cod._h, h.c, len(feats) - 1) == len(feats) and h.untouched()
    assert L.tjamd_coding_download(cod._h, h.c, len(feats)) == len(feats)
    h.check("out")
    same_records(h.view(CD), restate_cds(stream, feats, phase), CD)
    if torch.cuda.device_count() > 1:
        other = tj.Counter(5, device=1)
        rc = L.tjamd_variant_effects(other._h, cod._h, _p(_dev(good)), 1, None, 0, _p(_dev(good)))
        assert rc == -ERR_ARG and "the coding table lives on device 0, the counter on device 1" in L.tjamd_last_error().decode()
        other.close()
    same_records(dev_effects(counter, cod, good, tf), want, EF)


def test_annotation_and_coding_table_refuse_a_feature_alike():
    """one rule for a feature's contig, start and end, two tables: every row of BAD_FEATURES that a genome of two contigs can
    express (the contig rows of the two-contig streams, the start and end rows) is refused by tjamd_annotation_create and by
    tjamd_coding_create with the same clause behind the entry's own name, and neither leaves a handle or an interval"""
    L = tj.lib()
    g = b"ACGT\nAC\n"
    rows = {msg: f for s, f, msg in BAD_FEATURES if "contig" not in msg or len(contigs_of(s)) == 2}
    assert len(rows) == 4 and sorted(m.split(":")[1].split()[0] for m in rows) == ["contig", "contig", "end", "start"]
    counter = tj.Counter(5)
    ref = tj.Reference(counter, g)
    assert ref.n_contigs == 2
    for table in (lambda f: tj.Annotation(counter, ref, f), lambda f: tj.Coding(counter, g, f)):      # both tables take a good feature,
        table(one_feature(contig=1, start=1, end=2)).close()                                           # so an interval stands to be cleared
    assert counter.last_annotation_ms() > 0 and counter.last_coding_ms() > 0
    for msg, f in rows.items():
        said = []
        for name, call, ms in (("tjamd_annotation_create", lambda: L.tjamd_annotation_create(counter._h, ref._h, f.ctypes.data, 1), counter.last_annotation_ms),
                               ("tjamd_coding_create", lambda: L.tjamd_coding_create(counter._h, g, len(g), f.ctypes.data, 1, None), counter.last_coding_ms)):
            h = call()
            err = L.tjamd_last_error().decode()
            assert not h and ms() == -1.0 and err.startswith(name + ": "), (name, msg, err)
            said.append(err[len(name):])
        assert said[0] == said[1] == ": " + msg, (msg, said)
    ref.close()
    counter.close()


# ---- the pipeline ------------------------------------------------------------------------------------------------------

def class_counts(e):
    return {tj.EFFECT_CLASSES[c]: int((e["cls"] == c).sum()) for c in range(5)}


def test_eight_sample_pipeline_effects(monkeypatch, tmp_path):
    """the eight samples and the calls of tests/test_locate.py::test_eight_sample_pipeline_with_a_reference with the GFF3 file of
    tests/test_features.py: variants -> tract features -> effects.  Sample 0 carries two planted length changes in CDS tracts,
    +1 and +3, in the first CDS tracts that lie in front of their protein's first stop (the restatement chooses them).  Counts
    and times are printed, not asserted (749 records at 0.023 ms beside 0.037 ms for tjamd_tract_variants)."""
    torch = _torch()
    monkeypatch.delenv("TATAJUBA_AMD_EDIT_DISTANCE", raising=False)
    k, m, ns, maxd, lev, mm = 15, 4, 8, 1, 2, 1
    rng = random.Random(2024)
    pieces = make_genome(rng, n_tracts=2000)
    genome = "".join(left + DNA[b] * length + right for left, b, length, right in pieces)
    stream = (genome + "\n").encode()
    path = tmp_path / "genome.gff3"
    path.write_text(gff3_of([pieces], ["genome"]))
    feats, strings = tj.read_gff3(str(path), ["genome"])
    phase = tj.read_gff3_phase(str(path), ["genome"])
    assert len(phase) == len(feats) and set(phase[feats["cls"] == CDS].tolist()) == {0} and set(phase[feats["cls"] != CDS].tolist()) == {-1}
    at, start = 0, {}
    for i, (left, b, length, right) in enumerate(pieces):
        start[i] = (at + len(left), b, length)
        at += len(left) + length + len(right)

    def hand_effect(i, d, tract=0, tf=None):
        """the restatement's answer for piece i's tract d bases longer, in the CDS line that holds it"""
        pos0, b, length = start[i]
        if tf is None:
            inside = np.flatnonzero((feats["cls"] == CDS) & (feats["start"] <= pos0 + 1) & (pos0 + 1 <= feats["end"]))
            tf = np.array([(int(inside[0]), 0)], TF)
        return restate_effects(stream, feats, phase, np.array([variant_of(0, pos0 + length, DNA[b], length, length + d, tract=tract)], VAR), tf)[0]

    # the planted pieces: inside a CDS of gff3_of, without a variant of sample_of's, and in front of the protein's first stop
    # (the genome is random: most of a CDS line lies behind one), chosen by the restatement
    free = [i for i in range(len(pieces)) if i % 8 not in (1, 2, 3, 4) and 1 <= i % 10 <= 4 and i // 10 < len(pieces) // 10]
    plus1 = next(i for i in free if hand_effect(i, 1)["cls"] == FRAMESHIFT)
    plus3 = next(i for i in free if i != plus1 and hand_effect(i, 3)["cls"] == INFRAME)
    planted = {plus1: 1, plus3: 3}
    counters, ocov = [], []
    for smp in range(ns):
        mine = [[l, b, n + (planted.get(i, 0) if smp == 0 else 0), r] for i, (l, b, n, r) in enumerate(pieces)]
        s = reads_of(sample_of(mine, rng, smp), rng)
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
    ref = tj.Reference(merger, stream)
    entries = ref.download()
    n_located, loc = dev_locate(merger, ref, keys, mm, on_device=True)
    nt, lt = dev_located_tracts(merger, keys, mat, grouped["tracts"], loc, on_device=True)
    u = Tiling(lt["keys"], lt["mat"], lt["tracts"], lt["tract_loc"])
    want_var, want_off, _ = restate_tract_variants(u.keys, u.mat, u.tracts, u.tract_loc, entries, k)
    n, var, off = dev_variants(merger, ref, u, want=want_var)                 # every tract: the planted ones need not be "variable"
    ms_variants = merger.last_tract_variants_ms()
    assert var.tobytes() == want_var.tobytes()
    ann = tj.Annotation(merger, ref, feats)
    ms_annotation = merger.last_annotation_ms()
    tf = dev_tract_features(merger, ann, u)
    cod, _ = build(merger, stream, feats, phase)
    ms_coding = merger.last_coding_ms()
    got = check_effects(merger, cod, stream, feats, phase, var, tf)
    ms_effects = merger.last_variant_effects_ms()
    # the planted changes come back with the class and the window the restatement gives for them
    for i, d in planted.items():
        pos0, b, length = start[i]
        mine = [j for j in range(off[0], off[1]) if int(var["pos"][j]) == pos0 + length and int(var["alt_length"][j]) == length + d]
        assert len(mine) == 1 and int(var["ref_length"][mine[0]]) == length and int(var["base"][mine[0]]) == b, (i, mine)
        e = got[mine[0]]
        w = hand_effect(i, d)
        assert int(e["cls"]) == int(w["cls"]) == (FRAMESHIFT if d == 1 else INFRAME) and e["first_diff"] >= 0
        assert e.tolist()[1:] == w.tolist()[1:] and e["ref_aa"] != e["alt_aa"]
        assert tj.gff3_string(strings, int(feats["type_off"][e["feature"]])) == "CDS" and e.tolist() == hand_effect(i, d, int(var["tract"][mine[0]]), tf).tolist()
    print(f"\n[effects] {len(feats)} features ({int((feats['cls'] == CDS).sum())} CDS), {nt} tracts, {n} variant records: {class_counts(got)}; "
          f"tjamd_last_variant_effects_ms {ms_effects:.3f} ms beside tjamd_last_tract_variants_ms {ms_variants:.3f} ms; "
          f"tjamd_last_coding_ms {ms_coding:.3f} ms beside tjamd_last_annotation_ms {ms_annotation:.3f} ms")
    assert min(ms_effects, ms_coding) > 0
    cod.close(); ann.close(); ref.close()
    for c in counters + [merger]:
        c.close()


# ---- the example -------------------------------------------------------------------------------------------------------

def test_variant_effects_c_example(tmp_path):
    exe, libdir = str(tmp_path / "variant_effects"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "variant_effects.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", exe])
    k, m, mm = 10, 3, 1
    rng = random.Random(7)
    pieces = make_genome(rng, n_tracts=200)
    parts = (pieces[:120], pieces[120:])
    contigs = ["".join(left + DNA[b] * length + right for left, b, length, right in part) for part in parts]
    names = ["contig0", "chr|2"]
    fasta, gff = str(tmp_path / "ref.fa"), str(tmp_path / "ref.gff3")
    with open(fasta, "w") as fh:
        fh.write("".join(">%s some text\n%s\n" % (names[i], "\n".join(s[j: j + 70] for j in range(0, len(s), 70))) for i, s in enumerate(contigs)))
    with open(gff, "w") as fh:
        fh.write(gff3_of(parts, names).replace("\t0\tParent=rna-contig0-g1;", "\t2\tParent=rna-contig0-g1;"))
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
    r = subprocess.run([exe, "-r", fasta, "-g", gff, "-x", str(mm), "-k", str(k), "-m", str(m), "-c", "5", "-d", "1", "-l", "-1", "-o", str(out)] + files,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # the same pipeline from the oracle and the restatements, as tests/test_variants.py does for sample_vcfs.c
    _, _, keys_o, mat_o = orc.merge_samples(np.frombuffer(np.concatenate(recs).tobytes(), np.uint64).reshape(-1, 3), [len(x) for x in recs])
    g = oracle_union_grouping(keys_o, mat_o, k, 1, 2)
    first = np.asarray(g["groups"]["first"], np.int64)
    tracts = np.zeros(len(first), TR)
    tracts["first"], tracts["n_rows"] = first, np.diff(np.r_[first, len(keys_o)])
    tracts["n_context"], tracts["indel"] = g["groups"]["n_context"], g["groups"]["indel"]
    tracts["mode"], tracts["lev_distance"], tracts["integral"] = g["mode"], g["lev_distance"], g["integral"]
    stream = ("\n".join(contigs) + "\n").encode()
    entries, n_contigs = restate_reference_index(stream, k)
    loc = restate_locate(entries, keys_o, mm)
    lt = restate_located_tracts(keys_o, mat_o, tracts, loc)
    perm = lt["perm"]
    pk, pm = keys_o[perm], mat_o[perm]
    ids = np.repeat(np.arange(len(lt["tracts"])), lt["tracts"]["n_rows"])
    st = restate_union_tract_stats(pk, pm, covs, ids, lt["tracts"]["lev_distance"], ref_length=lt["ref_length"])
    var = np.flatnonzero(st["variable"])
    want, off, _ = restate_tract_variants(pk, pm, lt["tracts"], lt["tract_loc"], entries, k, lst=var)
    feats, strings = tj.read_gff3(gff, names)
    phase = tj.read_gff3_phase(gff, names)
    assert (phase == 2).sum() == 1
    tf = restate_tract_features(feats, pk, pm, lt["tracts"], lt["tract_loc"])
    eff = restate_effects(stream, feats, phase, want, tf)
    text = EFFECTS_HEADER
    for smp, sample in enumerate(("s0.fq", "s_1_.fq")):
        for j in range(off[smp], off[smp + 1]):
            f = int(eff["feature"][j])
            text += effects_tsv_line(sample, want[j], eff[j], names[int(want["contig"][j])], tj.gff3_string(strings, int(feats["id_off"][f])) if f >= 0 else "unannotated")
    assert (out / "variant_effects.tsv").read_text() == text
    cc = class_counts(eff)
    assert cc["FRAMESHIFT"] > 0 and cc["NONE"] > 0
    assert r.stdout.strip().splitlines()[-1] == (f"{len(want)} variants in 2 samples: {cc['NONE']} outside coding features, {cc['BOUNDARY']} across a boundary, "
                                                 f"{cc['IDENTICAL']} identical, {cc['INFRAME']} in frame, {cc['FRAMESHIFT']} frameshifts")
