"""The coding-effect step (include/tatajuba_effects.h) without a GPU: the entries are declared, exported and prototyped and
refuse bad arguments before any device call, the records match the header, tjamd_translate and tjamd_gff3_read_phase are
checked on inputs written here, and the restatement that the GPU tests (tests/test_effects.py) compare against is defined.

The restatement is plain strings, written from the rule in the header: apply the edit to the contig, slice the span,
reverse-complement it on strand 1, translate with a table built here from an amino-acid -> codons dictionary (not from the
library), cut the protein behind its first '*', compare the two proteins symbol by symbol."""
import ctypes as C
import fnmatch
import glob
import gzip
import os
import re

import numpy as np

import tatajuba_amd as tj
from tests.guarded import GuardedHost
from tests.test_features_cabi import GFF_LINES, NAMES, _fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_translate", "tjamd_gff3_read_phase", "tjamd_coding_create", "tjamd_coding_destroy", "tjamd_coding_features", "tjamd_coding_download",
               "tjamd_variant_effects", "tjamd_last_coding_ms", "tjamd_last_variant_effects_ms"]
ERR_NO_DEVICE, ERR_ARG, ERR_CAP = 1, 3, 4
FT, TF, VAR, CD, EF = tj.FEATURE_DTYPE, tj.TRACT_FEATURE_DTYPE, tj.VARIANT_DTYPE, tj.CDS_DTYPE, tj.EFFECT_DTYPE
REGION, CDS, OTHER = 0, 1, 2
NONE, BOUNDARY, IDENTICAL, INFRAME, FRAMESHIFT = range(5)
REF_STOP, ALT_STOP = 1, 2
DNA = "ACGT"

# ---- the restatement ---------------------------------------------------------------------------------------------------

# the standard genetic code (NCBI table 1), by amino acid
AA_CODONS = {
    "A": "GCT GCC GCA GCG", "R": "CGT CGC CGA CGG AGA AGG", "N": "AAT AAC", "D": "GAT GAC", "C": "TGT TGC", "Q": "CAA CAG", "E": "GAA GAG",
    "G": "GGT GGC GGA GGG", "H": "CAT CAC", "I": "ATT ATC ATA", "L": "TTA TTG CTT CTC CTA CTG", "K": "AAA AAG", "M": "ATG", "F": "TTT TTC",
    "P": "CCT CCC CCA CCG", "S": "TCT TCC TCA TCG AGT AGC", "T": "ACT ACC ACA ACG", "W": "TGG", "Y": "TAT TAC", "V": "GTT GTC GTA GTG",
    "*": "TAA TAG TGA"}
CODON_AA = {codon: aa for aa, codons in AA_CODONS.items() for codon in codons.split()}
assert len(CODON_AA) == 64


def plain(dna):
    """upper case, U as T, everything that is no base as N"""
    return "".join(ch if ch in DNA else "N" for ch in dna.upper().replace("U", "T"))


def revcomp(dna):
    return plain(dna).translate(str.maketrans("ACGTN", "TGCAN"))[::-1]


def restate_translate(dna, reverse=False):
    """every whole codon, no stop handling; a codon with anything but a base in it is X"""
    s = revcomp(dna) if reverse else plain(dna)
    return "".join(CODON_AA.get(s[i: i + 3], "X") for i in range(0, len(s) - 2, 3))


def protein(oriented, phase):
    """the amino acids from base `phase` on, up to and including the first '*'"""
    aas = restate_translate(oriented[phase:])
    return aas[: aas.index("*") + 1] if "*" in aas else aas


def contigs_of(stream):
    """contig c lies behind the c-th newline; what follows a last newline is a contig only if it has a byte"""
    parts = bytes(stream).split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    return [p.decode("latin-1") for p in parts]


def span_of(contigs, f):
    """(S, E, the span's string) of a feature: the end clipped to the contig, empty if it begins beyond it"""
    contig = contigs[int(f["contig"])]
    S, E = int(f["start"]) - 1, min(int(f["end"]), len(contig)) - 1
    return S, E, (contig[S: E + 1] if E >= S else "")


def is_coding(f):
    return int(f["cls"]) == CDS and int(f["strand"]) in (0, 1)


def phase_of(phase, i):
    return int(phase[i]) if phase is not None and int(phase[i]) in (1, 2) else 0


def restate_cds(stream, features, phase=None):
    """-> CDS_DTYPE per feature"""
    contigs = contigs_of(stream)
    out = np.full(len(features), -1, np.int32).repeat(4).view(CD) if len(features) else np.zeros(0, CD)
    for i, f in enumerate(features):
        if not is_coding(f):
            continue
        _, _, span = span_of(contigs, f)
        ph = phase_of(phase, i)
        p = protein(span if int(f["strand"]) == 0 else revcomp(span), ph)
        out[i] = (len(p.rstrip("*")), int(p.endswith("*")), max(len(span) - ph, 0) // 3, ph)
    return out


def ref_alt(v):
    """REF and ALT of a variant record (REF's flank bases do not matter: only its length is used)"""
    lr, la, nf, b = int(v["ref_length"]), int(v["alt_length"]), int(v["n_flank"]), DNA[int(v["base"]) & 3]
    flank = lambda w: "".join(DNA[(int(w) >> (2 * j)) & 3] for j in range(nf))
    return b * (max(lr - la, 0) + 1) + flank(v["ref_flank"]), b * (max(la - lr, 0) + 1) + flank(v["alt_flank"])


def pack8(symbols):
    return sum(ord(ch) << (8 * j) for j, ch in enumerate(symbols[:8]))


def unpack8(word):
    return "".join(chr((int(word) >> (8 * j)) & 0xFF) for j in range(8)).rstrip("\0")


def restate_effects(stream, features, phase, variants, tract_feat):
    """-> EFFECT_DTYPE per variant record; tract_feat None: no record has a feature"""
    contigs = contigs_of(stream)
    out = np.zeros(len(variants), EF)
    for i, v in enumerate(variants):
        f = int(tract_feat["feature"][int(v["tract"])]) if tract_feat is not None else -1
        out[i]["feature"], out[i]["first_diff"] = f, -1
        if f < 0 or not is_coding(features[f]):
            continue                                                         # NONE
        ft, ph = features[f], phase_of(phase, f)
        S, E, span = span_of(contigs, ft)
        strand = int(ft["strand"])
        orient = (lambda s: s) if strand == 0 else revcomp
        p_ref = protein(orient(span), ph)
        out[i]["ref_aa_len"], out[i]["flags"] = len(p_ref.rstrip("*")), REF_STOP * p_ref.endswith("*")
        ref, alt = ref_alt(v)
        p = int(v["pos"]) - 1
        q = p + len(ref) - 1
        if int(v["contig"]) != int(ft["contig"]) or p < S or q > E:
            out[i]["cls"] = BOUNDARY
            continue
        contig = contigs[int(v["contig"])]
        edited = contig[:p] + alt + contig[q + 1:]
        p_alt = protein(orient(edited[S: E + 1 + len(alt) - len(ref)]), ph)
        diff = next((j for j, (a, b) in enumerate(zip(p_ref, p_alt)) if a != b), -1)
        if diff < 0 and len(p_ref) != len(p_alt):
            diff = min(len(p_ref), len(p_alt))
        out[i]["cds_pos"] = int(v["pos"]) - S if strand == 0 else E - q
        out[i]["first_diff"] = diff
        out[i]["cls"] = IDENTICAL if diff < 0 else INFRAME if (int(v["alt_length"]) - int(v["ref_length"])) % 3 == 0 else FRAMESHIFT
        out[i]["alt_aa_len"] = len(p_alt.rstrip("*"))
        out[i]["flags"] |= ALT_STOP * p_alt.endswith("*")
        if diff >= 0:
            out[i]["ref_aa"], out[i]["alt_aa"] = pack8(p_ref[diff:]), pack8(p_alt[diff:])
    return out


def effects_tsv_line(sample, v, e, contig_name, feature_id):
    """one line of examples/variant_effects.c"""
    ref, alt = ref_alt(v)
    return "%s\ttid_%06d\t%s\t%d\t%s\t%s\t%s\t%s\t%d\t%d\t%s\t%s\t%d\t%d\n" % (
        sample, int(v["tract"]), contig_name, int(v["pos"]), ref, alt, feature_id, tj.EFFECT_CLASSES[int(e["cls"])], int(e["cds_pos"]), int(e["first_diff"]) + 1,
        unpack8(e["ref_aa"]) or ".", unpack8(e["alt_aa"]) or ".", int(e["ref_aa_len"]), int(e["alt_aa_len"]))


EFFECTS_HEADER = "sample\ttract_id\tcontig_name\tpos\tref\talt\tfeature\teffect\tcds_pos\tfirst_diff\tref_aa\talt_aa\tref_aa_len\talt_aa_len\n"


def variant_of(contig, pos, base, ref_length, alt_length, ref_flank="", alt_flank="", tract=0, sample=0):
    """a VARIANT_DTYPE record from strings (flat and row are not read by tjamd_variant_effects)"""
    assert len(ref_flank) == len(alt_flank)
    word = lambda s: sum(DNA.index(ch) << (2 * j) for j, ch in enumerate(s))
    v = np.zeros(1, VAR)[0]
    v["flat"], v["tract"], v["sample"], v["contig"], v["pos"], v["row"], v["base"] = -7, tract, sample, contig, pos, 3, DNA.index(base)
    v["ref_length"], v["alt_length"], v["n_flank"], v["ref_flank"], v["alt_flank"] = ref_length, alt_length, len(ref_flank), word(ref_flank), word(alt_flank)
    return v


def test_the_restatement_on_hand_cases():
    #         0         1         2
    #         0123456789012345678901234567
    contig = "CCATGAAAAAAGGTTAGCCCTGACC"                  # ATG AAA AAA GGT TAG  at 2 .. 16: M K K G *
    feats = np.zeros(2, FT)
    feats[0] = (0, 3, 17, CDS, 0, 1, 0, 0)
    feats[1] = (0, 3, 17, OTHER, 0, 2, 0, 0)
    cds = restate_cds(contig.encode() + b"\n", feats)
    assert cds[0].tolist() == (4, 1, 5, 0) and cds[1].tolist() == (-1, -1, -1, -1)
    tf = np.array([(0, 0), (1, 0), (-1, 0)], TF)
    # the run of six A at 5 .. 10; a record of tjamd_tract_variants has POS = run start + min (Lr, La)
    plus1 = variant_of(0, 5 + 6, "A", 6, 7)                                  # REF A, ALT AA at the run's last base
    plus3 = variant_of(0, 5 + 6, "A", 6, 9)
    minus1 = variant_of(0, 5 + 5, "A", 6, 5)                                 # REF AA, ALT A
    var = np.array([plus1, plus3, minus1, plus1, plus1], VAR)
    var["tract"] = [0, 0, 0, 1, 2]
    e = restate_effects(contig.encode(), feats, None, var, tf)
    # +1: ATG AAA AAA AGG TTA G -> M K K R L (the span ends; no read-through): frameshift at the 4th amino acid
    assert (e[0]["cls"], e[0]["first_diff"], unpack8(e[0]["ref_aa"]), unpack8(e[0]["alt_aa"])) == (FRAMESHIFT, 3, "G*", "RL")
    assert (e[0]["ref_aa_len"], e[0]["alt_aa_len"], e[0]["flags"], e[0]["cds_pos"]) == (4, 5, REF_STOP, 9)
    # +3: M K K K G *
    assert (e[1]["cls"], e[1]["first_diff"], unpack8(e[1]["ref_aa"]), unpack8(e[1]["alt_aa"]), e[1]["flags"]) == (INFRAME, 3, "G*", "KG*", REF_STOP | ALT_STOP)
    # -1: ATG AAA AAG GTT AG -> M K K V
    assert (e[2]["cls"], e[2]["first_diff"], unpack8(e[2]["alt_aa"]), e[2]["alt_aa_len"], e[2]["flags"]) == (FRAMESHIFT, 3, "V", 4, REF_STOP)
    assert [int(x) for x in e["cls"][3:]] == [NONE, NONE] and e[3]["feature"] == 1 and e[4]["feature"] == -1 and e[3]["first_diff"] == -1
    assert e[3]["ref_aa_len"] == 0 and e[3]["flags"] == 0
    # the same span read from the other strand: CTA ACC TTT TTT CAT, L T F F H and no stop
    feats[0]["strand"] = 1
    assert restate_cds(contig.encode(), feats)[0].tolist() == (5, 0, 5, 0)
    # a REF that crosses the span's end is a BOUNDARY
    edge = variant_of(0, 16, "A", 3, 1, "G", "C")                            # REF AAAG at 15 .. 18, E = 16
    feats[0]["strand"] = 0
    b = restate_effects(contig.encode(), feats, None, np.array([edge], VAR), tf)[0]
    assert (b["cls"], b["first_diff"], b["ref_aa_len"], b["flags"], b["alt_aa_len"]) == (BOUNDARY, -1, 4, REF_STOP, 0)


# ---- tjamd_translate ---------------------------------------------------------------------------------------------------

def test_translate_against_the_restatement():
    L = tj.lib()
    every = "".join(a + b + c for a in DNA for b in DNA for c in DNA)
    assert tj.translate(every) == "".join(CODON_AA[every[i: i + 3]] for i in range(0, 192, 3)) == restate_translate(every)
    assert tj.translate(every).count("*") == 3 and [every[3 * i: 3 * i + 3] for i, a in enumerate(tj.translate(every)) if a == "*"] == ["TAA", "TAG", "TGA"]
    for dna in (every, every.lower(), every.replace("T", "U"), every.replace("T", "u"), "ANGNNNACNTAAtaGuGaTAR-AAxyz\nAAATGAATN", "ACGTN"[::-1] * 13):
        for reverse in (False, True):
            assert tj.translate(dna, reverse) == restate_translate(dna, reverse), (dna, reverse)
    assert tj.translate("NAA") == "X" and tj.translate("TAN") == "X" and tj.translate("T\nA") == "X"
    assert tj.translate("TTATCA", True) == "**"
    assert tj.translate("NCAT", True) == "M" and tj.translate("CATN", True) == "X"       # the reverse reads from the end
    for n in range(8):
        dna = "ATGGCCTAAC"[:n]
        for reverse in (0, 1):
            out = GuardedHost(max(n // 3, 1))
            assert L.tjamd_translate(dna.encode(), n, reverse, out.c, n // 3) == n // 3
            out.check("out")
            assert out.view(np.uint8, n // 3).tobytes().decode() == restate_translate(dna, bool(reverse))
            assert (out.payload[n // 3:] == GuardedHost(max(n // 3, 1)).payload[n // 3:]).all()          # no NUL, nothing behind
            if n >= 3:                                                       # one short: the size comes back, nothing is written
                short = GuardedHost(n // 3)
                assert L.tjamd_translate(dna.encode(), n, reverse, short.c, n // 3 - 1) == n // 3 and short.untouched()
    assert L.tjamd_translate(None, 0, 0, None, 0) == 0
    for args, msg in [((b"ACG", -1, 0, None, 0), "n -1 < 0"), ((None, 3, 0, None, 0), "null dna"), ((b"ACG", 3, 0, None, 1), "null output buffer")]:
        assert L.tjamd_translate(*args) == -ERR_ARG
        err = L.tjamd_last_error().decode()
        assert err.startswith("tjamd_translate") and msg in err, err


# ---- tjamd_gff3_read_phase ---------------------------------------------------------------------------------------------

def phase_line(seqid, typ, start, end, strand, phase, attr="ID=x", cols=9):
    return "\t".join([seqid, "src", typ, str(start), str(end), ".", strand, phase, attr][:cols])


PHASE_LINES = GFF_LINES + [
    phase_line("chr1", "CDS", 10, 90, "+", "0"), phase_line("chr1", "CDS", 10, 90, "-", "1"), phase_line("chr10", "cds", 1, 9, "+", "2"),
    phase_line("chr1", "CDS", 10, 90, "+", "."), phase_line("chr1", "CDS", 10, 90, "+", "3"), phase_line("chr1", "CDS", 10, 90, "+", "junk"),
    phase_line("chr1", "CDS", 10, 90, "+", ""), phase_line("chr1", "CDS", 10, 90, "+", "01"), phase_line("chr1", "gene", 10, 90, "+", "2") + "\r",
    phase_line("nowhere", "CDS", 10, 90, "+", "1"),                           # skipped: not among the names
    phase_line("chr1", "CDS", 0, 90, "+", "1"),                               # skipped: start 0
    phase_line("chr1", "CDS", 10, 90, "+", "2", cols=8),                      # skipped: eight columns
    phase_line("ctg|2 x", "CDS", 5, 7, "-", "1"),                             # the last line, without a newline
]


def test_gff3_read_phase_against_gff3_read(tmp_path):
    L = tj.lib()
    text = "\n".join(PHASE_LINES)
    plain_path, gz = tmp_path / "p.gff3", tmp_path / "p.gff3.gz"
    plain_path.write_bytes(text.encode())
    with gzip.open(gz, "wb") as fh:
        fh.write(text.encode())
    feats, _ = tj.read_gff3(str(plain_path), NAMES)
    skipped = tj.read_gff3.last_skipped
    assert skipped == 8 + 3 and len(feats) == 8 + 10
    # what the lines say, by the line numbers tjamd_gff3_read kept
    want = []
    for f in feats:
        col = PHASE_LINES[int(f["line"]) - 1].rstrip("\r").split("\t")[7]
        want.append(int(col) if col in ("0", "1", "2") else -1)
    assert want[8:] == [0, 1, 2, -1, -1, -1, -1, -1, 2, 1] and want[:8] == [-1] * 8
    for path in (plain_path, gz):
        got = tj.read_gff3_phase(str(path), NAMES)
        assert got.dtype == np.int8 and got.tolist() == want, (path, got.tolist())
    # with a newline at the end, and cut at ##FASTA: the same lines as the reader
    plain_path.write_bytes(("\n".join(PHASE_LINES[:21]) + "\n##FASTA\n" + "\n".join(PHASE_LINES[21:]) + "\n").encode())
    assert tj.read_gff3_phase(str(plain_path), NAMES).tolist() == want[:10] and len(tj.read_gff3(str(plain_path), NAMES)[0]) == 10
    # sizing and capacity: one short writes nothing
    plain_path.write_bytes(text.encode())
    blob = "".join(n + "\n" for n in NAMES).encode()
    n = len(want)
    out = GuardedHost(n)
    assert L.tjamd_gff3_read_phase(os.fsencode(str(plain_path)), blob, len(NAMES), None, 0) == n
    assert L.tjamd_gff3_read_phase(os.fsencode(str(plain_path)), blob, len(NAMES), out.c, n - 1) == n and out.untouched()
    assert L.tjamd_gff3_read_phase(os.fsencode(str(plain_path)), blob, len(NAMES), out.c, n) == n
    out.check("out")
    assert out.view(np.int8).tolist() == want
    assert L.tjamd_gff3_read_phase(os.fsencode(str(tmp_path / "none.gff3")), blob, len(NAMES), None, 0) == -1
    assert len(tj.read_gff3_phase(str(plain_path), [])) == 0
    z = bytearray(gz.read_bytes())
    z[-6] ^= 0x40
    (tmp_path / "bad.gz").write_bytes(bytes(z))
    assert L.tjamd_gff3_read_phase(os.fsencode(str(tmp_path / "bad.gz")), blob, len(NAMES), None, 0) == -1


# ---- declarations and argument checks ----------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    own = strip(os.path.join(ROOT, "include", "tatajuba_effects.h"))
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.EFFECT_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_effects.h"]
    assert len(others) >= 6
    for s in NEW_ENTRIES:
        for path in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(path)), (s, path)   # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert "tatajuba_effects.h" in open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read()
    assert _fields(own, "tjamd_cds") == list(CD.names) and _fields(own, "tjamd_effect") == list(EF.names)
    assert CD.itemsize == 16 and [CD.fields[x][1] for x in CD.names] == [0, 4, 8, 12]
    assert EF.itemsize == 48 and [EF.fields[x][1] for x in EF.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert re.search(r"TJAMD_EFFECT_NONE = 0, TJAMD_EFFECT_BOUNDARY = 1, TJAMD_EFFECT_IDENTICAL = 2, TJAMD_EFFECT_INFRAME = 3, TJAMD_EFFECT_FRAMESHIFT = 4", own)
    assert re.search(r"TJAMD_EFFECT_REF_STOP = 1, TJAMD_EFFECT_ALT_STOP = 2", own)
    assert tj.EFFECT_CLASSES == ["NONE", "BOUNDARY", "IDENTICAL", "INFRAME", "FRAMESHIFT"]
    assert L.tjamd_last_coding_ms(None) == -1.0 and L.tjamd_last_variant_effects_ms(None) == -1.0
    assert L.tjamd_coding_features(None) == -1
    L.tjamd_coding_destroy(None)
    for name in ("variant_effects", "last_coding_ms", "last_variant_effects_ms"):
        assert hasattr(tj.Counter, name)
    assert all(hasattr(tj.Coding, x) for x in ("download", "close", "n_features"))


def one_feature(contig=0, start=1, end=9, cls=CDS, strand=0):
    f = np.zeros(1, FT)
    f[0] = (contig, start, end, cls, strand, 1, 0, 0)
    return f


# (stream, feature, what tjamd_coding_create says): the checks that read the caller's host buffers only
BAD_FEATURES = [(b"ACGT\nAC\n", one_feature(contig=2), "feature 0: contig 2 outside [0, 2)"), (b"ACGT\nAC", one_feature(contig=-1), "feature 0: contig -1 outside [0, 2)"),
                (b"ACGT\n\n", one_feature(contig=2), "feature 0: contig 2 outside [0, 2)"), (b"", one_feature(), "feature 0: contig 0 outside [0, 0)"),
                (b"ACGT", one_feature(start=0), "feature 0: start 0 < 1"), (b"ACGT", one_feature(start=5, end=4), "feature 0: end 4 < start 5")]


def test_entries_check_their_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first

    def call(c=None, cod=None, var=fake, n=10, tf=fake, nt=3, out=fake):
        rc = L.tjamd_variant_effects(c, cod, var, n, tf, nt, out)
        return rc, L.tjamd_last_error().decode()

    for kw, rc, msg in [({}, ERR_ARG, "null counter or coding table"), ({"cod": fake}, ERR_ARG, "null counter or coding table"),
                        ({"n": -1}, ERR_ARG, "n -1 < 0"), ({"n": 1 << 31}, ERR_CAP, "2147483648 records"),
                        ({"var": None}, ERR_ARG, "null variant or output buffer"), ({"out": None}, ERR_ARG, "null variant or output buffer"),
                        ({"nt": -1}, ERR_ARG, "n_tracts -1 < 0"), ({"tf": None, "nt": -1}, ERR_ARG, "null counter or coding table"),
                        ({"n": 0, "var": None, "out": None}, ERR_ARG, "null counter or coding table")]:
        got, err = call(**kw)
        assert got == -rc and err.startswith("tjamd_variant_effects") and msg in err, (kw, got, err)
    stream, one = b"ACGTACGTAC\n", one_feature()
    h = L.tjamd_coding_create(None, stream, len(stream), one.ctypes.data, 1, None)
    err = L.tjamd_last_error().decode()
    assert not h and err.startswith("tjamd_coding_create") and "null counter" in err
    assert L.tjamd_coding_download(None, None, 0) == -ERR_ARG and L.tjamd_last_error().decode().startswith("tjamd_coding_download")
    if tj.device_count() == 0:                     # a counter cannot exist: the pointer below stands for one and is never read
        got, err = call(c=fake)
        assert got == -ERR_ARG and "null counter or coding table" in err
        cases = [(None, 5, one, 1, "null stream"), (fake, 1 << 31, one, 1, "a stream of 2147483648 bytes"), (stream, len(stream), None, 1, "1 features with a null buffer"),
                 (stream, len(stream), one, -1, "-1 features"), (stream, len(stream), one, (1 << 30) + 1, "more than 2^30")]
        cases += [(s, len(s), f, 1, msg) for s, f, msg in BAD_FEATURES]
        for s, nb, f, n, msg in cases:
            h = L.tjamd_coding_create(fake, s, nb, f.ctypes.data if f is not None else None, n, None)
            err = L.tjamd_last_error().decode()
            assert not h and err.startswith("tjamd_coding_create") and msg in err, (msg, err)
        # good arguments, but nothing to run on: named, before the handles are read
        got, err = call(c=fake, cod=fake)
        assert got == -ERR_NO_DEVICE and err.startswith("tjamd_variant_effects") and "TJAMD_ERR_NO_DEVICE" in err, (got, err)
        h = L.tjamd_coding_create(fake, stream, len(stream), one.ctypes.data, 1, None)
        err = L.tjamd_last_error().decode()
        assert not h and err.startswith("tjamd_coding_create") and "TJAMD_ERR_NO_DEVICE" in err
