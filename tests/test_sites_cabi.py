"""The multi-sample step (include/tatajuba_sites.h: tjamd_merge_variants, tjamd_site_ref_alt) without a GPU: the entries are
declared, exported and prototyped and refuse bad arguments before any device call, the records match the header, the
restatement that the GPU tests (tests/test_sites.py) compare against reproduces the three hand cases of
tests/test_variants_cabi.py merged by hand, every input record applied to the genome through its site (site POS, REF, the
sample's ALT) gives the contig its own (POS, REF, ALT) gives, and tjamd_site_ref_alt writes the restatement's strings.

restate_merge_variants is written from the rule in include/tatajuba_sites.h with strings: flank words are decoded to text,
alleles are keyed and ordered by their text, the common anchor is string slicing.  The device does the same with a sort of
packed keys, head flags, scans and a segmented reduction."""
import ctypes as C
import fnmatch
import glob
import os
import random
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedHost
from tests.test_variants_cabi import (DNA, K, NS, fold, hand_case, locate_and_tile, pack, planted_union, ref_alt_of, restate_tract_variants, small_genome,
                                      unpack)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_merge_variants", "tjamd_site_ref_alt", "tjamd_last_merge_variants_ms"]
ERR_NO_DEVICE, ERR_ARG, ERR_CAP = 1, 3, 4
VAR, SITE, ALLELE = tj.VARIANT_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE
MAX_LENGTH = 1023


def site_text(site, allele=None):
    """REF (allele None) or an allele's ALT, from the records' own fields: B^(length - min_length + 1), then F flank bases"""
    length = int(site["ref_length"] if allele is None else allele["alt_length"])
    word = site["ref_flank"] if allele is None else allele["alt_flank"]
    return DNA[int(site["base"])] * (length - int(site["min_length"]) + 1) + unpack(word, int(site["n_flank"]))


def restate_merge_variants(records, n_samples, k, n_tracts=None):
    """-> dict: sites (SITE_DTYPE), alleles (ALLELE_DTYPE), genotype (int16 [n_sites, n_samples]), allele_of (int32 per input
    record), unique (VARIANT_DTYPE, one per allele), text ([(REF, [ALT, ...])] per site).  ValueError for what the entry refuses."""
    records = np.asarray(records, VAR)
    by_tract = {}
    for i, r in enumerate(records):
        t, s, nf, la = int(r["tract"]), int(r["sample"]), int(r["n_flank"]), int(r["alt_length"])
        if t < 0 or (n_tracts is not None and t >= n_tracts):
            raise ValueError("tract")
        if not 0 <= s < n_samples:
            raise ValueError("sample")
        if not 0 <= nf <= k:
            raise ValueError("n_flank")
        if not 0 <= la <= MAX_LENGTH:
            raise ValueError("alt_length")
        by_tract.setdefault(t, []).append(i)
    sites, alleles, text, unique = [], [], [], []
    genotype = np.full((len(by_tract), n_samples), -1, np.int16)
    allele_of = np.zeros(len(records), np.int32)
    for n_site, t in enumerate(sorted(by_tract)):
        mine = by_tract[t]
        first = records[mine[0]]
        samples = [int(records[i]["sample"]) for i in mine]
        if len(set(samples)) != len(samples):
            raise ValueError("pair")
        for i in mine:
            if any(records[i][f] != first[f] for f in ("flat", "contig", "base", "ref_length")):
                raise ValueError("disagree")
        F = max(int(records[i]["n_flank"]) for i in mine)
        R_ref = max(unpack(records[i]["ref_flank"], F)[::-1] for i in mine if int(records[i]["n_flank"]) == F)[::-1]
        groups = {}                                                           # (alt_length, n_flank, own alt flank text) -> input indices
        for i in mine:
            r = records[i]
            nf = int(r["n_flank"])
            if unpack(r["ref_flank"], nf) != R_ref[:nf]:
                raise ValueError("ref_flank")
            groups.setdefault((int(r["alt_length"]), nf, unpack(r["alt_flank"], nf)), []).append(i)
        # alt_flank compared as a number: base j has the weight 4^j, so the text is compared from its far end
        order = sorted(groups, key=lambda g: (g[0], g[1], [DNA.index(ch) for ch in reversed(g[2])]))
        Lr = int(first["ref_length"])
        min_length = min(Lr, min(g[0] for g in order))
        pos = min(int(records[i]["pos"]) for i in mine)
        B = DNA[int(first["base"])]
        alts = []
        for n_allele, g in enumerate(order):
            R_alt = g[2] + R_ref[g[1]:]                                       # beyond its own n_flank a record's flank is the genome's
            alleles.append((n_site, g[0], g[1], len(groups[g]), min(groups[g]), 0, pack(R_alt)))
            unique.append(records[min(groups[g])])
            alts.append(B * (g[0] - min_length + 1) + R_alt)
            for i in groups[g]:
                allele_of[i] = len(alleles) - 1
                genotype[n_site, int(records[i]["sample"])] = n_allele + 1
        sites.append((int(first["flat"]), t, int(first["contig"]), pos, int(first["base"]), Lr, min_length, F, len(order), len(alleles) - len(order),
                      len(mine), min(mine), 0, pack(R_ref)))
        text.append((B * (Lr - min_length + 1) + R_ref, alts))
    out = {"sites": np.array(sites, SITE), "alleles": np.array(alleles, ALLELE), "genotype": genotype, "allele_of": allele_of,
           "unique": np.array(unique, VAR) if unique else np.zeros(0, VAR), "text": text}
    for s, (REF, alts) in zip(out["sites"], text):                            # the text from the records' fields is the text from the strings
        mine = out["alleles"][int(s["first_allele"]): int(s["first_allele"]) + int(s["n_alleles"])]
        assert site_text(s) == REF and [site_text(s, a) for a in mine] == alts
    return out


MERGED_HEADER = ('##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
                 '##INFO=<ID=AC,Number=A,Type=Integer,Description="samples that carry each ALT allele">\n'
                 '##INFO=<ID=AN,Number=1,Type=Integer,Description="samples with a call">\n'
                 '##INFO=<ID=TID,Number=A,Type=String,Description="tract ID">\n')


def merged_vcf_text(names, lengths, sample_names, m):
    """the multi-sample VCF as examples/merged_vcf.c writes it, from a restate_merge_variants result"""
    out = MERGED_HEADER + "".join("##contig=<ID=%s,length=%d>\n" % (n, l) for n, l in zip(names, lengths))
    out += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n" % "\t".join(sample_names)
    for s, (REF, alts), row in zip(m["sites"], m["text"], m["genotype"]):
        mine = m["alleles"][int(s["first_allele"]): int(s["first_allele"]) + int(s["n_alleles"])]
        out += "%s\t%d\t.\t%s\t%s\t.\t.\tAC=%s;AN=%d;TID=tid_%06d\tGT\t%s\n" % (
            names[int(s["contig"])], int(s["pos"]), REF, ",".join(alts), ",".join(str(int(a["n_samples"])) for a in mine), int(s["n_called"]),
            int(s["tract"]), "\t".join("." if g < 0 else str(int(g)) for g in row))
    return out


def unique_vcf_text(names, lengths, m):
    """the tutorial's concatenation as examples/merged_vcf.c -u writes it: one row per allele, N8's own REF and ALT"""
    out = ('##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
           '##INFO=<ID=TID,Number=A,Type=String,Description="tract ID">\n') + "".join("##contig=<ID=%s,length=%d>\n" % (n, l) for n, l in zip(names, lengths))
    out += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tall_samples\n"
    for r in m["unique"]:
        REF, ALT = ref_alt_of(r)
        out += "%s\t%d\t.\t%s\t%s\t.\t.\tTID=tid_%06d\tGT\t1\n" % (names[int(r["contig"])], int(r["pos"]), REF, ALT, int(r["tract"]))
    return out


# ---- the three hand cases of N8, merged by hand --------------------------------------------------------------------------
# (tract, contig, POS, REF, [ALT, ...] in allele order, [samples per allele], genotype row of samples 0-8), from HAND_PLAIN,
# HAND_NEXT and HAND_NEAR of tests/test_variants_cabi.py.  'plain', the AAA tract at 4 (Lr = 3):
#   s0, s5, s6: A -> AA (La 4, no flank)   s1: AA -> A (La 2)   s3: AG -> AAT (La 4, one flank base)   s4: AGCAG -> AAGCAT (La 4, four)
#   F = 4, R_ref = GCAG; the shortest allele has 2 bases, so min_length = 2, POS = 4 + 2 and REF = A^(3 - 2 + 1) + GCAG;
#   alleles by (alt_length, n_flank, alt_flank): (2, 0) A + GCAG; (4, 0) AAA + GCAG; (4, 1, T) AAA + T + CAG; (4, 4, GCAT) AAA + GCAT
#   the TTTTT tract at 11 (Lr = 5): s0, s7: T -> TT (La 6)   s1: TTCAG -> TCAT (La 4, three flank bases): F = 3, R_ref = CAG,
#   min_length = 4, POS = 15, REF = TT + CAG; alleles (4, 3, CAT) T + CAT; (6, 0) TTT + CAG
#   the CCCCC tract of contig 1: one record, one allele: N8's own POS, REF and ALT
HAND_SITES = {
    "plain": [(1, 0, 6, "AAGCAG", ["AGCAG", "AAAGCAG", "AAATCAG", "AAAGCAT"], [1, 3, 1, 1], [2, 1, -1, 3, 4, 2, 2, -1, -1]),
              (2, 0, 15, "TTCAG", ["TCAT", "TTTCAG"], [1, 2], [2, 1, -1, -1, -1, -1, -1, 2, -1]),
              (3, 1, 9, "C", ["CCC"], [1], [1, -1, -1, -1, -1, -1, -1, -1, -1])],
    # 'next': the G tract starts right after the run, no flank is left (k_eff = 0); every sample has G -> GG there
    "next": [(0, 0, 6, "AA", ["A", "AAA"], [1, 5], [2, 1, -1, 2, 2, 2, 2, -1, -1]),
             (1, 0, 8, "G", ["GG"], [9], [1, 1, 1, 1, 1, 1, 1, 1, 1])],
    # 'near': three flank bases are left: s3's difference next to the tract stays (F = 1), s4's at the far end is cut off
    "near": [(0, 0, 6, "AAG", ["AG", "AAAG", "AAAT"], [1, 4, 1], [2, 1, -1, 3, 2, 2, 2, -1, -1])],
}


def hand_records(which):
    keys, mat, tracts, loc, entries = hand_case(which)
    return restate_tract_variants(keys, mat, tracts, loc, entries, K)[0]


def test_the_rule_on_the_hand_cases():
    for which, want in HAND_SITES.items():
        recs = hand_records(which)
        m = restate_merge_variants(recs, NS, K)
        got = []
        for s, (REF, alts), row in zip(m["sites"], m["text"], m["genotype"]):
            mine = m["alleles"][int(s["first_allele"]): int(s["first_allele"]) + int(s["n_alleles"])]
            got.append((int(s["tract"]), int(s["contig"]), int(s["pos"]), REF, alts, [int(a["n_samples"]) for a in mine], row.tolist()))
        assert got == want, which
        assert [int(s["n_called"]) for s in m["sites"]] == [sum(w[5]) for w in want]
        assert len(m["unique"]) == len(m["alleles"]) == sum(len(w[4]) for w in want)
        assert (m["sites"]["pad"] == 0).all() and (m["alleles"]["pad"] == 0).all()
    m = restate_merge_variants(hand_records("plain"), NS, K)
    s = m["sites"][0]                                                         # the AAA site, field by field
    assert tuple(s.tolist()) == (4, 1, 0, 6, 0, 3, 2, 4, 4, 0, 6, 0, 0, pack("GCAG"))
    assert [tuple(a.tolist()) for a in m["alleles"][:4]] == [(0, 2, 0, 1, 3, 0, pack("GCAG")), (0, 4, 0, 3, 0, 0, pack("GCAG")), (0, 4, 1, 1, 5, 0, pack("TCAG")),
                                                             (0, 4, 4, 1, 6, 0, pack("GCAT"))]
    assert m["allele_of"].tolist() == [1, 5, 6, 0, 4, 2, 3, 1, 1, 5]
    assert m["unique"].tobytes() == hand_records("plain")[[3, 0, 5, 6, 4, 1, 2]].tobytes()
    # a site with one allele is N8's record
    r = m["unique"][6]
    assert (site_text(m["sites"][2]), site_text(m["sites"][2], m["alleles"][6])) == ref_alt_of(r) and int(m["sites"][2]["pos"]) == int(r["pos"])
    # the order of the input does not number the sites: a list given in descending order
    keys, mat, tracts, loc, entries = hand_case("plain")
    back = restate_tract_variants(keys, mat, tracts, loc, entries, K, lst=[3, 2, 1, 0])[0]
    mb = restate_merge_variants(back, NS, K)
    assert mb["sites"]["tract"].tolist() == [1, 2, 3] and mb["text"] == m["text"] and (mb["genotype"] == m["genotype"]).all()
    # what is refused
    twice = restate_tract_variants(keys, mat, tracts, loc, entries, K, lst=[1, 1])[0]
    recs = hand_records("plain")
    bad = {"pair": twice, "sample": recs.copy(), "n_flank": recs.copy(), "disagree": recs.copy(), "ref_flank": recs.copy(), "tract": recs.copy()}
    bad["sample"]["sample"][2] = NS
    bad["n_flank"]["n_flank"][0] = K + 1
    bad["disagree"]["flat"][3] += 1
    bad["ref_flank"]["ref_flank"][5] ^= 1
    bad["tract"]["tract"][0] = 4
    for what, b in bad.items():
        with pytest.raises(ValueError, match=what):
            restate_merge_variants(b, NS, K, n_tracts=4)
    assert len(restate_merge_variants(recs[:0], NS, K)["sites"]) == 0


# ---- an invariant that does not depend on the rule's wording -------------------------------------------------------------

def applied(g, pos, REF, ALT):
    at = pos - 1
    assert g[at: at + len(REF)] == REF, (pos, REF)
    return g[:at] + ALT + g[at + len(REF):]


@pytest.mark.parametrize("k,ns,seed", [(4, 8, 11), (4, 3, 12), (15, 5, 13), (15, 9, 14), (32, 4, 15), (32, 6, 16)])
def test_every_record_through_its_site_gives_the_same_contig(k, ns, seed):
    """for every input record: (site POS, REF, the sample's ALT) applied to the genome gives the contig the record's own (POS,
    REF, ALT) gives -- no exceptions and no share of cases left out"""
    rng = random.Random(seed)
    stream = small_genome(rng, k)
    p = planted_union(stream, k, ns, rng, max_sites=120)
    keys, mat, tracts, loc = locate_and_tile(p)
    recs, _, _ = restate_tract_variants(keys, mat, tracts, loc, p["entries"], k)
    assert len(recs) > 20
    m = restate_merge_variants(recs, ns, k, n_tracts=len(tracts))
    contigs = [fold(c) for c in bytes(stream).split(b"\n")]
    site_of = m["alleles"]["site"][m["allele_of"]]
    for i, r in enumerate(recs):
        s, a = m["sites"][site_of[i]], m["alleles"][m["allele_of"][i]]
        g = contigs[int(r["contig"])]
        own = applied(g, int(r["pos"]), *ref_alt_of(r))
        assert int(m["genotype"][site_of[i], int(r["sample"])]) == int(m["allele_of"][i]) - int(s["first_allele"]) + 1
        assert applied(g, int(s["pos"]), site_text(s), site_text(s, a)) == own, (i, r)
        assert int(s["tract"]) == int(r["tract"]) and int(s["contig"]) == int(r["contig"])
    assert (m["sites"]["n_alleles"] > 1).any() and (m["sites"]["n_alleles"] == 1).any() and (m["sites"]["n_flank"] > 0).any()
    assert (m["genotype"] == -1).any() or ns < 4
    assert m["sites"]["n_called"].sum() == len(recs) == m["alleles"]["n_samples"].sum()
    assert (np.diff(m["sites"]["tract"]) > 0).all()
    assert any(int(a["n_flank"]) < int(m["sites"][int(a["site"])]["n_flank"]) for a in m["alleles"])      # an allele completed from the site's flank


# ---- tjamd_site_ref_alt ----------------------------------------------------------------------------------------------------

def c_site_text(site, allele, k, capacity="fit"):
    """-> (return value, the text written or None)"""
    L = tj.lib()
    sb = np.asarray(site, SITE).reshape(1).copy()
    ab = None if allele is None else np.asarray(allele, ALLELE).reshape(1).copy()
    ap = None if ab is None else ab.ctypes.data
    n = L.tjamd_site_ref_alt(sb.ctypes.data, ap, k, None, 0)
    if n < 0:
        return n, None
    cap = n + 1 if capacity == "fit" else capacity
    out = GuardedHost(max(cap, 0))
    assert L.tjamd_site_ref_alt(sb.ctypes.data, ap, k, out.c, cap) == n
    out.check("out")
    if cap <= n:
        assert out.untouched()
        return n, None
    got = bytes(out.payload[: n + 1])
    assert got[-1] == 0
    return n, got[:-1].decode()


@pytest.mark.parametrize("k", [1, 4, 15, 32])
def test_site_ref_alt_writes_the_restatements_text(k):
    rng = random.Random(300 + k)
    n_pairs = 0
    for trial in range(1100):
        F = (0, k)[trial] if trial < 2 else rng.randint(0, k)
        ml = rng.randint(0, 40)
        Lr = ml + (rng.choice([0, 1, 2, 5, 400, MAX_LENGTH - ml]))
        site = np.zeros(1, SITE)[0]
        site["base"], site["ref_length"], site["min_length"], site["n_flank"] = rng.randrange(4), Lr, ml, F
        site["ref_flank"] = rng.getrandbits(2 * F) if F else 0
        site["flat"], site["tract"], site["pos"] = rng.randrange(1 << 40), rng.randrange(1 << 20), rng.randrange(1, 1 << 30)
        want = site_text(site)
        assert c_site_text(site, None, k) == (len(want), want) and len(want) == Lr - ml + 1 + F
        n_pairs += 1
        for la in (ml, rng.randint(ml, MAX_LENGTH)) if trial % 2 else (MAX_LENGTH,):
            al = np.zeros(1, ALLELE)[0]
            al["alt_length"], al["n_flank"], al["alt_flank"] = la, rng.randint(0, F), (rng.getrandbits(2 * F) if F else 0)
            want = site_text(site, al)
            assert c_site_text(site, al, k) == (len(want), want)
            n_pairs += 1
        if trial < 40:                                                       # one short, and much too short: sized, nothing written
            assert c_site_text(site, None, k, capacity=len(site_text(site))) == (len(site_text(site)), None)
            assert c_site_text(site, al, k, capacity=len(want)) == (len(want), None)
            assert c_site_text(site, al, k, capacity=0) == (len(want), None)
            assert tj.site_ref_alt(site, al, k) == want and tj.site_ref_alt(site, None, k) == site_text(site)
    assert n_pairs >= 2000
    # what has no text
    L = tj.lib()
    good, al = np.zeros(1, SITE), np.zeros(1, ALLELE)
    good["ref_length"], good["min_length"], al["alt_length"] = 3, 2, 2
    buf = GuardedHost(64)
    assert L.tjamd_site_ref_alt(None, None, k, buf.c, 64) == -1 and L.tjamd_site_ref_alt(None, al.ctypes.data, k, buf.c, 64) == -1
    assert L.tjamd_site_ref_alt(good.ctypes.data, None, k, buf.c, 64) == 2
    for field, value in (("n_flank", -1), ("n_flank", k + 1), ("base", 4), ("base", -1), ("min_length", 4)):
        bad = good.copy()
        bad[field] = value
        assert L.tjamd_site_ref_alt(bad.ctypes.data, None, k, buf.c, 64) == -1, (field, value)
    for kk in (0, 33, -1):
        assert L.tjamd_site_ref_alt(good.ctypes.data, al.ctypes.data, kk, buf.c, 64) == -1
    al["alt_length"] = 1                                                      # an allele shorter than min_length
    assert L.tjamd_site_ref_alt(good.ctypes.data, al.ctypes.data, k, buf.c, 64) == -1
    buf.check("out")
    with pytest.raises(tj.TatajubaAmdError):
        tj.site_ref_alt(good[0], al[0], k)


# ---- declarations and argument checks --------------------------------------------------------------------------------------

def _fields(code, name):
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s\s*;" % name, code)
    return [w for part in m.group(1).split(";") for w in re.sub(r"\s", "", re.sub(r"^\s*(long long|int|uint64_t)\s", "", part.strip())).split(",") if w]


def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    own = strip(os.path.join(ROOT, "include", "tatajuba_sites.h"))
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.SITE_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_sites.h"]
    assert len(others) >= 7
    for s in NEW_ENTRIES:
        for path in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(path)), (s, path)   # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS + tj.EFFECT_EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert "tatajuba_sites.h" in open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read()
    assert '#include "tatajuba_variants.h"' in own
    assert _fields(own, "tjamd_site") == list(SITE.names) and _fields(own, "tjamd_allele") == list(ALLELE.names)
    assert SITE.itemsize == 64 and [SITE.fields[x][1] for x in SITE.names] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56]
    assert ALLELE.itemsize == 32 and [ALLELE.fields[x][1] for x in ALLELE.names] == [0, 4, 8, 12, 16, 20, 24]
    assert L.tjamd_last_merge_variants_ms(None) == -1.0
    for name in ("merge_variants", "last_merge_variants_ms"):
        assert hasattr(tj.Counter, name)
    assert callable(tj.site_ref_alt)


def test_merge_variants_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    # (but for the counter where a device is visible: a refused call clears that counter's interval, so it is a real one there)
    counter = tj.Counter(15) if tj.device_count() > 0 else None
    handle = C.c_void_p(counter._h) if counter else fake
    na = GuardedHost(8)

    def call(c=handle, k=15, rec=fake, n=10, ns=2, nt=5, sites=fake, scap=10, alleles=fake, acap=10, gt=fake, aof=fake, uniq=fake, n_alleles=na.c):
        rc = L.tjamd_merge_variants(c, k, rec, n, ns, nt, sites, scap, alleles, acap, gt, aof, uniq, n_alleles)
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"rec": None}, "null record buffer"), ({"sites": None}, "null site or allele buffer"),
                    ({"alleles": None}, "null site or allele buffer"), ({"n_alleles": None}, "null h_n_alleles"),
                    ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"), ({"n": -1}, "n_records -1 outside"),
                    ({"n": 1 << 32}, "n_records 4294967296 outside"), ({"n": 1 << 31}, "n_records 2147483648 outside"),
                    ({"k": 0}, "kmer_size 0 outside [2,32]"), ({"k": 33}, "kmer_size 33 outside [2,32]"), ({"nt": -1}, "n_tracts -1 < 0"),
                    ({"scap": -1}, "capacities -1 and 10"), ({"acap": -1}, "capacities 10 and -1")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_merge_variants") and msg in err, (kw, got, err)
    assert na.untouched()
    na.check("h_n_alleles")
    if tj.device_count() == 0:                     # good arguments, but nothing to run on: named, before the handle is read
        for kw in ({}, {"n": 0}, {"gt": None, "aof": None, "uniq": None}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_merge_variants") and "TJAMD_ERR_NO_DEVICE" in err, (got, err)
        assert na.untouched()
    else:
        assert counter.last_merge_variants_ms() == -1.0
        counter.close()
