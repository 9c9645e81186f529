"""The depth step (include/tatajuba_depths.h: tjamd_site_depths) without a GPU: the entries are declared in their own header,
exported and prototyped and refuse bad arguments before any device call, the record matches the header, and the restatement
that the GPU tests (tests/test_depths.py) compare against is pinned two ways: the three hand cases of
tests/test_variants_cabi.py with GT, DP and AD written out by hand, and every row's class against what the N8 restatement
calls for a sample that has that row alone.  Then properties on planted corpora.

restate_site_depths is written from the rule in include/tatajuba_depths.h with strings: flank words are decoded to forward
text, a row is matched to an allele by comparing text.  The device does it with packed words, an XOR and a count of leading
zeros, once per row, and sums the counts in registers."""
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
from tests.test_sites_cabi import restate_merge_variants
from tests.test_variants_cabi import (A_MAT, C_MAT, DNA, K, NS, T_MAT, canonical_row, forward_right, hand_case, locate_and_tile, planted_union,
                                      restate_tract_variants, revcomp, signed_length, small_genome, unpack)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_site_depths", "tjamd_last_site_depths_ms"]
ERR_NO_DEVICE, ERR_ARG, ERR_CAP = 1, 3, 4
TR, LOC, SD = tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE, tj.SITE_DEPTH_DTYPE
INT32_MAX = 2 ** 31 - 1
OTHER = -1


def restate_site_depths(keys, mat, tracts, tract_loc, entries, k, merged):
    """-> dict: genotype (int16 [n_sites, ns]), depth (int32 [n_sites, ns]), allele_depth (int32 [n_sites + n_alleles, ns]),
    summary (SITE_DEPTH_DTYPE per site), classes (per site, the class of every row of its tract: 0 REF, j, OTHER = -1).
    ValueError for what the entry refuses on the device."""
    keys = np.asarray(keys, np.uint64).reshape(-1, 3)
    mat = np.asarray(mat)
    ns = mat.shape[1]
    sites, alleles = merged["sites"], merged["alleles"]
    at = {int(f): i for i, f in enumerate(entries["flat"].tolist())}
    want_first = 0
    for t in range(len(tracts)):
        if int(tracts["first"][t]) != want_first or int(tracts["n_rows"][t]) < 1:
            raise ValueError("tile")
        want_first += int(tracts["n_rows"][t])
    if want_first != len(keys):
        raise ValueError("tile")
    chain = 0
    for i, s in enumerate(sites):
        if int(s["n_alleles"]) < 1:
            raise ValueError("n_alleles")
        if int(s["first_allele"]) != chain:
            raise ValueError("chain")
        chain += int(s["n_alleles"])
    if len(sites) and chain != len(alleles):
        raise ValueError("chain")
    genotype = np.full((len(sites), ns), -1, np.int16)
    depth = np.zeros((len(sites), ns), np.int32)
    allele_depth = np.zeros((len(sites) + len(alleles), ns), np.int32)
    summary = np.zeros(len(sites), SD)
    classes = []
    for i, s in enumerate(sites):
        t = int(s["tract"])
        if not 0 <= t < len(tracts):
            raise ValueError("tract")
        loc = tract_loc[t]
        if int(loc["flat"]) < 0 or int(loc["flat"]) not in at:
            raise ValueError("entry")
        e = entries[at[int(loc["flat"])]]
        Lr, neg = int(e["length"]), int(e["neg_strand"])
        if int(s["flat"]) != int(loc["flat"]) or int(s["contig"]) != int(loc["contig"]) or int(s["ref_length"]) != Lr:
            raise ValueError("entry")
        mine = alleles[int(s["first_allele"]): int(s["first_allele"]) + int(s["n_alleles"])]
        for a in mine:
            if int(a["site"]) != i:
                raise ValueError("allele site")
            if not 0 <= int(a["n_flank"]) <= k:
                raise ValueError("n_flank")
        k_eff = k
        if t + 1 < len(tracts) and tract_loc["flat"][t + 1] >= 0 and tract_loc["contig"][t + 1] == loc["contig"]:
            overlap = int(loc["pos"]) + Lr + k - int(tract_loc["pos"][t + 1])
            if overlap > 0:
                k_eff = max(k - overlap, 0)
        R_ref = forward_right(e["ctx0"], e["ctx1"], k, neg)[:k_eff]
        texts = [(int(a["alt_length"]), int(a["n_flank"]), unpack(a["alt_flank"], int(a["n_flank"]))) for a in mine]
        first, n_rows = int(tracts["first"][t]), int(tracts["n_rows"][t])
        cls, lengths = [], []
        for row in range(first, first + n_rows):
            La = signed_length(keys[row, 2])
            lengths.append(La)
            if La < 1:
                cls.append(OTHER)
            elif La == Lr:
                cls.append(0)
            else:
                R_alt = forward_right(keys[row, 0], keys[row, 1], k, neg)[:k_eff]
                l1 = 0
                while l1 < k_eff and R_ref[k_eff - 1 - l1] == R_alt[k_eff - 1 - l1]:
                    l1 += 1
                nf = k_eff - l1
                hits = [j + 1 for j, (al, anf, text) in enumerate(texts) if al == La and anf == nf and text == R_alt[:nf]]
                cls.append(hits[0] if hits else OTHER)
        classes.append(cls)
        base = int(s["first_allele"]) + i
        n_alt = 0
        for smp in range(ns):
            col = np.maximum(mat[first: first + n_rows, smp].astype(np.int64), 0)
            depth[i, smp] = min(int(col.sum()), INT32_MAX)
            summary["depth"][i] += int(col.sum())
            for j in range(len(mine) + 1):
                allele_depth[base + j, smp] = min(sum(int(col[r]) for r in range(n_rows) if cls[r] == j), INT32_MAX)
            if col.max() > 0:
                m = int(np.argmax(col))                                       # the first of equal counts
                if lengths[m] >= 1:
                    if cls[m] == OTHER:
                        raise ValueError("modal")
                    genotype[i, smp] = cls[m]
            n_alt += genotype[i, smp] >= 1
        if n_alt != int(s["n_called"]):
            raise ValueError("n_called")
        summary["n_ref"][i] = (genotype[i] == 0).sum()
        summary["n_missing"][i] = (genotype[i] < 0).sum()
    return {"genotype": genotype, "depth": depth, "allele_depth": allele_depth, "summary": summary, "classes": classes}


def restate_both(keys, mat, tracts, loc, entries, k, lst=None):
    """N8, N12 and N13 restated on one tiling -> (records, merged, depths)"""
    recs, _, _ = restate_tract_variants(keys, mat, tracts, loc, entries, k, lst=lst)
    merged = restate_merge_variants(recs, np.asarray(mat).shape[1], k, n_tracts=len(tracts))
    return recs, merged, restate_site_depths(keys, mat, tracts, loc, entries, k, merged)


def tiling_of(entries, k, parts):
    """a permuted union built straight on index entries, as hand_case builds its own: parts = [(entry index or None, rows, counts
    [n_rows, ns])] in tiling order, a row = (length, forward right flank text or None for the entry's own).  The rows take the
    entry's left flank.  -> keys, mat, tracts, tract_loc"""
    from tests.test_locate_cabi import NOWHERE
    keys, mats, tracts, locs = [], [], [], []
    for ei, rows, m in parts:
        m = np.asarray(m, np.int32).reshape(len(rows), -1)
        tracts.append((len(keys), len(rows), 1, len(keys), 0, 0, 0))
        if ei is None:
            keys += [canonical_row("A", "T" * k, "T" * k, length) for length, _ in rows]
            locs.append(NOWHERE)
        else:
            e = entries[ei]
            neg = int(e["neg_strand"])
            B = DNA[3 - int(e["base"]) if neg else int(e["base"])]
            R = forward_right(e["ctx0"], e["ctx1"], k, neg)
            Lf = revcomp(unpack(e["ctx1"], k)) if neg else unpack(e["ctx0"], k)
            keys += [canonical_row(B, Lf, R if right is None else right, length) for length, right in rows]
            locs.append((int(e["flat"]), int(e["contig"]), int(e["pos"]), int(e["length"]), 0, neg, 1))
        mats.append(m)
    return np.array(keys, np.uint64).reshape(-1, 3), np.concatenate(mats), np.array(tracts, TR), np.array(locs, LOC)


# ---- the three hand cases of N8 and N12, with GT, DP and AD by hand -------------------------------------------------------
# Row classes of the AAA tract (Lr = 3; the rows a0 .. a6 and the matrices are those of tests/test_variants_cabi.py):
#   'plain' (k_eff = 4), alleles (2, 0) (4, 0) (4, 1, T) (4, 4, GCAT):  a0 REF  a1 2  a2 1  a3 REF (its length is the genome's,
#           whatever its flank)  a4 3  a5 4  a6 2 (the left flank is ignored)
#   'next'  (k_eff = 0), alleles (2, 0) (4, 0):  a0 REF  a1 2  a2 1  a3 REF  a4 2  a5 2  a6 2 (no flank is left to differ in)
#   'near'  (k_eff = 3), alleles (2, 0) (4, 0) (4, 1, T):  a0 REF  a1 2  a2 1  a3 REF  a4 3  a5 2 (its difference is cut off)  a6 2
# of the TTTTT tract (Lr = 5), alleles (4, 3, CAT) (6, 0):  t0 REF  t1 2  t2 1;   of the CCCCC tract (Lr = 5), allele (7, 0):  c0 REF  c1 1
# A sample's genotype is the class of its modal row: s2 (a3) and s8 (a0) have genotype 0 at AAA, s7 has no read there: -1.
A0, A1, A2, A3, A4, A5, A6 = [A_MAT[r].tolist() for r in range(7)]
_sum = lambda *rows: [sum(x) for x in zip(*rows)]
HAND_DEPTHS = {
    #            tract, GT of samples 0-8,                       DP,                           AD rows REF, allele 1, 2, ...
    "plain": [(1, [2, 1, 0, 3, 4, 2, 2, -1, 0], [8, 8, 8, 7, 9, 7, 11, 0, 10],
               [[1, 1, 8, 0, 0, 0, 1, 0, 9], [0, 7, 0, 0, 0, 0, 5, 0, 1], [7, 0, 0, 0, 0, 7, 5, 0, 0], [0, 0, 0, 7, 2, 0, 0, 0, 0], [0, 0, 0, 0, 7, 0, 0, 0, 0]]),
              (2, [2, 1, 0, -1, 0, 0, 0, 2, 0], [7, 6, 4, 0, 4, 4, 4, 4, 4],
               [[1, 0, 4, 0, 4, 4, 4, 1, 4], [0, 6, 0, 0, 0, 0, 0, 0, 0], [6, 0, 0, 0, 0, 0, 0, 3, 0]]),
              (3, [1, 0, 0, 0, 0, 0, -1, -1, -1], [5, 5, 5, 5, 5, 5, 0, 0, 0],
               [[2, 5, 5, 5, 5, 5, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0, 0, 0]])],
    "next": [(0, [2, 1, 0, 2, 2, 2, 2, -1, 0], [8, 8, 8, 7, 9, 7, 11, 0, 10],
              [[1, 1, 8, 0, 0, 0, 1, 0, 9], [0, 7, 0, 0, 0, 0, 5, 0, 1], [7, 0, 0, 7, 9, 7, 5, 0, 0]]),
             (1, [1] * 9, [1] * 9, [[0] * 9, [1] * 9])],
    "near": [(0, [2, 1, 0, 3, 2, 2, 2, -1, 0], [8, 8, 8, 7, 9, 7, 11, 0, 10],
              [[1, 1, 8, 0, 0, 0, 1, 0, 9], [0, 7, 0, 0, 0, 0, 5, 0, 1], [7, 0, 0, 0, 7, 7, 5, 0, 0], [0, 0, 0, 7, 2, 0, 0, 0, 0]])],
}
HAND_CLASSES = {"plain": [[0, 2, 1, 0, 3, 4, 2], [0, 2, 1], [0, 1]], "next": [[0, 2, 1, 0, 2, 2, 2], [1]], "near": [[0, 2, 1, 0, 3, 2, 2]]}


def test_the_rule_on_the_hand_cases():
    # the hand-written AD rows are sums of the matrices' rows by the classes in the comment above
    assert HAND_DEPTHS["plain"][0][3] == [_sum(A0, A3), A2, _sum(A1, A6), A4, A5] and HAND_DEPTHS["plain"][0][2] == A_MAT.sum(0).tolist()
    assert HAND_DEPTHS["next"][0][3] == [_sum(A0, A3), A2, _sum(A1, A4, A5, A6)] and HAND_DEPTHS["near"][0][3] == [_sum(A0, A3), A2, _sum(A1, A5, A6), A4]
    assert HAND_DEPTHS["plain"][1][3] == [T_MAT[0].tolist(), T_MAT[2].tolist(), T_MAT[1].tolist()] and HAND_DEPTHS["plain"][2][3] == C_MAT.tolist()
    for which, want in HAND_DEPTHS.items():
        keys, mat, tracts, loc, entries = hand_case(which)
        recs, m, d = restate_both(keys, mat, tracts, loc, entries, K)
        assert m["sites"]["tract"].tolist() == [w[0] for w in want], which
        assert d["classes"] == HAND_CLASSES[which], which
        row = 0
        for i, (_, gt, dp, ad) in enumerate(want):
            assert d["genotype"][i].tolist() == gt and d["depth"][i].tolist() == dp, (which, i)
            assert row == int(m["sites"]["first_allele"][i]) + i and len(ad) == int(m["sites"]["n_alleles"][i]) + 1
            assert d["allele_depth"][row: row + len(ad)].tolist() == ad, (which, i)
            row += len(ad)
            assert tuple(d["summary"][i].tolist()) == (gt.count(0), gt.count(-1), sum(dp))
        assert row == len(d["allele_depth"]) == len(m["sites"]) + len(m["alleles"])          # no holes
        # N12's genotype where it has one; its -1 cells split into 0 and -1
        assert ((d["genotype"] == m["genotype"]) | ((m["genotype"] == -1) & (d["genotype"] <= 0))).all()
    # what is refused
    keys, mat, tracts, loc, entries = hand_case("plain")
    recs, m, d = restate_both(keys, mat, tracts, loc, entries, K)

    def bad(what, **change):
        mm = {"sites": m["sites"].copy(), "alleles": m["alleles"].copy()}
        for name, (idx, value) in change.items():
            which, field = name.split("__")
            mm[which][field][idx] = value
        with pytest.raises(ValueError, match=what):
            restate_site_depths(keys, mat, tracts, loc, entries, K, mm)

    bad("tract", sites__tract=(0, 4))
    bad("entry", sites__tract=(0, 0))                                         # the unlocated tract
    bad("entry", sites__flat=(1, 12))
    bad("entry", sites__ref_length=(2, 6))
    bad("chain", sites__first_allele=(1, 3))
    bad("chain", sites__n_alleles=(2, 2))
    bad("n_alleles", sites__n_alleles=(0, 0))
    bad("allele site", alleles__site=(4, 0))
    bad("n_flank", alleles__n_flank=(2, K + 1))
    bad("modal", alleles__alt_length=(6, 8))                                  # s0's modal row c1 has no allele any more
    bad("n_called", sites__n_called=(0, 5))
    with pytest.raises(ValueError, match="n_called"):                         # the sites of a subset of the records
        restate_site_depths(keys, mat, tracts, loc, entries, K, restate_merge_variants(recs[recs["sample"] != 7], NS, K))
    with pytest.raises(ValueError, match="tile"):
        restate_site_depths(keys, mat, tracts[:-1], loc[:-1], entries, K, m)


def n8_class(keys, tracts, loc, entries, k, merged, site, row):
    """the class of a row by the N8 restatement: what it calls for a sample that has this row alone"""
    t = int(merged["sites"]["tract"][site])
    one = np.zeros((len(keys), 1), np.int32)
    one[row, 0] = 1
    recs, _, _ = restate_tract_variants(keys, one, tracts, loc, entries, k, lst=[t])
    La = signed_length(np.asarray(keys, np.uint64).reshape(-1, 3)[row, 2])
    if len(recs) == 0:
        return 0 if La == int(merged["sites"]["ref_length"][site]) else OTHER
    r = recs[0]
    assert len(recs) == 1 and int(r["row"]) == row and La >= 1
    s = merged["sites"][site]
    for j in range(int(s["n_alleles"])):
        a = merged["alleles"][int(s["first_allele"]) + j]
        nf = int(a["n_flank"])
        if int(a["alt_length"]) == int(r["alt_length"]) and nf == int(r["n_flank"]) and unpack(a["alt_flank"], nf) == unpack(r["alt_flank"], nf):
            return j + 1
    return OTHER


def check_classes_against_n8(keys, tracts, loc, entries, k, merged, d, max_rows=None):
    n = 0
    for i, cls in enumerate(d["classes"]):
        first = int(tracts["first"][int(merged["sites"]["tract"][i])])
        for r, c in enumerate(cls[:max_rows]):
            assert c == n8_class(keys, tracts, loc, entries, k, merged, i, first + r), (i, r)
            n += 1
    return n


def test_row_classes_are_what_n8_calls_for_the_row_alone():
    for which in ("plain", "next", "near"):
        keys, mat, tracts, loc, entries = hand_case(which)
        recs, m, d = restate_both(keys, mat, tracts, loc, entries, K)
        assert check_classes_against_n8(keys, tracts, loc, entries, K, m, d) == sum(map(len, HAND_CLASSES[which]))


# ---- properties on planted corpora ----------------------------------------------------------------------------------------

def planted_case(k, ns, seed, max_sites=60):
    """a planted union, located and tiled, with one sample's column zeroed on a few sites' tracts
    -> keys, mat, tracts, loc, entries, and the stream"""
    rng = random.Random(seed)
    stream = small_genome(rng, k)
    p = planted_union(stream, k, ns, rng, max_sites=max_sites)
    keys, mat, tracts, loc = locate_and_tile(p)
    mat = mat.copy()
    recs, m, _ = restate_both(keys, mat, tracts, loc, p["entries"], k)
    for i in range(0, len(m["sites"]), 3):                                    # unseen there: genotype -1
        t = int(m["sites"]["tract"][i])
        mat[int(tracts["first"][t]): int(tracts["first"][t]) + int(tracts["n_rows"][t]), i % ns] = 0
    return keys, mat, tracts, loc, p["entries"], stream


@pytest.mark.parametrize("k,ns,seed", [(4, 8, 21), (15, 5, 22), (32, 6, 23)])
def test_properties_on_planted_corpora(k, ns, seed):
    keys, mat, tracts, loc, entries, _ = planted_case(k, ns, seed)
    recs, m, d = restate_both(keys, mat, tracts, loc, entries, k)
    gt, dp, ad, sm = d["genotype"], d["depth"], d["allele_depth"], d["summary"]
    assert len(m["sites"]) > 10
    assert (gt[m["genotype"] >= 1] == m["genotype"][m["genotype"] >= 1]).all() and (gt[m["genotype"] < 0] <= 0).all()
    other = 0
    for i, s in enumerate(m["sites"]):
        t = int(s["tract"])
        rows = mat[int(tracts["first"][t]): int(tracts["first"][t]) + int(tracts["n_rows"][t])]
        assert (dp[i] == np.maximum(rows, 0).sum(0)).all()
        mine = ad[int(s["first_allele"]) + i: int(s["first_allele"]) + i + int(s["n_alleles"]) + 1]
        assert (mine.sum(0) <= dp[i]).all()
        other += int((dp[i] - mine.sum(0)).sum())
        for smp in range(ns):
            if gt[i, smp] >= 0:
                assert mine[gt[i, smp], smp] >= rows[:, smp].max() > 0
            else:
                assert rows[:, smp].max() <= 0                                # (no row of a planted union has a length below 1)
        assert tuple(sm[i].tolist()) == ((gt[i] == 0).sum(), (gt[i] < 0).sum(), dp[i].astype(np.int64).sum())
        assert (gt[i] >= 1).sum() == int(s["n_called"])
    # a corpus that holds every kind of cell
    assert (gt == 0).any() and (gt == -1).any() and (gt >= 1).any() and (m["sites"]["n_alleles"] >= 2).any() and other > 0
    assert check_classes_against_n8(keys, tracts, loc, entries, k, m, d, max_rows=12) > 50


# ---- declarations and argument checks --------------------------------------------------------------------------------------

def _fields(code, name):
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s\s*;" % name, code)
    return [w for part in m.group(1).split(";") for w in re.sub(r"\s", "", re.sub(r"^\s*(long long|int|uint64_t)\s", "", part.strip())).split(",") if w]


def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    own = strip(os.path.join(ROOT, "include", "tatajuba_depths.h"))
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.DEPTH_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_depths.h"]
    assert len(others) >= 8
    for s in NEW_ENTRIES:
        for path in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(path)), (s, path)   # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS + tj.EFFECT_EXPORTS + tj.SITE_EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert "tatajuba_depths.h" in open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read()
    assert '#include "tatajuba_sites.h"' in own
    assert _fields(own, "tjamd_site_depth") == list(SD.names)
    assert SD.itemsize == 16 and [SD.fields[x][1] for x in SD.names] == [0, 4, 8]
    assert L.tjamd_last_site_depths_ms(None) == -1.0
    for name in ("site_depths", "last_site_depths_ms"):
        assert hasattr(tj.Counter, name)


def test_site_depths_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    outs = [GuardedHost(64) for _ in range(4)]

    def call(c=fake, ref=fake, keys=fake, counts=fake, n=10, ns=2, tr=fake, nt=5, loc=fake, sites=fake, n_sites=3, alleles=fake, n_alleles=4, nulls=False):
        o = [None] * 4 if nulls else [x.c for x in outs]
        rc = L.tjamd_site_depths(c, ref, keys, counts, n, ns, tr, nt, loc, sites, n_sites, alleles, n_alleles, *o)
        return rc, L.tjamd_last_error().decode()

    for kw, rc, msg in [({"c": None}, ERR_ARG, "null counter or reference"), ({"ref": None}, ERR_ARG, "null counter or reference"),
                        ({"n": -1}, ERR_ARG, "n_union -1 < 0"), ({"n": 1 << 31}, ERR_CAP, "union rows"),
                        ({"ns": 0}, ERR_ARG, "n_samples 0 outside 1..4096"), ({"ns": 4097}, ERR_ARG, "n_samples 4097 outside 1..4096"),
                        ({"keys": None}, ERR_ARG, "null union buffers"), ({"counts": None}, ERR_ARG, "null union buffers"),
                        ({"nt": 0}, ERR_ARG, "n_tracts 0 for a union of 10 rows"), ({"nt": 11}, ERR_ARG, "n_tracts 11 for a union of 10 rows"),
                        ({"tr": None}, ERR_ARG, "null tract or tract location buffer"), ({"loc": None}, ERR_ARG, "null tract or tract location buffer"),
                        ({"n_sites": -1}, ERR_ARG, "n_sites -1, n_alleles 4: a count below 0"), ({"n_alleles": -1}, ERR_ARG, "n_sites 3, n_alleles -1: a count below 0"),
                        ({"sites": None}, ERR_ARG, "null site or allele buffer"), ({"alleles": None}, ERR_ARG, "null site or allele buffer"),
                        ({"n_sites": 6, "n_alleles": 6}, ERR_ARG, "6 sites for 5 tracts"), ({"n_alleles": 2}, ERR_ARG, "2 alleles for 3 sites"),
                        ({"ns": 4096, "n": 1 << 20, "nt": 1 << 19, "n_sites": 1 << 18, "n_alleles": 1 << 18}, ERR_ARG, "x 4096 samples: 2^31 cells or more"),
                        ({"n_alleles": 1 << 40}, ERR_ARG, "2^31 cells or more")]:
        got, err = call(**kw)
        assert got == -rc and err.startswith("tjamd_site_depths") and msg in err, (kw, got, err)
    if tj.device_count() == 0:                     # good arguments, but nothing to run on: named, before the handles are read
        for kw in ({}, {"n_sites": 0, "n_alleles": 0}, {"nulls": True}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_site_depths") and "TJAMD_ERR_NO_DEVICE" in err, (got, err)
    for x in outs:                                 # host memory handed in as the outputs stays as it was
        assert x.untouched()
        x.check("output")
