"""tjamd_merge_variants on the GPU against the string restatement of tests/test_sites_cabi.py: the hand cases field for field,
planted corpora (records from tjamd_tract_variants itself) at the segment widths on both sides of a wavefront, synthetic record
sets at the edges of the sort's and the scan's blocks, of the key's width and of the pass count, the widest site, every
refusal raised on the device, capacities and optional outputs, the eight-sample pipeline of tests/test_locate.py with the
features of tests/test_features.py (effects once per allele), and examples/merged_vcf.c.  d_sites, d_alleles, d_genotype,
d_allele_of and d_unique always sit in guarded buffers (tests/guarded.py), h_n_alleles in a guarded host buffer, every const
input is held frozen, and every call is made twice and must give the same bytes."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, GuardedHost, frozen, payload_pattern
from tests.test_effects import build as build_coding, dev_effects
from tests.test_features import dev_tract_features, gff3_of
from tests.test_locate import _dev, _p, dev_locate, dev_located_tracts, random_genome, same_entries, stats_on
from tests.test_sites_cabi import hand_records, merged_vcf_text, restate_merge_variants, site_text, unique_vcf_text, HAND_SITES
from tests.test_union_tracts import DNA, device_union, make_genome, reads_of, sample_of
from tests.test_variants import Tiling, dev_variants
from tests.test_variants_cabi import K, NS, pack, planted_union, restate_tract_variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAP = 3, 4
VAR, SITE, ALLELE, EF = tj.VARIANT_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE, tj.EFFECT_DTYPE
OUTPUTS = ("sites", "alleles", "genotype", "allele_of", "unique")


def _torch():
    return pytest.importorskip("torch")


def dev_merge(counter, k, recs, ns, n_tracts, want=None, site_cap="fit", allele_cap="fit", nulls=(), rd=None):
    """two calls of tjamd_merge_variants -> dict of the outputs as numpy (those not in `nulls`), n_sites, n_alleles; or, when the
    call is refused, (negative code, message, the guarded buffers).  Capacities: 'fit' = what the restatement finds, or a number"""
    torch = _torch()
    L = tj.lib()
    n = len(recs)
    rd = rd if rd is not None else (_dev(recs) if n else torch.zeros(64, dtype=torch.uint8, device="cuda"))
    scap = len(want["sites"]) if site_cap == "fit" else int(site_cap)
    acap = len(want["alleles"]) if allele_cap == "fit" else int(allele_cap)
    runs = []
    for _ in range(2):
        buf = {"sites": GuardedDevice(scap * SITE.itemsize), "alleles": GuardedDevice(acap * ALLELE.itemsize), "genotype": GuardedDevice(scap * ns * 2),
               "allele_of": GuardedDevice(n * 4), "unique": GuardedDevice(acap * VAR.itemsize)}
        na = GuardedHost(8)
        ptr = {x: (None if x in nulls else buf[x].c) for x in OUTPUTS}
        torch.cuda.synchronize()
        with frozen(rd):
            rc = L.tjamd_merge_variants(counter._h, k, _p(rd), n, ns, n_tracts, ptr["sites"], scap, ptr["alleles"], acap, ptr["genotype"], ptr["allele_of"],
                                        ptr["unique"], na.c)
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        for x in OUTPUTS:
            buf[x].check("d_" + x)
            assert x not in nulls or buf[x].untouched(), x
        na.check("h_n_alleles")
        if rc < 0:
            assert na.untouched() and counter.last_merge_variants_ms() == -1.0 and err.startswith("tjamd_merge_variants")
            return rc, err, buf
        n_sites, n_alleles = rc, int(na.view(np.int64)[0])
        assert n_sites <= scap and n_alleles <= acap and (n == 0 or counter.last_merge_variants_ms() > 0)
        got = {"n_sites": n_sites, "n_alleles": n_alleles, "sites": buf["sites"].view(SITE, n_sites), "alleles": buf["alleles"].view(ALLELE, n_alleles),
               "genotype": buf["genotype"].view(np.int16, n_sites * ns).reshape(n_sites, ns), "allele_of": buf["allele_of"].view(np.int32, n),
               "unique": buf["unique"].view(VAR, n_alleles)}
        for x, used in (("sites", n_sites * SITE.itemsize), ("alleles", n_alleles * ALLELE.itemsize), ("genotype", n_sites * ns * 2), ("unique", n_alleles * VAR.itemsize)):
            if x not in nulls:                                                # nothing behind what was found
                assert (buf[x].view(np.uint8)[used:] == payload_pattern(buf[x].nbytes)[used:]).all(), x
        runs.append(got)
    for x in OUTPUTS:
        assert runs[0][x].tobytes() == runs[1][x].tobytes(), x                # two runs: the same bytes
    return runs[0]


def check_merge(got, want, nulls=()):
    assert got["n_sites"] == len(want["sites"]) and got["n_alleles"] == len(want["alleles"])
    for x, dt in (("sites", SITE), ("alleles", ALLELE), ("unique", VAR)):
        if x in nulls:
            continue
        for f in dt.names:
            bad = np.flatnonzero(got[x][f] != want[x][f])
            assert len(bad) == 0, (x, f, bad[:5], got[x][bad[:3]], want[x][bad[:3]])
        assert got[x].tobytes() == want[x].tobytes(), x
    if "genotype" not in nulls:
        assert (got["genotype"] == want["genotype"]).all()
    if "allele_of" not in nulls:
        assert (got["allele_of"] == want["allele_of"]).all()


def merge_and_check(counter, k, recs, ns, n_tracts, **kw):
    want = restate_merge_variants(recs, ns, k, n_tracts=n_tracts)
    got = dev_merge(counter, k, recs, ns, n_tracts, want=want, **kw)
    assert isinstance(got, dict), got[:2]
    check_merge(got, want, kw.get("nulls", ()))
    return got, want


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(K)
    yield c
    c.close()


# ---- the hand cases ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["plain", "next", "near"])
def test_hand_cases(counter, which):
    recs = hand_records(which)
    got, want = merge_and_check(counter, K, recs, NS, 4)
    rows = []
    for s, row in zip(got["sites"], got["genotype"]):
        mine = got["alleles"][int(s["first_allele"]): int(s["first_allele"]) + int(s["n_alleles"])]
        rows.append((int(s["tract"]), int(s["contig"]), int(s["pos"]), tj.site_ref_alt(s, None, K), [tj.site_ref_alt(s, a, K) for a in mine],
                     [int(a["n_samples"]) for a in mine], row.tolist()))
    assert rows == HAND_SITES[which]


# ---- planted corpora -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [1, 2, 3, 8, 63, 64, 65, 130])
@pytest.mark.parametrize("k", [4, 15])
def test_planted_corpus(k, ns):
    """records from tjamd_tract_variants itself; the first site of planted_union has every sample (more than 64 and more than
    128 records at the two widest), the second one allele for all of them"""
    rng = random.Random(7000 * k + ns)
    g = random_genome(rng, 1500 if k == 4 else 3000, k)
    p = planted_union(g, k, ns, rng, max_sites=max(16, 1200 // ns))
    c = tj.Counter(k)
    ref = tj.Reference(c, g)
    same_entries(ref.download(), p["entries"])
    n_loc, loc = dev_locate(c, ref, p["keys"], 1)
    nt, lt = dev_located_tracts(c, p["keys"], p["mat"], p["tracts"], loc)
    u = Tiling(lt["keys"], lt["mat"], lt["tracts"], lt["tract_loc"])
    want_var, _, _ = restate_tract_variants(u.keys, u.mat, u.tracts, u.tract_loc, p["entries"], k)
    n, recs, off = dev_variants(c, ref, u, want=want_var)
    assert n > 0 and recs.tobytes() == want_var.tobytes()
    got, want = merge_and_check(c, k, recs, ns, nt)
    assert got["sites"]["n_called"].max() == ns and got["sites"]["n_called"].sum() == n
    if ns >= 8:
        assert (got["sites"]["n_alleles"] > 1).any() and (got["genotype"] == -1).any()
        one = got["sites"][(got["sites"]["n_alleles"] == 1) & (got["sites"]["n_called"] == ns)]
        assert len(one) >= 1                                                  # the site where every sample has the same allele
    # the order of the list N8 was given does not number the sites
    lst = list(range(nt))[::-1]
    want_rev, _, _ = restate_tract_variants(u.keys, u.mat, u.tracts, u.tract_loc, p["entries"], k, lst=lst)
    n2, rev, _ = dev_variants(c, ref, u, lst=lst, want=want_rev)
    got2, _ = merge_and_check(c, k, rev, ns, nt)
    assert got2["sites"]["tract"].tolist() == got["sites"]["tract"].tolist() and (got2["genotype"] == got["genotype"]).all()
    for f in ("pos", "ref_flank", "n_alleles", "n_called", "min_length"):
        assert (got2["sites"][f] == got["sites"][f]).all(), f
    ref.close()
    c.close()


# ---- synthetic record sets -------------------------------------------------------------------------------------------------

def synth_records(rng, n_records, ns, n_tracts, k, tracts=None, fill=0.8):
    """valid records built on the host, sample-major: per tract a place, a base, a reference length and reference flank, and a
    small pool of alleles (lengths, flank variants) that the samples draw from.  -> exactly n_records records"""
    per_sample = -(-n_records // ns)
    want_tracts = min(n_tracts, max(2, int(per_sample / fill) + 2))
    tracts = sorted(rng.sample(range(n_tracts), want_tracts)) if tracts is None else tracts
    if n_tracts - 1 not in tracts:
        tracts[-1] = n_tracts - 1                                            # the ends of the tract range
    if 0 not in tracts:
        tracts[0] = 0
    tracts = sorted(set(tracts))
    info = {}
    for t in tracts:
        Lr, F = rng.randint(1, 30), rng.choice([0, 0, 1, rng.randint(0, k), k])
        R_ref = "".join(rng.choice(DNA) for _ in range(k))
        pool = []
        for _ in range(rng.randint(1, 4)):
            la = rng.choice([x for x in (Lr - 2, Lr - 1, Lr + 1, Lr + 2, Lr + 9, 1023) if x >= 1])
            nf = rng.choice([0, F, rng.randint(0, F)])
            alt = list(R_ref[:nf])
            if nf:
                alt[nf - 1] = rng.choice([x for x in DNA if x != alt[nf - 1]])      # the outermost base differs, as N8 leaves it
            pool.append((la, nf, "".join(alt)))
        info[t] = (rng.randrange(1 << 40), rng.randrange(3), rng.randrange(1, 1 << 28), rng.randrange(4), Lr, R_ref, pool)
    recs = []
    for s in range(ns):
        for t in tracts:
            if len(recs) == n_records:
                break
            if rng.random() > fill and len(tracts) * (ns - s) > n_records - len(recs) + len(tracts):
                continue
            flat, contig, pos0, base, Lr, R_ref, pool = info[t]
            la, nf, alt = rng.choice(pool)
            recs.append((flat, t, s, contig, pos0 + min(la, Lr), rng.randrange(1 << 20), base, Lr, la, nf, 0, pack(R_ref[:nf]), pack(alt)))
    assert len(recs) == n_records, (len(recs), n_records)
    return np.array(recs, VAR)


@pytest.mark.parametrize("n_records", [1, 1023, 1024, 1025, 4095, 4096, 4097, 5000])
def test_sort_block_and_scan_block(counter, n_records):
    """n_records across the sort's block of 1024 and the scan's block of 4096; a site whose records and an allele run whose
    records straddle the boundary"""
    rng = random.Random(n_records)
    ns, nt, k = 40, 3000, 15
    recs = synth_records(rng, n_records, ns, nt, k) if n_records > 1 else synth_records(rng, 1, 1, nt, k, tracts=[0, 5, nt - 1])
    got, want = merge_and_check(counter, k, recs, ns, nt)
    if n_records >= 1025:
        srt = np.repeat(np.arange(got["n_sites"]), got["sites"]["n_called"])  # the site of every sorted position
        for edge in (1024, 4096):
            if n_records > edge:
                assert srt[edge - 1] == srt[edge], edge                       # a site's records on both sides of the block boundary
    if n_records == 5000:                                                     # one allele over the whole of such a site: its run straddles both boundaries
        for edge in (1024, 4096):
            recs2 = recs.copy()
            t_edge = int(got["sites"]["tract"][np.repeat(np.arange(got["n_sites"]), got["sites"]["n_called"])[edge]])
            mine = recs2["tract"] == t_edge
            first = recs2[np.flatnonzero(mine)[0]]
            for f in ("alt_length", "n_flank", "ref_flank", "alt_flank", "pos"):
                recs2[f][mine] = first[f]
            g2, _ = merge_and_check(counter, k, recs2, ns, nt)
            s2 = g2["sites"][g2["sites"]["tract"] == t_edge][0]
            assert s2["n_alleles"] == 1 and s2["n_called"] == mine.sum() > 1


def test_widest_site(counter):
    """4096 samples at one site: 4096 distinct alleles, and one allele"""
    ns, k = 4096, 15
    rng = random.Random(5)
    R_ref = "".join(rng.choice(DNA) for _ in range(k))
    lengths = [x for x in range(1, 1024) if x != 20]
    distinct, same = [], []
    for s in range(ns):
        la = lengths[s % len(lengths)]
        nf = 1 + s // len(lengths)                                           # the same length again: another flank
        alt = R_ref[: nf - 1] + DNA[(DNA.index(R_ref[nf - 1]) + 1) % 4]
        distinct.append((77, 3, s, 0, 1000 + min(la, 20), s, 2, 20, la, nf, 0, pack(R_ref[:nf]), pack(alt)))
        same.append((77, 3, s, 0, 1020, s, 2, 20, 21, 0, 0, 0, 0))
    got, _ = merge_and_check(counter, k, np.array(distinct, VAR), ns, 9)
    assert got["n_sites"] == 1 and got["n_alleles"] == ns and sorted(got["genotype"][0].tolist()) == list(range(1, ns + 1))
    got, _ = merge_and_check(counter, k, np.array(same, VAR), ns, 9)
    assert got["n_sites"] == 1 and got["n_alleles"] == 1 and (got["genotype"] == 1).all() and got["alleles"]["n_samples"][0] == ns
    # beside other sites, in the same wavefront of the reduction: a wide site among narrow ones
    mixed = np.concatenate([np.array(same[:70], VAR), synth_records(rng, 300, 70, 9, k, tracts=[0, 1, 2, 5, 8])])
    mixed = mixed[np.argsort(mixed["sample"], kind="stable")]
    merge_and_check(counter, k, mixed, 70, 9)


def test_key_width(counter):
    """alleles that differ only in the top base of a 32-base flank and alleles that differ only in n_flank, under a two-word
    key; then the same records under a one-word key (k = 15) and under two-word keys (k = 20 and k = 32 with 70 000 tracts)"""
    rng = random.Random(9)
    R = "".join(rng.choice(DNA) for _ in range(32))
    other = lambda ch: DNA[(DNA.index(ch) + 1) % 4]
    recs = []
    for s, (nf, alt) in enumerate([(32, R[:31] + other(R[31])), (32, R[:31] + other(other(R[31]))), (32, R[:31] + other(R[31])),
                                   (31, R[:30] + other(R[30])), (0, ""), (1, other(R[0])), (1, other(R[0]))]):
        recs.append((900, 6, s, 1, 5000 + 7, 3, 1, 7, 9, nf, 0, pack(R[:nf]), pack(alt)))
    # alleles that differ only in n_flank: the same alt_flank word (zero: all A) under two n_flank values
    A = "A" * 32
    Rc = "C" * 32
    for s, nf in enumerate((2, 3, 2)):
        recs.append((1200, 8, s, 1, 7000 + 4, 3, 3, 4, 6, nf, 0, pack(Rc[:nf]), pack(A[:nf])))
    recs = np.array(sorted(recs, key=lambda r: r[2]), VAR)
    got, _ = merge_and_check(counter, 32, recs, 7, 1 << 20)
    assert got["sites"]["n_alleles"].tolist() == [5, 2] and got["sites"]["n_flank"].tolist() == [32, 3]
    top = got["alleles"][got["alleles"]["n_flank"] == 32]
    assert len(top) == 2 and int(top[0]["alt_flank"]) ^ int(top[1]["alt_flank"]) >= 1 << 62 and top["n_samples"].tolist() in ([2, 1], [1, 2])
    assert got["alleles"][5:]["n_flank"].tolist() == [2, 3] and got["alleles"][5:]["n_samples"].tolist() == [2, 1]
    # random records: 17 bits of tract + 16 + 2k is 63 bits at k = 15 (one word) and 73 at k = 20 (two); k = 32 always has two
    base = synth_records(rng, 3000, 25, 70000, 15)
    first, _ = merge_and_check(counter, 15, base, 25, 70000)
    for k, nt in ((20, 70000), (32, 70000), (32, 1 << 31)):
        g, _ = merge_and_check(counter, k, base, 25, nt)
        assert all(g[x].tobytes() == first[x].tobytes() for x in OUTPUTS)       # the key's layout does not show in the result
    wide = synth_records(rng, 2000, 10, 3000, 32)
    merge_and_check(counter, 32, wide, 10, 3000)


@pytest.mark.parametrize("n_tracts", [1, 255, 256, 257, 65537])
def test_tract_range(counter, n_tracts):
    """tract 0 and tract n_tracts - 1 at the pass-count edges of the key"""
    rng = random.Random(n_tracts)
    for k in (4, 15):
        recs = synth_records(rng, 200 if n_tracts > 1 else 6, 6, n_tracts, k)
        assert recs["tract"].min() == 0 and recs["tract"].max() == n_tracts - 1
        merge_and_check(counter, k, recs, 6, n_tracts)


# ---- refusals raised on the device -----------------------------------------------------------------------------------------

def test_device_refusals(counter):
    rng = random.Random(21)
    k, ns, nt = 15, 12, 50
    good = synth_records(rng, 300, ns, nt, k)
    want = restate_merge_variants(good, ns, k, n_tracts=nt)
    check_merge(dev_merge(counter, k, good, ns, nt, want=want), want)
    t0 = int(good["tract"][0])
    same_tract = np.flatnonzero(good["tract"] == t0)
    assert len(same_tract) >= 2
    a, b = int(same_tract[0]), int(same_tract[1])
    cases = []
    dup = good.copy()                                                         # another record of b's sample moves to b's tract, with another allele
    j = int(np.flatnonzero((good["sample"] == good["sample"][b]) & (good["tract"] != t0))[0])
    dup[j] = dup[b]
    dup["alt_length"][j] = int(dup["alt_length"][b]) % 1000 + 1
    cases.append((dup, "a (tract, sample) pair occurs twice"))
    twice = np.concatenate([good, good[same_tract[:1]]])                      # the same record again (a list that names a tract twice)
    cases.append((twice, "a (tract, sample) pair occurs twice"))
    flat = good.copy(); flat["flat"][same_tract[1]] += 1
    cases.append((flat, "disagree in flat, contig, base or ref_length"))
    rf = good.copy()                                                          # two records of one tract whose reference flanks differ next to the tract
    rf["n_flank"][[a, b]] = 2
    rf["ref_flank"][a], rf["ref_flank"][b] = pack("AC"), pack("CC")
    rf["alt_flank"][[a, b]] = pack("GG")
    cases.append((rf, "disagree in ref_flank"))
    tr = good.copy(); tr["tract"][5] = nt
    cases.append((tr, "tract is outside [0, 50)"))
    sm = good.copy(); sm["sample"][299] = ns
    cases.append((sm, "sample is outside [0, 12)"))
    nf = good.copy(); nf["n_flank"][64] = k + 1
    cases.append((nf, "n_flank is outside 0..15"))
    neg = good.copy(); neg["n_flank"][1] = -1
    cases.append((neg, "n_flank is outside 0..15"))
    la = good.copy(); la["alt_length"][7] = 1024
    cases.append((la, "alt_length is outside 0..1023"))
    assert len(cases) == 9
    for bad, msg in cases:
        try:
            restate_merge_variants(bad, ns, k, n_tracts=nt)
            raise AssertionError("the restatement accepts: " + msg)
        except ValueError:
            pass
        rc, err, buf = dev_merge(counter, k, bad, ns, nt, site_cap=len(bad), allele_cap=len(bad))
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert all(buf[x].untouched() for x in OUTPUTS), msg                   # nothing was written
        check_merge(dev_merge(counter, k, good, ns, nt, want=want), want)     # the counter serves the next good call
    # host refusals with a real handle
    L = tj.lib()
    na = GuardedHost(8)
    assert L.tjamd_merge_variants(counter._h, k, None, 5, ns, nt, None, 0, None, 0, None, None, None, na.c) == -ERR_ARG
    assert L.tjamd_merge_variants(counter._h, 33, None, 0, ns, nt, None, 0, None, 0, None, None, None, na.c) == -ERR_ARG
    assert L.tjamd_merge_variants(counter._h, k, None, 0, 4097, nt, None, 0, None, 0, None, None, None, na.c) == -ERR_ARG
    assert na.untouched() and counter.last_merge_variants_ms() == -1.0


# ---- capacities and optional outputs ---------------------------------------------------------------------------------------

def test_capacity_and_null_outputs(counter):
    rng = random.Random(33)
    k, ns, nt = 15, 9, 400
    recs = synth_records(rng, 700, ns, nt, k)
    want = restate_merge_variants(recs, ns, k, n_tracts=nt)
    n_sites, n_alleles = len(want["sites"]), len(want["alleles"])
    assert n_alleles > n_sites > 10
    check_merge(dev_merge(counter, k, recs, ns, nt, want=want), want)
    # roomier buffers: nothing behind what was found (dev_merge checks the payload's pattern there)
    check_merge(dev_merge(counter, k, recs, ns, nt, want=want, site_cap=n_sites + 7, allele_cap=n_alleles + 5), want)
    # one short, either way: refused, nothing at or beyond the capacity (the buffers end there: the guards), what fits in its place
    for scap, acap in ((n_sites - 1, n_alleles), (n_sites, n_alleles - 1), (0, 0)):
        rc, err, buf = dev_merge(counter, k, recs, ns, nt, site_cap=scap, allele_cap=acap)
        assert rc == -ERR_CAP and f"{n_sites} sites and {n_alleles} alleles, caller capacities {scap} and {acap}" in err
        assert buf["sites"].view(SITE).tobytes() == want["sites"][:scap].tobytes() and buf["alleles"].view(ALLELE).tobytes() == want["alleles"][:acap].tobytes()
        assert buf["unique"].view(VAR).tobytes() == want["unique"][:acap].tobytes()
        assert (buf["genotype"].view(np.int16).reshape(-1, ns) == want["genotype"][:scap]).all()
    # every NULL-able output NULL, in turn and all together
    for nulls in (("genotype",), ("allele_of",), ("unique",), ("genotype", "allele_of", "unique")):
        got = dev_merge(counter, k, recs, ns, nt, want=want, nulls=nulls)
        check_merge(got, want, nulls)
    # no records: no sites, h_n_alleles = 0, nothing written
    got = dev_merge(counter, k, recs[:0], ns, nt, want=restate_merge_variants(recs[:0], ns, k), site_cap=4, allele_cap=4)
    assert got["n_sites"] == 0 and got["n_alleles"] == 0
    assert counter.merge_variants(k, None, 0, ns, nt, None, 0, None, 0) == (0, 0)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipeline():
    """the eight samples, the genome and the calls of tests/test_locate.py::test_eight_sample_pipeline_with_a_reference, up to the
    variant records of the variable tracts"""
    torch = _torch()
    saved = os.environ.pop("TATAJUBA_AMD_EDIT_DISTANCE", None)
    k, m, ns, maxd, lev, mm = 15, 4, 8, 1, 2, 1
    rng = random.Random(2024)
    pieces = make_genome(rng, n_tracts=2000)
    genome = "".join(left + DNA[b] * length + right for left, b, length, right in pieces)
    counters, ocov, streams = [], [], []
    for smp in range(ns):
        s = reads_of(sample_of(pieces, rng, smp), rng)
        c = tj.Counter(k)
        c.scan_host(s, m)
        assert c.finalise(1, 5) == 0
        counters.append(c); ocov.append(c.coverage); streams.append(bytes(s))
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
    stream = (genome + "\n").encode()
    ref = tj.Reference(merger, stream)
    entries = ref.download()
    n_located, loc = dev_locate(merger, ref, keys, mm, on_device=True)
    nt, lt = dev_located_tracts(merger, keys, mat, grouped["tracts"], loc, on_device=True)
    var = stats_on(merger, lt, nt, ns, ocov)["variable"]
    u = Tiling(lt["keys"], lt["mat"], lt["tracts"], lt["tract_loc"])
    want, want_off, _ = restate_tract_variants(u.keys, u.mat, u.tracts, u.tract_loc, entries, k, lst=var)
    n, recs, off = dev_variants(merger, ref, u, lst=var.tolist(), want=want)
    assert recs.tobytes() == want.tobytes()
    ms_variants = merger.last_tract_variants_ms()
    yield {"k": k, "m": m, "ns": ns, "pieces": pieces, "genome": genome, "stream": stream, "streams": streams, "merger": merger, "ref": ref, "u": u, "nt": nt,
           "var": var, "recs": recs, "ms_variants": ms_variants}
    ref.close()
    for c in counters + [merger]:
        c.close()
    if saved is not None:
        os.environ["TATAJUBA_AMD_EDIT_DISTANCE"] = saved


def test_effects_once_per_allele(pipeline, tmp_path):
    """tjamd_variant_effects on every record and on d_unique: a record's effect is its allele's.  Counts and times are printed,
    not asserted."""
    p = pipeline
    merger, k, ns, recs = p["merger"], p["k"], p["ns"], p["recs"]
    path = tmp_path / "genome.gff3"
    path.write_text(gff3_of([p["pieces"]], ["genome"]))
    feats, strings = tj.read_gff3(str(path), ["genome"])
    phase = tj.read_gff3_phase(str(path), ["genome"])
    assert len(feats) == 601
    ann = tj.Annotation(merger, p["ref"], feats)
    tf = dev_tract_features(merger, ann, p["u"])
    cod, _ = build_coding(merger, p["stream"], feats, phase)
    got, want = merge_and_check(merger, k, recs, ns, p["nt"])
    ms_merge = merger.last_merge_variants_ms()
    assert got["n_alleles"] < len(recs)                                       # samples share alleles: fewer walks
    effects_all = dev_effects(merger, cod, recs, tf)
    ms_all = merger.last_variant_effects_ms()
    effects_unique = dev_effects(merger, cod, got["unique"], tf)
    ms_unique = merger.last_variant_effects_ms()
    assert len(effects_unique) == got["n_alleles"]
    back = effects_unique[got["allele_of"]]
    for f in EF.names:                                                       # (no field of an effect names the sample)
        assert (effects_all[f] == back[f]).all(), f
    assert effects_all.tobytes() == back.tobytes()
    print(f"\n[sites] {len(recs)} variant records of {ns} samples -> {got['n_sites']} sites, {got['n_alleles']} alleles; tjamd_last_merge_variants_ms {ms_merge:.3f} ms "
          f"beside tjamd_last_tract_variants_ms {p['ms_variants']:.3f} ms; tjamd_last_variant_effects_ms {ms_all:.3f} ms on all records, {ms_unique:.3f} ms on d_unique")
    cod.close(); ann.close()


def test_merged_vcf_c_example(pipeline, tmp_path):
    p = pipeline
    exe, libdir = str(tmp_path / "merged_vcf"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "merged_vcf.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", exe])
    genome = p["genome"]
    fasta, gff = str(tmp_path / "ref.fa"), str(tmp_path / "ref.gff3")
    with open(fasta, "w") as fh:
        fh.write(">genome some text\n%s\n" % "\n".join(genome[j: j + 70] for j in range(0, len(genome), 70)))
    with open(gff, "w") as fh:
        fh.write(gff3_of([p["pieces"]], ["genome"]))
    files, samples = [], []
    for smp, s in enumerate(p["streams"]):
        name = "s %d.fq" % smp if smp == 1 else "s%d.fq" % smp
        f = str(tmp_path / name)
        with open(f, "wb") as fh:
            fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rd, b"I" * len(rd)) for i, rd in enumerate(s.split(b"\n")[:-1])))
        files.append(f); samples.append(name.replace(" ", "_"))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, "-r", fasta, "-u", "-e", gff, "-x", "1", "-k", str(p["k"]), "-m", str(p["m"]), "-c", "5", "-d", "1", "-l", "2", "-o", str(out)] + files,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = restate_merge_variants(p["recs"], p["ns"], p["k"], n_tracts=p["nt"])
    assert (out / "merged.vcf").read_text() == merged_vcf_text(["genome"], [len(genome)], samples, m)
    uniq = (out / "unique_variants.vcf").read_text()
    assert uniq == unique_vcf_text(["genome"], [len(genome)], m)
    assert len([x for x in uniq.splitlines() if not x.startswith("#")]) == len(m["alleles"])      # one row per allele
    tsv = (out / "variant_effects.tsv").read_text().splitlines()
    assert len(tsv) == 1 + len(m["alleles"]) and [int(x.split("\t")[-1]) for x in tsv[1:]] == m["alleles"]["n_samples"].tolist()
    assert f"{len(m['sites'])} sites with {len(m['alleles'])} distinct alleles" in r.stdout
