"""tjamd_site_depths on the GPU against the string restatement of tests/test_depths_cabi.py, with no difference allowed: the hand
cases, tilings built on a genome's index entries at every segment width (tracts on both sides of a chunk of S rows, sites on
both sides of the eight class accumulators, both strands, every k_eff, ties, modal rows without a length, unseen samples,
saturation), every refusal raised on the device, optional outputs, scratch reuse on one counter, the eight-sample pipeline of
tests/test_sites.py and examples/merged_vcf.c -D.  Records and sites come from tjamd_tract_variants and tjamd_merge_variants on
the same counter.  Outputs always sit in guarded buffers (tests/guarded.py), every const input is held frozen, and every call
is made twice and must give the same bytes."""
import os
import random
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, frozen
from tests.test_depths_cabi import HAND_DEPTHS, INT32_MAX, restate_both, restate_site_depths, tiling_of
from tests.test_locate import _dev, _p, same_entries
from tests.test_locate_cabi import restate_reference_index
from tests.test_sites import dev_merge, check_merge, pipeline  # noqa: F401  (pipeline: the module-scoped fixture, built here as there)
from tests.test_sites_cabi import MERGED_HEADER, merged_vcf_text, restate_merge_variants
from tests.test_variants import Tiling, dev_variants
from tests.test_variants_cabi import DNA, HAND_GENOME, K, NS, forward_right, hand_case, restate_tract_variants, small_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 3
SD = tj.SITE_DEPTH_DTYPE
OUTPUTS = ("genotype", "depth", "allele_depth", "summary")


def _torch():
    return pytest.importorskip("torch")


def dev_depths(counter, ref, u, sites, alleles, nulls=(), nt=None):
    """two calls of tjamd_site_depths -> dict of the outputs as numpy (those not in `nulls`); or, when the call is refused,
    (negative code, message, the guarded buffers)"""
    torch = _torch()
    L = tj.lib()
    ns, n_sites, n_alleles = u.ns, len(sites), len(alleles)
    pad = lambda a: _dev(a) if len(a) else torch.zeros(64, dtype=torch.uint8, device="cuda")
    sd, ad = pad(sites), pad(alleles)
    runs = []
    for _ in range(2):
        buf = {"genotype": GuardedDevice(n_sites * ns * 2), "depth": GuardedDevice(n_sites * ns * 4),
               "allele_depth": GuardedDevice((n_sites + n_alleles) * ns * 4), "summary": GuardedDevice(n_sites * SD.itemsize)}
        ptr = {x: (None if x in nulls else buf[x].c) for x in OUTPUTS}
        torch.cuda.synchronize()
        with frozen(u.kd, u.md, u.td, u.ld, sd, ad):
            rc = L.tjamd_site_depths(counter._h, ref._h, _p(u.kd), _p(u.md), u.nu, ns, _p(u.td), u.nt if nt is None else nt, _p(u.ld),
                                     _p(sd), n_sites, _p(ad), n_alleles, ptr["genotype"], ptr["depth"], ptr["allele_depth"], ptr["summary"])
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        for x in OUTPUTS:
            buf[x].check("d_" + x)
            assert x not in nulls or buf[x].untouched(), x
        if rc < 0:
            assert counter.last_site_depths_ms() == -1.0 and err.startswith("tjamd_site_depths")
            return rc, err, buf
        assert rc == n_sites and (n_sites == 0 or counter.last_site_depths_ms() > 0)
        runs.append({"genotype": buf["genotype"].view(np.int16).reshape(n_sites, ns), "depth": buf["depth"].view(np.int32).reshape(n_sites, ns),
                     "allele_depth": buf["allele_depth"].view(np.int32).reshape(n_sites + n_alleles, ns), "summary": buf["summary"].view(SD)})
    for x in OUTPUTS:
        assert runs[0][x].tobytes() == runs[1][x].tobytes(), x                # two runs: the same bytes
    return runs[0]


def check_depths(got, want, nulls=()):
    assert isinstance(got, dict), got[:2]
    for x in OUTPUTS:
        if x in nulls:
            continue
        if x == "summary":
            for f in SD.names:
                assert (got[x][f] == want[x][f]).all(), (f, np.flatnonzero(got[x][f] != want[x][f])[:5])
        else:
            bad = np.argwhere(got[x] != want[x])
            assert len(bad) == 0, (x, bad[:5], got[x][tuple(bad[0])], want[x][tuple(bad[0])])
        assert got[x].tobytes() == want[x].tobytes(), x


def whole_chain(counter, ref, keys, mat, tracts, loc, entries, k, lst=None, u=None):
    """N8, N12 and N13 on the device, each against its restatement -> (the tiling, merged (device), depths (device), restated depths)"""
    u = u or Tiling(keys, mat, tracts, loc)
    want_recs, want_m, want_d = restate_both(u.keys, u.mat, u.tracts, u.tract_loc, entries, k, lst=lst)
    n, recs, _ = dev_variants(counter, ref, u, lst="all" if lst is None else lst, want=want_recs)
    assert n == len(want_recs) and recs.tobytes() == want_recs.tobytes()
    m = dev_merge(counter, k, recs, u.ns, u.nt, want=want_m)
    check_merge(m, want_m)
    got = dev_depths(counter, ref, u, m["sites"], m["alleles"])
    check_depths(got, want_d)
    return u, m, got, want_d


# ---- the hand cases ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hand():
    c = tj.Counter(K)
    ref = tj.Reference(c, HAND_GENOME)
    same_entries(ref.download(), restate_reference_index(HAND_GENOME, K)[0])
    yield c, ref
    ref.close()
    c.close()


@pytest.mark.parametrize("which", ["plain", "next", "near"])
def test_hand_cases(hand, which):
    c, ref = hand
    keys, mat, tracts, loc, entries = hand_case(which)
    u, m, got, _ = whole_chain(c, ref, keys, mat, tracts, loc, entries, K)
    row = 0
    for i, (t, gt, dp, ad) in enumerate(HAND_DEPTHS[which]):
        assert int(m["sites"]["tract"][i]) == t and got["genotype"][i].tolist() == gt and got["depth"][i].tolist() == dp
        assert got["allele_depth"][row: row + len(ad)].tolist() == ad and tuple(got["summary"][i].tolist()) == (gt.count(0), gt.count(-1), sum(dp))
        row += len(ad)
    assert row == len(got["allele_depth"])


# ---- tilings built on a genome's entries -----------------------------------------------------------------------------------

def edge_tiling(entries, k, ns, rng, n_parts=48):
    """consecutive index entries as tracts (neighbours cut each other's right flank: k_eff = k, reduced and 0), an unlocated tract
    in front.  Tracts of 1, S - 1, S, S + 1 and 70 rows in turn; rows of the genome's length, of other lengths with the entry's
    or a changed right flank, and of length 0 and -1; per sample absent, one modal row and sometimes a lesser one, a tie, or a
    modal row without a length.  With ns >= 9: sites of exactly 1, 7, 8, 9 and (ns >= 17) 17 alleles, then one whose two rows of
    one class hold 2^30 each for sample 0.  -> keys, mat, tracts, loc and the kinds planted"""
    S = 1
    while S < ns and S < 64:
        S <<= 1
    usable = [i for i in range(len(entries)) if entries["length"][i] < 200]
    chosen, at = [], rng.randrange(0, 20)
    while len(chosen) < n_parts:                                              # (every run is an entry: neighbours leave no flank at all)
        chosen.append(usable[at])
        at += rng.choice([1, 2, 3, 5, 9, 20, 40])
    sizes = [x for x in (1, S - 1, S, S + 1, 70) if x >= 1]
    exact = ([1, 7, 8, 9] + ([17] if ns >= 17 else [])) if ns >= 9 else []
    parts = [(None, [(9, None)], np.ones((1, ns), np.int32))]
    kinds = set()
    for n_part, ei in enumerate(chosen):
        e = entries[ei]
        Lr, neg = int(e["length"]), int(e["neg_strand"])
        R = forward_right(e["ctx0"], e["ctx1"], k, neg)

        def changed():
            j = rng.randrange(k)
            return R[:j] + rng.choice([x for x in DNA if x != R[j]]) + R[j + 1:]
        if n_part < len(exact):                                               # exactly n alleles: n lengths, each some sample's modal row
            n = exact[n_part]
            rows = [(Lr, None)] + [(Lr + 1 + j, None) for j in range(n)]
            m = np.zeros((len(rows), ns), np.int32)
            for s in range(ns):
                m[1 + s % n if s < n or rng.random() < 0.7 else 0, s] = 9
                m[rng.randrange(len(rows)), s] += 2
        elif n_part == len(exact):                                            # 2^30 + 2^30 in one class
            rows = [(Lr, None), (Lr + 1, None), (Lr + 1, None)]
            m = np.zeros((3, ns), np.int32)
            m[0, :] = 3
            m[1, 0] = m[2, 0] = 1 << 30
            kinds.add("saturated")
        else:
            n_rows = sizes[n_part % len(sizes)]
            rows = []
            for _ in range(n_rows):
                r = rng.random()
                length = Lr if r < 0.25 else 0 if r < 0.32 else -1 if r < 0.36 else max(1, Lr + rng.choice([-3, -2, -1, 1, 2, 3]))
                rows.append((length, changed() if rng.random() < 0.35 else None))
            m = np.zeros((n_rows, ns), np.int32)
            for s in range(ns):
                r = rng.random()
                if r < 0.15:
                    continue                                                  # all-zero counts: not seen
                top = rng.randrange(n_rows)
                if r < 0.3 and n_rows > 1:                                    # a tie: the first in union order
                    a, b = rng.sample(range(n_rows), 2)
                    m[a, s] = m[b, s] = 5
                    kinds.add("tie")
                else:
                    m[top, s] = 9
                    if rng.random() < 0.3:
                        m[rng.randrange(n_rows), s] += 2
                    if rows[top][0] < 1:
                        kinds.add("modal without a length")
                if rng.random() < 0.05:
                    m[rng.randrange(n_rows), s] = -4                          # a count below 0 contributes nothing
        parts.append((ei, rows, m))
    keys, mat, tracts, loc = tiling_of(entries, k, parts)
    return keys, mat, tracts, loc, kinds


@pytest.fixture(scope="module")
def genomes():
    """per k: a counter, a genome of three dense contigs, its reference on the device and its restated entries"""
    made = {}

    def get(k):
        if k not in made:
            stream = small_genome(random.Random(900 + k), k)
            c = tj.Counter(k)
            ref = tj.Reference(c, stream)
            entries = restate_reference_index(stream, k)[0]
            same_entries(ref.download(), entries)
            made[k] = (c, ref, entries)
        return made[k]
    yield get
    for c, ref, _ in made.values():
        ref.close()
        c.close()


@pytest.mark.parametrize("k,ns", [(4, 1), (15, 3), (32, 9), (15, 64), (4, 65), (32, 130), (15, 9)])
def test_segment_widths_chunk_edges_and_allele_groups(genomes, k, ns):
    c, ref, entries = genomes(k)
    rng = random.Random(100 * k + ns)
    keys, mat, tracts, loc, kinds = edge_tiling(entries, k, ns, rng)
    u, m, got, want = whole_chain(c, ref, keys, mat, tracts, loc, entries, k)
    sites = m["sites"]
    assert len(sites) >= 10 and (got["genotype"] >= 1).any()
    assert ns == 1 or ((got["genotype"] == 0).any() and (got["genotype"] == -1).any())      # (one sample: a site is where it has an allele)
    assert "tie" in kinds or ns == 1
    if ns >= 9:
        assert "saturated" in kinds and {1, 7, 8, 9} <= set(sites["n_alleles"].tolist()) and (ns < 17 or 17 in sites["n_alleles"])
        assert (got["depth"] == INT32_MAX).sum() == 1 and (got["allele_depth"] == INT32_MAX).sum() == 1 and got["summary"]["depth"].max() >= 1 << 31
        assert "modal without a length" in kinds
    # the strands, the flank cut to nothing, cut in part and whole, the last tract of the tiling and of a contig
    neg = np.array([int(loc["neg_strand"][int(t)]) for t in sites["tract"]])
    assert ns == 1 or ((neg == 0).any() and (neg == 1).any())
    k_eff = []
    for t in sites["tract"].tolist():
        cut = k
        if t + 1 < len(tracts) and loc["contig"][t + 1] == loc["contig"][t]:
            cut = min(k, max(0, int(loc["pos"][t + 1]) - int(loc["pos"][t]) - int(loc["ref_length"][t])))
        k_eff.append(cut)
    assert ns == 1 or (0 in k_eff and k in k_eff and any(0 < x < k for x in k_eff))
    other = got["depth"].astype(np.int64).sum() - got["allele_depth"].astype(np.int64).sum()
    assert other > 0 or ns == 1                                               # depth on rows of class OTHER


def test_last_tract_and_site_counts_around_a_block(genomes):
    """S = 4: 64 sites fill one block of the grid.  63, 64 and 65 sites, the last of them on the last tract of the tiling, which is
    also the last of its contig"""
    k, ns = 15, 3
    c, ref, entries = genomes(k)
    rng = random.Random(77)
    last = [i for i in range(len(entries)) if entries["contig"][i] == 0][-1]            # the last run of contig 0
    parts = []
    for ei in range(last - 79, last + 1):
        Lr = int(entries["length"][ei])
        m = np.zeros((2, ns), np.int32)
        m[1, rng.randrange(ns)] = 4
        m[0, :] += rng.randrange(0, 3)
        parts.append((ei, [(Lr, None), (Lr + 1, None)], m))
    keys, mat, tracts, loc = tiling_of(entries, k, parts)
    u = Tiling(keys, mat, tracts, loc)
    for n_sites in (63, 64, 65):
        lst = list(range(80 - n_sites, 80))
        _, m, got, _ = whole_chain(c, ref, keys, mat, tracts, loc, entries, k, lst=lst, u=u)
        assert len(m["sites"]) == n_sites and int(m["sites"]["tract"][-1]) == 79


# ---- refusals raised on the device -----------------------------------------------------------------------------------------

def test_device_refusals(hand):
    c, ref = hand
    keys, mat, tracts, loc, entries = hand_case("plain")
    u, m, good, want = whole_chain(c, ref, keys, mat, tracts, loc, entries, K)
    sites, alleles = m["sites"], m["alleles"]
    cases = []

    def case(msg, **change):
        s, a = sites.copy(), alleles.copy()
        for name, (idx, value) in change.items():
            which, field = name.split("__")
            (s if which == "sites" else a)[field][idx] = value
        cases.append((msg, s, a, u))

    case("a site's tract is outside [0, 4)", sites__tract=(0, 4))
    case("a site's tract is outside [0, 4)", sites__tract=(2, -1))
    case("has no index entry, or its flat, contig or ref_length", sites__tract=(0, 0))            # the unlocated tract
    case("has no index entry, or its flat, contig or ref_length", sites__flat=(1, 12))
    case("has no index entry, or its flat, contig or ref_length", sites__contig=(1, 1))
    case("has no index entry, or its flat, contig or ref_length", sites__ref_length=(2, 6))
    case("do not chain from 0 to 7", sites__first_allele=(0, 1))
    case("do not chain from 0 to 7", sites__first_allele=(1, 3))
    case("do not chain from 0 to 7", sites__n_alleles=(2, 2))
    case("do not chain from 0 to 7", sites__n_alleles=(2, 1 << 30))
    case("a site has n_alleles < 1", sites__n_alleles=(0, 0))
    case("a site has n_alleles < 1", sites__n_alleles=(1, -2))
    case("an allele's site is not the site that holds it", alleles__site=(4, 0))
    case("an allele's n_flank is outside 0..4", alleles__n_flank=(2, K + 1))
    case("an allele's n_flank is outside 0..4", alleles__n_flank=(5, -1))
    case("modal row is a variant that the site's alleles do not hold", alleles__alt_length=(6, 8))
    case("n_called is not the number of samples with an allele", sites__n_called=(0, 5))
    broken = tracts.copy()
    broken["n_rows"][1] += 1                                                  # tracts 1 and 2 overlap
    cases.append(("the tracts do not tile the union", sites.copy(), alleles.copy(), Tiling(keys, mat, broken, loc)))
    assert len(cases) == 18
    for msg, s, a, uu in cases:
        with pytest.raises(ValueError):
            restate_site_depths(uu.keys, uu.mat, uu.tracts, uu.tract_loc, entries, K, {"sites": s, "alleles": a})
        rc, err, buf = dev_depths(c, ref, uu, s, a)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert all(buf[x].untouched() for x in OUTPUTS), msg                   # nothing was written
        check_depths(dev_depths(c, ref, u, sites, alleles), want)              # the counter serves the next good call
    # the sites of a subset of the records
    sub = restate_merge_variants(restate_tract_variants(keys, mat, tracts, loc, entries, K)[0][:-1], NS, K, n_tracts=4)
    rc, err, buf = dev_depths(c, ref, u, sub["sites"], sub["alleles"])
    assert rc == -ERR_ARG and "n_called" in err and all(buf[x].untouched() for x in OUTPUTS)
    # a reference of another k; host refusals with real handles
    other = tj.Counter(K + 1)
    rc, err, _ = dev_depths(other, ref, u, sites, alleles)
    assert rc == -ERR_ARG and f"built with k = {K}, the counter has k = {K + 1}" in err
    other.close()
    L = tj.lib()
    assert L.tjamd_site_depths(c._h, ref._h, _p(u.kd), _p(u.md), u.nu, NS, _p(u.td), u.nt, _p(u.ld), None, 3, None, 7, None, None, None, None) == -ERR_ARG
    assert L.tjamd_site_depths(c._h, ref._h, _p(u.kd), _p(u.md), u.nu, NS, _p(u.td), u.nt, _p(u.ld), None, 0, None, 0, None, None, None, None) == 0
    check_depths(dev_depths(c, ref, u, sites, alleles), want)


# ---- optional outputs and scratch reuse ------------------------------------------------------------------------------------

def test_null_outputs(genomes):
    k, ns = 15, 9
    c, ref, entries = genomes(k)
    keys, mat, tracts, loc, _ = edge_tiling(entries, k, ns, random.Random(5), n_parts=20)
    u, m, got, want = whole_chain(c, ref, keys, mat, tracts, loc, entries, k)
    for nulls in (("genotype",), ("depth",), ("allele_depth",), ("summary",), OUTPUTS):
        check_depths(dev_depths(c, ref, u, m["sites"], m["alleles"], nulls=nulls), want, nulls)
    torch = _torch()
    gt = torch.zeros(len(m["sites"]) * ns, dtype=torch.int16, device="cuda")
    sd, ad = _dev(m["sites"]), _dev(m["alleles"])
    assert c.site_depths(ref, _p(u.kd), _p(u.md), u.nu, ns, _p(u.td), u.nt, _p(u.ld), _p(sd), len(m["sites"]), _p(ad), len(m["alleles"]),
                         d_genotype=_p(gt)) == len(m["sites"])
    assert (gt.cpu().numpy().reshape(-1, ns) == want["genotype"]).all() and c.last_site_depths_ms() > 0


def test_one_counter_large_small_and_after_a_refusal():
    """the call's scratch is cut from the counter's block: a large problem, a small one, a refused one, the small one again"""
    k = 15
    stream = small_genome(random.Random(31), k, total=9000)
    entries = restate_reference_index(stream, k)[0]
    c = tj.Counter(k)
    ref = tj.Reference(c, stream)
    big = edge_tiling(entries, k, 70, random.Random(1), n_parts=250)[:4]
    small = edge_tiling(entries, k, 3, random.Random(2), n_parts=12)[:4]
    whole_chain(c, ref, *big, entries, k)
    u, m, got, want = whole_chain(c, ref, *small, entries, k)
    bad = m["sites"].copy()
    bad["n_called"][0] += 1
    rc, err, buf = dev_depths(c, ref, u, bad, m["alleles"])
    assert rc == -ERR_ARG and all(buf[x].untouched() for x in OUTPUTS)
    check_depths(dev_depths(c, ref, u, m["sites"], m["alleles"]), want)
    whole_chain(c, ref, *big, entries, k)
    ref.close()
    c.close()


# ---- the pipeline ----------------------------------------------------------------------------------------------------------

def depth_vcf_text(names, lengths, sample_names, m, d):
    """the multi-sample VCF as examples/merged_vcf.c -D writes it, from the two restatements"""
    head = MERGED_HEADER.replace('##INFO=<ID=AC', '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="reads on the tract">\n'
                                 '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="reads on the reference length and on each ALT allele">\n##INFO=<ID=AC')
    head = head.replace('Description="samples with a call"', 'Description="samples with a genotype, the reference\'s included"')
    out = head + "".join("##contig=<ID=%s,length=%d>\n" % (n, l) for n, l in zip(names, lengths))
    out += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n" % "\t".join(sample_names)
    for i, (s, (REF, alts)) in enumerate(zip(m["sites"], m["text"])):
        mine = m["alleles"][int(s["first_allele"]): int(s["first_allele"]) + int(s["n_alleles"])]
        ad = d["allele_depth"][int(s["first_allele"]) + i: int(s["first_allele"]) + i + len(mine) + 1]
        cells = ["%s:%d:%s" % ("." if g < 0 else str(int(g)), dp, ",".join(str(int(x)) for x in ad[:, smp]))
                 for smp, (g, dp) in enumerate(zip(d["genotype"][i], d["depth"][i]))]
        out += "%s\t%d\t.\t%s\t%s\t.\t.\tAC=%s;AN=%d;TID=tid_%06d\tGT:DP:AD\t%s\n" % (
            names[int(s["contig"])], int(s["pos"]), REF, ",".join(alts), ",".join(str(int(a["n_samples"])) for a in mine),
            len(cells) - int(d["summary"]["n_missing"][i]), int(s["tract"]), "\t".join(cells))
    return out


def test_eight_sample_pipeline(pipeline):  # noqa: F811
    p = pipeline
    merger, ref, u, k, ns = p["merger"], p["ref"], p["u"], p["k"], p["ns"]
    want_m = restate_merge_variants(p["recs"], ns, k, n_tracts=p["nt"])
    m = dev_merge(merger, k, p["recs"], ns, p["nt"], want=want_m)
    check_merge(m, want_m)
    ms_merge = merger.last_merge_variants_ms()
    want = restate_site_depths(u.keys, u.mat, u.tracts, u.tract_loc, ref.download(), k, want_m)
    got = dev_depths(merger, ref, u, m["sites"], m["alleles"])
    check_depths(got, want)
    gt = got["genotype"]
    assert (gt[want_m["genotype"] >= 1] == want_m["genotype"][want_m["genotype"] >= 1]).all() and (gt[want_m["genotype"] < 0] <= 0).all()
    assert (gt == 0).any() and (got["summary"]["n_ref"] + got["summary"]["n_missing"] + m["sites"]["n_called"] == ns).all()
    print(f"\n[depths] {len(m['sites'])} sites, {len(m['alleles'])} alleles, {ns} samples: {(gt == 0).sum()} reference cells, {(gt < 0).sum()} unseen; "
          f"tjamd_last_site_depths_ms {merger.last_site_depths_ms():.3f} ms beside tjamd_last_tract_variants_ms {p['ms_variants']:.3f} ms and "
          f"tjamd_last_merge_variants_ms {ms_merge:.3f} ms")


def test_merged_vcf_c_example_with_depths(pipeline, tmp_path):  # noqa: F811
    p = pipeline
    exe, libdir = str(tmp_path / "merged_vcf"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "merged_vcf.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", exe])
    genome = p["genome"]
    fasta = str(tmp_path / "ref.fa")
    with open(fasta, "w") as fh:
        fh.write(">genome some text\n%s\n" % "\n".join(genome[j: j + 70] for j in range(0, len(genome), 70)))
    files, samples = [], []
    for smp, s in enumerate(p["streams"]):
        f = str(tmp_path / ("s%d.fq" % smp))
        with open(f, "wb") as fh:
            fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rd, b"I" * len(rd)) for i, rd in enumerate(s.split(b"\n")[:-1])))
        files.append(f); samples.append("s%d.fq" % smp)
    m = restate_merge_variants(p["recs"], p["ns"], p["k"], n_tracts=p["nt"])
    d = restate_site_depths(p["u"].keys, p["u"].mat, p["u"].tracts, p["u"].tract_loc, p["ref"].download(), p["k"], m)
    texts = {}
    for flag in ((), ("-D",)):
        out = tmp_path / ("out" + "".join(flag))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, *flag, "-x", "1", "-k", str(p["k"]), "-m", str(p["m"]), "-c", "5", "-d", "1", "-l", "2", "-o", str(out)] + files,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        texts[flag] = (out / "merged.vcf").read_text()
    assert texts[()] == merged_vcf_text(["genome"], [len(genome)], samples, m)              # without the flag: what it was
    assert texts[("-D",)] == depth_vcf_text(["genome"], [len(genome)], samples, m, d)
    assert "\t0:" in texts[("-D",)] and "\t.:" in texts[("-D",)]
