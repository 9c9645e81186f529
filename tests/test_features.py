"""tjamd_annotation_create / tjamd_annotation_download / tjamd_tract_features on the GPU against the restatements of
tests/test_features_cabi.py: hand cases of the rule, the sizes around the kernels' edges, the wavefront path of the build (one
gene over thousands of points: the table index by index), a random differential, the longest modal length at the segment
widths on both sides of a wavefront, refusals, the eight-sample pipeline of tests/test_locate.py with a GFF3 file written
from its genome, and examples/annotated_tracts.c.  Outputs always sit in guarded buffers (tests/guarded.py), const inputs
are held frozen, every call is made twice and must give the same bytes."""
import ctypes as C
import os
import random
import subprocess
import time

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests.guarded import GuardedDevice, GuardedHost, frozen
from tests.test_features_cabi import (CDS, OTHER, REGION, FT, TF, features_of, name_of_tract, places_for, random_features, restate_table, restate_tract_features,
                                      restate_winner, restate_winners)
from tests.test_locate import BAD_SPANS_LOCATED, _dev, _p, dev_locate, dev_located_tracts, selected_line_at, stats_on
from tests.test_locate_cabi import NOWHERE, restate_located_tracts, restate_locate, restate_reference_index
from tests.test_tract_stats_cabi import record
from tests.test_union_tracts import DNA, _oracle_sample, device_union, make_genome, reads_of, sample_of
from tests.test_union_tracts_cabi import SELECTED_HEADER, hand_union, oracle_union_grouping, restate_union_tract_stats
from tests.test_variants import Tiling

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 3
TR, LOC = tj.UNION_TRACT_DTYPE, tj.LOCATION_DTYPE
K, CONTIG = 5, 60


def _torch():
    return pytest.importorskip("torch")


def locations(places, contig_len=CONTIG):
    """LOCATION_DTYPE of the test's own: (contig, pos) -> a located tract; None -> an unlocated one"""
    loc = np.array([NOWHERE] * len(places), LOC)
    for t, pl in enumerate(places):
        if pl is not None:
            loc[t] = (pl[0] * (contig_len + 1) + pl[1], pl[0], pl[1], 1, 0, 0, 1)
    return loc


def plain_tiling(loc, ns=1, rng=None):
    """one row per tract: tjamd_tract_features reads nothing else of a union, so no scan is needed"""
    n = len(loc)
    keys = np.array([record(i & 1, i, 7 * i + 1, 2 + i % 9) for i in range(n)], np.uint64)
    mat = np.ones((n, ns), np.int32) if rng is None else np.array([[rng.randrange(3) for _ in range(ns)] for _ in range(n)], np.int32)
    tracts = np.zeros(n, TR)
    tracts["first"], tracts["n_rows"], tracts["mode"] = np.arange(n), 1, np.arange(n)
    return Tiling(keys, mat, tracts, loc)


def annotate(counter, ref, feats):
    """the annotation of a FEATURE_DTYPE array, built twice: the same table both times, the features left alone"""
    with frozen(feats):
        a, b = tj.Annotation(counter, ref, feats), tj.Annotation(counter, ref, feats)
    assert counter.last_annotation_ms() > 0
    (pa, wa), (pb, wb) = a.download(), b.download()
    assert pa.tobytes() == pb.tobytes() and wa.tobytes() == wb.tobytes() and a.n_features == len(feats)
    b.close()
    return a, pa, wa


def dev_tract_features(counter, ann, u=None, loc=None, nt=None, with_union=True, counts=True):
    """-> TRACT_FEATURE_DTYPE per tract, or (negative code, message) when the call is refused.  u: a Tiling; or loc alone"""
    torch = _torch()
    L = tj.lib()
    ld = u.ld if u is not None else _dev(loc)
    n = (u.nt if u is not None else len(loc)) if nt is None else nt
    have = u is not None and with_union
    args = (_p(u.kd) if have else None, _p(u.md) if have and counts else None, u.nu if have else -5, u.ns if have else -5, _p(u.td) if have else None)
    runs = []
    for _ in range(2):
        out = GuardedDevice(n * TF.itemsize)
        torch.cuda.synchronize()
        with frozen(ld, *((u.kd, u.md, u.td) if u is not None else ())):
            rc = L.tjamd_tract_features(counter._h, ann._h, *args, n, _p(ld), out.c)
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        out.check("d_out")
        if rc < 0:
            assert out.untouched()                                  # (a broken tiling is found on the device by a launch of its own, in front of the records)
            assert counter.last_tract_features_ms() == -1.0 and err.startswith("tjamd_tract_features")
            return rc, err
        assert rc == n and (n == 0 or counter.last_tract_features_ms() > 0)
        runs.append(out.view(TF, n))
    assert runs[0].tobytes() == runs[1].tobytes()
    return runs[0]


def same_records(got, want):
    for f in TF.names:
        assert (got[f] == want[f]).all(), (f, np.flatnonzero(got[f] != want[f])[:5], got[f][:8], want[f][:8])
    assert got.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def base():
    """a counter and a reference of three contigs of 60 bases (the annotation takes the number of contigs from it)"""
    rng = random.Random(5)
    genome = "".join("".join(rng.choice(DNA) for _ in range(CONTIG)) + "\n" for _ in range(3)).encode()
    c = tj.Counter(K)
    ref = tj.Reference(c, genome)
    assert ref.n_contigs == 3
    yield c, ref
    ref.close()
    c.close()


# ---- the hand cases ----------------------------------------------------------------------------------------------------

EVERYWHERE = [(ct, pos) for ct in range(3) for pos in range(CONTIG)] + [None]
GENE, MRNA, EXON, CDS1 = (0, 10, 50, OTHER), (0, 10, 50, OTHER), (0, 20, 30, OTHER), (0, 22, 28, CDS)
HAND = {  # name: (features, {(contig, pos): winner} for the tracts the case is about)
    "nested, the CDS last": ([GENE, MRNA, EXON, CDS1], {(0, 24): 3, (0, 20): 2, (0, 9): 1, (0, 8): -1, (0, 49): 1, (0, 50): -1, (1, 24): -1}),
    "nested, the CDS first": ([CDS1, EXON, MRNA, GENE], {(0, 24): 0, (0, 20): 3, (0, 29): 3, (0, 49): 3, (0, 50): -1}),
    "two overlapping CDSs": ([(1, 5, 20, CDS), (1, 10, 30, CDS)], {(1, 4): 0, (1, 12): 0, (1, 19): 0, (1, 20): 1, (1, 29): 1, (1, 30): -1}),
    "the later CDS first in the file": ([(1, 10, 30, CDS), (1, 5, 20, CDS)], {(1, 4): 1, (1, 12): 0, (1, 19): 0, (1, 20): 0, (1, 8): 1}),
    "gene then exon": ([(2, 1, 40, OTHER), (2, 5, 9, OTHER)], {(2, 6): 1, (2, 20): 0}),
    "exon then gene": ([(2, 5, 9, OTHER), (2, 1, 40, OTHER)], {(2, 6): 1, (2, 3): 1, (2, 20): 1}),
    "a region and nothing else": ([(0, 1, CONTIG, REGION), (0, 30, 40, OTHER)], {(0, 5): -1, (0, 35): 1, (0, 59): -1}),
    "only regions": ([(0, 1, CONTIG, REGION), (1, 1, CONTIG, REGION)], {(0, 5): -1, (1, 0): -1}),
    "two features that meet": ([(0, 3, 17, OTHER), (0, 18, 33, CDS)], {(0, 16): 0, (0, 17): 1, (0, 1): -1, (0, 2): 0, (0, 32): 1, (0, 33): -1}),
    "the whole contig": ([(1, 1, CONTIG, OTHER)], {(1, K): 0, (1, 0): 0, (1, CONTIG - 1): 0, (0, K): -1, (2, 0): -1}),
    "an end beyond the contig": ([(1, 50, 1 << 30, OTHER), (2, 1, 2147483647, CDS)], {(1, 48): -1, (1, 49): 0, (1, 59): 0, (2, 0): 1, (2, 59): 1, (0, 59): -1}),
    "the same coordinates on contigs 0 and 2": ([(0, 10, 20, OTHER), (2, 10, 20, CDS), (2, 10, 20, OTHER)], {(0, 12): 0, (1, 12): -1, (2, 12): 1, (0, 20): -1, (2, 9): 1}),
    "five sharing a start, five an end": ([(0, 10, 10 + j, OTHER) for j in range(5)] + [(1, 30 + j, 40, OTHER) for j in range(5)],
                                           {(0, 9): 4, (0, 10): 4, (0, 11): 4, (0, 13): 4, (0, 14): -1, (1, 29): 5, (1, 30): 6, (1, 33): 9, (1, 39): 9, (1, 40): -1}),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(base, name):
    c, ref = base
    rows, about = HAND[name]
    feats = features_of(rows)
    u = plain_tiling(locations(EVERYWHERE))
    a, points, winner = annotate(c, ref, feats)
    want_points, want_winner = restate_table(feats)
    assert points.tolist() == want_points.tolist() and winner.tolist() == want_winner.tolist()
    got = dev_tract_features(c, a, u)
    same_records(got, restate_tract_features(feats, u.keys, u.mat, u.tracts, u.tract_loc))
    assert got["feature"][-1] == -1                                          # the unlocated tract
    for place, w in about.items():
        assert restate_winner(feats, *place) == w, (name, place)             # (the case says what it claims to)
        assert int(got["feature"][EVERYWHERE.index(place)]) == w, (name, place)
    assert (got["max_length"] == [2 + i % 9 for i in range(u.nt)]).all()
    a.close()


# ---- sizes around the kernels' edges -----------------------------------------------------------------------------------

def test_feature_and_tract_counts_around_the_edges(base):
    c, ref = base
    rng = random.Random(11)
    length = 3000
    for nf in (0, 1, 63, 64, 65, 4097):
        feats = random_features(rng, nf, 3, length)
        a, points, winner = annotate(c, ref, feats)
        want_points, want_winner = restate_table(feats)
        assert points.tolist() == want_points.tolist() and winner.tolist() == want_winner.tolist(), nf
        for nt in (1, 64, 65, 4097):
            places = [(rng.randrange(3), rng.randrange(length)) if rng.random() < 0.9 else None for _ in range(nt)]
            loc = locations(places, length)
            got = dev_tract_features(c, a, loc=loc)                          # no union: the lookup alone
            want = restate_tract_features(feats, None, None, None, loc)
            same_records(got, want)
            assert nf == 0 or nt < 64 or (got["feature"] >= 0).any()
            assert (got["max_length"] == 0).all()
        a.close()


@pytest.mark.parametrize("ns", [1, 3, 64, 65, 130])
def test_longest_modal_length(base, ns):
    """tracts of one row up to more than 64, counts with ties (0 .. 2), a sample without counts, a tract without counts, length
    fields that read negative (512 .. 1023), a tract all of whose lengths do"""
    c, ref = base
    rng = random.Random(100 + ns)
    rows_of = [1, 2, 3, 70, 1, 5, 64, 65] + [rng.randint(1, 4) for _ in range(70)]
    nt, nu = len(rows_of), sum(rows_of)
    keys = np.array([record(rng.randrange(2), rng.getrandbits(2 * K), rng.getrandbits(2 * K), rng.choice([1, 2, 5, 17, 511, 512, 700, 1023])) for _ in range(nu)], np.uint64)
    mat = np.array([[rng.randrange(3) for _ in range(ns)] for _ in range(nu)], np.int32)
    if ns > 1:
        mat[:, ns // 2] = 0                                                  # a sample that has nothing anywhere
    tracts = np.zeros(nt, TR)
    tracts["n_rows"] = rows_of
    tracts["first"] = np.cumsum([0] + rows_of[:-1])
    mat[tracts["first"][4]] = 0                                              # a tract that no sample has
    first5 = int(tracts["first"][5])
    keys[first5: first5 + 5] = [record(0, i, i, 600 + i) for i in range(5)]       # every length of this tract reads negative
    mat[first5: first5 + 5, 0] = [1, 2, 2, 0, 1]
    places = [(t % 3, (7 * t) % CONTIG) if t % 5 else None for t in range(nt)]
    u = Tiling(keys, mat, tracts, locations(places))
    feats = features_of([(0, 1, 30, OTHER), (1, 10, 50, CDS), (2, 5, 55, OTHER), (2, 20, 25, CDS)])
    a, _, _ = annotate(c, ref, feats)
    got = dev_tract_features(c, a, u)
    want = restate_tract_features(feats, keys, mat, tracts, u.tract_loc)
    same_records(got, want)
    assert want["max_length"][4] == 0 and want["max_length"][5] < 0 and (ns > 1 or want["max_length"][5] == 601 - 1024) and (want["max_length"] > 0).any()
    assert (want["feature"] >= 0).any() and (want["feature"] == -1).any()
    # d_counts NULL: max_length 0, the features unchanged; so without a union at all
    for kw in ({"counts": False}, {"with_union": False}):
        again = dev_tract_features(c, a, u, **kw)
        assert (again["feature"] == want["feature"]).all() and (again["max_length"] == 0).all()
    a.close()


# ---- the wavefront path of the build -----------------------------------------------------------------------------------

def test_one_gene_over_thousands_of_points(base):
    """the gene's range of indices is beyond the lane's walk and beyond one scan block of 4096; so is the CDS's in its middle"""
    c, ref = base
    n = 5000
    rows = [(1, 1, n, OTHER), (1, 1000, 3500, CDS)] + [(1, i, i, CDS if i % 7 == 0 else OTHER) for i in range(1, n + 1)] + [(1, 1, n + 50, REGION), (1, 2000, 2600, CDS)]
    feats = features_of(rows)
    a, points, winner = annotate(c, ref, feats)
    want_points, want_winner = restate_table(feats)
    assert len(points) == 2 * (n + 3)
    assert points.tolist() == want_points.tolist()
    bad = np.flatnonzero(winner != want_winner)
    assert len(bad) == 0, (bad[:5], winner[bad[:5]], want_winner[bad[:5]])
    places = [(1, p) for p in range(n + 2)] + [(0, 5), (2, 5)]
    loc = locations(places, n + 100)
    got = dev_tract_features(c, a, loc=loc)
    want = restate_winners(feats, places)
    assert (got["feature"] == want).all(), np.flatnonzero(got["feature"] != want)[:5]
    assert want[999] == 1 and want[998] == 1000 and want[6] == 8 and want[5] == 7 and want[n] == -1 and want[3600] == 3602
    a.close()


# ---- random differential -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_feature_sets_against_the_rule(base, seed):
    c, ref = base
    rng = random.Random(seed)
    length = 5000
    feats = random_features(rng, 300, 3, length)
    a, points, winner = annotate(c, ref, feats)
    want_points, want_winner = restate_table(feats)
    assert points.tolist() == want_points.tolist() and winner.tolist() == want_winner.tolist()
    places = places_for(rng, feats, 3, length, 2000)
    got = dev_tract_features(c, a, loc=locations(places, length))
    want = np.array([restate_winner(feats, ct, pos) for ct, pos in places], np.int32)
    differences = int((got["feature"] != want).sum())
    assert differences == 0 and len(places) > 2500 and (want >= 0).sum() > 500 and (want < 0).sum() > 10
    a.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refusals(base):
    torch = _torch()
    c, ref = base
    L = tj.lib()
    good = features_of([(0, 1, 30, OTHER), (1, 10, 50, CDS)])
    a, _, _ = annotate(c, ref, good)
    u = plain_tiling(locations(EVERYWHERE))
    dev_tract_features(c, a, u)
    assert c.last_annotation_ms() > 0 and c.last_tract_features_ms() > 0
    for row, msg in [((-1, 1, 2, OTHER), "feature 1: contig -1 outside [0, 3)"), ((3, 1, 2, OTHER), "feature 1: contig 3 outside [0, 3)"), ((0, 0, 2, CDS), "feature 1: start 0 < 1"),
                     ((0, -4, 2, REGION), "feature 1: start -4 < 1"), ((0, 5, 4, OTHER), "feature 1: end 4 < start 5"), ((0, 1, 2, 3), "feature 1: cls 3 outside 0..2"),
                     ((0, 1, 2, -1), "feature 1: cls -1 outside 0..2")]:
        bad = features_of([(0, 1, 2, OTHER), row])
        with frozen(bad):
            h = L.tjamd_annotation_create(c._h, ref._h, bad.ctypes.data, len(bad))
        err = L.tjamd_last_error().decode()
        assert not h and err.startswith("tjamd_annotation_create") and msg in err, (row, err)
        assert c.last_annotation_ms() == -1.0
        with pytest.raises(tj.TatajubaAmdError):
            tj.Annotation(c, ref, bad)
    # the annotation built before is as it was
    got = dev_tract_features(c, a, u)
    same_records(got, restate_tract_features(good, u.keys, u.mat, u.tracts, u.tract_loc))
    # n_samples, with a union only
    for ns in (0, 4097):
        rc = L.tjamd_tract_features(c._h, a._h, _p(u.kd), _p(u.md), u.nu, ns, _p(u.td), u.nt, _p(u.ld), _p(u.ld))
        assert rc == -ERR_ARG and f"n_samples {ns} outside 1..4096" in L.tjamd_last_error().decode() and c.last_tract_features_ms() == -1.0
    # tracts that do not tile the union (five rows, as the spans are written)
    k5, m5, _ = hand_union()
    for spans in BAD_SPANS_LOCATED:
        bad = np.zeros(len(spans), TR)
        bad["first"], bad["n_rows"] = [s[0] for s in spans], [s[1] for s in spans]
        b = Tiling(k5, m5, bad, locations([(0, 3)] * len(spans)))
        rc, err = dev_tract_features(c, a, b)
        assert rc == -ERR_ARG and "do not tile the union" in err, (spans, rc, err)
        got = dev_tract_features(c, a, b, with_union=False)                  # without a union the tiling is not read
        assert (got["feature"] == 0).all() and (got["max_length"] == 0).all()
    # n_tracts = 0 writes nothing; an empty annotation gives -1 everywhere
    assert len(dev_tract_features(c, a, loc=locations([(0, 3)]), nt=0)) == 0
    empty, points, _ = annotate(c, ref, features_of([]))
    assert len(points) == 0 and empty.n_features == 0
    assert (dev_tract_features(c, empty, u)["feature"] == -1).all()
    # download: a capacity one short writes nothing and says what is needed
    hp, hw = GuardedHost(4 * 8), GuardedHost(4 * 4)
    assert L.tjamd_annotation_download(a._h, hp.c, hw.c, 3) == 4 and hp.untouched() and hw.untouched()
    assert L.tjamd_annotation_download(a._h, hp.c, hw.c, 4) == 4
    hp.check("h_points"); hw.check("h_winner")
    assert hp.view(np.uint64).tolist() == [1, 31, (1 << 32) | 10, (1 << 32) | 51] and hw.view(np.int32).tolist() == [0, -1, 1, -1]
    # another device: only where there is one
    if torch.cuda.device_count() > 1:
        other = tj.Counter(K, device=1)
        with pytest.raises(tj.TatajubaAmdError, match="the reference lives on device 0, the counter on device 1"):
            tj.Annotation(other, ref, good)
        rc = L.tjamd_tract_features(other._h, a._h, None, None, 0, 0, None, 1, _p(u.ld), _p(u.ld))
        assert rc == -ERR_ARG and "the annotation lives on device 0, the counter on device 1" in L.tjamd_last_error().decode()
        other.close()
    empty.close()
    a.close()


# ---- the pipeline ------------------------------------------------------------------------------------------------------

def gff3_of(pieces_per_contig, names):
    """a GFF3 text from make_genome's pieces: per contig one region, and per ten pieces a gene over the first seven, an mRNA
    over the same and a CDS over the second to the fifth; the last three pieces of every ten are intergenic"""
    lines = ["##gff-version 3"]
    for name, pieces in zip(names, pieces_per_contig):
        starts, at = [], 0
        for left, b, length, right in pieces:
            starts.append(at)
            at += len(left) + length + len(right)
        starts.append(at)
        lines.append(f"{name}\ttest\tregion\t1\t{at}\t.\t+\t.\tID={name}:1..{at}")
        for j in range(0, len(pieces) - 9, 10):
            g = f"{name}-g{j // 10}"
            strand = "+-"[(j // 10) % 2]
            lines.append(f"{name}\ttest\tgene\t{starts[j] + 1}\t{starts[j + 7]}\t.\t{strand}\t.\tID=gene-{g};Name={g}")
            lines.append(f"{name}\ttest\tmRNA\t{starts[j] + 1}\t{starts[j + 7]}\t.\t{strand}\t.\tID=rna-{g};Parent=gene-{g}")
            lines.append(f"{name}\ttest\tCDS\t{starts[j + 1] + 1}\t{starts[j + 5]}\t.\t{strand}\t0\tParent=rna-{g};ID=cds-{g};product=x")
    return "\n".join(lines) + "\n"


def test_eight_sample_pipeline_features(monkeypatch, tmp_path):
    """the eight samples, the genome and the calls of tests/test_locate.py::test_eight_sample_pipeline_with_a_reference, then
    the features of a GFF3 file written from the genome's pieces.  The times are printed, not asserted."""
    torch = _torch()
    monkeypatch.delenv("TATAJUBA_AMD_EDIT_DISTANCE", raising=False)
    k, m, ns, maxd, lev, mm = 15, 4, 8, 1, 2, 1
    rng = random.Random(2024)
    pieces = make_genome(rng, n_tracts=2000)
    genome = "".join(left + DNA[b] * length + right for left, b, length, right in pieces)
    counters, ocov = [], []
    for smp in range(ns):
        s = reads_of(sample_of(pieces, rng, smp), rng)
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
    ref = tj.Reference(merger, (genome + "\n").encode())
    n_located, loc = dev_locate(merger, ref, keys, mm, on_device=True)
    nt, lt = dev_located_tracts(merger, keys, mat, grouped["tracts"], loc, on_device=True)
    stats = stats_on(merger, lt, nt, ns, ocov)
    u = Tiling(lt["keys"], lt["mat"], lt["tracts"], lt["tract_loc"])
    # the GFF3 file, gzip as annotations usually come
    import gzip
    path = tmp_path / "genome.gff3.gz"
    with gzip.open(path, "wt") as fh:
        fh.write(gff3_of([pieces], ["genome"]))
    feats, strings = tj.read_gff3(str(path), ["genome"])
    assert len(feats) == 1 + 3 * 200 and tj.read_gff3.last_skipped == 0
    with frozen(feats):
        ann = tj.Annotation(merger, ref, feats)
    ms_build = [merger.last_annotation_ms()]
    again = tj.Annotation(merger, ref, feats)
    ms_build.append(merger.last_annotation_ms())
    assert ann.download()[1].tobytes() == again.download()[1].tobytes()
    again.close()
    got = dev_tract_features(merger, ann, u)
    want = restate_tract_features(feats, u.keys, u.mat, u.tracts, u.tract_loc)
    same_records(got, want)
    sel = stats["selected"]
    n_yes, n_no = int((got["feature"][sel] >= 0).sum()), int((got["feature"][sel] < 0).sum())
    assert n_yes > 0 and n_no > 0, (n_yes, n_no)
    located = u.tract_loc["flat"] >= 0
    assert (got["feature"][~located] == -1).all() and (got["max_length"][located] > 0).all()
    types = [tj.gff3_string(strings, int(feats["type_off"][f])) for f in got["feature"] if f >= 0]
    assert set(types) == {"CDS", "mRNA"}                                     # the CDS where there is one, else the last of gene and mRNA
    # the times: the timers of the first and the second call, then tjamd_tract_features beside the yardstick tjamd_locate on
    # the same union, both between two events on one stream
    out = torch.zeros(nt * TF.itemsize, dtype=torch.uint8, device="cuda")
    locs = torch.zeros(nu * LOC.itemsize, dtype=torch.uint8, device="cuda")
    ms_timer = []
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    merger.set_stream(side.cuda_stream)
    ms = {}
    with torch.cuda.stream(side):
        for name in ("locate", "features", "locate", "features"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(side)
            if name == "features":
                rc = L.tjamd_tract_features(merger._h, ann._h, _p(u.kd), _p(u.md), u.nu, ns, _p(u.td), u.nt, _p(u.ld), _p(out))
            else:
                rc = L.tjamd_locate(merger._h, ref._h, _p(keys), nu, mm, _p(locs))
            e1.record(side)
            e1.synchronize()
            assert rc >= 0, L.tjamd_last_error()
            ms[name] = (e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0))
            ms_timer.append(merger.last_tract_features_ms() if name == "features" else merger.last_locate_ms())
    print(f"\n[features] {len(feats)} features, {2 * int((feats['cls'] != 0).sum())} points; union {nu} rows x {ns} samples, {nt} tracts, {len(sel)} selected "
          f"({n_yes} annotated, {n_no} not): tjamd_last_annotation_ms {ms_build[0]:.3f} ms (second call {ms_build[1]:.3f} ms); "
          f"tjamd_last_tract_features_ms {ms_timer[1]:.3f} ms (second call {ms_timer[3]:.3f} ms), tjamd_last_locate_ms {ms_timer[0]:.3f} ms ({ms_timer[2]:.3f} ms); "
          f"between events on one stream, wait included: tjamd_tract_features {ms['features'][0]:.3f} ms (host {ms['features'][1]:.3f} ms), "
          f"tjamd_locate {ms['locate'][0]:.3f} ms (host {ms['locate'][1]:.3f} ms)")
    assert min(ms_build) > 0 and min(ms_timer) > 0
    merger.set_stream(0)
    ann.close()
    ref.close()
    for c in counters + [merger]:
        c.close()


# ---- the example -------------------------------------------------------------------------------------------------------

TRACT_LIST_HEADER = "tract_id\tcontig_name\tfeature_type\tfeature\tlocation_in_contig\tmax_tract_length\tref_tract_length\ttract\tref_tract\n"
ANNOTATED_HEADER = SELECTED_HEADER.replace("tract_id\t", "tract_id\tGFF3_info\t", 1)


def test_annotated_tracts_c_example(tmp_path):
    exe, libdir = str(tmp_path / "annotated_tracts"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "annotated_tracts.c"),
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
        fh.write(gff3_of(parts, names) + "other\ttest\tgene\t1\t100\t.\t+\t.\tID=elsewhere\n##FASTA\n>contig0\nACGT\n")
    files, recs, covs = [], [], []
    for smp in range(2):
        s = reads_of(sample_of(pieces, rng, smp), rng)
        reads = bytes(s).split(b"\n")[:-1]
        f = str(tmp_path / f"s{smp}.fq")
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
    # the same pipeline from the oracle and the restatements, as tests/test_locate.py does for located_tracts.c
    _, _, keys_o, mat_o = orc.merge_samples(np.frombuffer(np.concatenate(recs).tobytes(), np.uint64).reshape(-1, 3), [len(x) for x in recs])
    g = oracle_union_grouping(keys_o, mat_o, k, 1, 2)
    first = np.asarray(g["groups"]["first"], np.int64)
    tracts = np.zeros(len(first), TR)
    tracts["first"], tracts["n_rows"] = first, np.diff(np.r_[first, len(keys_o)])
    tracts["n_context"], tracts["indel"] = g["groups"]["n_context"], g["groups"]["indel"]
    tracts["mode"], tracts["lev_distance"], tracts["integral"] = g["mode"], g["lev_distance"], g["integral"]
    entries, n_contigs = restate_reference_index(("\n".join(contigs) + "\n").encode(), k)
    loc = restate_locate(entries, keys_o, mm)
    lt = restate_located_tracts(keys_o, mat_o, tracts, loc)
    perm = lt["perm"]
    pk, pm, tl = keys_o[perm], mat_o[perm], lt["tract_loc"]
    ids = np.repeat(np.arange(len(lt["tracts"])), lt["tracts"]["n_rows"])
    st = restate_union_tract_stats(pk, pm, covs, ids, lt["tracts"]["lev_distance"], ref_length=lt["ref_length"])
    sel, var = np.flatnonzero(st["selected"]), np.flatnonzero(st["variable"])
    nt = len(lt["tracts"])
    feats, strings = tj.read_gff3(gff, names)
    assert tj.read_gff3.last_skipped == 1 and len(feats) == 2 + 3 * 20 and (feats["contig"] == 1).any()
    tf = restate_tract_features(feats, pk, pm, lt["tracts"], tl)
    ident = lambda t: tj.gff3_string(strings, int(feats["id_off"][tf["feature"][t]]))
    yes, no = [t for t in sel if tf["feature"][t] >= 0], [t for t in sel if tf["feature"][t] < 0]
    assert len(yes) > 0 and len(no) > 0 and (tl["contig"][yes] == 1).any()
    assert r.stdout.strip().splitlines()[-1] == f"From {nt} tracts, {len(yes)} interesting ones are annotated and {len(no)} interesting ones are not annotated"
    line = lambda t: selected_line_at(t, tl["flat"][t], st["n_present"][t], st["lev_distance"][t], st["reldiff"][t])
    assert (out / "selected_tracts_unknown.tsv").read_text() == SELECTED_HEADER + "".join(line(t) for t in no)
    assert (out / "selected_tracts_annotated.tsv").read_text() == ANNOTATED_HEADER + "".join(line(t).replace("\t", "\t" + ident(t) + "\t", 1) for t in yes)
    at = {int(f): i for i, f in enumerate(entries["flat"])}
    want = TRACT_LIST_HEADER
    for t in range(nt):
        if tl["flat"][t] < 0:
            continue
        e, f, mode = entries[at[int(tl["flat"][t])]], int(tf["feature"][t]), pk[int(lt["tracts"]["mode"][t])]
        want += "tid_%06d\t%s\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (
            t, names[int(tl["contig"][t])], tj.gff3_string(strings, int(feats["type_off"][f])) if f >= 0 else "nc", ident(t) if f >= 0 else "unannotated",
            tl["pos"][t], tf["max_length"][t], e["length"], name_of_tract(mode[0], mode[1], int(mode[2]) & 3, k, tl["neg_strand"][t]),
            name_of_tract(e["ctx0"], e["ctx1"], e["base"], k, e["neg_strand"]))
    assert (out / "tract_list.tsv").read_text() == want
    assert "\tnc\tunannotated\t" in want and "\tCDS\tcds-" in want and "\tmRNA\trna-" in want and (tl["flat"] < 0).any() and (tl["neg_strand"] == 1).any()
    bed = "".join("%s\t%d\t%d\ttid_%06d\n" % (names[int(tl["contig"][t])], tl["pos"][t], tl["pos"][t] + tl["ref_length"][t], t) for t in var if tl["flat"][t] >= 0)
    assert (out / "variable_tracts.bed").read_text() == bed and len(bed) > 0
