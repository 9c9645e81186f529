"""Where the variant layer writes (N8-N13: tjamd_tract_variants, tjamd_tract_features, tjamd_variant_effects,
tjamd_merge_variants, tjamd_site_depths, and the two downloads beside them).  The value tests of this layer allocate each output
at the size asked for; here every output sits in a guarded buffer of exactly the header's size (tests/guarded.py, through the
callers of tests/bounds_calls.py), every const input is held frozen, and every result is compared bit for bit with the Python
restatements of the per-entry tests, at exact fit, at capacity = need - 1, 1 and 0, with each optional output NULL, with n = 0
and on refused calls, at tract, record and sample counts on both sides of every constant the kernels cut their work by.

One chain per problem, built as tests/test_counter_reuse.py builds its own: a union of random families cut behind its
grouping's n-th tract, every tract placed in turn on an entry of a random genome's index (every seventh entry, so that the next
tract cuts the right flank to every width from nothing to k; one tract in thirteen unlocated), then N8 -> N12 -> N13, and N9 ->
N11 beside them.  Nothing is workload-sized: the largest union has 4097 tracts of 3 samples.

Not here: tract or record counts past the 65 536-block cap of tract_grid or of variant_effects_kernel's grid, which take more
than 16 M threads' worth of input."""
import functools
import random
import types

import numpy as np
import pytest

import tatajuba_amd as tj
from tests import bounds_calls as bc
from tests.bounds_calls import ERR_ARG, ERR_CAP, SIZES, Union
from tests.guarded import payload_pattern
from tests.test_depths_cabi import restate_site_depths, tiling_of
from tests.test_effects import features_of
from tests.test_effects_cabi import restate_cds, restate_effects
from tests.test_features_cabi import restate_table, restate_tract_features
from tests.test_locate import random_genome, same_entries
from tests.test_locate_cabi import NOWHERE, contigs_of, restate_reference_index
from tests.test_sites_cabi import restate_merge_variants
from tests.test_union_tracts import random_families
from tests.test_union_tracts_cabi import oracle_union_grouping
from tests.test_variants_cabi import restate_tract_variants

pytestmark = pytest.mark.gpu

K, MAXD, LEV = 10, 1, 2
K_TWO_WORDS = 32                         # tbits + 16 + 2k > 64 whatever the tracts: the flank word is sorted apart
STEP = 7                                 # every seventh index entry: neighbours in the tiling are a few bases apart
# (tracts, samples): the tract counts are SIZES; the sample counts take segments of 1, 2, 4, 8, 16, 32 and 64 lanes, and a second
# stride of the sample loop at 65 and 130
PAIRS = [(1, 1), (63, 9), (64, 64), (65, 65), (255, 3), (256, 17), (257, 130), (1023, 2), (1024, 5), (1025, 33), (4095, 1), (4096, 2), (4097, 3)]
VAR, TF, EF, ST, AL, SDP, LOC = tj.VARIANT_DTYPE, tj.TRACT_FEATURE_DTYPE, tj.EFFECT_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE, tj.SITE_DEPTH_DTYPE, tj.LOCATION_DTYPE
SD_GROUP = 8                             # the class accumulators of one walk of site_depths_kernel
MV_OPTIONAL = ("d_genotype", "d_allele_of", "d_unique")
SD_OUTPUTS = bc.DEVICE["tjamd_site_depths"]


# ---- the genome, and what is built on it once ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def genome():
    """-> (stream, restated index entries, features): 40 000 bases give some 28 000 entries, 4097 tracts at every seventh"""
    rng = random.Random(606)
    stream = random_genome(rng, 40000, K)
    entries, _ = restate_reference_index(stream, K)
    assert len(entries) >= STEP * 4097
    sizes = [len(s) for s in contigs_of(stream)]
    last = len(sizes) - 1
    feats = features_of([(0, 1, sizes[0], 0, 0), (0, 1, sizes[0] // 2, 2, 0), (0, 4, sizes[0] // 3, 1, 0), (0, sizes[0] // 2, sizes[0] - 2, 1, 1),
                         (last, 1, sizes[last], 0, 0), (last, 2, sizes[last] - 1, 1, 0), (3, 10, 300, 1, 1)])
    return stream, entries, feats


class World:
    """a counter with the genome's index, annotation and coding table on the device"""

    def __init__(self):
        self.stream, self.entries, self.feats = genome()
        self.c = tj.Counter(K)
        self.ref = tj.Reference(self.c, self.stream)
        same_entries(self.ref.download(), self.entries)
        self.ann = tj.Annotation(self.c, self.ref, self.feats)
        self.cod = tj.Coding(self.c, self.stream, self.feats)

    def close(self):
        for h in (self.cod, self.ann, self.ref, self.c):
            h.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


class Chain:
    """a union of exactly nt tracts by ns samples on the genome, its restatements (each made at its first use, once), and the
    device copies of its inputs"""

    def __init__(self, nt, ns, seed=None):
        seed = 1000 * nt + ns if seed is None else seed
        _, entries, _ = genome()
        n_fam = nt // 2 + 20
        while True:
            keys, mat = random_families(K, ns, seed, n_fam=n_fam)
            g = oracle_union_grouping(keys, mat, K, MAXD, LEV)
            if len(g["groups"]["first"]) > nt:
                break
            n_fam *= 2
        tr = bc.tracts_from_grouping(g, len(keys))[:nt]
        n = int(tr["first"][-1]) + int(tr["n_rows"][-1])
        self.nt, self.ns, self.tracts_host = nt, ns, tr
        self.u = Union(keys[:n], mat[:n], [30] * ns)
        at = entries[(np.arange(nt) * STEP) % len(entries)]
        tl = np.zeros(nt, LOC)
        for f, e in (("flat", "flat"), ("contig", "contig"), ("pos", "pos"), ("ref_length", "length"), ("neg_strand", "neg_strand")):
            tl[f] = at[e]
        tl["n_hits"] = 1
        if nt > 1:
            tl[5::13] = NOWHERE
        self.loc_host = tl

    @functools.cached_property
    def tracts(self):
        return bc.dev(self.tracts_host)

    @functools.cached_property
    def tract_loc(self):
        return bc.dev(self.loc_host)

    def restate_variants(self, lst=None):
        """-> (records, offsets)"""
        recs, offsets, _ = restate_tract_variants(self.u.keys, self.u.mat, self.tracts_host, self.loc_host, genome()[1], K, lst=lst)
        return recs, offsets

    @functools.cached_property
    def want_v(self):
        return self.restate_variants()

    @functools.cached_property
    def want_m(self):
        return restate_merge_variants(self.want_v[0], self.ns, K, n_tracts=self.nt)

    @functools.cached_property
    def want_d(self):
        return restate_site_depths(self.u.keys, self.u.mat, self.tracts_host, self.loc_host, genome()[1], K, self.want_m)

    @functools.cached_property
    def want_tf(self):
        return restate_tract_features(genome()[2], self.u.keys, self.u.mat, self.tracts_host, self.loc_host)

    @functools.cached_property
    def variants(self):
        """the restated records on the device, never empty"""
        return bc.dev(self.want_v[0]) if len(self.want_v[0]) else bc.torch().zeros(64, dtype=bc.torch().uint8, device="cuda")

    def broken_tracts(self):
        bad = self.tracts_host.copy()
        bad["n_rows"][len(bad) // 2] += 1
        return bc.dev(bad)


@functools.lru_cache(maxsize=None)
def chain(nt, ns):
    return Chain(nt, ns)


# ---- comparisons -------------------------------------------------------------------------------------------------------------

def same(g, want, what):
    """a guarded output holds exactly the restatement's bytes"""
    want = np.ascontiguousarray(want)
    got = g.view(want.dtype, want.size).reshape(want.shape)
    assert g.nbytes == want.nbytes, (what, g.nbytes, want.nbytes)
    if got.tobytes() != want.tobytes():
        for f in want.dtype.names or ():
            bad = np.flatnonzero(got[f] != want[f])
            assert len(bad) == 0, (what, f, bad[:5], got[f][bad[:3]], want[f][bad[:3]])
        bad = np.argwhere(got != want)
        assert False, (what, bad[:5])


def written_is_right(g, want, what):
    """of a refused call's buffer, shorter than what was found: every element that was changed holds the restatement's element of
    that index (where the header leaves open what lies below the capacity)"""
    want = np.ascontiguousarray(want)
    size = want.dtype.itemsize
    n = g.nbytes // size
    assert n <= len(want) and n * size == g.nbytes, (what, n, len(want))
    if not n:
        return 0
    got = g.view(np.uint8).reshape(n, size)
    changed = (got != payload_pattern(g.nbytes).reshape(n, size)).any(axis=1)
    assert (got[changed] == want[:n].view(np.uint8).reshape(n, size)[changed]).all(), (what, np.flatnonzero(changed)[:5])
    return int(changed.sum())


def all_untouched(r, what):
    assert all(g is None or g.untouched() for g in r.outs.values()), what


def short_capacities(need):
    """need - 1, 1 and 0, those below the need"""
    return [cap for cap in sorted({need - 1, 1, 0}) if 0 <= cap < need]


# ---- tjamd_tract_variants ----------------------------------------------------------------------------------------------------

def variants_at_every_capacity(w, ch, lst=None, want=None):
    recs, offsets = ch.want_v if want is None else want
    need = len(recs)
    r = bc.call_tract_variants(w.c, w.ref, ch.u, ch.tracts, ch.nt, ch.tract_loc, need, lst=lst)
    assert r.rc == need and r.ms > 0, (r.rc, r.err)
    same(r["d_out"], recs, "d_out")
    assert r["h_offsets"].view(np.int64).tolist() == offsets
    for cap in short_capacities(need):                                        # need - 1, 1, and 0 with d_out NULL
        r = bc.call_tract_variants(w.c, w.ref, ch.u, ch.tracts, ch.nt, ch.tract_loc, cap, lst=lst)
        r.refused(ERR_CAP, "tjamd_tract_variants", f"{need} records, caller capacity {cap}")
        assert r["h_offsets"].untouched() and r.ms == -1.0, cap                # written on success only; no timing of a refused call
        written_is_right(r["d_out"], recs, f"d_out at capacity {cap}")         # (nothing at or beyond the capacity: the guards)
    return need


@pytest.mark.parametrize("nt,ns", PAIRS)
def test_tract_variants_every_tract(world, nt, ns):
    ch = chain(nt, ns)
    need = variants_at_every_capacity(world, ch)
    assert need > 0 or nt == 1
    # n_list = 0: no record, every offset 0, at a capacity of 0
    r = bc.call_tract_variants(world.c, world.ref, ch.u, ch.tracts, ch.nt, ch.tract_loc, 0, lst=bc.arange_dev(1), n_list=0)
    assert r.rc == 0 and r["h_offsets"].view(np.int64).tolist() == [0] * (ns + 1)


@pytest.mark.parametrize("n_list", SIZES)
def test_tract_variants_lists_in_reverse_with_repeats(world, n_list):
    ch = chain(1024, 5)
    lst = [(ch.nt - 1 - i) % ch.nt for i in range(n_list)]
    for i in range(4, n_list, 5):
        lst[i] = lst[i - 1]                                                   # a tract twice, next to itself
    assert n_list < 3 or lst[0] > lst[1] and (n_list < 5 or lst[3] == lst[4])
    need = variants_at_every_capacity(world, ch, lst=bc.dev(np.array(lst, np.int32), np.int32), want=ch.restate_variants(lst))
    assert need > 0 or n_list < 3


def test_tract_variants_refused_on_the_device(world):
    """the header promises nothing about d_out here: the guards (in the caller), h_offsets and the timer.  Under a list with an id
    outside the tracts, what is written is the records of the list without it"""
    ch = chain(257, 130)
    r = bc.call_tract_variants(world.c, world.ref, ch.u, ch.broken_tracts(), ch.nt, ch.tract_loc, len(ch.want_v[0]))
    r.refused(ERR_ARG, "tjamd_tract_variants", "do not tile the union")
    assert r["h_offsets"].untouched() and r.ms == -1.0
    listed = ch.restate_variants([1, 0])[0]
    assert len(listed) > 100
    r = bc.call_tract_variants(world.c, world.ref, ch.u, ch.tracts, ch.nt, ch.tract_loc, len(listed), lst=bc.dev(np.array([1, ch.nt, 0, -1], np.int32), np.int32))
    r.refused(ERR_ARG, "tjamd_tract_variants", "a listed tract id is outside")
    assert r["h_offsets"].untouched() and r.ms == -1.0
    written_is_right(r["d_out"], listed, "d_out under a list with an id outside")


# ---- tjamd_merge_variants ----------------------------------------------------------------------------------------------------

def check_merge(r, want, n_sites, n_alleles, ns, null=()):
    assert r.rc == n_sites and r.n_alleles == n_alleles and r.ms > 0, (r.rc, r.err)
    for name, w in (("d_sites", want["sites"]), ("d_alleles", want["alleles"]), ("d_genotype", want["genotype"]), ("d_allele_of", want["allele_of"]),
                    ("d_unique", want["unique"])):
        if name not in null:
            same(r[name], w, name)


def merge_at_every_capacity(c, recs_dev, n, ns, nt, want, kmers=(K, K_TWO_WORDS)):
    n_sites, n_alleles = len(want["sites"]), len(want["alleles"])
    for k in kmers:
        call = lambda sc, ac, null=(): bc.call_merge_variants(c, k, recs_dev, n, ns, nt, sc, ac, null=null)
        check_merge(call(n_sites, n_alleles), want, n_sites, n_alleles, ns)
        for null in [(x,) for x in MV_OPTIONAL] + [MV_OPTIONAL]:              # each optional output NULL, and all three
            check_merge(call(n_sites, n_alleles, null), want, n_sites, n_alleles, ns, null)
        for sc, ac in ((n_sites - 1, n_alleles), (n_sites, n_alleles - 1), (1, 1), (0, 0)):
            if sc >= n_sites and ac >= n_alleles:
                continue                                                      # (one site of one allele: (1, 1) is the exact fit)
            r = call(sc, ac)
            r.refused(ERR_CAP, "tjamd_merge_variants", f"{n_sites} sites and {n_alleles} alleles, caller capacities {sc} and {ac}")
            assert r.n_alleles == -1 and r.ms == -1.0, (sc, ac)                # *h_n_alleles is left alone
            # nothing at or beyond either capacity (the guards; d_genotype has site_capacity rows); what lies below is in its place
            written_is_right(r["d_sites"], want["sites"], "d_sites")
            written_is_right(r["d_alleles"], want["alleles"], "d_alleles")
            written_is_right(r["d_unique"], want["unique"], "d_unique")
            written_is_right(r["d_genotype"], want["genotype"].reshape(-1), "d_genotype")
            written_is_right(r["d_allele_of"], want["allele_of"], "d_allele_of")


@pytest.mark.parametrize("n", SIZES)
def test_merge_variants_prefixes_of_the_largest_chain(world, n):
    """the key sort cuts at RS_ITEMS (1024), the scans at SC_ITEMS (4096); the one-word key and the two-word key"""
    ch = chain(4097, 3)
    recs = ch.want_v[0]
    assert len(recs) >= SIZES[-1]
    want = restate_merge_variants(recs[:n], ch.ns, K, n_tracts=ch.nt)
    merge_at_every_capacity(world.c, ch.variants, n, ch.ns, ch.nt, want)


@pytest.mark.parametrize("nt,ns", PAIRS)
def test_merge_variants_of_every_chain(world, nt, ns):
    ch = chain(nt, ns)
    if len(ch.want_v[0]) == 0:                                                # (one tract of one sample may have no record)
        r = bc.call_merge_variants(world.c, K, ch.variants, 0, ns, nt, 0, 0)
        assert r.rc == 0 and r.n_alleles == 0
        return
    merge_at_every_capacity(world.c, ch.variants, len(ch.want_v[0]), ns, nt, ch.want_m, kmers=(K,))


def test_merge_variants_key_width_on_both_sides_of_64_bits(world):
    """tbits + 16 + 2k <= 64 is the one-word key: 4096 tracts have 12 bits and 4097 have 13, so k = 18 is 64 and 65 bits on the
    same records; k = 17 and 19 beside it.  (No record has more than 10 flank bases: the restatement is the same under every k)"""
    ch = chain(4096, 2)
    n, want = len(ch.want_v[0]), ch.want_m
    assert int(ch.want_v[0]["n_flank"].max()) <= K and int(ch.want_v[0]["tract"].max()) < 4096
    for k, nt in ((17, 4097), (18, 4096), (18, 4097), (19, 4096)):
        assert (bc.SIZES[-2] - 1).bit_length() + 16 + 2 * 18 == 64
        r = bc.call_merge_variants(world.c, k, ch.variants, n, ch.ns, nt, len(want["sites"]), len(want["alleles"]))
        check_merge(r, want, len(want["sites"]), len(want["alleles"]), ch.ns)


def test_merge_variants_past_the_grid_stride_cap(world):
    """grid_for stops at 4096 blocks, 1 048 576 threads: 1025 tracts x 1025 samples, one identical allele per tract, take the loops
    of mv_write_kernel (1 050 625 records) and of mv_fill_kernel (as many cells) round again.  The expectation is a closed form"""
    nt = ns = 1025
    n = nt * ns
    t, s = np.tile(np.arange(nt), ns), np.repeat(np.arange(ns), nt)           # sample-major, as N8 writes
    recs = np.zeros(n, VAR)
    recs["flat"], recs["tract"], recs["sample"], recs["pos"], recs["row"], recs["base"] = 1000 * t, t, s, 100 * t + 5, 2 * t, t % 4
    recs["ref_length"], recs["alt_length"] = 5, 6
    one = np.arange(nt)
    sites, alleles = np.zeros(nt, ST), np.zeros(nt, AL)
    sites["flat"], sites["tract"], sites["pos"], sites["base"] = 1000 * one, one, 100 * one + 5, one % 4
    sites["ref_length"] = sites["min_length"] = 5
    sites["n_alleles"], sites["first_allele"], sites["n_called"], sites["first_record"] = 1, one, ns, one
    alleles["site"], alleles["alt_length"], alleles["n_samples"], alleles["first_record"] = one, 6, ns, one
    want = {"sites": sites, "alleles": alleles, "genotype": np.ones((nt, ns), np.int16), "allele_of": t.astype(np.int32), "unique": recs[:nt]}
    r = bc.call_merge_variants(world.c, K, bc.dev(recs), n, ns, nt, nt, nt)
    check_merge(r, want, nt, nt, ns)
    r = bc.call_merge_variants(world.c, K, bc.dev(recs), n, ns, nt, nt - 1, nt)
    r.refused(ERR_CAP, "1025 sites and 1025 alleles, caller capacities 1024 and 1025")
    assert written_is_right(r["d_genotype"], want["genotype"].reshape(-1), "d_genotype") == (nt - 1) * ns


def test_merge_variants_no_record(world):
    r = bc.call_merge_variants(world.c, K, bc.torch().zeros(64, dtype=bc.torch().uint8, device="cuda"), 0, 3, 5, 0, 0)
    assert r.rc == 0 and r.n_alleles == 0
    all_untouched(r, "n_records = 0")


# ---- tjamd_site_depths -------------------------------------------------------------------------------------------------------

def call_depths(w, u, tracts, nt, tract_loc, m, null=(), n_sites=None):
    n_sites = len(m["sites"]) if n_sites is None else n_sites
    n_alleles = len(m["alleles"]) if n_sites else 0
    sd = bc.dev(m["sites"]) if n_sites else None
    ad = bc.dev(m["alleles"]) if n_alleles else None
    return bc.call_site_depths(w.c, w.ref, u, tracts, nt, tract_loc, sd, n_sites, ad, n_alleles, null=null)


def check_depths(r, want, n_sites, null=()):
    assert r.rc == n_sites and (r.ms > 0 or n_sites == 0), (r.rc, r.err)
    for name, x in zip(SD_OUTPUTS, ("genotype", "depth", "allele_depth", "summary")):
        if name not in null:
            same(r[name], want[x], name)


def depths_with_every_output_null(w, u, tracts, nt, tract_loc, m, want):
    n_sites = len(m["sites"])
    check_depths(call_depths(w, u, tracts, nt, tract_loc, m), want, n_sites)
    for null in [(x,) for x in SD_OUTPUTS] + [SD_OUTPUTS]:                     # each of the four NULL, and all: n_sites back, nothing written
        check_depths(call_depths(w, u, tracts, nt, tract_loc, m, null=null), want, n_sites, null)


@pytest.mark.parametrize("nt,ns", PAIRS)
def test_site_depths_of_every_chain(world, nt, ns):
    ch = chain(nt, ns)
    m = ch.want_m
    if len(m["sites"]) == 0:
        m = {"sites": np.zeros(0, ST), "alleles": np.zeros(0, AL)}
    depths_with_every_output_null(world, ch.u, ch.tracts, nt, ch.tract_loc, m, ch.want_d)
    r = call_depths(world, ch.u, ch.tracts, nt, ch.tract_loc, m, n_sites=0)   # n_sites = 0: nothing to write, nothing written
    assert r.rc == 0
    if len(m["sites"]) == 0:
        return
    # refused on the device by the first pass, which writes nothing: a broken tiling, an n_called off by one
    bad = {"sites": m["sites"].copy(), "alleles": m["alleles"]}
    bad["sites"]["n_called"][len(bad["sites"]) // 2] += 1
    for r, words in ((call_depths(world, ch.u, ch.broken_tracts(), nt, ch.tract_loc, m), "do not tile the union"), (call_depths(world, ch.u, ch.tracts, nt, ch.tract_loc, bad), "n_called")):
        r.refused(ERR_ARG, "tjamd_site_depths", words)
        all_untouched(r, words)
        assert r.ms == -1.0
    check_depths(call_depths(world, ch.u, ch.tracts, nt, ch.tract_loc, m), ch.want_d, len(m["sites"]))


@functools.lru_cache(maxsize=None)
def planted(n_classes, ns):
    """five tracts on the genome, the last a site of n_classes classes (REF and n_classes - 1 alleles, each some sample's modal
    row), so that the rows of its classes end on the last byte of AD.  No call of fewer samples than alleles has such a site: there
    the sites are those of the same tiling under 16 samples, of which the call is given the first ns, n_called counted anew.
    -> (keys, mat, tracts, loc, sites and alleles, restated depths)"""
    _, entries, _ = genome()
    rng = random.Random(100 * n_classes + ns)
    n_alt = n_classes - 1
    wide = max(ns, 16)
    usable = [i for i in range(len(entries)) if entries["length"][i] < 100]
    parts = []
    for j in range(5):
        Lr = int(entries["length"][usable[20 + 9 * j]])
        n_here = n_alt if j == 4 else 1 + j % 3
        rows = [(Lr, None)] + [(Lr + 1 + a, None) for a in range(n_here)]
        m = np.zeros((len(rows), wide), np.int32)
        for s in range(wide):
            m[1 + s % n_here if s < n_here or rng.random() < 0.7 else 0, s] = 9
            m[rng.randrange(len(rows)), s] += 2
        parts.append((usable[20 + 9 * j], rows, m))
    keys, mat, tracts, loc = tiling_of(entries, K, parts)
    recs, _, _ = restate_tract_variants(keys, mat, tracts, loc, entries, K)
    m = restate_merge_variants(recs, wide, K, n_tracts=len(tracts))
    assert len(m["sites"]) == 5 and int(m["sites"]["n_alleles"][-1]) == n_alt
    sites = m["sites"].copy()
    sites["n_called"] = (m["genotype"][:, :ns] >= 1).sum(axis=1)
    m = {"sites": sites, "alleles": m["alleles"]}
    mat = np.ascontiguousarray(mat[:, :ns])
    return keys, mat, tracts, loc, m, restate_site_depths(keys, mat, tracts, loc, entries, K, m)


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("n_classes", [2, 7, 8, 9, 15, 16, 17])
def test_site_depths_last_site_around_the_class_groups(world, n_classes, ns):
    """2, 7, 8, 9, 15, 16 and 17 classes around SD_GROUP: a last walk of 2, 7, 8, 1, 7, 8 and 1 classes under the eight guards"""
    keys, mat, tracts, loc, m, want = planted(n_classes, ns)
    assert (n_classes - 1) % SD_GROUP + 1 in (2, 7, 8, 1) and want["allele_depth"].shape == (5 + len(m["alleles"]), ns)
    assert want["allele_depth"][-1].any() or ns < n_classes - 1               # the last class row holds counts
    u = Union(keys, mat, [30] * ns)
    depths_with_every_output_null(world, u, bc.dev(tracts), len(tracts), bc.dev(loc), m, want)


# ---- tjamd_tract_features, tjamd_annotation_download ---------------------------------------------------------------------------

@pytest.mark.parametrize("nt", SIZES)
def test_tract_features(world, nt):
    ch = chain(nt, dict(PAIRS).get(nt, 2))
    r = bc.call_tract_features(world.c, world.ann, ch.u, ch.tracts, nt, ch.tract_loc)
    assert r.rc == nt and r.ms > 0, r.err
    same(r["d_out"], ch.want_tf, "d_out")
    assert nt < 63 or ((ch.want_tf["feature"] >= 0).any() and (ch.want_tf["feature"] < 0).any())
    nothing = types.SimpleNamespace(kd=None, md=None, n=0, ns=ch.ns)           # n_tracts = 0, of an empty union: nothing written
    r = bc.call_tract_features(world.c, world.ann, nothing, ch.tracts, 0, ch.tract_loc)
    assert r.rc == 0 and r["d_out"].nbytes == 0
    r = bc.call_tract_features(world.c, world.ann, ch.u, ch.broken_tracts(), nt, ch.tract_loc)
    r.refused(ERR_ARG, "tjamd_tract_features", "do not tile the union")
    assert r["d_out"].untouched() and r.ms == -1.0                             # a refused call writes nothing


def test_annotation_and_coding_downloads(world):
    points, winner = restate_table(world.feats)
    need = len(points)
    r = bc.call_annotation_download(world.ann, need)
    assert r.rc == need > 0
    same(r["h_points"], points, "h_points"); same(r["h_winner"], winner, "h_winner")
    for cap in (need - 1, 0):
        r = bc.call_annotation_download(world.ann, cap)
        assert r.rc == need
        all_untouched(r, f"tjamd_annotation_download at capacity {cap}")
    cds = restate_cds(world.stream, world.feats)
    need = len(cds)
    r = bc.call_coding_download(world.cod, need)
    assert r.rc == need == len(world.feats)
    same(r["out"], cds, "out")
    for cap in (need - 1, 0):
        r = bc.call_coding_download(world.cod, cap)
        assert r.rc == need
        all_untouched(r, f"tjamd_coding_download at capacity {cap}")


# ---- tjamd_variant_effects ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_variant_effects(world, n):
    ch = chain(4097, 3)
    stream, _, feats = genome()
    recs = ch.want_v[0][:n]
    tf = bc.dev(ch.want_tf)
    for feat_dev, feat_host, nt in ((tf, ch.want_tf, ch.nt), (None, None, 0)):  # d_tract_feat given and NULL
        want = restate_effects(stream, feats, None, recs, feat_host)
        r = bc.call_variant_effects(world.c, world.cod, ch.variants, n, feat_dev, nt)
        assert r.rc == n and r.ms > 0, r.err
        same(r["d_out"], want, "d_out")
        assert (want["cls"] == 0).all() if feat_host is None else n < 255 or len(set(want["cls"].tolist())) >= 2
    r = bc.call_variant_effects(world.c, world.cod, ch.variants, 0, tf, ch.nt)                # n = 0: nothing written
    assert r.rc == 0 and r["d_out"].nbytes == 0
    bad = recs.copy()
    bad["contig"][n // 2] = 1 << 20
    r = bc.call_variant_effects(world.c, world.cod, bc.dev(bad), n, tf, ch.nt)
    r.refused(ERR_ARG, "tjamd_variant_effects", "contig is outside")
    assert r["d_out"].untouched() and r.ms == -1.0                             # a refused call writes nothing
