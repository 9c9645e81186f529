"""Scratch carried between calls.  A counter's device scratch only grows, and the entries share it (the flags, positions
and segment ids of the scans, the histogram and the work area of the key-value sort, the row totals, the error words): a
kernel that read scratch it had not written in this call -- the tail a larger problem left, an error word a refused call
left -- would pass every test that takes a fresh counter.  Here one counter goes through a fixed sequence: every entry on
a large problem (4097 rows by 70 samples), then on a small one of another shape (65 rows by 3 samples), then on the small
one directly after each kind of refused call on the large one, with a sample scanned, the counter reset and another
scanned, and a reference built, used, closed and built again smaller; the annotation layer (variants, features, the seed
order and the gapped lookup, coding effects, merged sites, site depths) goes through the same sequence on tracts placed on the genome.
Every result is bit for bit that of the same call on a fresh counter; every output sits in a guarded buffer
(tests/bounds_calls.py)."""
import random

import numpy as np
import pytest

import tatajuba_amd as tj
from tatajuba_amd import capi
from oracle import orc
from tests import bounds_calls as bc
from tests.bounds_calls import ERR_ARG, ERR_CAP, Union
from tests.test_effects import features_of
from tests.guarded import GuardedHost, frozen
from tests.test_locate import queries_for, random_genome
from tests.test_locate_cabi import contigs_of, restate_reference_index
from tests.test_union_tracts import random_families
from tests.test_union_tracts_cabi import oracle_union_grouping

pytestmark = pytest.mark.gpu

K, MAXD, LEV, MM = 10, 1, 2, 2


class Problem:
    """a union, what the entries need beside it (made once, on counters of their own), and a genome with queries"""

    def __init__(self, name, n_rows, ns, n_fam, seed, genome_bytes, n_queries):
        self.name = name
        keys, mat = random_families(K, ns, seed, n_fam=n_fam)
        assert len(keys) >= n_rows
        rng = random.Random(seed)
        self.u = Union(keys[:n_rows], mat[:n_rows], rng.choices(range(20, 80), k=ns))
        self.records, self.counts = self.u.sample_records()
        g = oracle_union_grouping(self.u.keys, self.u.mat, K, MAXD, LEV)
        self.tracts_host = bc.tracts_from_grouping(g, self.u.n)
        self.group_ids = g["tract_id"].astype(np.int32)
        self.n_ctx = int(orc.tract_ids(self.u.keys)[1])
        self.nt = len(self.tracts_host)
        self.tracts = bc.dev(self.tracts_host)
        self.loc_host = bc.planted_locations(self.u.keys, seed)
        self.loc = bc.dev(self.loc_host)
        self.genome = random_genome(rng, genome_bytes, K)
        entries, _ = restate_reference_index(self.genome, K)
        self.queries = bc.dev(queries_for(rng, entries, K, n_queries // 4, n_queries))
        self.n_queries = self.queries.numel() // 24
        prep = tj.Counter(K)                                                  # the summaries the sample statistics read
        ts = bc.call_tract_stats(prep, self.u, self.n_ctx)
        us = bc.call_union_tract_stats(prep, self.u, self.tracts, self.nt)
        assert ts.rc == self.n_ctx and us.rc == self.nt
        self.ts_summary, self.us_summary = ts["d_summary"].payload.clone(), us["d_summary"].payload.clone()
        # the annotation layer: every tract placed on an entry of the genome's index (in turn), a handful of features on the
        # genome, and the variant records tjamd_tract_variants itself gives
        at = entries[np.arange(self.nt) % len(entries)]
        tl = np.zeros(self.nt, tj.LOCATION_DTYPE)
        for f, g in (("flat", "flat"), ("contig", "contig"), ("pos", "pos"), ("ref_length", "length"), ("neg_strand", "neg_strand")):
            tl[f] = at[g]
        tl["n_hits"] = 1
        self.tract_loc = bc.dev(tl)
        sizes = [len(s) for s in contigs_of(self.genome)]
        last = len(sizes) - 1
        self.features = features_of([(0, 1, sizes[0], 0, 0), (0, 1, sizes[0] // 2, 2, 0), (0, 4, sizes[0] // 3, 1, 0), (0, sizes[0] // 2, sizes[0] - 2, 1, 1),
                                     (last, 1, sizes[last], 0, 0), (last, 2, sizes[last] - 1, 1, 0), (3, 10, 300, 1, 1)])
        ref, ann, cod = tj.Reference(prep, self.genome), None, None
        try:
            assert ref.add_seeds(prep) == ref.n_entries == len(entries) > 0
            ann, cod = tj.Annotation(prep, ref, self.features), tj.Coding(prep, self.genome, self.features)
            tv = bc.call_tract_variants(prep, ref, self.u, self.tracts, self.nt, self.tract_loc, self.nt * self.u.ns)
            tf = bc.call_tract_features(prep, ann, self.u, self.tracts, self.nt, self.tract_loc)
            assert tv.rc > 0 and tf.rc == self.nt > 0
            self.n_variants, self.variants = tv.rc, tv["d_out"].payload[: tv.rc * tj.VARIANT_DTYPE.itemsize].clone()
            self.tract_feat = tf["d_out"].payload.clone()
            lg = bc.call_locate_gapped(prep, ref, self.queries, self.n_queries, MM, MM)
            ve = bc.call_variant_effects(prep, cod, self.variants, self.n_variants, self.tract_feat, self.nt)
            mv = bc.call_merge_variants(prep, K, self.variants, self.n_variants, self.u.ns, self.nt, self.nt, self.n_variants)
            assert lg.rc > 0 and ve.rc == self.n_variants and mv.rc > 0 and mv.n_alleles >= mv.rc
            self.n_sites, self.n_alleles = mv.rc, mv.n_alleles
            self.sites_host, self.sites = mv["d_sites"].view(tj.SITE_DTYPE, mv.rc), mv["d_sites"].payload.clone()      # what tjamd_site_depths reads
            self.alleles = mv["d_alleles"].payload[: mv.n_alleles * tj.ALLELE_DTYPE.itemsize].clone()
            sd = bc.call_site_depths(prep, ref, self.u, self.tracts, self.nt, self.tract_loc, self.sites, self.n_sites, self.alleles, self.n_alleles)
            assert sd.rc == self.n_sites, sd.err
        finally:
            for h in (cod, ann, ref):
                if h is not None:
                    h.close()
        prep.close()


def signature(r, *more):
    """a call's return value, its counts and every byte of its outputs"""
    return (r.rc, tuple(more), {name: g.view(np.uint8).tobytes() for name, g in r.outs.items() if g is not None})


def run_reference(c, p):
    ref = tj.Reference(c, p.genome)
    try:
        index = ref.download().tobytes()
        r = bc.call_locate(c, ref, p.queries, p.n_queries, MM)
        assert r.rc > 0
        return signature(r, ref.n_entries, ref.n_contigs, index)
    finally:
        ref.close()


def with_reference(c, p, call, seeds=False):
    """a call that takes the genome's index, built on this counter for the call"""
    ref = tj.Reference(c, p.genome)
    try:
        assert not seeds or ref.add_seeds(c) == ref.n_entries
        r = call(ref)
        assert r.rc > 0
        return signature(r, ref.has_seeds)
    finally:
        ref.close()


def run_features(c, p):
    ref = tj.Reference(c, p.genome)
    ann = tj.Annotation(c, ref, p.features)
    try:
        table = tuple(x.tobytes() for x in ann.download())
        return signature(bc.call_tract_features(c, ann, p.u, p.tracts, p.nt, p.tract_loc), table)
    finally:
        ann.close()
        ref.close()


def run_effects(c, p):
    cod = tj.Coding(c, p.genome, p.features)
    try:
        return signature(bc.call_variant_effects(c, cod, p.variants, p.n_variants, p.tract_feat, p.nt), cod.download().tobytes())
    finally:
        cod.close()


ENTRIES = {
    "tjamd_merge_samples": lambda c, p: signature(bc.call_merge_samples(c, p.records, p.counts, p.u.ns, p.u.n)),
    "tjamd_tract_ids": lambda c, p: signature(bc.call_tract_ids(c, p.u)),
    "tjamd_tract_stats": lambda c, p: (lambda r: signature(r, r.n_var))(bc.call_tract_stats(c, p.u, p.n_ctx)),
    "tjamd_tract_stats (caller ids)": lambda c, p: (lambda r: signature(r, r.n_var))(bc.call_tract_stats(c, p.u, p.nt, ids=bc.dev(p.group_ids, np.int32))),
    "tjamd_tract_sample_stats": lambda c, p: signature(bc.call_tract_sample_stats(c, p.u, p.ts_summary, p.n_ctx, bc.arange_dev(p.n_ctx))),
    "tjamd_union_tracts": lambda c, p: signature(bc.call_union_tracts(c, p.u, MAXD, LEV, p.nt), c.last_union_tract_candidates()),
    "tjamd_union_tract_stats": lambda c, p: (lambda r: signature(r, r.n_var, r.n_sel))(bc.call_union_tract_stats(c, p.u, p.tracts, p.nt)),
    "tjamd_union_tract_sample_stats": lambda c, p: signature(bc.call_union_tract_sample_stats(c, p.u, p.us_summary, p.nt, bc.arange_dev(p.nt))),
    "tjamd_reference_create, tjamd_locate": run_reference,
    "tjamd_located_tracts": lambda c, p: signature(bc.call_located_tracts(c, p.u, p.tracts, p.nt, p.loc, p.u.n)),
    "tjamd_located_tracts (no tracts)": lambda c, p: signature(bc.call_located_tracts(c, p.u, None, 0, p.loc, p.u.n)),
    "tjamd_tract_variants": lambda c, p: with_reference(c, p, lambda ref: bc.call_tract_variants(c, ref, p.u, p.tracts, p.nt, p.tract_loc, p.n_variants)),
    "tjamd_annotation_create, tjamd_tract_features": run_features,
    "tjamd_reference_add_seeds, tjamd_locate_gapped": lambda c, p: with_reference(c, p, lambda ref: bc.call_locate_gapped(c, ref, p.queries, p.n_queries, MM, MM), seeds=True),
    "tjamd_coding_create, tjamd_variant_effects": run_effects,
    "tjamd_merge_variants": lambda c, p: (lambda r: signature(r, r.n_alleles))(bc.call_merge_variants(c, K, p.variants, p.n_variants, p.u.ns, p.nt, p.n_sites, p.n_alleles)),
    "tjamd_site_depths": lambda c, p: with_reference(c, p, lambda ref: bc.call_site_depths(c, ref, p.u, p.tracts, p.nt, p.tract_loc, p.sites, p.n_sites, p.alleles, p.n_alleles)),
}


def refuse_capacity(c, p):
    bc.call_tract_stats(c, p.u, 1).refused(ERR_CAP, "caller capacity 1")
    bc.call_union_tracts(c, p.u, MAXD, LEV, 1).refused(ERR_CAP, "caller capacity 1")
    bc.call_located_tracts(c, p.u, p.tracts, p.nt, p.loc, 1).refused(ERR_CAP, "caller capacity 1")
    bc.call_merge_samples(c, p.records, p.counts, p.u.ns, 1).refused(ERR_CAP, "caller capacity 1")


def refuse_bad_ids(c, p):
    bad = p.group_ids.copy()
    bad[p.u.n // 2:] += 2
    bc.call_tract_stats(c, p.u, p.nt + 2, ids=bc.dev(bad, np.int32)).refused(ERR_ARG, "tract ids must start at 0")
    listed = bc.dev(np.array([0, p.nt, -1], np.int32), np.int32)
    bc.call_tract_sample_stats(c, p.u, p.ts_summary, p.n_ctx, bc.dev(np.array([0, p.n_ctx], np.int32), np.int32)).refused(ERR_ARG, "outside [0,")
    bc.call_union_tract_sample_stats(c, p.u, p.us_summary, p.nt, listed).refused(ERR_ARG, "outside [0,")


def refuse_tiling(c, p):
    bad = p.tracts_host.copy()
    bad["n_rows"][len(bad) // 2] += 1
    bc.call_union_tract_stats(c, p.u, bc.dev(bad), len(bad)).refused(ERR_ARG, "must tile the union")
    bc.call_located_tracts(c, p.u, bc.dev(bad), len(bad), p.loc, p.u.n).refused(ERR_ARG, "do not tile the union")


def refuse_flat(c, p):
    far = p.loc_host.copy()
    far["flat"][np.flatnonzero(far["flat"] >= 0)[::3]] = 1 << 45
    bc.call_located_tracts(c, p.u, p.tracts, p.nt, bc.dev(far), p.u.n).refused(ERR_ARG, "flat >= 2^45")
    bc.call_located_tracts(c, p.u, None, 0, bc.dev(far), p.u.n).refused(ERR_ARG, "flat >= 2^45")


def refuse_on_the_genome(c, p):
    """the entries that take the genome's index or a table built on it"""
    bad = p.tracts_host.copy()
    bad["n_rows"][len(bad) // 2] += 1
    ref = tj.Reference(c, p.genome)
    ann = tj.Annotation(c, ref, p.features)
    try:
        for f in (lambda: tj.Annotation(c, ref, features_of([(ref.n_contigs, 1, 2, 1, 0)])), lambda: tj.Coding(c, p.genome, features_of([(0, 5, 4, 1, 0)]))):
            with pytest.raises(tj.TatajubaAmdError, match="feature 0"):
                f()
        bc.call_locate_gapped(c, ref, p.queries, p.n_queries, MM, MM).refused(ERR_ARG, "no seed order")
        bc.call_tract_features(c, ann, p.u, bc.dev(bad), len(bad), p.tract_loc).refused(ERR_ARG, "do not tile the union")
        listed = bc.dev(np.array([0, p.nt], np.int32), np.int32)
        bc.call_tract_variants(c, ref, p.u, p.tracts, p.nt, p.tract_loc, p.n_variants, lst=listed).refused(ERR_ARG, "a listed tract id is outside")
        miscounted = p.sites_host.copy()                                      # tjamd_site_depths cuts scratch (SdShared): one of its device refusals
        miscounted["n_called"][len(miscounted) // 2] += 1
        r = bc.call_site_depths(c, ref, p.u, p.tracts, p.nt, p.tract_loc, bc.dev(miscounted), p.n_sites, p.alleles, p.n_alleles)
        r.refused(ERR_ARG, "n_called is not the number of samples with an allele")
        assert all(g.untouched() for g in r.outs.values()) and r.ms == -1.0
    finally:
        ann.close()
        ref.close()


def refuse_records(c, p):
    v = np.frombuffer(p.variants.cpu().numpy().tobytes(), tj.VARIANT_DTYPE).copy()
    twice = bc.dev(np.concatenate([v, v[:1]]))
    bc.call_merge_variants(c, K, twice, len(v) + 1, p.u.ns, p.nt, p.n_sites, p.n_alleles).refused(ERR_ARG, "pair occurs twice")
    v["contig"][len(v) // 2] = 1 << 20
    cod = tj.Coding(c, p.genome, p.features)
    try:
        bc.call_variant_effects(c, cod, bc.dev(v), len(v), p.tract_feat, p.nt).refused(ERR_ARG, "contig is outside")
    finally:
        cod.close()


REFUSALS = {"capacity": refuse_capacity, "bad ids": refuse_bad_ids, "tracts that do not tile": refuse_tiling, "flat too large": refuse_flat,
            "on the genome": refuse_on_the_genome, "bad records": refuse_records}


def sample_state(c, m):
    """what the host entries give of a scanned counter, before and after its finalise: every byte"""
    L = tj.lib()
    out = {"raw": np.sort(c.download_raw(), order=("ctx0", "ctx1", "meta")).tobytes(), "undefined": c.undefined_runs()}
    out["status"] = c.finalise(1, 5)
    n, ni = c.n_kept, c.n_idx
    kept, a, b = GuardedHost(n * 40), GuardedHost(ni * 4), GuardedHost(ni * 4)
    assert L.tjamd_download_kept(c._h, kept.c, n) == n and L.tjamd_download_idx(c._h, a.c, b.c, ni) == ni
    gof, groups = GuardedHost(n * 4), GuardedHost(n * tj.GROUP_DTYPE.itemsize)
    ng = L.tjamd_group_contexts(c._h, 1, gof.c, groups.c, n)
    h = {name: GuardedHost(n * size) for name, size in (("group_of", 4), ("join_type", 4), ("groups", capi.CONTEXT_GROUP_DTYPE.itemsize), ("hist", 8))}
    nh = L.tjamd_context_histograms(c._h, 1, 2, *[g.c for g in h.values()], n)
    assert ng > 0 and nh > 0
    for g in [kept, a, b, gof, groups] + list(h.values()):
        g.check()
    grp = h["groups"].view(capi.CONTEXT_GROUP_DTYPE, nh)
    hist = h["hist"].view(capi.LENGTH_FREQ_DTYPE)
    out.update(kept=kept.payload.tobytes(), idx=(a.payload.tobytes(), b.payload.tobytes()), coverage=c.coverage, group_of=gof.payload.tobytes(),
               groups=groups.view(tj.GROUP_DTYPE, ng).tobytes(), h_group_of=h["group_of"].payload.tobytes(), h_join=h["join_type"].payload.tobytes(),
               h_groups=grp.tobytes(), h_hist=[hist[int(f): int(f) + int(k)].tobytes() for f, k in zip(grp["first"], grp["n_len"])])
    return out


def test_one_counter_through_a_fixed_sequence():
    big = Problem("big", 4097, 70, 1000, 11, 60000, 2000)
    small = Problem("small", 65, 3, 25, 12, 9000, 100)
    assert (big.u.n, big.u.ns, small.u.n, small.u.ns) == (4097, 70, 65, 3) and big.nt != small.nt and big.n_ctx != small.n_ctx
    streams = {"big": tj.synth_stream(60000, 150, 300000, variant_seed=1), "small": tj.synth_stream(3000, 100, 20000, seed_reads=99, variant_seed=2)}
    m = 3
    fresh = {}
    for p in (big, small):                                                    # every entry on a counter of its own
        for name, entry in ENTRIES.items():
            f = tj.Counter(K)
            fresh[name, p.name] = entry(f, p)
            f.close()
    for name, s in streams.items():
        f = tj.Counter(K)
        f.scan_host(s, m)
        fresh["sample", name] = sample_state(f, m)
        f.close()
    assert fresh["sample", "big"]["status"] == 0 == fresh["sample", "small"]["status"] and fresh["sample", "big"]["kept"] != fresh["sample", "small"]["kept"]

    c = tj.Counter(K)
    c.scan_host(streams["big"], m)                                            # a sample of its own: the cross-sample entries leave it as it is
    assert sample_state(c, m) == fresh["sample", "big"]
    kept_before = c.download_kept().tobytes()
    for p in (big, small):                                                    # every entry on the large problem, then on the small one
        for name, entry in ENTRIES.items():
            assert entry(c, p) == fresh[name, p.name], (name, p.name)
    for kind, refuse in REFUSALS.items():                                     # every entry directly after each kind of refused call
        for name, entry in ENTRIES.items():
            refuse(c, big)
            assert entry(c, small) == fresh[name, "small"], (name, "after a refusal:", kind)
    assert c.download_kept().tobytes() == kept_before and c.n_kept * 40 == len(kept_before)
    for name, entry in ENTRIES.items():                                       # and the large problem once more, after all that
        assert entry(c, big) == fresh[name, "big"], (name, "big again")
    c.reset()                                                                 # forget the sample, keep the buffers; scan a smaller one
    assert c.raw_count() == 0
    c.scan_host(streams["small"], m)
    assert sample_state(c, m) == fresh["sample", "small"]
    for name, entry in ENTRIES.items():
        assert entry(c, small) == fresh[name, "small"], (name, "after the reset")
    c.reset()
    stream = bc.dev(streams["big"])                                           # from device memory this time: the stream is a const input
    with frozen(stream):
        c.scan_device(stream.data_ptr(), stream.numel(), m)
        assert sample_state(c, m) == fresh["sample", "big"]
    c.close()
