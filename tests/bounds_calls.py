"""The case table of the bounds tests (every exported entry that takes an output pointer, and what it writes through it)
and one caller per device entry that puts every output into a guarded buffer of exactly the size the header asks for,
holds the const inputs frozen, makes the call, and checks guards and inputs before it returns.
tests/test_buffer_bounds.py, tests/test_sample_widths.py, tests/test_variant_bounds.py and tests/test_counter_reuse.py all call
through these.  The sample-comparison layer (N14-N21) has its callers and its part of the table in tests/sample_calls.py."""
import ctypes as C
import functools
import random

import numpy as np

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, GuardedHost, frozen

ERR_ARG, ERR_CAP = 3, 4
TS, TR, SU, LOC = tj.TRACT_SUMMARY_DTYPE, tj.UNION_TRACT_DTYPE, tj.UNION_TRACT_SUMMARY_DTYPE, tj.LOCATION_DTYPE
VAR, TF, EF, ST, AL = tj.VARIANT_DTYPE, tj.TRACT_FEATURE_DTYPE, tj.EFFECT_DTYPE, tj.SITE_DTYPE, tj.ALLELE_DTYPE
SDP = tj.SITE_DEPTH_DTYPE
N_STATS = 5                              # TJAMD_N_TRACT_STATS

# row counts, tract counts and query counts of the device entries: one on each side of, and at, every constant by which the
# cross-sample kernels cut their work: the wavefront (64), the block (256), RS_ITEMS (1024: a block's items in the
# key-value sort; RS_WAVE_ITEMS, 256, is a wavefront's share of them) and SC_ITEMS (4096: a block's items in the scans)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)

# entry -> the outputs it writes through caller pointers.  DEVICE: device memory, tests/test_buffer_bounds.py
DEVICE = {
    "tjamd_merge_samples": ("d_out_keys", "d_out_counts"),
    "tjamd_tract_ids": ("d_tract_id", "h_tract_id"),
    "tjamd_tract_stats": ("d_summary", "d_var"),
    "tjamd_tract_sample_stats": ("d_values", "d_modal_len", "d_n_context"),
    "tjamd_union_tracts": ("d_tract_id", "d_join_type", "d_tracts"),
    "tjamd_union_tract_stats": ("d_summary", "d_var", "d_sel"),
    "tjamd_union_tract_sample_stats": ("d_values", "d_modal_len", "d_n_context", "d_n_len"),
    "tjamd_locate": ("d_loc",),
    "tjamd_located_tracts": ("d_perm", "d_out_keys", "d_out_counts", "d_out_tracts", "d_tract_loc", "d_ref_length"),
    # the variant layer, N8-N13, each declared in a header of its own (tests/test_locate_gapped_bounds.py, tests/test_variant_bounds.py)
    "tjamd_locate_gapped": ("d_loc", "d_how"),
    "tjamd_tract_variants": ("d_out", "h_offsets"),
    "tjamd_tract_features": ("d_out",),
    "tjamd_variant_effects": ("d_out",),
    "tjamd_merge_variants": ("d_sites", "d_alleles", "d_genotype", "d_allele_of", "d_unique"),
    "tjamd_site_depths": ("d_genotype", "d_depth", "d_allele_depth", "d_summary"),
}
# HOST: host memory, written by an entry that needs a GPU (tests/test_buffer_bounds.py)
HOST = {
    "tjamd_download_raw": ("out",),
    "tjamd_download_kept": ("out",),
    "tjamd_download_idx": ("idx_initial", "idx_final"),
    "tjamd_scan_host_located": ("out",),
    "tjamd_group_contexts": ("group_of", "groups"),
    "tjamd_context_histograms": ("group_of", "join_type", "groups", "hist"),
    "tjamd_reference_download": ("out",),
    "tjamd_scan_windows": ("out", "window_of"),
    "tjamd_device_download": ("host",),
    "tjamd_gather_histograms": ("counts",),
    "tjamd_annotation_download": ("h_points", "h_winner"),
    "tjamd_coding_download": ("out",),
}
# CPU: host memory, written without a GPU (tests/test_host_bounds.py)
CPU = {
    "tjamd_read_file_stream": ("out",),
    "tjamd_read_file_stream_mt": ("out",),
    "tjamd_synth_stream": ("out",),
    "tjamd_peer_access_report": ("out",),
    "tjamd_read_file_names": ("out",),
    "tjamd_gff3_read": ("out", "strings"),
    "tjamd_translate": ("out",),
    "tjamd_gff3_read_phase": ("out",),
    "tjamd_site_ref_alt": ("out",),
}
# entries of the headers under include/ with a pointer parameter that is not const and that the tables above leave out, and why
ALLOW = {
    "tjamd_counter_set_stream": "hip_stream is a handle that is stored, nothing is written through it",
    "tjamd_counter_set_order_stream": "hip_stream is a handle that is stored, nothing is written through it",
    "tjamd_comm_set_stream": "hip_stream is a handle that is stored, nothing is written through it",
    "tjamd_host_free": "takes back a pointer of tjamd_host_alloc, writes nothing",
    "tjamd_device_free": "takes back a pointer of tjamd_device_alloc, writes nothing",
    "tjamd_finalise": "writes one int through a pointer to a scalar",
    "tjamd_finalise_end": "writes one int through a pointer to a scalar",
    "tjamd_comm_unique_id": "writes the fixed TJAMD_COMM_ID_BYTES that RCCL's ncclGetUniqueId fills; no size of the caller's to overrun",
    "tjamd_comm_last_exchange": "writes three scalars through pointers to scalars",
    "tjamd_allgather_histograms": "a collective between processes: counts[world] and one pointer, run by tests/test_dist_gloo.py",
}


def torch():
    """imported at the first use, so that the CPU tests can read the tables without it; a torch that does not import is an
    error of the test that needs it, never a skip"""
    import torch as t
    return t


def dev(a, dt=np.uint8):
    """a numpy array as a flat device tensor of its bytes (or of dt)"""
    return torch().from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()


def _p(x):
    if x is None:
        return None
    if isinstance(x, (GuardedDevice, GuardedHost)):
        return x.c
    return C.c_void_p(x.data_ptr()) if x.numel() else None


def _p0(g, cap):
    """an output with a capacity: NULL at a capacity of 0, as a caller with nothing to receive passes it"""
    return _p(g) if cap else None


class Union:
    """a union (keys uint64 [n, 3], mat int32 [n, n_samples]) and its samples' coverages, on the host and on the device"""

    def __init__(self, keys, mat, cov):
        self.keys = np.ascontiguousarray(np.asarray(keys, np.uint64).reshape(-1, 3))
        self.mat = np.ascontiguousarray(np.asarray(mat, np.int32))
        assert self.mat.ndim == 2 and len(self.mat) == len(self.keys)
        self.n, self.ns = int(self.mat.shape[0]), int(self.mat.shape[1])
        self.cov = [int(x) for x in cov]
        assert len(self.cov) == self.ns
        self.cov_c = (C.c_int * self.ns)(*self.cov)

    @functools.cached_property
    def kd(self):
        return dev(self.keys)

    @functools.cached_property
    def md(self):
        return torch().from_numpy(self.mat.copy()).cuda()

    def cut(self, n):
        return Union(self.keys[:n], self.mat[:n], self.cov)

    def sample_records(self):
        """each sample's records in union order, the count field holding the sample's count: what tjamd_merge_samples
        merges back into this union -> (uint64 [total, 3], [records per sample])"""
        recs = []
        for s in range(self.ns):
            rows = np.flatnonzero(self.mat[:, s] > 0)
            r = self.keys[rows].copy()
            r[:, 2] = (r[:, 2] & ~np.uint64(0xFFFFF << 12)) | ((self.mat[rows, s].astype(np.uint64) & np.uint64(0xFFFFF)) << np.uint64(12))
            recs.append(r)
        return np.concatenate(recs), [len(r) for r in recs]


class Result:
    def __init__(self, rc, outs, **extra):
        self.rc = int(rc)
        self.err = tj.lib().tjamd_last_error().decode(errors="replace") if rc < 0 else ""
        self.outs = outs
        self.__dict__.update(extra)

    def __getitem__(self, name):
        return self.outs[name]

    def refused(self, code, *words):
        assert self.rc == -code and all(w in self.err for w in words), (self.rc, self.err)

    def bytes_of(self, name):
        return self.outs[name].view(np.uint8).tobytes()


def _buffers(spec, null, host=()):
    """{name: bytes} -> {name: guarded buffer, or None for the names in null}"""
    assert set(null) <= set(spec), (null, list(spec))
    return {name: None if name in null else (GuardedHost if name in host else GuardedDevice)(nb) for name, nb in spec.items()}


def _checked(outs):
    torch().cuda.synchronize()
    for name, g in outs.items():
        if g is not None:
            g.check(name)


def call_merge_samples(c, records, counts, ns, cap):
    rd = dev(records)
    cnt = (C.c_long * ns)(*counts)
    outs = _buffers({"d_out_keys": cap * 24, "d_out_counts": cap * ns * 4}, ())
    with frozen(rd):
        rc = tj.lib().tjamd_merge_samples(c._h, _p(rd), cnt, ns, _p(outs["d_out_keys"]), _p(outs["d_out_counts"]), cap)
        _checked(outs)
    return Result(rc, outs)


def call_tract_ids(c, u, n=None, null=()):
    n = u.n if n is None else n
    outs = _buffers({"d_tract_id": n * 4, "h_tract_id": n * 4}, null, host=("h_tract_id",))
    with frozen(u.kd):
        rc = tj.lib().tjamd_tract_ids(c._h, _p(u.kd), n, _p(outs["d_tract_id"]), _p(outs["h_tract_id"]))
        _checked(outs)
    return Result(rc, outs)


def call_tract_stats(c, u, cap, ids=None, ref=None, n=None, null=()):
    """ids, ref: device int32 tensors or None; null may also name n_var"""
    n = u.n if n is None else n
    outs = _buffers({"d_summary": cap * TS.itemsize, "d_var": cap * 4}, set(null) - {"n_var"})
    nv = C.c_long(-1)
    with frozen(u.kd, u.md, ids, ref):
        rc = tj.lib().tjamd_tract_stats(c._h, _p(u.kd), _p(u.md), n, u.ns, _p(ids), u.cov_c, _p(ref), _p(outs["d_summary"]), _p(outs["d_var"]), cap,
                                        None if "n_var" in null else C.byref(nv))
        _checked(outs)
    return Result(rc, outs, n_var=nv.value)


def call_tract_sample_stats(c, u, summary, nt, lst, n_list=None, null=()):
    """summary: device bytes of tjamd_tract_summary[nt]; lst: device int32 tensor"""
    n_list = int(lst.numel()) if n_list is None else n_list
    outs = _buffers({"d_values": n_list * N_STATS * u.ns * 8, "d_modal_len": n_list * u.ns * 4, "d_n_context": n_list * u.ns * 4}, null)
    with frozen(u.kd, u.md, summary, lst):
        rc = tj.lib().tjamd_tract_sample_stats(c._h, _p(u.kd), _p(u.md), u.n, u.ns, u.cov_c, _p(summary), nt, _p(lst), n_list,
                                               _p(outs["d_values"]), _p(outs["d_modal_len"]), _p(outs["d_n_context"]))
        _checked(outs)
    return Result(rc, outs)


def call_union_tracts(c, u, maxd, lev, cap, n=None, null=()):
    n = u.n if n is None else n
    outs = _buffers({"d_tract_id": n * 4, "d_join_type": n * 4, "d_tracts": cap * TR.itemsize}, null)
    with frozen(u.kd, u.md):
        rc = tj.lib().tjamd_union_tracts(c._h, _p(u.kd), _p(u.md), n, u.ns, maxd, lev, _p(outs["d_tract_id"]), _p(outs["d_join_type"]), _p(outs["d_tracts"]), cap)
        _checked(outs)
    return Result(rc, outs)


def call_union_tract_stats(c, u, tracts, nt, ref=None, n=None, null=()):
    """tracts: device bytes of tjamd_union_tract[nt]; null may also name n_var, n_sel"""
    n = u.n if n is None else n
    outs = _buffers({"d_summary": nt * SU.itemsize, "d_var": nt * 4, "d_sel": nt * 4}, set(null) - {"n_var", "n_sel"})
    nv, nsel = C.c_long(-1), C.c_long(-1)
    with frozen(u.kd, u.md, tracts, ref):
        rc = tj.lib().tjamd_union_tract_stats(c._h, _p(u.kd), _p(u.md), n, u.ns, _p(tracts), nt if n else 0, u.cov_c, _p(ref), _p(outs["d_summary"]), _p(outs["d_var"]),
                                              None if "n_var" in null else C.byref(nv), _p(outs["d_sel"]), None if "n_sel" in null else C.byref(nsel))
        _checked(outs)
    return Result(rc, outs, n_var=nv.value, n_sel=nsel.value)


def call_union_tract_sample_stats(c, u, summary, nt, lst, n_list=None, null=()):
    n_list = int(lst.numel()) if n_list is None else n_list
    per = n_list * u.ns * 4
    outs = _buffers({"d_values": n_list * N_STATS * u.ns * 8, "d_modal_len": per, "d_n_context": per, "d_n_len": per}, null)
    with frozen(u.kd, u.md, summary, lst):
        rc = tj.lib().tjamd_union_tract_sample_stats(c._h, _p(u.kd), _p(u.md), u.n, u.ns, u.cov_c, _p(summary), nt, _p(lst), n_list,
                                                     _p(outs["d_values"]), _p(outs["d_modal_len"]), _p(outs["d_n_context"]), _p(outs["d_n_len"]))
        _checked(outs)
    return Result(rc, outs)


def call_locate(c, ref, kd, n, mm):
    """kd: device bytes of tjamd_record[>= n]"""
    outs = _buffers({"d_loc": n * LOC.itemsize}, ())
    with frozen(kd):
        rc = tj.lib().tjamd_locate(c._h, ref._h, _p(kd), n, mm, _p(outs["d_loc"]))
        _checked(outs)
    return Result(rc, outs)


def call_located_tracts(c, u, tracts, nt, loc, cap, n=None, null=()):
    """tracts: device bytes of tjamd_union_tract[nt], or None (the context-keyed tracts); loc: device bytes of tjamd_location[n]"""
    n = u.n if n is None else n
    outs = _buffers({"d_perm": n * 4, "d_out_keys": n * 24, "d_out_counts": n * u.ns * 4, "d_out_tracts": cap * TR.itemsize,
                     "d_tract_loc": cap * LOC.itemsize, "d_ref_length": cap * 4}, null)
    with frozen(u.kd, u.md, tracts, loc):
        rc = tj.lib().tjamd_located_tracts(c._h, _p(u.kd), _p(u.md), n, u.ns, _p(tracts), nt if tracts is not None else 0, _p(loc),
                                           *[_p(outs[name]) for name in DEVICE["tjamd_located_tracts"]], cap)
        _checked(outs)
    return Result(rc, outs)


def call_locate_gapped(c, ref, kd, n, max_edits, max_shift):
    """kd: device bytes of tjamd_record[>= n]; d_loc goes in with no row located, so the call tries every row"""
    from tests.test_locate_cabi import NOWHERE
    outs = _buffers({"d_loc": n * LOC.itemsize, "d_how": n * 4}, ())
    outs["d_loc"].payload.copy_(dev(np.array([NOWHERE] * n, LOC)))
    with frozen(kd):
        rc = tj.lib().tjamd_locate_gapped(c._h, ref._h, _p(kd), n, max_edits, max_shift, _p(outs["d_loc"]), _p(outs["d_how"]))
        _checked(outs)
    return Result(rc, outs)


def call_tract_variants(c, ref, u, tracts, nt, tract_loc, cap, lst=None, n_list=None):
    """tracts, tract_loc: device bytes of tjamd_union_tract[nt] and tjamd_location[nt]; lst: device int32 tensor, or None (every tract);
    n_list: the entries of lst to take (all of them).  Capacity 0 passes a NULL d_out.  .ms: the entry's timer after the call"""
    outs = _buffers({"d_out": cap * VAR.itemsize, "h_offsets": (u.ns + 1) * 8}, (), host=("h_offsets",))
    n_list = (0 if lst is None else int(lst.numel())) if n_list is None else n_list
    with frozen(u.kd, u.md, tracts, tract_loc, lst):
        rc = tj.lib().tjamd_tract_variants(c._h, ref._h, _p(u.kd), _p(u.md), u.n, u.ns, _p(tracts), nt, _p(tract_loc), None if lst is None else C.c_void_p(lst.data_ptr()), n_list,
                                           _p0(outs["d_out"], cap), cap, _p(outs["h_offsets"]))
        _checked(outs)
    return Result(rc, outs, ms=c.last_tract_variants_ms())


def call_tract_features(c, ann, u, tracts, nt, tract_loc):
    outs = _buffers({"d_out": nt * TF.itemsize}, ())
    with frozen(u.kd, u.md, tracts, tract_loc):
        rc = tj.lib().tjamd_tract_features(c._h, ann._h, _p(u.kd), _p(u.md), u.n, u.ns, _p(tracts), nt, _p(tract_loc), _p(outs["d_out"]))
        _checked(outs)
    return Result(rc, outs, ms=c.last_tract_features_ms())


def call_variant_effects(c, cod, variants, n, tract_feat=None, nt=0):
    """variants: device bytes of tjamd_variant[n]; tract_feat: device bytes of tjamd_tract_feature[nt], or None"""
    outs = _buffers({"d_out": n * EF.itemsize}, ())
    with frozen(variants, tract_feat):
        rc = tj.lib().tjamd_variant_effects(c._h, cod._h, _p(variants), n, _p(tract_feat), nt, _p(outs["d_out"]))
        _checked(outs)
    return Result(rc, outs, ms=c.last_variant_effects_ms())


def call_merge_variants(c, k, variants, n, ns, nt, site_cap, allele_cap, null=()):
    """variants: device bytes of tjamd_variant[>= n]; null: the optional outputs (d_genotype, d_allele_of, d_unique) passed as NULL;
    d_sites and d_alleles are NULL at a capacity of 0.  d_genotype is sized by the site capacity, as the header sizes it"""
    assert set(null) <= {"d_genotype", "d_allele_of", "d_unique"}
    outs = _buffers({"d_sites": site_cap * ST.itemsize, "d_alleles": allele_cap * AL.itemsize, "d_genotype": site_cap * ns * 2, "d_allele_of": n * 4,
                     "d_unique": allele_cap * VAR.itemsize}, null)
    na = C.c_long(-1)
    with frozen(variants):
        rc = tj.lib().tjamd_merge_variants(c._h, k, _p(variants), n, ns, nt, _p0(outs["d_sites"], site_cap), site_cap, _p0(outs["d_alleles"], allele_cap), allele_cap,
                                           _p(outs["d_genotype"]), _p(outs["d_allele_of"]), _p(outs["d_unique"]), C.byref(na))
        _checked(outs)
    return Result(rc, outs, n_alleles=na.value, ms=c.last_merge_variants_ms())


def call_site_depths(c, ref, u, tracts, nt, tract_loc, sites, n_sites, alleles, n_alleles, null=()):
    """sites, alleles: device bytes of tjamd_site[n_sites] and tjamd_allele[n_alleles] (None with a count of 0); null: the outputs passed
    as NULL.  AD is guarded at exactly (n_sites + n_alleles) * n_samples ints: a site's last class row ends on the payload's last byte"""
    outs = _buffers({"d_genotype": n_sites * u.ns * 2, "d_depth": n_sites * u.ns * 4, "d_allele_depth": (n_sites + n_alleles) * u.ns * 4,
                     "d_summary": n_sites * SDP.itemsize}, null)
    with frozen(u.kd, u.md, tracts, tract_loc, sites, alleles):
        rc = tj.lib().tjamd_site_depths(c._h, ref._h, _p(u.kd), _p(u.md), u.n, u.ns, _p(tracts), nt, _p(tract_loc), _p(sites), n_sites, _p(alleles), n_alleles,
                                        *[_p(outs[name]) for name in DEVICE["tjamd_site_depths"]])
        _checked(outs)
    return Result(rc, outs, ms=c.last_site_depths_ms())


def call_annotation_download(ann, cap):
    outs = _buffers({"h_points": cap * 8, "h_winner": cap * 4}, (), host=("h_points", "h_winner"))
    rc = tj.lib().tjamd_annotation_download(ann._h, _p(outs["h_points"]), _p(outs["h_winner"]), cap)
    _checked(outs)
    return Result(rc, outs)


def call_coding_download(cod, cap):
    outs = _buffers({"out": cap * tj.CDS_DTYPE.itemsize}, (), host=("out",))
    rc = tj.lib().tjamd_coding_download(cod._h, _p(outs["out"]), cap)
    _checked(outs)
    return Result(rc, outs)


# ---- the outputs in the shape the suite's checks take (tests/test_tract_stats.py, test_union_tracts.py, test_locate.py) ----

def arange_dev(n):
    return torch().arange(n, dtype=torch().int32, device="cuda")


def tract_stats_of(c, u, cap, ids=None, ref=None):
    """tjamd_tract_stats at capacity cap, then tjamd_tract_sample_stats on every tract -> (n_tracts, dict for
    check_against_restatement), or (rc, Result) if the first call is refused"""
    r = call_tract_stats(c, u, cap, ids=ids, ref=ref)
    if r.rc < 0:
        return r.rc, r
    nt = r.rc
    v = call_tract_sample_stats(c, u, r["d_summary"].payload, nt, arange_dev(nt))
    assert v.rc == nt, v.err
    return nt, {"summary": r["d_summary"].view(TS, nt), "variable": r["d_var"].view(np.int32, r.n_var),
                "values": v["d_values"].view(np.float64).reshape(nt, N_STATS, u.ns), "modal_len": v["d_modal_len"].view(np.int32).reshape(nt, u.ns),
                "n_context": v["d_n_context"].view(np.int32).reshape(nt, u.ns), "raw": (r, v)}


def union_stats_of(c, u, tracts, nt, ref=None):
    """tjamd_union_tract_stats, then tjamd_union_tract_sample_stats on every tract -> dict for check_stats"""
    s = call_union_tract_stats(c, u, tracts, nt, ref=ref)
    assert s.rc == nt, s.err
    v = call_union_tract_sample_stats(c, u, s["d_summary"].payload, nt, arange_dev(nt))
    assert v.rc == nt, v.err
    per = lambda name: v[name].view(np.int32).reshape(nt, u.ns)
    return {"summary": s["d_summary"].view(SU, nt), "variable": s["d_var"].view(np.int32, s.n_var), "selected": s["d_sel"].view(np.int32, s.n_sel),
            "values": v["d_values"].view(np.float64).reshape(nt, N_STATS, u.ns), "modal_len": per("d_modal_len"), "n_context": per("d_n_context"),
            "n_len": per("d_n_len"), "raw": (s, v)}


def union_tracts_of(c, u, maxd, lev, cap):
    """tjamd_union_tracts at capacity cap and both statistics entries -> (n_tracts, dict for check_grouping and check_stats)"""
    g = call_union_tracts(c, u, maxd, lev, cap)
    if g.rc < 0:
        return g.rc, g
    nt = g.rc
    got = union_stats_of(c, u, g["d_tracts"].payload, nt)
    got.update({"tract_id": g["d_tract_id"].view(np.int32), "join_type": g["d_join_type"].view(np.int32), "tracts": g["d_tracts"].view(TR, nt),
                "d_tracts": g["d_tracts"].payload, "raw": (g,) + got["raw"]})
    return nt, got


def located_tracts_of(c, u, tracts, nt_in, loc, cap):
    """-> (n_tracts, dict for check_located_tracts, with the guarded outputs under "raw")"""
    r = call_located_tracts(c, u, tracts, nt_in, loc, cap)
    if r.rc < 0:
        return r.rc, r
    nt = r.rc
    return nt, {"perm": r["d_perm"].view(np.int32), "keys": r["d_out_keys"].view(np.uint64).reshape(-1, 3), "mat": r["d_out_counts"].view(np.int32).reshape(u.n, u.ns),
                "tracts": r["d_out_tracts"].view(TR, nt), "tract_loc": r["d_tract_loc"].view(LOC, nt), "ref_length": r["d_ref_length"].view(np.int32, nt), "raw": r}


def tracts_from_grouping(g, n):
    """oracle_union_grouping's tracts as tjamd_union_tract (UNION_TRACT_DTYPE)"""
    first = np.asarray(g["groups"]["first"], np.int64)
    tr = np.zeros(len(first), TR)
    tr["first"], tr["n_rows"] = first, np.diff(np.r_[first, n])
    tr["n_context"], tr["indel"] = g["groups"]["n_context"], g["groups"]["indel"]
    tr["mode"], tr["lev_distance"], tr["integral"] = g["mode"], g["lev_distance"], g["integral"]
    return tr


def planted_locations(keys, seed):
    """a place per context as tests/test_locate.py plants them: many contexts share one, a fifth have none"""
    from tests.test_locate_cabi import NOWHERE
    rng = random.Random(seed)
    place = {}
    loc = np.zeros(len(keys), LOC)
    for i, (c0, c1, meta) in enumerate(np.asarray(keys, np.uint64).reshape(-1, 3).tolist()):
        ctx = (c0, c1, meta & 3)
        if ctx not in place:
            flat = rng.randrange(0, 400) if rng.random() < 0.5 else (1 << 33) + rng.randrange(0, 1 << 20)
            place[ctx] = NOWHERE if rng.random() < 0.2 else (flat, flat % 7, flat % 1000, rng.randrange(1, 15), rng.randrange(3), rng.randrange(2), rng.randrange(1, 3))
        loc[i] = place[ctx]
    return loc
