"""ctypes mirror of the C boundary (include/tatajuba_hopo.h, include/tatajuba_amd.h, include/tatajuba_variants.h and
include/tatajuba_features.h).

Two views of the same library:
  * HopoCounter / Options -- the drop-in API with the reference's names (new_or_append_hopo_counter_from_file,
    update_hopo_counter_from_seq, finalise_hopo_counter, del_hopo_counter; reference: src/hopo_counter.h:68-80), so that
    parity tests read like calls into tatajuba itself;
  * Counter -- the tjamd_* extension for device-resident read streams (benchmark, multi-GPU).
Nothing here computes: every result comes from the HIP kernels through the C ABI, and a missing library or GPU raises.
"""
import ctypes as C
import os

import numpy as np

from .build import build_library, library_path

ELEM_DTYPE = np.dtype([("ctx0", "<u8"), ("ctx1", "<u8"), ("meta", "<u8"), ("read_offset", "<i4"),
                       ("loc_ref_id", "<i4"), ("loc_pos", "<i4"), ("loc_last", "<i4")])
RECORD_DTYPE = np.dtype([("ctx0", "<u8"), ("ctx1", "<u8"), ("meta", "<u8")])
GROUP_DTYPE = np.dtype([("first", "<i4"), ("n_elem", "<i4"), ("n_context", "<i4"), ("mode", "<i4"), ("integral", "<i8")])
# tjamd_context_group / tjamd_length_freq (include/tatajuba_amd.h)
CONTEXT_GROUP_DTYPE = np.dtype([("first", "<i4"), ("n_elem", "<i4"), ("n_context", "<i4"), ("mode", "<i4"), ("indel", "<i4"), ("n_len", "<i4"),
                                ("modal_len", "<i4"), ("modal_freq", "<i4"), ("integral", "<i8")])
LENGTH_FREQ_DTYPE = np.dtype([("length", "<i4"), ("freq", "<i4")])
LOCATED_DTYPE = np.dtype([("ctx0", "<u8"), ("ctx1", "<u8"), ("meta", "<u8"), ("pos", "<u8")])
# tjamd_tract_summary (include/tatajuba_amd.h): reldiff in the order of TJAMD_STAT_* (avg length, modal freq, prop coverage,
# coverage per context, entropy)
N_TRACT_STATS = 5
TRACT_SUMMARY_DTYPE = np.dtype([("first", "<i4"), ("n_rows", "<i4"), ("n_present", "<i4"), ("variable", "<i4"), ("reldiff", "<f8", (N_TRACT_STATS,))])
assert TRACT_SUMMARY_DTYPE.itemsize == 56
# tjamd_union_tract / tjamd_union_tract_summary (include/tatajuba_amd.h): reldiff in TJAMD_STAT_* order, as above
UNION_TRACT_DTYPE = np.dtype([("first", "<i4"), ("n_rows", "<i4"), ("n_context", "<i4"), ("mode", "<i4"), ("indel", "<i4"),
                              ("lev_distance", "<i4"), ("integral", "<i8")])
assert UNION_TRACT_DTYPE.itemsize == 32
UNION_TRACT_SUMMARY_DTYPE = np.dtype([("first", "<i4"), ("n_rows", "<i4"), ("n_present", "<i4"), ("variable", "<i4"), ("selected", "<i4"),
                                      ("lev_distance", "<i4"), ("reldiff", "<f8", (N_TRACT_STATS,))])
assert UNION_TRACT_SUMMARY_DTYPE.itemsize == 64
# tjamd_ref_entry / tjamd_location (include/tatajuba_amd.h): the reference index and a row's place on it
REF_ENTRY_DTYPE = np.dtype([("ctx0", "<u8"), ("ctx1", "<u8"), ("flat", "<i8"), ("contig", "<i4"), ("pos", "<i4"), ("length", "<i4"),
                            ("base", "<i4"), ("neg_strand", "<i4"), ("pad", "<i4")])
assert REF_ENTRY_DTYPE.itemsize == 48
LOCATION_DTYPE = np.dtype([("flat", "<i8"), ("contig", "<i4"), ("pos", "<i4"), ("ref_length", "<i4"), ("mismatches", "<i4"),
                           ("neg_strand", "<i4"), ("n_hits", "<i4")])
assert LOCATION_DTYPE.itemsize == 32
# tjamd_variant (include/tatajuba_variants.h): one tract-length variant of one sample, the fields of a VCF record
VARIANT_DTYPE = np.dtype([("flat", "<i8"), ("tract", "<i4"), ("sample", "<i4"), ("contig", "<i4"), ("pos", "<i4"), ("row", "<i4"), ("base", "<i4"),
                          ("ref_length", "<i4"), ("alt_length", "<i4"), ("n_flank", "<i4"), ("pad", "<i4"), ("ref_flank", "<u8"), ("alt_flank", "<u8")])
assert VARIANT_DTYPE.itemsize == 64
# tjamd_feature and tjamd_tract_feature (include/tatajuba_features.h): one feature line of a GFF3 file; a tract's feature and longest modal length
FEATURE_DTYPE = np.dtype([("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("cls", "<i4"), ("strand", "<i4"), ("line", "<i4"), ("type_off", "<i4"), ("id_off", "<i4")])
assert FEATURE_DTYPE.itemsize == 32
TRACT_FEATURE_DTYPE = np.dtype([("feature", "<i4"), ("max_length", "<i4")])
assert TRACT_FEATURE_DTYPE.itemsize == 8
# tjamd_cds and tjamd_effect (include/tatajuba_effects.h): where a feature's protein ends; what a variant record does to it
CDS_DTYPE = np.dtype([("aa_len", "<i4"), ("has_stop", "<i4"), ("n_codons", "<i4"), ("phase", "<i4")])
assert CDS_DTYPE.itemsize == 16
EFFECT_DTYPE = np.dtype([("feature", "<i4"), ("cls", "<i4"), ("cds_pos", "<i4"), ("first_diff", "<i4"), ("ref_aa_len", "<i4"), ("alt_aa_len", "<i4"),
                         ("flags", "<i4"), ("pad", "<i4"), ("ref_aa", "<u8"), ("alt_aa", "<u8")])
assert EFFECT_DTYPE.itemsize == 48
EFFECT_CLASSES = ["NONE", "BOUNDARY", "IDENTICAL", "INFRAME", "FRAMESHIFT"]      # TJAMD_EFFECT_*
# tjamd_site and tjamd_allele (include/tatajuba_sites.h): a tract with records, merged over the samples; one of its distinct alleles
SITE_DTYPE = np.dtype([("flat", "<i8"), ("tract", "<i4"), ("contig", "<i4"), ("pos", "<i4"), ("base", "<i4"), ("ref_length", "<i4"), ("min_length", "<i4"),
                       ("n_flank", "<i4"), ("n_alleles", "<i4"), ("first_allele", "<i4"), ("n_called", "<i4"), ("first_record", "<i4"), ("pad", "<i4"),
                       ("ref_flank", "<u8")])
assert SITE_DTYPE.itemsize == 64
ALLELE_DTYPE = np.dtype([("site", "<i4"), ("alt_length", "<i4"), ("n_flank", "<i4"), ("n_samples", "<i4"), ("first_record", "<i4"), ("pad", "<i4"),
                         ("alt_flank", "<u8")])
assert ALLELE_DTYPE.itemsize == 32
SITE_DEPTH_DTYPE = np.dtype([("n_ref", "<i4"), ("n_missing", "<i4"), ("depth", "<i8")])      # tjamd_site_depth (include/tatajuba_depths.h)
assert SITE_DEPTH_DTYPE.itemsize == 16
SAMPLE_DISTANCE_DTYPE = np.dtype([("n_both", "<i4"), ("n_differ", "<i4"), ("length_diff", "<i8")])      # tjamd_sample_distance (include/tatajuba_distances.h)
assert SAMPLE_DISTANCE_DTYPE.itemsize == 16
LINK_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("key", "<i8")])      # tjamd_link (include/tatajuba_linkage.h)
assert LINK_DTYPE.itemsize == 16
LINK_DIFFER, LINK_LENGTH, LINK_DIFFER_RATE = 0, 1, 2                     # TJAMD_LINK_*: the metric of tjamd_sample_linkage
GROUP_CALL_DTYPE = np.dtype([("n_called", "<i4"), ("fixed", "<i4"), ("n_outside", "<i4"), ("mark", "<i4")])            # tjamd_group_call (include/tatajuba_groups.h)
GROUP_SITE_DTYPE = np.dtype([("n_called", "<i4"), ("n_genotypes", "<i4"), ("n_marks", "<i4"), ("first_group", "<i4")])  # tjamd_group_site
GROUP_MARK_DTYPE = np.dtype([("site", "<i4"), ("group", "<i4"), ("genotype", "<i4"), ("n_called", "<i4")])             # tjamd_group_mark
assert GROUP_CALL_DTYPE.itemsize == 16 and GROUP_SITE_DTYPE.itemsize == 16 and GROUP_MARK_DTYPE.itemsize == 16
TREE_NODE_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4"), ("first", "<i4"), ("size", "<i4")])    # tjamd_tree_node (include/tatajuba_clades.h)
assert TREE_NODE_DTYPE.itemsize == 16
CONSENSUS_NODE_DTYPE = np.dtype([("parent", "<i4"), ("count", "<i4"), ("first", "<i4"), ("size", "<i4")])   # tjamd_consensus_node (include/tatajuba_consensus.h)
assert CONSENSUS_NODE_DTYPE.itemsize == 16


class TatajubaAmdError(RuntimeError):
    pass


def _sx(v, bits):
    v = v.astype(np.int64) & ((1 << bits) - 1)
    return np.where(v >= (1 << (bits - 1)), v - (1 << bits), v)


def decode_meta(meta):
    """hopo_element bitfield word -> signed fields (layout: include/tatajuba_hopo.h)"""
    m = np.asarray(meta, dtype=np.uint64)
    sh = lambda s: (m >> np.uint64(s))
    return {"base": _sx(sh(0), 2), "length": _sx(sh(2), 10), "count": _sx(sh(12), 20),
            "mismatches": _sx(sh(32), 12), "multi": _sx(sh(44), 3), "neg_strand": _sx(sh(47), 2),
            "canon_flag": _sx(sh(49), 3)}


class Options(C.Structure):
    """tatajuba_options_t (reference: src/hopo_counter.h:20-32), passed by value"""
    _fields_ = [("reference_fasta_filename", C.c_char_p), ("outdir", C.c_char_p),
                ("paired_end", C.c_bool), ("remove_biased", C.c_bool), ("save_vcf", C.c_bool),
                ("gff", C.c_void_p),
                ("max_distance_per_flank", C.c_int), ("kmer_size", C.c_int), ("min_tract_size", C.c_int),
                ("levenshtein_distance", C.c_int), ("min_coverage", C.c_int), ("n_samples", C.c_int),
                ("n_threads", C.c_int)]

    @classmethod
    def defaults(cls, kmer_size=25, min_tract_size=4, min_coverage=5, remove_biased=True, paired_end=False):
        # defaults and clamps of the reference CLI: src/main.c:56-60,184-192
        o = cls()
        o.kmer_size, o.min_tract_size, o.min_coverage = kmer_size, min_tract_size, min_coverage
        o.remove_biased, o.paired_end = remove_biased, paired_end
        o.max_distance_per_flank, o.levenshtein_distance, o.n_samples, o.n_threads = 1, 2, 1, 1
        return o


class _HopoCounterStruct(C.Structure):
    """struct hopo_counter_struct (reference: src/hopo_counter.h:51-59)"""
    _fields_ = [("elem", C.c_void_p), ("name", C.c_char_p),
                ("ref_start", C.c_int), ("n_elem", C.c_int), ("n_alloc", C.c_int), ("kmer_size", C.c_int),
                ("coverage", C.c_int),
                ("idx_initial", C.POINTER(C.c_int)), ("idx_final", C.POINTER(C.c_int)), ("n_idx", C.c_int),
                ("opt", Options), ("ref_counter", C.c_int)]


assert C.sizeof(Options) == 64 and C.sizeof(_HopoCounterStruct) == 136

_LIB = None

# every symbol the two headers declare (checked by tests/test_cabi.py against the .so and the header text)
EXPORTS = [
    "new_hopo_counter", "del_hopo_counter", "new_or_append_hopo_counter_from_file", "update_hopo_counter_from_seq",
    "update_hopo_counter_from_seq_all_monomers",
    "finalise_hopo_counter", "compare_hopo_element_decreasing", "compare_hopo_context",
    "generate_name_from_flanking_contexts", "generate_tract_as_string", "print_tatajuba_options",
    "distance_between_single_context_kmer", "distance_between_context_kmer_pair", "distance_between_context_kmer_pair_with_edit_shift",
    "leftmost_hopo_name_and_length_from_string", "hopo_counter_histogram_integral",
    "dna_in_2_bits", "bit_2_dna",
    "tjamd_device_count", "tjamd_source_hash", "tjamd_last_error", "tjamd_version", "tjamd_counter_create", "tjamd_counter_destroy",
    "tjamd_counter_reset", "tjamd_counter_set_stream", "tjamd_counter_set_order_stream", "tjamd_counter_device", "tjamd_scan_device", "tjamd_scan_host",
    "tjamd_scan_host_located",
    "tjamd_fastq_begin", "tjamd_fastq_push_device", "tjamd_fastq_push_host", "tjamd_fastq_end", "tjamd_fastq_reads", "tjamd_fastq_stop", "tjamd_fastq_stream",
    "tjamd_fastq_stream_bytes", "tjamd_fastq_tile_bytes", "tjamd_last_fastq_ms",
    "tjamd_read_file_stream_mt", "tjamd_host_alloc", "tjamd_host_free", "tjamd_device_alloc", "tjamd_device_free", "tjamd_device_download", "tjamd_sync", "tjamd_mark", "tjamd_wait_mark", "tjamd_reserve", "tjamd_raw_count",
    "tjamd_download_raw", "tjamd_undefined_runs", "tjamd_upload_raw", "tjamd_finalise", "tjamd_finalise_begin", "tjamd_finalise_end", "tjamd_kept_count",
    "tjamd_n_idx", "tjamd_coverage", "tjamd_download_kept", "tjamd_download_idx", "tjamd_kept_device_ptr",
    "tjamd_merge_samples", "tjamd_gather_histograms", "tjamd_peer_access_report", "tjamd_comm_unique_id", "tjamd_comm_create", "tjamd_comm_destroy",
    "tjamd_comm_set_stream", "tjamd_comm_rank", "tjamd_comm_world", "tjamd_comm_collectives", "tjamd_comm_count", "tjamd_comm_last_exchange", "tjamd_last_merge_ms", "tjamd_allgather_histograms", "tjamd_tract_ids", "tjamd_tract_stats", "tjamd_tract_sample_stats", "tjamd_last_tract_stats_ms", "tjamd_union_tracts", "tjamd_union_tract_stats", "tjamd_union_tract_sample_stats", "tjamd_last_union_tracts_ms", "tjamd_last_union_tract_stats_ms", "tjamd_last_union_tract_candidates",
    "tjamd_reference_create", "tjamd_reference_destroy", "tjamd_reference_entries", "tjamd_reference_contigs",
    "tjamd_reference_download", "tjamd_last_reference_ms", "tjamd_locate", "tjamd_last_locate_ms", "tjamd_located_tracts", "tjamd_last_located_tracts_ms",
    "tjamd_last_tract_variants_ms",
    "tjamd_group_contexts", "tjamd_context_histograms", "tjamd_scan_windows", "tjamd_thread_cleanup", "tjamd_last_scan_ms", "tjamd_last_partition_ms", "tjamd_counter_uses_log", "tjamd_last_finalise_ms", "tjamd_last_scan_launches", "tjamd_plan_mismatches",
    "tjamd_synth_stream", "tjamd_read_file_stream",
    # include/tatajuba_context.h
    "new_genomic_context_list", "del_genomic_context_list", "del_context_histogram",
    "distance_between_context_histogram_and_hopo_context", "indel_distance_between_context_histogram_and_hopo_context",
]

# what include/tatajuba_variants.h declares on top of them
VARIANT_EXPORTS = ["tjamd_tract_variants", "tjamd_read_file_names"]
# ... and include/tatajuba_features.h
FEATURE_EXPORTS = ["tjamd_gff3_read", "tjamd_annotation_create", "tjamd_annotation_destroy", "tjamd_annotation_features", "tjamd_annotation_download",
                   "tjamd_tract_features", "tjamd_last_annotation_ms", "tjamd_last_tract_features_ms"]
# ... and include/tatajuba_locate.h
LOCATE_EXPORTS = ["tjamd_flank_edit_distance", "tjamd_reference_add_seeds", "tjamd_reference_has_seeds", "tjamd_locate_gapped",
                  "tjamd_last_seed_order_ms", "tjamd_last_locate_gapped_ms"]
# ... and include/tatajuba_effects.h
EFFECT_EXPORTS = ["tjamd_translate", "tjamd_gff3_read_phase", "tjamd_coding_create", "tjamd_coding_destroy", "tjamd_coding_features", "tjamd_coding_download",
                  "tjamd_variant_effects", "tjamd_last_coding_ms", "tjamd_last_variant_effects_ms"]
# ... and include/tatajuba_sites.h
SITE_EXPORTS = ["tjamd_merge_variants", "tjamd_site_ref_alt", "tjamd_last_merge_variants_ms"]
# ... and include/tatajuba_depths.h
DEPTH_EXPORTS = ["tjamd_site_depths", "tjamd_last_site_depths_ms"]
# ... and include/tatajuba_distances.h
DISTANCE_EXPORTS = ["tjamd_sample_distances", "tjamd_last_sample_distances_ms"]
# ... and include/tatajuba_linkage.h
LINKAGE_EXPORTS = ["tjamd_sample_linkage", "tjamd_linkage_clusters", "tjamd_last_sample_linkage_ms", "tjamd_last_linkage_clusters_ms"]
# ... and include/tatajuba_agglomerate.h
AGGLOMERATE_EXPORTS = ["tjamd_sample_agglomerate", "tjamd_last_sample_agglomerate_ms"]
AGGL_COMPLETE, AGGL_AVERAGE = 1, 2                                        # TJAMD_AGGL_*: the linkage of tjamd_sample_agglomerate
# ... and include/tatajuba_groups.h
GROUP_EXPORTS = ["tjamd_group_sites", "tjamd_last_group_sites_ms"]
# ... and include/tatajuba_clades.h
CLADE_EXPORTS = ["tjamd_linkage_tree", "tjamd_clade_sites", "tjamd_last_linkage_tree_ms", "tjamd_last_clade_sites_ms"]
# ... and include/tatajuba_bootstrap.h
BOOTSTRAP_EXPORTS = ["tjamd_bootstrap_weights", "tjamd_sample_distances_weighted", "tjamd_clade_support",
                     "tjamd_last_bootstrap_weights_ms", "tjamd_last_sample_distances_weighted_ms", "tjamd_last_clade_support_ms"]
# ... and include/tatajuba_replicate_trees.h
REPLICATE_TREE_EXPORTS = ["tjamd_replicate_trees", "tjamd_last_replicate_trees_ms"]
TREE_SINGLE = 0                                                            # TJAMD_TREE_SINGLE: the third linkage of tjamd_replicate_trees, beside AGGL_*
# ... and include/tatajuba_consensus.h
CONSENSUS_EXPORTS = ["tjamd_consensus_tree", "tjamd_last_consensus_tree_ms"]
MAX_SHIFT = 3                     # TJAMD_MAX_SHIFT


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch's wheel bundles its own libamdhip64.so (soname libamdhip64.so.7, the same
    soname our library needs); if ours pulled in /opt/rocm's copy first, a later `import torch` would load a second
    runtime and see no GPU.  So when torch is installed, map its copy first (without importing torch) and let the
    dynamic loader bind libtatajuba_amd.so to it by soname.  TATAJUBA_AMD_HIP_RUNTIME=system skips this."""
    if os.environ.get("TATAJUBA_AMD_HIP_RUNTIME", "") == "system":
        return
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        build_library()
    _share_hip_runtime_with_torch()
    L = C.CDLL(path)
    P = C.POINTER(_HopoCounterStruct)
    L.new_hopo_counter.restype = P; L.new_hopo_counter.argtypes = [C.c_int]
    L.del_hopo_counter.restype = None; L.del_hopo_counter.argtypes = [P]
    L.new_or_append_hopo_counter_from_file.restype = P
    L.new_or_append_hopo_counter_from_file.argtypes = [P, C.c_char_p, Options]
    L.update_hopo_counter_from_seq.restype = None
    L.update_hopo_counter_from_seq.argtypes = [P, C.c_char_p, C.c_int, C.c_int]
    L.update_hopo_counter_from_seq_all_monomers.restype = None
    L.update_hopo_counter_from_seq_all_monomers.argtypes = [P, C.c_char_p, C.c_int]
    L.finalise_hopo_counter.restype = None; L.finalise_hopo_counter.argtypes = [P]
    L.generate_name_from_flanking_contexts.restype = C.c_void_p
    L.generate_name_from_flanking_contexts.argtypes = [C.POINTER(C.c_uint64), C.c_int8, C.c_int, C.c_bool]
    L.generate_tract_as_string.restype = C.c_void_p
    L.generate_tract_as_string.argtypes = [C.POINTER(C.c_uint64), C.c_int8, C.c_int, C.c_int, C.c_bool]
    L.compare_hopo_element_decreasing.restype = C.c_int
    L.compare_hopo_element_decreasing.argtypes = [C.c_void_p, C.c_void_p]

    L.tjamd_device_count.restype = C.c_int
    L.tjamd_last_error.restype = C.c_char_p
    L.tjamd_version.restype = C.c_char_p
    L.tjamd_counter_create.restype = C.c_void_p; L.tjamd_counter_create.argtypes = [C.c_int, C.c_int]
    L.tjamd_counter_destroy.restype = None; L.tjamd_counter_destroy.argtypes = [C.c_void_p]
    L.tjamd_counter_reset.argtypes = [C.c_void_p]
    L.tjamd_counter_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.tjamd_counter_device.argtypes = [C.c_void_p]
    L.tjamd_scan_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.tjamd_scan_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.tjamd_scan_host_located.restype = C.c_long
    L.tjamd_scan_host_located.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_long]
    L.tjamd_host_alloc.restype = C.c_void_p; L.tjamd_host_alloc.argtypes = [C.c_size_t]
    L.tjamd_host_free.restype = None; L.tjamd_host_free.argtypes = [C.c_void_p]
    L.tjamd_sync.argtypes = [C.c_void_p]
    L.tjamd_raw_count.restype = C.c_long; L.tjamd_raw_count.argtypes = [C.c_void_p]
    L.tjamd_download_raw.restype = C.c_long; L.tjamd_download_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_undefined_runs.restype = C.c_long; L.tjamd_undefined_runs.argtypes = [C.c_void_p]
    L.tjamd_upload_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_finalise.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.tjamd_finalise_begin.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.tjamd_finalise_end.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.tjamd_kept_count.restype = C.c_long; L.tjamd_kept_count.argtypes = [C.c_void_p]
    L.tjamd_n_idx.argtypes = [C.c_void_p]
    L.tjamd_coverage.argtypes = [C.c_void_p]
    L.tjamd_download_kept.restype = C.c_long; L.tjamd_download_kept.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_download_idx.restype = C.c_long
    L.tjamd_download_idx.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_kept_device_ptr.restype = C.c_void_p; L.tjamd_kept_device_ptr.argtypes = [C.c_void_p]
    L.tjamd_merge_samples.restype = C.c_long
    L.tjamd_merge_samples.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_long), C.c_int, C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_gather_histograms.restype = C.c_long
    L.tjamd_gather_histograms.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_long)]
    L.tjamd_tract_ids.restype = C.c_long; L.tjamd_tract_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    L.tjamd_tract_stats.restype = C.c_long
    L.tjamd_tract_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.tjamd_tract_sample_stats.restype = C.c_long
    L.tjamd_tract_sample_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_long,
                                           C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tjamd_last_tract_stats_ms.restype = C.c_double; L.tjamd_last_tract_stats_ms.argtypes = [C.c_void_p]
    L.tjamd_union_tracts.restype = C.c_long
    L.tjamd_union_tracts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_union_tract_stats.restype = C.c_long
    L.tjamd_union_tract_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_int), C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.POINTER(C.c_long), C.c_void_p, C.POINTER(C.c_long)]
    L.tjamd_union_tract_sample_stats.restype = C.c_long
    L.tjamd_union_tract_sample_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_long,
                                                 C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tjamd_last_union_tracts_ms.restype = C.c_double; L.tjamd_last_union_tracts_ms.argtypes = [C.c_void_p]
    L.tjamd_last_union_tract_stats_ms.restype = C.c_double; L.tjamd_last_union_tract_stats_ms.argtypes = [C.c_void_p]
    L.tjamd_last_union_tract_candidates.restype = C.c_long; L.tjamd_last_union_tract_candidates.argtypes = [C.c_void_p]
    L.tjamd_reference_create.restype = C.c_void_p; L.tjamd_reference_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.tjamd_reference_destroy.restype = None; L.tjamd_reference_destroy.argtypes = [C.c_void_p]
    L.tjamd_reference_entries.restype = C.c_long; L.tjamd_reference_entries.argtypes = [C.c_void_p]
    L.tjamd_reference_contigs.restype = C.c_long; L.tjamd_reference_contigs.argtypes = [C.c_void_p]
    L.tjamd_reference_download.restype = C.c_long; L.tjamd_reference_download.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_locate.restype = C.c_long; L.tjamd_locate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p]
    L.tjamd_located_tracts.restype = C.c_long
    L.tjamd_located_tracts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_last_reference_ms.restype = C.c_double; L.tjamd_last_reference_ms.argtypes = [C.c_void_p]
    L.tjamd_last_locate_ms.restype = C.c_double; L.tjamd_last_locate_ms.argtypes = [C.c_void_p]
    L.tjamd_last_located_tracts_ms.restype = C.c_double; L.tjamd_last_located_tracts_ms.argtypes = [C.c_void_p]
    L.tjamd_flank_edit_distance.restype = C.c_int; L.tjamd_flank_edit_distance.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int]
    L.tjamd_reference_add_seeds.restype = C.c_long; L.tjamd_reference_add_seeds.argtypes = [C.c_void_p, C.c_void_p]
    L.tjamd_reference_has_seeds.restype = C.c_int; L.tjamd_reference_has_seeds.argtypes = [C.c_void_p]
    L.tjamd_locate_gapped.restype = C.c_long
    L.tjamd_locate_gapped.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.tjamd_last_seed_order_ms.restype = C.c_double; L.tjamd_last_seed_order_ms.argtypes = [C.c_void_p]
    L.tjamd_last_locate_gapped_ms.restype = C.c_double; L.tjamd_last_locate_gapped_ms.argtypes = [C.c_void_p]
    L.tjamd_tract_variants.restype = C.c_long
    L.tjamd_tract_variants.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_void_p,
                                       C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p]
    L.tjamd_last_tract_variants_ms.restype = C.c_double; L.tjamd_last_tract_variants_ms.argtypes = [C.c_void_p]
    L.tjamd_read_file_names.restype = C.c_long
    L.tjamd_read_file_names.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.tjamd_gff3_read.restype = C.c_long
    L.tjamd_gff3_read.argtypes = [C.c_char_p, C.c_char_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.tjamd_annotation_create.restype = C.c_void_p; L.tjamd_annotation_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_annotation_destroy.restype = None; L.tjamd_annotation_destroy.argtypes = [C.c_void_p]
    L.tjamd_annotation_features.restype = C.c_long; L.tjamd_annotation_features.argtypes = [C.c_void_p]
    L.tjamd_annotation_download.restype = C.c_long; L.tjamd_annotation_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_tract_features.restype = C.c_long
    L.tjamd_tract_features.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    L.tjamd_last_annotation_ms.restype = C.c_double; L.tjamd_last_annotation_ms.argtypes = [C.c_void_p]
    L.tjamd_last_tract_features_ms.restype = C.c_double; L.tjamd_last_tract_features_ms.argtypes = [C.c_void_p]
    L.tjamd_translate.restype = C.c_long; L.tjamd_translate.argtypes = [C.c_char_p, C.c_long, C.c_int, C.c_void_p, C.c_long]
    L.tjamd_gff3_read_phase.restype = C.c_long; L.tjamd_gff3_read_phase.argtypes = [C.c_char_p, C.c_char_p, C.c_long, C.c_void_p, C.c_long]
    L.tjamd_coding_create.restype = C.c_void_p; L.tjamd_coding_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_long, C.c_void_p]
    L.tjamd_coding_destroy.restype = None; L.tjamd_coding_destroy.argtypes = [C.c_void_p]
    L.tjamd_coding_features.restype = C.c_long; L.tjamd_coding_features.argtypes = [C.c_void_p]
    L.tjamd_coding_download.restype = C.c_long; L.tjamd_coding_download.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.tjamd_variant_effects.restype = C.c_long
    L.tjamd_variant_effects.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p]
    L.tjamd_last_coding_ms.restype = C.c_double; L.tjamd_last_coding_ms.argtypes = [C.c_void_p]
    L.tjamd_last_variant_effects_ms.restype = C.c_double; L.tjamd_last_variant_effects_ms.argtypes = [C.c_void_p]
    L.tjamd_merge_variants.restype = C.c_long
    L.tjamd_merge_variants.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tjamd_site_ref_alt.restype = C.c_int; L.tjamd_site_ref_alt.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.tjamd_last_merge_variants_ms.restype = C.c_double; L.tjamd_last_merge_variants_ms.argtypes = [C.c_void_p]
    L.tjamd_site_depths.restype = C.c_long
    L.tjamd_site_depths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_void_p,
                                    C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tjamd_last_site_depths_ms.restype = C.c_double; L.tjamd_last_site_depths_ms.argtypes = [C.c_void_p]
    L.tjamd_sample_distances.restype = C.c_long
    L.tjamd_sample_distances.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    L.tjamd_last_sample_distances_ms.restype = C.c_double; L.tjamd_last_sample_distances_ms.argtypes = [C.c_void_p]
    L.tjamd_sample_linkage.restype = C.c_long
    L.tjamd_sample_linkage.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.tjamd_linkage_clusters.restype = C.c_long
    L.tjamd_linkage_clusters.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_longlong, C.c_void_p]
    L.tjamd_last_sample_linkage_ms.restype = C.c_double; L.tjamd_last_sample_linkage_ms.argtypes = [C.c_void_p]
    L.tjamd_last_linkage_clusters_ms.restype = C.c_double; L.tjamd_last_linkage_clusters_ms.argtypes = [C.c_void_p]
    L.tjamd_sample_agglomerate.restype = C.c_long
    L.tjamd_sample_agglomerate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    L.tjamd_last_sample_agglomerate_ms.restype = C.c_double; L.tjamd_last_sample_agglomerate_ms.argtypes = [C.c_void_p]
    L.tjamd_group_sites.restype = C.c_long
    L.tjamd_group_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long,
                                    C.POINTER(C.c_long)]
    L.tjamd_last_group_sites_ms.restype = C.c_double; L.tjamd_last_group_sites_ms.argtypes = [C.c_void_p]
    L.tjamd_linkage_tree.restype = C.c_long
    L.tjamd_linkage_tree.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p]
    L.tjamd_clade_sites.restype = C.c_long
    L.tjamd_clade_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_long, C.POINTER(C.c_long)]
    L.tjamd_last_linkage_tree_ms.restype = C.c_double; L.tjamd_last_linkage_tree_ms.argtypes = [C.c_void_p]
    L.tjamd_last_clade_sites_ms.restype = C.c_double; L.tjamd_last_clade_sites_ms.argtypes = [C.c_void_p]
    L.tjamd_bootstrap_weights.restype = C.c_long
    L.tjamd_bootstrap_weights.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_ulonglong, C.c_void_p]
    L.tjamd_sample_distances_weighted.restype = C.c_long
    L.tjamd_sample_distances_weighted.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.tjamd_clade_support.restype = C.c_long
    L.tjamd_clade_support.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_void_p]
    L.tjamd_last_bootstrap_weights_ms.restype = C.c_double; L.tjamd_last_bootstrap_weights_ms.argtypes = [C.c_void_p]
    L.tjamd_last_sample_distances_weighted_ms.restype = C.c_double; L.tjamd_last_sample_distances_weighted_ms.argtypes = [C.c_void_p]
    L.tjamd_last_clade_support_ms.restype = C.c_double; L.tjamd_last_clade_support_ms.argtypes = [C.c_void_p]
    L.tjamd_replicate_trees.restype = C.c_long
    L.tjamd_replicate_trees.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.tjamd_last_replicate_trees_ms.restype = C.c_double; L.tjamd_last_replicate_trees_ms.argtypes = [C.c_void_p]
    L.tjamd_consensus_tree.restype = C.c_long
    L.tjamd_consensus_tree.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_long)]
    L.tjamd_last_consensus_tree_ms.restype = C.c_double; L.tjamd_last_consensus_tree_ms.argtypes = [C.c_void_p]
    L.tjamd_group_contexts.restype = C.c_long
    L.tjamd_group_contexts.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
    L.new_genomic_context_list.restype = C.POINTER(GenomicContextListStruct); L.new_genomic_context_list.argtypes = [P]
    L.del_genomic_context_list.restype = None; L.del_genomic_context_list.argtypes = [C.POINTER(GenomicContextListStruct)]
    L.tjamd_comm_unique_id.argtypes = [C.c_void_p]
    L.tjamd_comm_create.restype = C.c_void_p; L.tjamd_comm_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.tjamd_comm_destroy.restype = None; L.tjamd_comm_destroy.argtypes = [C.c_void_p]
    L.tjamd_comm_rank.argtypes = [C.c_void_p]; L.tjamd_comm_world.argtypes = [C.c_void_p]
    L.tjamd_comm_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.tjamd_comm_collectives.restype = C.c_long; L.tjamd_comm_collectives.argtypes = [C.c_void_p]
    L.tjamd_allgather_histograms.restype = C.c_long
    L.tjamd_allgather_histograms.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_long)]
    L.tjamd_peer_access_report.argtypes = [C.c_char_p, C.c_int]
    L.tjamd_context_histograms.restype = C.c_long
    L.tjamd_context_histograms.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    # (without these ctypes truncates the 64-bit device pointer to a C int)
    L.tjamd_device_alloc.restype = C.c_void_p; L.tjamd_device_alloc.argtypes = [C.c_void_p, C.c_size_t]
    L.tjamd_device_free.restype = None; L.tjamd_device_free.argtypes = [C.c_void_p, C.c_void_p]
    L.tjamd_device_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.tjamd_scan_windows.restype = C.c_long
    L.tjamd_scan_windows.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
    U64P = C.POINTER(C.c_uint64)
    L.distance_between_single_context_kmer.argtypes = [U64P, U64P, C.c_int]
    L.distance_between_context_kmer_pair.argtypes = [U64P, U64P]
    L.distance_between_context_kmer_pair_with_edit_shift.argtypes = [U64P, U64P, C.POINTER(C.c_int)]
    L.leftmost_hopo_name_and_length_from_string.restype = C.c_void_p
    L.leftmost_hopo_name_and_length_from_string.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.hopo_counter_histogram_integral.argtypes = [P, C.c_int]
    L.tjamd_last_scan_ms.restype = C.c_double; L.tjamd_last_scan_ms.argtypes = [C.c_void_p]
    L.tjamd_last_finalise_ms.restype = C.c_double; L.tjamd_last_finalise_ms.argtypes = [C.c_void_p]
    L.tjamd_last_partition_ms.restype = C.c_double; L.tjamd_last_partition_ms.argtypes = [C.c_void_p]
    L.tjamd_last_scan_launches.restype = C.c_long; L.tjamd_last_scan_launches.argtypes = [C.c_void_p]
    L.tjamd_synth_stream.restype = C.c_long
    L.tjamd_synth_stream.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_long, C.c_long, C.c_int, C.c_int,
                                     C.c_void_p, C.c_long, C.c_int]
    L.tjamd_read_file_stream.restype = C.c_long
    L.tjamd_read_file_stream.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.tjamd_fastq_begin.restype = C.c_int; L.tjamd_fastq_begin.argtypes = [C.c_void_p, C.c_int]
    L.tjamd_fastq_push_device.restype = C.c_int; L.tjamd_fastq_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.tjamd_fastq_push_host.restype = C.c_int; L.tjamd_fastq_push_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.tjamd_fastq_end.restype = C.c_long; L.tjamd_fastq_end.argtypes = [C.c_void_p]
    L.tjamd_fastq_reads.restype = C.c_long; L.tjamd_fastq_reads.argtypes = [C.c_void_p]
    L.tjamd_fastq_stop.restype = C.c_int; L.tjamd_fastq_stop.argtypes = [C.c_void_p]
    L.tjamd_fastq_stream.restype = C.c_void_p; L.tjamd_fastq_stream.argtypes = [C.c_void_p]
    L.tjamd_fastq_stream_bytes.restype = C.c_long; L.tjamd_fastq_stream_bytes.argtypes = [C.c_void_p]
    L.tjamd_fastq_tile_bytes.restype = C.c_int; L.tjamd_fastq_tile_bytes.argtypes = []
    L.tjamd_last_fastq_ms.restype = C.c_double; L.tjamd_last_fastq_ms.argtypes = [C.c_void_p]
    _LIB = L
    return L


def _err():
    return (lib().tjamd_last_error() or b"").decode(errors="replace")


def device_count():
    return lib().tjamd_device_count()


def synth_stream(n_reads, read_len, genome_len, seed_genome=0x7A7A0001, seed_reads=0x7A7A1000, variant_seed=0,
                 read_len_max=0, n_threads=8, out=None):
    """Synthetic '\\n'-delimited read stream as a numpy uint8 array (host memory)."""
    need = -lib().tjamd_synth_stream(seed_genome, seed_reads, variant_seed, genome_len, n_reads, read_len, read_len_max,
                                     None, 0, n_threads)
    if need <= 0:
        raise TatajubaAmdError("bad synthetic-stream parameters")
    if out is None:
        out = np.empty(need, dtype=np.uint8)
    assert out.dtype == np.uint8 and out.size >= need and out.flags["C_CONTIGUOUS"]
    got = lib().tjamd_synth_stream(seed_genome, seed_reads, variant_seed, genome_len, n_reads, read_len, read_len_max,
                                   out.ctypes.data, out.size, n_threads)
    if got != need:
        raise TatajubaAmdError("synthetic stream generation failed")
    return out[:need]


def read_file_stream_mt(path, n_threads=4, window_bytes=0):
    """read_file_stream through the multi-threaded feeder (plain files; host-only)."""
    L = lib()
    L.tjamd_read_file_stream_mt.restype = C.c_long
    L.tjamd_read_file_stream_mt.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.c_int, C.c_long]
    n = C.c_long(0)
    need = L.tjamd_read_file_stream_mt(os.fsencode(path), None, 0, C.byref(n), n_threads, window_bytes)
    if need < 0:
        raise FileNotFoundError(path)
    out = np.empty(max(need, 1), dtype=np.uint8)
    got = L.tjamd_read_file_stream_mt(os.fsencode(path), out.ctypes.data, need, C.byref(n), n_threads, window_bytes)
    assert got == need
    return out[:need], n.value


def read_file_stream(path):
    """Parse a FASTA/FASTQ(.gz) file with the product's host reader -> (uint8 stream, n_reads).  Host-only."""
    n = C.c_long(0)
    need = lib().tjamd_read_file_stream(os.fsencode(path), None, 0, C.byref(n))
    if need < 0:
        raise FileNotFoundError(path)
    out = np.empty(max(need, 1), dtype=np.uint8)
    got = lib().tjamd_read_file_stream(os.fsencode(path), out.ctypes.data, need, C.byref(n))
    assert got == need
    return out[:need], n.value


def read_gff3(path, names):
    """The feature lines of a GFF3 file (plain, gzip, BGZF) -> (FEATURE_DTYPE array, the strings its type_off / id_off point
    into, as bytes).  names: the contig names in the reference's order (what tjamd_read_file_names gives).  Host-only.
    The lines that were skipped are counted in read_gff3.last_skipped."""
    blob = b"".join((n if isinstance(n, bytes) else str(n).encode()) + b"\n" for n in names)
    nb, sk = C.c_long(0), C.c_long(0)
    n = lib().tjamd_gff3_read(os.fsencode(path), blob, len(names), None, 0, None, 0, C.byref(nb), C.byref(sk))
    if n < 0:
        raise FileNotFoundError(path)
    out = np.zeros(n, dtype=FEATURE_DTYPE)
    strings = np.zeros(max(nb.value, 1), dtype=np.uint8)
    got = lib().tjamd_gff3_read(os.fsencode(path), blob, len(names), out.ctypes.data, n, strings.ctypes.data, nb.value, C.byref(nb), C.byref(sk))
    assert got == n
    read_gff3.last_skipped = sk.value
    return out, strings[: nb.value].tobytes()


def read_gff3_phase(path, names):
    """Column 8 of the feature lines read_gff3 keeps, in its order -> int8 array (0, 1, 2; -1 for '.' or anything else).
    Host-only."""
    blob = b"".join((n if isinstance(n, bytes) else str(n).encode()) + b"\n" for n in names)
    n = lib().tjamd_gff3_read_phase(os.fsencode(path), blob, len(names), None, 0)
    if n < 0:
        raise FileNotFoundError(path)
    out = np.zeros(n, dtype=np.int8)
    got = lib().tjamd_gff3_read_phase(os.fsencode(path), blob, len(names), out.ctypes.data if n else None, n)
    assert got == n
    return out


def translate(dna, reverse=False):
    """tjamd_translate: the amino acids of a DNA string's whole codons (of its reverse complement with reverse), no stop
    handling -> str.  Host-only."""
    b = dna if isinstance(dna, bytes) else str(dna).encode()
    out = np.zeros(max(len(b) // 3, 1), dtype=np.uint8)
    n = lib().tjamd_translate(b, len(b), 1 if reverse else 0, out.ctypes.data, len(b) // 3)
    if n < 0:
        raise TatajubaAmdError(_err())
    return out[:n].tobytes().decode()


def site_ref_alt(site, allele, k):
    """the text of a SITE_DTYPE record's REF (allele None) or of one of its ALLELE_DTYPE records' ALT (host only)"""
    sb = np.asarray(site, SITE_DTYPE).reshape(1).tobytes()
    ab = None if allele is None else np.asarray(allele, ALLELE_DTYPE).reshape(1).tobytes()
    n = lib().tjamd_site_ref_alt(sb, ab, k, None, 0)
    if n < 0:
        raise TatajubaAmdError("tjamd_site_ref_alt: a site or allele that has no text")
    out = C.create_string_buffer(n + 1)
    assert lib().tjamd_site_ref_alt(sb, ab, k, out, n + 1) == n
    return out.value.decode()


def gff3_string(strings, off):
    """the NUL-terminated string at an offset of read_gff3's strings"""
    return strings[off: strings.index(b"\0", off)].decode(errors="replace")


class EmpfreqElement(C.Structure):
    _fields_ = [("freq", C.c_int), ("idx", C.c_int)]


class EmpfreqStruct(C.Structure):
    _fields_ = [("i", C.POINTER(EmpfreqElement)), ("n", C.c_int), ("min", C.c_int), ("max", C.c_int)]


class ContextHistogramStruct(C.Structure):
    """struct context_histogram_struct (include/tatajuba_context.h; reference src/context_histogram.h:18-43 without gffeature)"""
    _fields_ = [("context", C.POINTER(C.c_uint64)),
                ("base", C.c_int32, 2), ("multi", C.c_int32, 3), ("indel", C.c_int32, 2), ("neg_strand", C.c_int32, 1), ("mismatches", C.c_int32, 12),
                ("name", C.c_char_p), ("n_context", C.c_int), ("integral", C.c_int), ("location", C.c_int), ("loc2d", C.c_int * 3),
                ("coverage", C.c_int), ("n_tracts", C.c_int), ("mode_context_count", C.c_int), ("mode_context_length", C.c_int),
                ("mode_context_id", C.c_int), ("tmp_count", C.POINTER(C.c_int)), ("tmp_length", C.POINTER(C.c_int)), ("index", C.c_int),
                ("h", C.POINTER(EmpfreqStruct)), ("tract_id", C.c_int), ("ref_counter", C.c_int)]


class GenomicContextListStruct(C.Structure):
    _fields_ = [("hist", C.POINTER(C.POINTER(ContextHistogramStruct))), ("name", C.c_char_p), ("opt", Options),
                ("n_hist", C.c_int), ("coverage", C.c_int), ("ref_start", C.c_int)]


class Comm:
    """tjamd_comm: the process-per-GPU exchange of the C library (ncclAllGather over RCCL behind tjamd_allgather_histograms)."""

    ID_BYTES = 128

    @staticmethod
    def unique_id():
        """rank 0: the bytes every rank passes to Comm(...) (hand them over with whatever the job has: MPI, a file, a store)"""
        buf = C.create_string_buffer(Comm.ID_BYTES)
        if lib().tjamd_comm_unique_id(buf) != 0:
            raise TatajubaAmdError(_err())
        return buf.raw

    def __init__(self, counter, ident, rank, world):
        self.world = world
        self._id = C.create_string_buffer(bytes(ident), Comm.ID_BYTES)
        self._h = lib().tjamd_comm_create(counter._h, self._id, rank, world)
        if not self._h:
            raise TatajubaAmdError(_err())

    def set_stream(self, hip_stream):
        if lib().tjamd_comm_set_stream(self._h, C.c_void_p(hip_stream)) != 0:
            raise TatajubaAmdError(_err())

    def allgather(self, counter):
        """(device pointer of all ranks' kept records back to back, ctypes long array of records per rank, total)"""
        ptr, cnt = C.c_void_p(), (C.c_long * self.world)()
        tot = lib().tjamd_allgather_histograms(counter._h, self._h, C.byref(ptr), cnt)
        if tot < 0:
            raise TatajubaAmdError(_err())
        return ptr, cnt, tot

    @property
    def collectives(self):
        return lib().tjamd_comm_collectives(self._h)

    @property
    def count(self):
        """ranks RCCL reports for the communicator (ncclCommCount)"""
        lib().tjamd_comm_count.restype = C.c_int
        lib().tjamd_comm_count.argtypes = [C.c_void_p]
        return int(lib().tjamd_comm_count(self._h))

    def last_exchange(self):
        """(device ms, bytes delivered to this rank, collectives) of the last allgather; None before the first"""
        f = lib().tjamd_comm_last_exchange
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_long)]
        ms, nb, nc = C.c_double(), C.c_long(), C.c_long()
        if f(self._h, C.byref(ms), C.byref(nb), C.byref(nc)) != 0:
            return None
        return ms.value, nb.value, nc.value

    def close(self):
        if getattr(self, "_h", None):
            lib().tjamd_comm_destroy(self._h)
            self._h = None

    __del__ = close


def flank_edit_distance(a, b, k, side, max_shift):
    """tjamd_flank_edit_distance: the banded edit distance of two packed flanks, anchored at the tract (host arithmetic)"""
    d = lib().tjamd_flank_edit_distance(int(a), int(b), k, side, max_shift)
    if d < 0:
        raise TatajubaAmdError(_err())
    return int(d)


class Reference:
    """tjamd_reference: the index of a genome's runs (contigs as a stream of reads, each followed by a newline), built on
    the counter's device with the counter's k"""

    def __init__(self, counter, stream):
        buf = np.frombuffer(bytes(stream), dtype=np.uint8)
        self._h = lib().tjamd_reference_create(counter._h, buf.ctypes.data if len(buf) else None, len(buf))
        if not self._h:
            raise TatajubaAmdError(_err())

    def add_seeds(self, counter):
        """tjamd_reference_add_seeds: the seed order tjamd_locate_gapped needs (built once); -> number of entries"""
        n = lib().tjamd_reference_add_seeds(counter._h, self._h)
        if n < 0:
            raise TatajubaAmdError(_err())
        return int(n)

    @property
    def has_seeds(self):
        return bool(lib().tjamd_reference_has_seeds(self._h))

    @property
    def n_entries(self):
        return int(lib().tjamd_reference_entries(self._h))

    @property
    def n_contigs(self):
        return int(lib().tjamd_reference_contigs(self._h))

    def download(self):
        out = np.zeros(self.n_entries, dtype=REF_ENTRY_DTYPE)
        n = lib().tjamd_reference_download(self._h, out.ctypes.data if len(out) else None, len(out))
        if n < 0:
            raise TatajubaAmdError(_err())
        return out[:n]

    def close(self):
        if self._h:
            lib().tjamd_reference_destroy(self._h)
            self._h = None

    __del__ = close


class Annotation:
    """tjamd_annotation: the features of a GFF3 file (a FEATURE_DTYPE array, as read_gff3 gives it) as an elementary-interval
    table on the counter's device; ref gives the number of contigs"""

    def __init__(self, counter, ref, features):
        f = np.ascontiguousarray(features, dtype=FEATURE_DTYPE)
        self._h = lib().tjamd_annotation_create(counter._h, ref._h, f.ctypes.data if len(f) else None, len(f))
        if not self._h:
            raise TatajubaAmdError(_err())

    @property
    def n_features(self):
        return int(lib().tjamd_annotation_features(self._h))

    def download(self):
        """(points, winner): the sorted points and, per index, the file index of the winning feature or -1"""
        n = lib().tjamd_annotation_download(self._h, None, None, 0)
        if n < 0:
            raise TatajubaAmdError(_err())
        points, winner = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int32)
        if n and lib().tjamd_annotation_download(self._h, points.ctypes.data, winner.ctypes.data, n) != n:
            raise TatajubaAmdError(_err())
        return points, winner

    def close(self):
        if getattr(self, "_h", None):
            lib().tjamd_annotation_destroy(self._h)
            self._h = None

    __del__ = close


class Coding:
    """tjamd_coding: the genome's bases (the stream a Reference was built from) and the coding features of a GFF3 file (a
    FEATURE_DTYPE array, with the phases read_gff3_phase gives, or None) as a table on the counter's device"""

    def __init__(self, counter, stream, features, phase=None):
        buf = np.frombuffer(bytes(stream), dtype=np.uint8)
        f = np.ascontiguousarray(features, dtype=FEATURE_DTYPE)
        ph = None if phase is None else np.ascontiguousarray(phase, dtype=np.int8)
        assert ph is None or len(ph) == len(f)
        self._h = lib().tjamd_coding_create(counter._h, buf.ctypes.data if len(buf) else None, len(buf), f.ctypes.data if len(f) else None, len(f),
                                            ph.ctypes.data if ph is not None and len(ph) else None)
        if not self._h:
            raise TatajubaAmdError(_err())

    @property
    def n_features(self):
        return int(lib().tjamd_coding_features(self._h))

    def download(self):
        """a CDS_DTYPE record per feature: -1 everywhere for a feature that is not coding"""
        out = np.zeros(self.n_features, dtype=CDS_DTYPE)
        n = lib().tjamd_coding_download(self._h, out.ctypes.data if len(out) else None, len(out))
        if n < 0:
            raise TatajubaAmdError(_err())
        return out[:n]

    def close(self):
        if getattr(self, "_h", None):
            lib().tjamd_coding_destroy(self._h)
            self._h = None

    __del__ = close


class Counter:
    """tjamd_counter: device-side per-sample accumulator (include/tatajuba_amd.h)."""

    def __init__(self, kmer_size, device=0):
        self.k = kmer_size
        self._h = lib().tjamd_counter_create(device, kmer_size)
        if not self._h:
            raise TatajubaAmdError(_err())

    def close(self):
        if getattr(self, "_h", None):
            lib().tjamd_counter_destroy(self._h)
            self._h = None

    __del__ = close

    def _chk(self, rc):
        if rc != 0:
            raise TatajubaAmdError(_err())

    def _chkn(self, n):
        if n < 0:
            raise TatajubaAmdError(_err())
        return n

    def reset(self):
        self._chk(lib().tjamd_counter_reset(self._h))

    def set_stream(self, hip_stream):
        self._chk(lib().tjamd_counter_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_order_stream(self, hip_stream):
        """second stream for the ordering step of finalise_begin / finalise_end (tjamd_counter_set_order_stream); None: none"""
        lib().tjamd_counter_set_order_stream.argtypes = [C.c_void_p, C.c_void_p]
        self._chk(lib().tjamd_counter_set_order_stream(self._h, C.c_void_p(hip_stream) if hip_stream else None))

    def sync(self):
        self._chk(lib().tjamd_sync(self._h))

    def scan_device(self, dptr, n_bytes, m):
        self._chk(lib().tjamd_scan_device(self._h, C.c_void_p(dptr), n_bytes, m))

    def scan_host(self, buf, m):
        a = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf)
        self._chk(lib().tjamd_scan_host(self._h, a.ctypes.data, a.size, m))
        self.sync()           # `a` may be a temporary

    def scan_host_located(self, buf, m):
        a = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf)
        cap = a.size // 2 + 2
        out = np.zeros(cap, dtype=LOCATED_DTYPE)
        n = self._chkn(lib().tjamd_scan_host_located(self._h, a.ctypes.data, a.size, m, out.ctypes.data, cap))
        return out[:n]

    # FASTQ text parsed on the device (tjamd_fastq_*, include/tatajuba_amd.h): a session is begin, pushes, end
    def fastq_begin(self, m=-1):
        """m >= 1: every push's stream is scanned as scan_device would; -1: parse only, the stream is kept"""
        self._chk(lib().tjamd_fastq_begin(self._h, m))

    def fastq_push_host(self, buf, final=False):
        a = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf)
        self._chk(lib().tjamd_fastq_push_host(self._h, a.ctypes.data if a.size else None, a.size, int(final)))

    def fastq_push_device(self, dptr, n_bytes, final=False):
        """dptr: 16-byte aligned device memory that stays as it is until fastq_end"""
        self._chk(lib().tjamd_fastq_push_device(self._h, C.c_void_p(dptr) if n_bytes else None, n_bytes, int(final)))

    def fastq_end(self):
        """waits; (bytes of text consumed, records, stop code, bytes of stream)"""
        consumed = self._chkn(lib().tjamd_fastq_end(self._h))
        return consumed, lib().tjamd_fastq_reads(self._h), lib().tjamd_fastq_stop(self._h), lib().tjamd_fastq_stream_bytes(self._h)

    def fastq_stream(self):
        """the stream of the last parse-only session, downloaded (bytes)"""
        n, p = lib().tjamd_fastq_stream_bytes(self._h), lib().tjamd_fastq_stream(self._h)
        out = np.zeros(max(n, 0), np.uint8)
        if n > 0:
            if not p:
                raise TatajubaAmdError("the last session kept no stream (it scanned)")
            self._chk(lib().tjamd_device_download(self._h, out.ctypes.data, C.c_void_p(p), n))
        return out.tobytes()

    def fastq_parse(self, text, cuts=()):
        """One parse-only session over text, pushed from host memory in the pieces that the ascending offsets `cuts` make
        of it, the last one final -> (consumed, reads, stop, stream bytes)."""
        text = bytes(text)
        edges = [0] + [int(x) for x in cuts] + [len(text)]
        self.fastq_begin(-1)
        for i in range(len(edges) - 1):
            self.fastq_push_host(text[edges[i]: edges[i + 1]], final=(i == len(edges) - 2))
        consumed, reads, stop, _ = self.fastq_end()
        return consumed, reads, stop, self.fastq_stream()

    def last_fastq_ms(self):
        return lib().tjamd_last_fastq_ms(self._h)

    def raw_count(self):
        return self._chkn(lib().tjamd_raw_count(self._h))

    def undefined_runs(self):
        return self._chkn(lib().tjamd_undefined_runs(self._h))

    def download_raw(self):
        n = self.raw_count()
        out = np.zeros(n, dtype=RECORD_DTYPE)
        self._chkn(lib().tjamd_download_raw(self._h, out.ctypes.data, n))
        return out

    def upload_raw(self, elems):
        e = np.ascontiguousarray(elems, dtype=ELEM_DTYPE)
        self._chk(lib().tjamd_upload_raw(self._h, e.ctypes.data, e.size))

    def finalise(self, remove_biased, min_coverage):
        st = C.c_int(-1)
        self._chk(lib().tjamd_finalise(self._h, int(bool(remove_biased)), int(min_coverage), C.byref(st)))
        return st.value

    def finalise_begin(self, remove_biased, min_coverage):
        """queue the device finalise and return; finalise_end() fetches the outcome (tjamd_finalise_begin / _end)"""
        self._chk(lib().tjamd_finalise_begin(self._h, int(bool(remove_biased)), int(min_coverage)))

    def finalise_end(self):
        st = C.c_int(-1)
        self._chk(lib().tjamd_finalise_end(self._h, C.byref(st)))
        return st.value

    @property
    def n_kept(self):
        return lib().tjamd_kept_count(self._h)

    @property
    def n_idx(self):
        return lib().tjamd_n_idx(self._h)

    @property
    def coverage(self):
        return lib().tjamd_coverage(self._h)

    @property
    def kept_device_ptr(self):
        return lib().tjamd_kept_device_ptr(self._h)

    def download_kept(self):
        n = self.n_kept
        out = np.zeros(n, dtype=ELEM_DTYPE)
        self._chkn(lib().tjamd_download_kept(self._h, out.ctypes.data, n))
        return out

    def download_idx(self):
        n = self.n_idx
        a, b = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._chkn(lib().tjamd_download_idx(self._h, a.ctypes.data, b.ctypes.data, n))
        return a, b

    def group_contexts(self, max_distance_per_flank):
        """(group_of int32[n_kept], groups structured array) -- tjamd_group_contexts"""
        n = self.n_kept
        gof = np.zeros(max(n, 1), dtype=np.int32)
        grp = np.zeros(max(n, 1), dtype=GROUP_DTYPE)
        ng = self._chkn(lib().tjamd_group_contexts(self._h, max_distance_per_flank, gof.ctypes.data, grp.ctypes.data, n))
        return gof[:n], grp[:ng]

    def context_histograms(self, max_distance_per_flank, levenshtein_distance):
        """tjamd_context_histograms: dict of group_of, join_type (int32[n_kept]), groups (CONTEXT_GROUP_DTYPE), hist
        (LENGTH_FREQ_DTYPE[n_kept]: histogram g's entries at [first, first + n_len))"""
        n = self.n_kept
        gof, jt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        grp = np.zeros(max(n, 1), dtype=CONTEXT_GROUP_DTYPE)
        hist = np.zeros(max(n, 1), dtype=LENGTH_FREQ_DTYPE)
        ng = self._chkn(lib().tjamd_context_histograms(self._h, max_distance_per_flank, levenshtein_distance, gof.ctypes.data, jt.ctypes.data,
                                                       grp.ctypes.data, hist.ctypes.data, n))
        return {"group_of": gof[:n], "join_type": jt[:n], "groups": grp[:ng], "hist": hist[:n]}

    def last_scan_launches(self):
        return int(lib().tjamd_last_scan_launches(self._h))

    def plan_mismatches(self):
        lib().tjamd_plan_mismatches.restype = C.c_long
        lib().tjamd_plan_mismatches.argtypes = [C.c_void_p]
        return int(lib().tjamd_plan_mismatches(self._h))

    def last_scan_ms(self):
        return lib().tjamd_last_scan_ms(self._h)

    def last_partition_ms(self):
        return lib().tjamd_last_partition_ms(self._h)

    def bucket_counts(self):
        """raw records per hash bucket (diagnostic: tjamd_debug_bucket_counts; synchronises)"""
        import numpy as np
        f = lib().tjamd_debug_bucket_counts
        f.restype = C.c_long
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        b = np.zeros(256, np.uint32)
        if f(self._h, b.ctypes.data, 256) < 0:
            raise TatajubaAmdError(_err())
        return b

    def last_merge_ms(self):
        lib().tjamd_last_merge_ms.restype = C.c_double
        lib().tjamd_last_merge_ms.argtypes = [C.c_void_p]
        return lib().tjamd_last_merge_ms(self._h)

    def last_tract_stats_ms(self):
        return lib().tjamd_last_tract_stats_ms(self._h)

    def last_union_tracts_ms(self):
        return lib().tjamd_last_union_tracts_ms(self._h)

    def last_union_tract_stats_ms(self):
        return lib().tjamd_last_union_tract_stats_ms(self._h)

    def last_union_tract_candidates(self):
        return int(lib().tjamd_last_union_tract_candidates(self._h))

    def last_reference_ms(self):
        return lib().tjamd_last_reference_ms(self._h)

    def last_locate_ms(self):
        return lib().tjamd_last_locate_ms(self._h)

    def last_located_tracts_ms(self):
        return lib().tjamd_last_located_tracts_ms(self._h)

    def locate_gapped(self, ref, d_keys, n, max_edits, max_shift, d_loc, d_how=None):
        """tjamd_locate_gapped on device pointers (ints): d_loc is in/out, d_how may be None; -> rows located by this call"""
        got = lib().tjamd_locate_gapped(self._h, ref._h, d_keys, n, max_edits, max_shift, d_loc, d_how)
        if got < 0:
            raise TatajubaAmdError(_err())
        return int(got)

    def last_seed_order_ms(self):
        return lib().tjamd_last_seed_order_ms(self._h)

    def last_locate_gapped_ms(self):
        return lib().tjamd_last_locate_gapped_ms(self._h)

    def last_tract_variants_ms(self):
        return lib().tjamd_last_tract_variants_ms(self._h)

    def last_annotation_ms(self):
        return lib().tjamd_last_annotation_ms(self._h)

    def last_tract_features_ms(self):
        return lib().tjamd_last_tract_features_ms(self._h)

    def variant_effects(self, coding, d_variants, n, d_out, d_tract_feat=None, n_tracts=0):
        """tjamd_variant_effects on device pointers: n VARIANT_DTYPE records -> n EFFECT_DTYPE records at d_out; d_tract_feat:
        the TRACT_FEATURE_DTYPE records of tjamd_tract_features (None: no record has a feature).  -> n"""
        return self._chkn(lib().tjamd_variant_effects(self._h, coding._h, d_variants, n, d_tract_feat, n_tracts, d_out))

    def last_coding_ms(self):
        return lib().tjamd_last_coding_ms(self._h)

    def last_variant_effects_ms(self):
        return lib().tjamd_last_variant_effects_ms(self._h)

    def merge_variants(self, kmer_size, d_records, n_records, n_samples, n_tracts, d_sites, site_capacity, d_alleles, allele_capacity,
                       d_genotype=None, d_allele_of=None, d_unique=None):
        """tjamd_merge_variants on device pointers: n_records VARIANT_DTYPE records -> SITE_DTYPE records at d_sites, ALLELE_DTYPE
        records at d_alleles; optionally int16 genotypes [site][sample], the allele of every input record (int32) and one
        VARIANT_DTYPE record per allele.  -> (number of sites, number of alleles)"""
        n_alleles = C.c_long(-1)
        n_sites = self._chkn(lib().tjamd_merge_variants(self._h, kmer_size, d_records, n_records, n_samples, n_tracts, d_sites, site_capacity,
                                                        d_alleles, allele_capacity, d_genotype, d_allele_of, d_unique, C.byref(n_alleles)))
        return n_sites, n_alleles.value

    def last_merge_variants_ms(self):
        return lib().tjamd_last_merge_variants_ms(self._h)

    def site_depths(self, ref, d_keys, d_counts, n_union, n_samples, d_tracts, n_tracts, d_tract_loc, d_sites, n_sites, d_alleles, n_alleles,
                    d_genotype=None, d_depth=None, d_allele_depth=None, d_summary=None):
        """tjamd_site_depths on device pointers: the permuted union and tiling tjamd_tract_variants was given and the sites and
        alleles of tjamd_merge_variants -> optionally int16 genotypes [site][sample] (0 = reference, -1 = not seen), int32 DP
        [site][sample], int32 AD [(n_sites + n_alleles)][sample] and one SITE_DEPTH_DTYPE record per site.  -> n_sites"""
        return self._chkn(lib().tjamd_site_depths(self._h, ref._h, d_keys, d_counts, n_union, n_samples, d_tracts, n_tracts, d_tract_loc,
                                                  d_sites, n_sites, d_alleles, n_alleles, d_genotype, d_depth, d_allele_depth, d_summary))

    def last_site_depths_ms(self):
        return lib().tjamd_last_site_depths_ms(self._h)

    def sample_distances(self, d_sites, n_sites, d_alleles, n_alleles, d_genotype, n_samples, d_out):
        """tjamd_sample_distances on device pointers: the sites and alleles of tjamd_merge_variants and an int16 genotype matrix
        [site][sample] (that of tjamd_site_depths, or of tjamd_merge_variants) -> one SAMPLE_DISTANCE_DTYPE record per pair of
        samples at d_out, [sample][sample], full and symmetric.  -> n_sites"""
        return self._chkn(lib().tjamd_sample_distances(self._h, d_sites, n_sites, d_alleles, n_alleles, d_genotype, n_samples, d_out))

    def last_sample_distances_ms(self):
        return lib().tjamd_last_sample_distances_ms(self._h)

    def sample_linkage(self, d_dist, n_samples, metric, min_both, d_links):
        """tjamd_sample_linkage on device pointers: the [sample][sample] matrix of tjamd_sample_distances -> the single-linkage
        tree of the samples under the metric (LINK_DIFFER, LINK_LENGTH, LINK_DIFFER_RATE) over the pairs with n_both >= min_both,
        one LINK_DTYPE record per merge at d_links, ascending in (key, a, b).  -> n_links"""
        return self._chkn(lib().tjamd_sample_linkage(self._h, d_dist, n_samples, metric, min_both, d_links))

    def linkage_clusters(self, d_links, n_links, n_samples, threshold, d_cluster):
        """tjamd_linkage_clusters on device pointers: the links with key <= threshold -> a dense cluster id per sample at
        d_cluster (int32), clusters numbered in the order of their smallest member.  -> n_clusters"""
        return self._chkn(lib().tjamd_linkage_clusters(self._h, d_links, n_links, n_samples, threshold, d_cluster))

    def last_sample_linkage_ms(self):
        return lib().tjamd_last_sample_linkage_ms(self._h)

    def last_linkage_clusters_ms(self):
        return lib().tjamd_last_linkage_clusters_ms(self._h)

    def sample_agglomerate(self, d_dist, n_samples, metric, min_both, linkage, d_links):
        """tjamd_sample_agglomerate on device pointers: the [sample][sample] matrix of tjamd_sample_distances -> the complete
        (AGGL_COMPLETE) or average (AGGL_AVERAGE) linkage tree of the samples under the metric over the pairs with n_both >=
        min_both, one LINK_DTYPE record per merge at d_links, ascending in (key, round, a, b).  -> (n_links, n_rounds)"""
        n_rounds = C.c_int(0)
        n = self._chkn(lib().tjamd_sample_agglomerate(self._h, d_dist, n_samples, metric, min_both, linkage, d_links, C.byref(n_rounds)))
        return n, n_rounds.value

    def last_sample_agglomerate_ms(self):
        return lib().tjamd_last_sample_agglomerate_ms(self._h)

    def group_sites(self, d_sites, n_sites, d_genotype, n_samples, d_group, n_groups, min_called, d_calls=None, d_site_out=None, d_group_marks=None,
                    d_marks=None, mark_capacity=0):
        """tjamd_group_sites on device pointers: the int16 genotypes [site][sample] of n_sites SITE_DTYPE records read by the
        group of every sample (int32 at d_group, -1: takes no part) -> optionally GROUP_CALL_DTYPE [site][group] at d_calls,
        GROUP_SITE_DTYPE [site] at d_site_out, int32 marks per group at d_group_marks and the marked (site, group) pairs as
        GROUP_MARK_DTYPE at d_marks.  -> the number of marks; more than mark_capacity raises, and .n_marks of the error is the
        number to size for"""
        n_marks = C.c_long(-1)
        rc = lib().tjamd_group_sites(self._h, d_sites, n_sites, d_genotype, n_samples, d_group, n_groups, min_called, d_calls, d_site_out, d_group_marks,
                                     d_marks, mark_capacity, C.byref(n_marks))
        if rc < 0:
            e = TatajubaAmdError(_err())
            e.n_marks = n_marks.value
            raise e
        return rc

    def last_group_sites_ms(self):
        return lib().tjamd_last_group_sites_ms(self._h)

    def linkage_tree(self, d_links, n_links, n_samples, d_nodes, d_order):
        """tjamd_linkage_tree on device pointers: n_links LINK_DTYPE records over n_samples samples -> one TREE_NODE_DTYPE per
        link at d_nodes (children, and the clade as an interval of the leaf order) and the leaf order (int32) at d_order.
        -> n_links"""
        return self._chkn(lib().tjamd_linkage_tree(self._h, d_links, n_links, n_samples, d_nodes, d_order))

    def clade_sites(self, d_sites, n_sites, d_genotype, n_samples, d_nodes, n_nodes, d_order, min_called, d_calls=None, d_site_out=None, d_node_marks=None,
                    d_marks=None, mark_capacity=0):
        """tjamd_clade_sites on device pointers: the int16 genotypes [site][sample] of n_sites SITE_DTYPE records read by the
        clade of every node (TREE_NODE_DTYPE at d_nodes: an interval of the leaf order at d_order) -> optionally
        GROUP_CALL_DTYPE [site][node] at d_calls, GROUP_SITE_DTYPE [site] at d_site_out, int32 marks per node at d_node_marks
        and the marked (site, node) pairs as GROUP_MARK_DTYPE at d_marks.  -> the number of marks; more than mark_capacity
        raises, and .n_marks of the error is the number to size for"""
        n_marks = C.c_long(-1)
        rc = lib().tjamd_clade_sites(self._h, d_sites, n_sites, d_genotype, n_samples, d_nodes, n_nodes, d_order, min_called, d_calls, d_site_out, d_node_marks,
                                     d_marks, mark_capacity, C.byref(n_marks))
        if rc < 0:
            e = TatajubaAmdError(_err())
            e.n_marks = n_marks.value
            raise e
        return rc

    def last_linkage_tree_ms(self):
        return lib().tjamd_last_linkage_tree_ms(self._h)

    def last_clade_sites_ms(self):
        return lib().tjamd_last_clade_sites_ms(self._h)

    def bootstrap_weights(self, n_sites, n_replicates, seed, d_weights):
        """tjamd_bootstrap_weights on a device pointer: n_replicates rows of n_sites int32 weights at d_weights, each the counts of
        n_sites draws with replacement under the rule of include/tatajuba_bootstrap.h.  -> n_replicates"""
        return self._chkn(lib().tjamd_bootstrap_weights(self._h, n_sites, n_replicates, seed & 0xFFFFFFFFFFFFFFFF, d_weights))

    def sample_distances_weighted(self, d_sites, n_sites, d_alleles, n_alleles, d_genotype, n_samples, d_out, d_weights, n_replicates):
        """tjamd_sample_distances_weighted on device pointers: the inputs of sample_distances and int32 weights
        [replicate][site] -> one [sample][sample] matrix of SAMPLE_DISTANCE_DTYPE per replicate at d_out.  -> n_sites"""
        return self._chkn(lib().tjamd_sample_distances_weighted(self._h, d_sites, n_sites, d_alleles, n_alleles, d_genotype, n_samples, d_out, d_weights, n_replicates))

    def clade_support(self, d_nodes, n_nodes, d_order, n_samples, d_rep_nodes, d_rep_order, rep_n_nodes, d_support):
        """tjamd_clade_support on device pointers: the tree (TREE_NODE_DTYPE at d_nodes over the leaf order at d_order) and, per
        replicate r, rep_n_nodes[r] nodes at d_rep_nodes[r * (n_samples - 1)] over the order at d_rep_order[r * n_samples]
        (rep_n_nodes: a host sequence, one count per replicate) -> int32 at d_support, per node the replicates that hold its
        clade.  -> n_nodes"""
        counts = (C.c_int * len(rep_n_nodes))(*[int(x) for x in rep_n_nodes])
        return self._chkn(lib().tjamd_clade_support(self._h, d_nodes, n_nodes, d_order, n_samples, d_rep_nodes, d_rep_order, counts, len(rep_n_nodes), d_support))

    def last_bootstrap_weights_ms(self):
        return lib().tjamd_last_bootstrap_weights_ms(self._h)

    def last_sample_distances_weighted_ms(self):
        return lib().tjamd_last_sample_distances_weighted_ms(self._h)

    def last_clade_support_ms(self):
        return lib().tjamd_last_clade_support_ms(self._h)

    def replicate_trees(self, d_dist, n_samples, n_replicates, metric, min_both, linkage, d_rep_links, d_rep_nodes, d_rep_order):
        """tjamd_replicate_trees on device pointers: the [replicate][sample][sample] matrices of sample_distances_weighted -> per
        replicate the links of sample_linkage (TREE_SINGLE) or sample_agglomerate (AGGL_COMPLETE, AGGL_AVERAGE) at
        d_rep_links[r * (n_samples - 1)] (None: not handed out), and the nodes and the leaf order of linkage_tree on them at
        d_rep_nodes[r * (n_samples - 1)] and d_rep_order[r * n_samples]: what clade_support takes.
        -> (rep_n_nodes, rep_n_rounds), a list of one count per replicate each"""
        counts, rounds = (C.c_int * n_replicates)(), (C.c_int * n_replicates)()
        self._chkn(lib().tjamd_replicate_trees(self._h, d_dist, n_samples, n_replicates, metric, min_both, linkage, d_rep_links, d_rep_nodes, d_rep_order, counts, rounds))
        return list(counts), list(rounds)

    def last_replicate_trees_ms(self):
        return lib().tjamd_last_replicate_trees_ms(self._h)

    def consensus_tree(self, d_rep_nodes, d_rep_order, rep_n_nodes, n_samples, min_count, d_nodes, d_order, d_rep_count=None):
        """tjamd_consensus_tree on device pointers: the replicates as clade_support takes them (rep_n_nodes: a host sequence, one
        count per replicate) -> the majority-rule consensus tree, CONSENSUS_NODE_DTYPE at d_nodes over the leaf order at
        d_order, the classes held by at least min_count replicates; and, where d_rep_count is given, per node of every
        replicate the count of its class at d_rep_count[r * (n_samples - 1) + k].  -> (n_nodes, n_classes)"""
        counts = (C.c_int * len(rep_n_nodes))(*[int(x) for x in rep_n_nodes])
        n_classes = C.c_long(-1)
        n = self._chkn(lib().tjamd_consensus_tree(self._h, d_rep_nodes, d_rep_order, counts, n_samples, len(rep_n_nodes), min_count, d_nodes, d_order, d_rep_count, C.byref(n_classes)))
        return n, n_classes.value

    def last_consensus_tree_ms(self):
        return lib().tjamd_last_consensus_tree_ms(self._h)

    def uses_log(self):
        lib().tjamd_counter_uses_log.restype = C.c_int
        lib().tjamd_counter_uses_log.argtypes = [C.c_void_p]
        return bool(lib().tjamd_counter_uses_log(self._h))

    def last_finalise_ms(self):
        return lib().tjamd_last_finalise_ms(self._h)


class HopoCounter:
    """The reference's hopo_counter through the drop-in C functions (include/tatajuba_hopo.h)."""

    def __init__(self, ptr):
        self._p = ptr

    # reference: new_hopo_counter (src/hopo_counter.c:159)
    @classmethod
    def new(cls, kmer_size):
        return cls(lib().new_hopo_counter(kmer_size))

    # reference: new_or_append_hopo_counter_from_file (src/hopo_counter.c:135); hc=None creates
    @classmethod
    def new_or_append_from_file(cls, hc, filename, opt):
        p = lib().new_or_append_hopo_counter_from_file(hc._p if hc is not None else None, os.fsencode(filename), opt)
        if hc is not None:
            return hc
        return cls(p)

    # reference: update_hopo_counter_from_seq (src/hopo_counter.c:219)
    def update_from_seq(self, seq, min_tract_size):
        if isinstance(seq, str):
            seq = seq.encode("latin-1")
        lib().update_hopo_counter_from_seq(self._p, seq, len(seq), min_tract_size)

    # reference: update_hopo_counter_from_seq_all_monomers (src/hopo_counter.c:260)
    def update_from_seq_all_monomers(self, seq):
        if isinstance(seq, str):
            seq = seq.encode("latin-1")
        lib().update_hopo_counter_from_seq_all_monomers(self._p, seq, len(seq))

    # reference: finalise_hopo_counter (src/hopo_counter.c:339)
    def finalise(self):
        lib().finalise_hopo_counter(self._p)

    # reference: del_hopo_counter (src/hopo_counter.c:175)
    def delete(self):
        if self._p:
            lib().del_hopo_counter(self._p)
            self._p = None

    __del__ = delete

    @property
    def c(self):
        return self._p.contents

    def elems(self, n=None):
        n = self.c.n_elem if n is None else n
        if n == 0:
            return np.zeros(0, dtype=ELEM_DTYPE)
        buf = (C.c_char * (n * 40)).from_address(self.c.elem)
        return np.frombuffer(buf, dtype=ELEM_DTYPE).copy()

    def idx(self):
        n = self.c.n_idx
        if n == 0 or not self.c.idx_initial:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        return (np.ctypeslib.as_array(self.c.idx_initial, (n,)).copy(),
                np.ctypeslib.as_array(self.c.idx_final, (n,)).copy())
