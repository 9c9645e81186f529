"""tatajuba_amd -- MI355X-native homopolymer-tract counting engine (tatajuba's hopo_counter hot path).

The product is libtatajuba_amd.so: a C-ABI shared library (include/tatajuba_hopo.h, include/tatajuba_amd.h) whose host
side is C and whose compute is hand-written HIP for gfx950.  This Python package only loads it through ctypes for the
tests and the benchmark; it holds no compute of its own and never touches oracle/.
"""
from .build import build_library, library_path  # noqa: F401
from .capi import (Counter, Comm, Reference, Annotation, REF_ENTRY_DTYPE, LOCATION_DTYPE, VARIANT_DTYPE, FEATURE_DTYPE, TRACT_FEATURE_DTYPE, HopoCounter, Options, lib, device_count, synth_stream, ELEM_DTYPE, RECORD_DTYPE,  # noqa: F401
                   LOCATED_DTYPE, GROUP_DTYPE, TRACT_SUMMARY_DTYPE, UNION_TRACT_DTYPE, UNION_TRACT_SUMMARY_DTYPE, decode_meta, TatajubaAmdError, read_file_stream, EXPORTS, VARIANT_EXPORTS, FEATURE_EXPORTS, LOCATE_EXPORTS, MAX_SHIFT, flank_edit_distance,
                   read_gff3, gff3_string,
                   Coding, CDS_DTYPE, EFFECT_DTYPE, EFFECT_CLASSES, EFFECT_EXPORTS, translate, read_gff3_phase,
                   SITE_DTYPE, ALLELE_DTYPE, SITE_EXPORTS, site_ref_alt,
                   SITE_DEPTH_DTYPE, DEPTH_EXPORTS,
                   SAMPLE_DISTANCE_DTYPE, DISTANCE_EXPORTS,
                   LINK_DTYPE, LINK_DIFFER, LINK_LENGTH, LINK_DIFFER_RATE, LINKAGE_EXPORTS,
                   AGGL_COMPLETE, AGGL_AVERAGE, AGGLOMERATE_EXPORTS,
                   GROUP_CALL_DTYPE, GROUP_SITE_DTYPE, GROUP_MARK_DTYPE, GROUP_EXPORTS,
                   TREE_NODE_DTYPE, CLADE_EXPORTS,
                   BOOTSTRAP_EXPORTS,
                   TREE_SINGLE, REPLICATE_TREE_EXPORTS,
                   CONSENSUS_NODE_DTYPE, CONSENSUS_EXPORTS)
