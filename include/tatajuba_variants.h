/* tatajuba_variants.h -- the VCF step on top of tatajuba_amd.h: each sample's tract-length variants against the reference
 * genome as the fields of VCF records, and the contig names a VCF header needs.  Same conventions as tatajuba_amd.h
 * (extern "C", plain pointers and sizes, a count or a negative TJAMD_ERR_* back, tjamd_last_error for the message).
 *
 * Reference interface replaced:
 *   tjamd_tract_variants : generate_vcf_files()                                          src/analyse_variable_tracts.c:13-33,147-233
 */
#ifndef TATAJUBA_VARIANTS_H
#define TATAJUBA_VARIANTS_H

#include "tatajuba_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-sample tract variants against the reference, as the fields of VCF records (N8; reference: generate_vcf_files,
 * src/analyse_variable_tracts.c:13-33, which walks the variable tracts and calls, per sample histogram,
 * update_vcf_file_from_context_histogram :147-190 with get_next_ht_location_from_same_contig :192-203 and
 * find_ref_alt_ht_variants_from_strings :205-233).  The reference compares two strings, "tract + right context" of the
 * genome and of the sample's modal context; here both are packed words: the index entry at a tract's location holds the
 * genome's own flanks and run length in the canonical packing of the union rows.
 *   Inputs: the permuted union and tiling tjamd_located_tracts writes (d_out_keys, d_out_counts, d_out_tracts, d_tract_loc),
 *     the tjamd_reference they were located on, and a list of tract ids (d_list NULL: every tract, n_list is not read).  The
 *     reference program walks only the variable tracts (:28): pass d_var of tjamd_union_tract_stats.
 *   Per (tract t of the list, sample s):
 *     No call if t is unlocated (flat < 0), if no index entry has t's flat, or if s has no count above 0 in t's rows.
 *     The sample's allele is its modal row: the row of t with the highest count for s, the first in union order on a tie.
 *       La = that row's length field, read signed (10 bits) as everywhere else; La < 1: no call.  Its context gives the alt flanks.
 *     The reference allele is the index entry whose flat equals the tract's location (entries are in ascending flat and one
 *       position has one run, so flat identifies it).  Lr = its length (a plain int); its context gives the ref flanks.
 *     Orientation: forward genome coordinates.  B = the forward base: the entry's canonical base, complemented if its
 *       neg_strand is set.  R_ref, R_alt = the k bases that follow the run on the forward strand, read outward from the
 *       tract: the canonical right flank (ctx1) as stored when neg_strand == 0, the reverse complement of the canonical left
 *       flank (ctx0) when it is 1.  Changes in the forward-left flank are ignored, as in the reference (:212-213).
 *     Stop at the next tract (:162-169,192-203): next = tract t + 1 of the tiling (of the whole tiling, not of the list), if
 *       it is located in the same contig; overlap = pos + Lr + k - next.pos; if overlap > 0 both right flanks lose their
 *       last `overlap` bases, k_eff = k - overlap (runs are maximal, so 0 <= k_eff <= k on a tiling of tjamd_located_tracts;
 *       a caller's own locations that give less are taken as 0); otherwise k_eff = k.
 *     Same length: La == Lr is no call, whatever the flanks (:216).
 *     Otherwise (:218-231): l0 = min (Lr, La); l1 = the number of trailing positions at which R_ref[:k_eff] and R_alt[:k_eff]
 *       agree, counted from the end and stopping at the first difference; n_flank = k_eff - l1;
 *         REF = B^(max (Lr - La, 0) + 1) + R_ref[:n_flank]      ALT = B^(max (La - Lr, 0) + 1) + R_alt[:n_flank]
 *         POS (1-based, in the contig) = pos + l0
 *       l0 and l1 stand for common_prefix_suffix_lengths_from_strings of biomcmc-lib, absent from the reference tree, in its
 *       plain reading: the longest common prefix (always l0 here: one string goes on with B where the other has left its
 *       run), then the longest common suffix of what the prefix leaves.
 *   Output record (64 bytes): flat, contig = the tract's location; pos = POS; row = the modal row's index in the permuted
 *     union; base = B (0..3 = A, C, G, T, forward); ref_length = Lr, alt_length = La; ref_flank / alt_flank hold forward base j
 *     of R_ref / R_alt in bits 2j and 2j + 1, j = 0 next to the tract: the first n_flank bases, the rest zero; pad = 0.
 *   Order: sample-major.  All of sample 0's records come first, and inside a sample they are in list order (ascending
 *     location when the list is ascending).  h_offsets (host, long[n_samples + 1]) receives the boundaries: sample s has
 *     records [h_offsets[s], h_offsets[s + 1]).  The places come from a scan of flags, not from atomics: the output is
 *     bit-identical from run to run.
 * Returns the number of records.  Refused with TJAMD_ERR_ARG (from an error flag raised on the device, as in
 * tjamd_union_tract_stats, where only the device can tell): tracts that do not tile the union, a list id outside
 * [0, n_tracts), a reference of another k or device, n_samples outside 1 ... 4096.  A capacity below the records found is
 * TJAMD_ERR_CAPACITY, with nothing written at or beyond d_out[capacity]; without a device, TJAMD_ERR_NO_DEVICE.  Changes
 * none of its inputs nor the counter's finalised state; h_offsets is written on success only.  Waits once, at the end.
 * Not built: the reference may write two rows for one place and sample when two tracts share it (:178-179 FIXME; here
 * tjamd_located_tracts has merged them), and gzip output is the caller's. */
typedef struct { long long flat; int tract, sample, contig, pos, row, base, ref_length, alt_length, n_flank, pad;
                 uint64_t ref_flank, alt_flank; } tjamd_variant;   /* 64 bytes */
long tjamd_tract_variants (tjamd_counter *c, const tjamd_reference *ref, const void *d_keys, const void *d_counts, long n_union,
                           int n_samples, const tjamd_union_tract *d_tracts, long n_tracts, const tjamd_location *d_tract_loc,
                           const int *d_list, long n_list, tjamd_variant *d_out, long capacity, long *h_offsets);

/* Host-only: the names of the records tjamd_read_file_stream parses, in file order: the header line after its '>' or '@' up to the first space or
 * tab, each followed by '\n' (a reference FASTA's contig names, for a VCF's ##contig lines and #CHROM column; a contig's
 * length is the distance between the delimiters of the stream).  Stops where tjamd_read_file_stream stops, so *n_records
 * equals its *n_reads.  Returns the bytes needed and writes them when capacity suffices (out = NULL to size); -1 if the
 * file cannot be opened. */
long tjamd_read_file_names (const char *path, char *out, long capacity, long *n_records);

#ifdef __cplusplus
}
#endif
#endif
