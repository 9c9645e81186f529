/* tatajuba_effects.h -- the coding effect of a tract variant, on top of tatajuba_amd.h: the genome's bases and the coding
 * features of a GFF3 file as a table on the device, and per variant record of tjamd_tract_variants what the length change does
 * to the protein of the feature tjamd_tract_features found (nothing, amino acids dropped or added, a frameshift).  Same
 * conventions as tatajuba_amd.h (extern "C", plain pointers and sizes, a count or a negative TJAMD_ERR_* back,
 * tjamd_last_error for the message, which starts with the function's name).
 *
 * Reference interface replaced: none.  The reference program's documentation ("Mutational effect") says what a length change
 * inside a coding region does and sends the user to snpEff, VEP or bcftools with the VCF files; its protein_from_dna_string
 * (src/genome_set.c) is called by nothing and never resets its codon.  N11 of DESIGN.md section 3.5.
 */
#ifndef TATAJUBA_EFFECTS_H
#define TATAJUBA_EFFECTS_H

#include "tatajuba_amd.h"
#include "tatajuba_variants.h"
#include "tatajuba_features.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- codes and translation -----------------------------------------------------------------------------------------------
 * A base has a code: A C G T/U in either case are 0 to 3, every other byte is 4.  A codon of three codes below 4 has the
 * index b0 << 4 | b1 << 2 | b2; its amino acid is that of the standard genetic code (NCBI table 1; table 11, the bacterial
 * one, has the same codon-to-amino-acid map), one upper-case letter, the stops TAA, TAG and TGA written '*'.  A codon with a
 * code 4 in it is 'X'; 'X' is not a stop and equals only 'X'.
 *   tjamd_translate (host only): reverse = 0: codon i is dna[3i .. 3i + 2]; reverse = 1: the reverse complement is
 *     translated, its base j being the complement of dna[n - 1 - j] (code c -> 3 - c, 4 stays 4).  Returns n / 3 and writes that
 *     many bytes when capacity suffices, otherwise nothing; translation does not end at a stop and no NUL is written.
 *     -TJAMD_ERR_ARG for n < 0, a null dna with n > 0 or a null out with something to write. */
long tjamd_translate (const char *dna, long n, int reverse, char *out, long capacity);

/* ---- the phase column (host only) ----------------------------------------------------------------------------------------
 * One byte per feature that tjamd_gff3_read (tatajuba_features.h) keeps: the same lines in the same order with the same
 * skips (one line walker serves both).  The byte is column 8 as 0, 1 or 2, and -1 for "." or anything else.  Returns the number
 * of features and writes them when out is given and capacity suffices, otherwise nothing is written; -1 if the file cannot be
 * opened or is not what its gzip header says. */
long tjamd_gff3_read_phase (const char *path, const char *contig_names, long n_contigs, signed char *out, long capacity);

/* ---- the coding table (N11) ----------------------------------------------------------------------------------------------
 * Genome and contigs: h_stream is the stream tjamd_reference_create was given.  Contig 0 begins at byte 0, contig c behind the
 *   c-th '\n'; the numbering is tjamd_reference_create's, an empty contig included, and what follows a last '\n' is a contig
 *   only if it has a byte.  A contig's length is the distance to its delimiter, or to the end of the stream.
 * Coding features: feature i is coding when cls == TJAMD_FEATURE_CDS and strand is 0 or 1.  Its span is forward [S, E] of its
 *   contig, S = start - 1 and E = min (end, contig length) - 1: an end beyond the contig is clipped, as tjamd_annotation_create
 *   accepts it, and a span that begins beyond its contig is empty (length 0).  Its phase is h_phase[i] when h_phase is given and
 *   the value is 1 or 2, else 0.  Its CDS-oriented sequence is the span on strand 0 and the span's reverse complement on
 *   strand 1.  Translation starts at CDS-oriented base `phase` and has n_codons = max (span length - phase, 0) / 3 whole codons.
 *   The protein P is the amino acids up to and including the first '*', or all n_codons if there is none; aa_len is the number
 *   of amino acids before the '*', has_stop is 0 or 1.  Every other feature has -1 in all four fields of its tjamd_cds.
 *   Each GFF3 line is a feature of its own.
 *   Not built: the lines of a CDS written over several lines (a spliced gene) are not joined -- the genomes this tool is used
 *   on are bacterial; there are no start-codon rules.
 * tjamd_coding_create copies the stream and the features to the counter's device, turns the stream into one code per byte,
 *   finds the contig starts from the delimiters and scans every coding feature for its first stop; one wait, at the end.  NULL
 *   with TJAMD_ERR_ARG for a null counter, a null stream with n_bytes > 0, n_features < 0 or a null h_features with n_features
 *   > 0, more than 2^30 features, and a feature with contig outside the stream's contigs, start < 1 or end < start (these read
 *   only the caller's host buffers, so they come before the device is looked for); TJAMD_ERR_CAPACITY for a stream of 2^31
 *   bytes or more; TJAMD_ERR_NO_DEVICE without a device.  n_features = 0 and n_bytes = 0 are valid.  The table keeps its own
 *   memory: it needs neither the caller's buffers nor a tjamd_reference afterwards.
 * tjamd_coding_features: n_features (-1 for NULL).
 * tjamd_coding_download: returns n_features; the tjamd_cds records are written when capacity suffices, otherwise nothing. */
typedef struct { int aa_len, has_stop, n_codons, phase; } tjamd_cds;             /* 16 bytes, one per feature */
typedef struct tjamd_coding tjamd_coding;
tjamd_coding *tjamd_coding_create (tjamd_counter *c, const void *h_stream, size_t n_bytes,
                                   const tjamd_feature *h_features, long n_features, const signed char *h_phase);
void tjamd_coding_destroy (tjamd_coding *cod);
long tjamd_coding_features (const tjamd_coding *cod);
long tjamd_coding_download (const tjamd_coding *cod, tjamd_cds *out, long capacity);

/* ---- the effect of a variant record (N11) --------------------------------------------------------------------------------
 * A variant record v (tatajuba_variants.h): Lr = ref_length, La = alt_length, B = the base (its low two bits),
 *   REF = B^(max (Lr - La, 0) + 1) + R_ref[:n_flank], ALT = B^(max (La - Lr, 0) + 1) + R_alt[:n_flank], POS = v.pos, 1-based.
 *   REF occupies forward [p, q] of contig v.contig, p = POS - 1 and q = p + |REF| - 1.  REF's bases are NOT compared with the
 *   genome: the replaced span comes from pos, the two lengths and n_flank alone (ref_flank is not read).
 * The feature of a record: f = d_tract_feat[v.tract].feature, the winner tjamd_tract_features wrote.  d_tract_feat = NULL
 *   means no record has a feature, and n_tracts and v.tract are not read.
 * The output record:
 *   feature = f.
 *   f < 0 or f not coding: cls = TJAMD_EFFECT_NONE, first_diff = -1, the rest 0.
 *   [p, q] not inside [S, E] of f, or v.contig another contig than f's: cls = TJAMD_EFFECT_BOUNDARY; ref_aa_len and the
 *     TJAMD_EFFECT_REF_STOP bit come from the table, first_diff = -1, the rest 0.
 *   Otherwise the alternative span is the forward span with [p, q] replaced by ALT, its length the span length + |ALT| - |REF|,
 *     and P_alt is its translation by the same rule with the same strand and phase (no read-through beyond the annotated end).
 *     cds_pos: the first CDS-oriented base that may differ, POS - S on strand 0 and E - q on strand 1 (on strand 0 that is the
 *       base behind REF's first one, which REF and ALT share; the comparison itself takes base p along, so that a REF that is
 *       not the genome's still gets the rule as written).
 *     first_diff: the first index at which P_ref and P_alt differ, the '*' compared like any symbol; if one is a proper prefix
 *       of the other, the shorter one's length; -1 if they are equal.
 *     cls: TJAMD_EFFECT_IDENTICAL when first_diff == -1, else TJAMD_EFFECT_INFRAME when (La - Lr) % 3 == 0, else
 *       TJAMD_EFFECT_FRAMESHIFT.
 *     ref_aa_len, alt_aa_len: the amino acids before the '*'.  flags: TJAMD_EFFECT_REF_STOP when P_ref ends in '*',
 *       TJAMD_EFFECT_ALT_STOP when P_alt does.
 *     ref_aa, alt_aa: the up to eight symbols P[first_diff .. first_diff + 8), ASCII, symbol j in bits 8j .. 8j + 7, the '*'
 *       included, zero beyond the protein's end; both 0 when identical.
 *   pad = 0.
 * Returns n and writes exactly n records (n = 0: returns 0, writes nothing).  Refused with TJAMD_ERR_ARG from an error flag
 * raised on the device by a first pass that writes nothing (nothing is read outside any array, and d_out is left as it was): a contig
 * outside the stream's contigs; pos < 1, or q beyond the contig; n_flank outside 0 .. 32; ref_length or alt_length below 1;
 * with d_tract_feat given, a tract outside [0, n_tracts) or a feature index outside [-1, n_features).  Refused on the host
 * with TJAMD_ERR_ARG: n < 0, null buffers, a null counter or table, a coding table of another device; TJAMD_ERR_CAPACITY for
 * 2^31 records or more; without a device, TJAMD_ERR_NO_DEVICE.  Changes none of its inputs nor the counter's finalised
 * state.  Two launches (the check, the walk); waits once, at the end.
 * Not built: equal (tract, alt_length) records of several samples are walked once each; deduplicating them first is the step
 * after. */
enum { TJAMD_EFFECT_NONE = 0, TJAMD_EFFECT_BOUNDARY = 1, TJAMD_EFFECT_IDENTICAL = 2, TJAMD_EFFECT_INFRAME = 3, TJAMD_EFFECT_FRAMESHIFT = 4 };
enum { TJAMD_EFFECT_REF_STOP = 1, TJAMD_EFFECT_ALT_STOP = 2 };                 /* bits of flags */
typedef struct { int feature, cls, cds_pos, first_diff, ref_aa_len, alt_aa_len, flags, pad;
                 uint64_t ref_aa, alt_aa; } tjamd_effect;                        /* 48 bytes */
long tjamd_variant_effects (tjamd_counter *c, const tjamd_coding *cod, const tjamd_variant *d_variants, long n,
                            const tjamd_tract_feature *d_tract_feat, long n_tracts, tjamd_effect *d_out);

/* -1.0 for a NULL counter and after a refused call */
double tjamd_last_coding_ms (tjamd_counter *c);            /* the kernels of the last tjamd_coding_create on this counter (the copies to the device not included) */
double tjamd_last_variant_effects_ms (tjamd_counter *c);   /* the kernel of the last tjamd_variant_effects */

#ifdef __cplusplus
}
#endif
#endif
