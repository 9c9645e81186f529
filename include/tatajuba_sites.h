/* tatajuba_sites.h -- the multi-sample step on top of tatajuba_variants.h: the per-sample variant records of
 * tjamd_tract_variants merged into sites (one per tract that has a record), each with its distinct alleles, a genotype per
 * sample, and one record per allele for tjamd_variant_effects.  Same conventions as tatajuba_amd.h (extern "C", plain
 * pointers and sizes, a count or a negative TJAMD_ERR_* back, tjamd_last_error for the message, which starts with the
 * function's name).
 *
 * Reference interface replaced: none.  The reference program leaves this step to its user: docs/tutorial.md, "Downstream
 * analyses", concatenates the per-sample VCF files (sort | uniq) to see each event once, and merges them with bcftools
 * (norm, bgzip, index, merge) into one multi-sample file.  Here the records are on the device and every record of one tract
 * has one index entry, hence one anchor: both recipes are a sort and a few segmented reductions, and no normalisation
 * against a FASTA is needed.  N12 of DESIGN.md section 3.5.
 */
#ifndef TATAJUBA_SITES_H
#define TATAJUBA_SITES_H

#include "tatajuba_variants.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule (N12) ------------------------------------------------------------------------------------------------------
 * Input: d_records is what one tjamd_tract_variants call wrote: sample-major, at most one record per (sample, tract).  Flank
 *   words are read on their first n_flank bases only (bits above are ignored, as N8 leaves them zero).
 * Site: a tract that has at least one record.  Sites are numbered in ascending tract, whatever the order of the list N8 was
 *   given.  flat, contig, base and ref_length (Lr) are those of the site's records; n_called is the number of its records,
 *   first_record the smallest input index among them.
 * Allele: two records of one site are the same allele exactly when alt_length, n_flank and alt_flank agree (beyond its own
 *   n_flank a record's right flank is the genome's, by N8's definition of l1).  The alleles of a site are in ascending
 *   (alt_length, n_flank, alt_flank), alt_flank compared as a number; alleles are numbered globally in site order, a site's
 *   being [first_allele, first_allele + n_alleles).  n_samples is the number of records that carry the allele, first_record
 *   the smallest input index among them.
 * Common anchor: F = site.n_flank = the largest n_flank of the site's records; site.ref_flank = the ref_flank of such a
 *   record, the first F forward bases of R_ref; min_length = min (Lr, smallest alt_length); site.pos = the smallest pos of the
 *   site's records, which is the tract's 0-based position plus min_length: N8's POS rule with l0 taken over all alleles.
 *   allele.alt_flank is completed to F bases: the record's own bases below its n_flank, site.ref_flank's from there up to F,
 *   zero above F.  allele.n_flank keeps the record's own value.
 * Text: REF = B^(Lr - min_length + 1) + R_ref[:F], ALT_a = B^(alt_length_a - min_length + 1) + R_alt_a[:F].  A site with one
 *   allele reproduces N8's record exactly.
 *   tjamd_site_ref_alt (host only, needs no device): the text of REF (allele = NULL) or of an allele's ALT.  Returns its
 *   length and writes the text and a NUL when capacity > length, otherwise nothing (out = NULL to size).  -1 for a null site, a
 *   kmer_size outside 1 .. 32, a site n_flank outside 0 .. kmer_size, a base outside 0 .. 3 or a length below min_length.
 * Genotype: d_genotype[site * n_samples + s] is the 1-based index, within the site, of sample s's allele, and -1 where s has
 *   no record there: bcftools merge's ".".  N8 does not say whether a sample without a record equals the reference or was not
 *   seen, and this step does not guess: tjamd_site_depths (tatajuba_depths.h, N13) reads the union's counts and tells the two
 *   apart.  Rows at or beyond the number of sites are not written.
 * d_allele_of[i] (optional) is the global allele index of input record i; d_unique[a] (optional) is record first_record of
 *   allele a, unchanged: the input of tjamd_variant_effects that walks every distinct allele once.
 * Returns the number of sites and sets *h_n_alleles.  n_records == 0 returns 0 and sets it to 0, with no launch.
 * Refused with TJAMD_ERR_ARG, from an error flag raised on the device as in N8 (no output is written, *h_n_alleles is left
 *   alone): a record whose tract is outside [0, n_tracts) or whose sample is outside [0, n_samples); a (tract, sample) pair
 *   that occurs twice (a list that names a tract twice gives one); records of one tract that disagree in flat, contig, base or
 *   ref_length, or whose ref_flank does not agree with the site's on their own n_flank bases; n_flank outside 0 .. kmer_size;
 *   alt_length outside 0 .. 1023 (the 10 bits the union's rows have for it).
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter, null d_records with records, null
 *   d_sites or d_alleles with a capacity above 0, null h_n_alleles, n_records < 0 or >= 2^31 (indices are ints), n_samples
 *   outside 1 .. 4096, kmer_size outside 2 .. 32 (the counter's range), n_tracts < 0, a capacity < 0.
 * A capacity below what was found is TJAMD_ERR_CAPACITY, with nothing written at or beyond either capacity (what lies below
 *   both is in its place); without a device, TJAMD_ERR_NO_DEVICE.
 * Changes none of its inputs nor the counter's finalised state.  Waits once, at the end.  No atomic decides a place (the error
 *   flag is the only global atomic): two runs give the same bytes.
 * Not built: left-alignment to the base in front of the run (bcftools norm's form; the anchor here is N8's, the last base the
 *   alleles share); phasing of two tracts; gzip output.  (A reference genotype 0 for samples that N8 leaves without a record is
 *   N13's, tatajuba_depths.h.) */
typedef struct { long long flat; int tract, contig, pos, base, ref_length, min_length, n_flank,
                 n_alleles, first_allele, n_called, first_record, pad; uint64_t ref_flank; } tjamd_site;    /* 64 bytes */
typedef struct { int site, alt_length, n_flank, n_samples, first_record, pad; uint64_t alt_flank; } tjamd_allele;   /* 32 bytes */

long tjamd_merge_variants (tjamd_counter *c, int kmer_size, const tjamd_variant *d_records, long n_records,
                           int n_samples, long n_tracts,
                           tjamd_site *d_sites, long site_capacity, tjamd_allele *d_alleles, long allele_capacity,
                           int16_t *d_genotype,      /* [site_capacity * n_samples], site-major; may be NULL */
                           int *d_allele_of,         /* [n_records]: global allele index of input record i; may be NULL */
                           tjamd_variant *d_unique,  /* [allele_capacity]: record first_record of each allele; may be NULL */
                           long *h_n_alleles);
int tjamd_site_ref_alt (const tjamd_site *site, const tjamd_allele *allele /* NULL: REF */, int kmer_size, char *out, int capacity);

/* the kernels of the last tjamd_merge_variants on this counter, first launch to last; -1.0 for a NULL counter and after a
 * refused call */
double tjamd_last_merge_variants_ms (tjamd_counter *c);

#ifdef __cplusplus
}
#endif
#endif
