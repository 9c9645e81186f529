/* tatajuba_depths.h -- the step behind tatajuba_sites.h: per merged site and sample the read depth on the tract (DP), the depth
 * on the reference length and on each allele of the site (AD), and a genotype that tells a sample that equals the reference
 * (0) from one that was not seen (-1): the GT:DP:AD of a multi-sample VCF.  Same conventions as tatajuba_amd.h (extern "C",
 * plain pointers and sizes, a count or a negative TJAMD_ERR_* back, tjamd_last_error for the message, which starts with the
 * function's name).
 *
 * Reference interface replaced: none.  The reference program writes per-sample VCF files that hold variant rows only, and
 * bcftools merge fills "." for a sample without a row unless it is given -0 or a gVCF; the distinction is in the count matrix
 * of the union, which is still on the device here.  N13 of DESIGN.md section 3.5.
 */
#ifndef TATAJUBA_DEPTHS_H
#define TATAJUBA_DEPTHS_H

#include "tatajuba_sites.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule (N13) ------------------------------------------------------------------------------------------------------
 * Inputs: the permuted union, tiling and tract locations tjamd_tract_variants was given (d_out_keys, d_out_counts,
 *   d_out_tracts, d_tract_loc of tjamd_located_tracts), the same tjamd_reference, and d_sites / d_alleles exactly as
 *   tjamd_merge_variants wrote them from the records of that tjamd_tract_variants call.
 * Per site i: t = site.tract with rows [first, first + n_rows) of the union; e = the index entry whose flat is the tract's
 *   location (found as in N8), Lr = e.length; k_eff is N8's: k, less what the next tract of the whole tiling takes of the
 *   right flank when it is located in the same contig (never below 0).
 * Row class, a property of the row and not of a sample.  La = the row's length field, read signed (10 bits):
 *     La < 1                class OTHER
 *     La == Lr              class 0 (REF), whatever the flanks: N8's "same length"
 *     otherwise             nf = N8's n_flank of this row (k_eff less the trailing positions at which the row's forward right
 *                           flank agrees with the entry's) and fa = the row's forward right flank, exactly as N8 computes them
 *                           for a modal row.  The row has class j (1-based within the site) when allele first_allele + j - 1
 *                           has alt_length == La, n_flank == nf and the bases of fa on its first nf bases of alt_flank.  The
 *                           alleles of a site are distinct in these three fields, so at most one matches; none: class OTHER.
 * DP: d_depth[i * n_samples + s] = the sum of sample s's counts over the tract's rows; counts <= 0 contribute nothing.
 * AD: the same sum over the rows of class j, j = 0 .. site.n_alleles, at d_allele_depth[(site.first_allele + i + j) * n_samples
 *   + s]: every site owns n_alleles + 1 consecutive rows (REF first) and the matrix of n_sites + n_alleles rows has no holes.
 *   DP - sum_j AD is the depth on rows of class OTHER.  Sums are formed in 64 bits and stored saturated at INT32_MAX.
 * GT: d_genotype[i * n_samples + s], from the sample's modal row m by N8's definition (the highest count above 0, the first in
 *   union order on a tie):  no modal row: -1;  m has La < 1: -1;  m has class 0: 0;  m has class j >= 1: j.  A modal row with
 *   La >= 1, La != Lr and class OTHER is a record of N8 that the alleles do not hold: the inputs do not belong together, and
 *   the call is refused.  On consistent inputs the result equals tjamd_merge_variants' d_genotype wherever that is >= 1, and
 *   splits its -1 cells into 0 (the sample's reads show the genome's own length) and -1 (no usable read on the tract).
 * Summary: d_summary[i].n_ref = the samples with genotype 0, n_missing = those with -1, depth = the 64-bit sum of DP over the
 *   samples, taken before saturation.  If the samples with a genotype >= 1 are not site.n_called, the sites were merged from
 *   another list or a subset of the records: refused.
 * Returns n_sites.  n_sites == 0 returns 0 with no launch.
 * Refused with TJAMD_ERR_ARG, from an error flag raised on the device by a first pass that writes nothing (N8's idiom: no
 *   output is written by a refused call): tracts that do not tile the union; a site.tract outside [0, n_tracts); a site with
 *   no index entry, or whose flat, contig or ref_length is not that of the tract's location and its entry; first_allele /
 *   n_alleles that do not chain (site 0 starts at 0, each site where the one before ends, the last ends at n_alleles);
 *   n_alleles < 1 in a site; an allele whose site is not its site; an allele n_flank outside 0 .. k; and the two cases above.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter or reference; n_union < 0, n_samples
 *   outside 1 .. 4096, null union buffers (n_union >= 2^31: TJAMD_ERR_CAPACITY), as in tjamd_tract_variants; n_tracts that a
 *   union of n_union rows cannot have; null tracts or locations; n_sites or n_alleles < 0; null sites or alleles with a count
 *   above 0; n_sites > n_tracts; n_alleles < n_sites; (n_sites + n_alleles) * n_samples >= 2^31 (indices are ints).  Then,
 *   without a device, TJAMD_ERR_NO_DEVICE; a reference of another k or device: TJAMD_ERR_ARG.
 * Changes none of its inputs nor the counter's finalised state.  Waits once, at the end.  No atomic decides a value or a place
 *   (the error flag is the only global atomic): two runs give the same bytes.
 * Not built: genotype likelihoods or any caller beyond N8's modal-row rule; left-alignment; phasing; gzip output. */
typedef struct { int n_ref, n_missing; long long depth; } tjamd_site_depth;   /* 16 bytes */

long tjamd_site_depths (tjamd_counter *c, const tjamd_reference *ref,
                        const void *d_keys, const void *d_counts, long n_union, int n_samples,
                        const tjamd_union_tract *d_tracts, long n_tracts, const tjamd_location *d_tract_loc,
                        const tjamd_site *d_sites, long n_sites, const tjamd_allele *d_alleles, long n_alleles,
                        int16_t *d_genotype,        /* [n_sites * n_samples], site-major; may be NULL */
                        int *d_depth,               /* DP [n_sites * n_samples]; may be NULL */
                        int *d_allele_depth,        /* AD [(n_sites + n_alleles) * n_samples]; may be NULL */
                        tjamd_site_depth *d_summary /* [n_sites]; may be NULL */);

/* the kernels of the last tjamd_site_depths on this counter, first launch to last; -1.0 for a NULL counter and after a
 * refused call */
double tjamd_last_site_depths_ms (tjamd_counter *c);

#ifdef __cplusplus
}
#endif
#endif
