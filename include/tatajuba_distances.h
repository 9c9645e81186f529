/* tatajuba_distances.h -- the step behind tatajuba_depths.h: how far apart the samples are over the merged sites.  Per pair of
 * samples the sites at which both have a genotype, those at which the two genotypes differ, and the sum of the differences of
 * their tract lengths: what a tree, a clustering or an outbreak cut is built from.  Same conventions as tatajuba_amd.h (extern
 * "C", plain pointers and sizes, a count or a negative TJAMD_ERR_* back, tjamd_last_error for the message, which starts with
 * the function's name).
 *
 * Reference interface replaced: none.  The reference program ends at per-sample VCF files and its tutorial at their merge;
 * the site x sample genotype matrix of N12 and N13 is on the device here, and this reduction is the one step of the chain
 * whose work grows with the square of the sample count.  N14 of DESIGN.md section 3.5.
 */
#ifndef TATAJUBA_DISTANCES_H
#define TATAJUBA_DISTANCES_H

#include "tatajuba_depths.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule (N14) ------------------------------------------------------------------------------------------------------
 * Inputs: d_sites / d_alleles exactly as tjamd_merge_variants wrote them, and a genotype matrix [n_sites * n_samples],
 *   site-major: that of tjamd_site_depths (the intended input) or that of tjamd_merge_variants.  A cell g is -1 (no call), 0
 *   (the genome's own length) or j >= 1 (allele first_allele + j - 1 of the site).  N12's matrix has -1 where N13's has 0:
 *   with it, samples that equal the reference count as not called.  No union, tiling or reference is needed.
 * Length of a cell: L(0) = site.ref_length; L(j) = alleles[site.first_allele + j - 1].alt_length.
 * Per pair (a, b), over all sites:
 *     n_both       the sites where g_a >= 0 and g_b >= 0
 *     n_differ     those of them where g_a != g_b
 *     length_diff  the sum of |L(g_a) - L(g_b)| over them, formed exactly in 64 bits
 *   Two alleles of one site may share a length and differ in the flank: such a site counts in n_differ and adds 0 to
 *   length_diff.
 * Output: d_out[a * n_samples + b] holds the three values for every a and b; the matrix is full and symmetric.  On the diagonal
 *   n_both is the number of sites at which the sample is called, and the other two values are 0.
 * Returns n_sites.  n_sites == 0 zeroes the matrix with a memset, launches no kernel and returns 0.
 * Refused with TJAMD_ERR_ARG, from an error flag raised on the device by a first pass that writes nothing of the caller's (N13's
 *   idiom: d_out is untouched by a refused call): a genotype cell below -1 or above its site's n_alleles; first_allele /
 *   n_alleles that do not chain (site 0 starts at 0, each site where the one before ends, the last ends at n_alleles);
 *   n_alleles < 1 in a site; an allele whose site is not its site; an alt_length outside 0 .. 1023; a ref_length below 0.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter; a null d_out; n_sites or n_alleles
 *   < 0; null sites, alleles or genotype with a count above 0; n_samples outside 1 .. 4096; n_alleles < n_sites; n_alleles
 *   >= 2^31; n_sites * n_samples >= 2^31 (indices are ints).  Then, without a device, TJAMD_ERR_NO_DEVICE.
 * Changes none of its inputs nor the counter's finalised state.  Waits once, at the end.  Where the sites are split over
 *   workgroups their partial sums lie in scratch and are added by a further pass, in a fixed order: no atomic decides a value
 *   (the error flag is the only global atomic), and two runs give the same bytes.
 * Scratch, from the counter's block (it grows to the largest call and is kept): 4 bytes per genotype cell, n_sites * n_samples
 *   ints, twice the genotype matrix -- the first pass leaves every cell's length there and the tiles read it beside the cell
 *   (2 GB at 125 000 sites x 4096 samples, under 8 GB at the limit of 2^31 cells); and, only where the sites are split, one
 *   tile of 16-byte sums per workgroup, 16 MB at most on 256 compute units.  Nothing grows with n_samples^2 x slices.  The
 *   lengths are ints and not int16 because ref_length is one.  A call whose scratch cannot be had returns TJAMD_ERR_HIP.
 * Not built: a site list or mask; weights; any distance on read depths.  A tree and a clustering are not built here: the
 *   single-linkage ones are the next step, tatajuba_linkage.h. */
typedef struct { int n_both, n_differ; long long length_diff; } tjamd_sample_distance;   /* 16 bytes */

long tjamd_sample_distances (tjamd_counter *c,
                             const tjamd_site *d_sites, long n_sites, const tjamd_allele *d_alleles, long n_alleles,
                             const int16_t *d_genotype,          /* [n_sites * n_samples], site-major */
                             int n_samples,
                             tjamd_sample_distance *d_out        /* [n_samples * n_samples], row-major */);

/* the kernels of the last tjamd_sample_distances on this counter, first launch to last; -1.0 for a NULL counter and after a
 * refused call */
double tjamd_last_sample_distances_ms (tjamd_counter *c);

#ifdef __cplusplus
}
#endif
#endif
