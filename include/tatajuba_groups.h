/* tatajuba_groups.h -- the step behind tatajuba_linkage.h: what sets a group of samples apart.  The site x sample genotype
 * matrix of N13 (or N12) read by group: per site and group whether the called members all carry one genotype, how many called
 * samples of other groups carry it too, and the short list of (site, group) pairs where nobody outside does: the markers of a
 * cluster.  Same conventions as tatajuba_amd.h (extern "C", plain pointers and sizes, a count or a negative TJAMD_ERR_* back,
 * tjamd_last_error for the message, which starts with the function's name).
 *
 * Reference interface replaced: none.  The reference program ends at per-sample VCFs and has no step that reads genotypes by
 * group; the matrix is on the device here, 512 M cells at 125 000 sites x 4096 samples, and the answer is a short list.  Through
 * d_unique of tjamd_merge_variants and tjamd_variant_effects a mark comes with a coding effect.  N16 of DESIGN.md section 3.5.
 */
#ifndef TATAJUBA_GROUPS_H
#define TATAJUBA_GROUPS_H

#include "tatajuba_linkage.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule (N16) ------------------------------------------------------------------------------------------------------
 * Input: d_sites and d_genotype[site * n_samples + s] as tjamd_merge_variants or tjamd_site_depths wrote them (-1: not called;
 *   0: the genome's own length; a > 0: the site's a-th allele); of a site only n_alleles is read.  d_group[s] is the group of
 *   sample s.
 * Who takes part: sample s takes part if and only if d_group[s] >= 0.  A sample with -1 is neither a member nor an outsider
 *   anywhere.  d_cluster of tjamd_linkage_clusters, with its return value as n_groups, is a valid input as it stands.  A group
 *   may have no members.
 * Per site i and group G (d_calls[i * n_groups + G]): the called members are the samples of G with a genotype g >= 0 at i.
 *     n_called   the number of called members
 *     fixed      the one genotype they all carry; -1 if none is called, -2 if they carry more than one
 *     n_outside  the number of called samples of other groups that carry `fixed`; 0 when fixed < 0
 *     mark       1 if and only if fixed >= 0, n_called >= min_called, n_outside == 0 and at least one sample of another group
 *                is called at i; otherwise 0.  A group is not set apart from samples nobody saw.
 * Per site (d_site_out[i]): n_called counts the called samples that take part, n_genotypes the distinct genotypes among them,
 *   n_marks the groups marked there, first_group the smallest such group or -1.
 * d_group_marks[G] is the number of sites at which G is marked.
 * d_marks holds the marked (site, group) pairs, ascending in (site, group), each with the fixed genotype and the group's
 *   n_called.
 * Returns the number of marks and sets *h_n_marks.  More marks than mark_capacity is -TJAMD_ERR_CAPACITY: nothing is written
 *   at or beyond the capacity, what lies below it is in its place, the other three outputs are complete and *h_n_marks is set,
 *   so that a caller may size with capacity 0 and call again.
 * Refused with TJAMD_ERR_ARG, from an error flag raised on the device by a first pass that reads everything and writes nothing
 *   of the caller's (N13's idiom: no output is touched by a refused call, *h_n_marks is left alone, and the timer reads -1.0
 *   after one): a label below -1 or at or above n_groups; a site with n_alleles < 1 or n_alleles > n_samples; a genotype cell
 *   below -1 or above its site's n_alleles.  (N12 gives a sample at most one record per tract and every allele has a record:
 *   its sites never have more alleles than there are samples.  The bound lets a table be indexed by genotype.)
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter; n_sites < 0; null d_sites or
 *   d_genotype with n_sites > 0; a null d_group; n_samples or n_groups outside 1 .. 4096; min_called < 1; mark_capacity < 0; a
 *   null d_marks with a capacity above 0; n_sites * n_samples >= 2^31; with d_calls given, n_sites * n_groups >= 2^31.  Then,
 *   without a device, TJAMD_ERR_NO_DEVICE.
 * n_sites == 0 returns 0, sets *h_n_marks to 0, zeroes d_group_marks with a memset and launches no kernel.
 * Changes none of its inputs nor the counter's finalised state.  Waits once, at the end.  Every value is a count or a minimum
 *   of integers and the list's places come from a scan: two runs give the same bytes.
 * Scratch, from the counter's block (it grows to the largest call and is kept): the error and count words (one per group
 *   among them) and one int per site (its marks, then their offsets).  A call whose scratch cannot be had returns TJAMD_ERR_HIP.
 *
 * Not built: a test statistic or p-value per site; groups that overlap; weights; marks that allow a share of exceptions;
 *   read depths; marks of a tree's inner nodes without a cut. */
typedef struct { int n_called, fixed, n_outside, mark; } tjamd_group_call;             /* 16 bytes, per (site, group) */
typedef struct { int n_called, n_genotypes, n_marks, first_group; } tjamd_group_site;  /* 16 bytes, per site */
typedef struct { int site, group, genotype, n_called; } tjamd_group_mark;              /* 16 bytes, the list */

long tjamd_group_sites (tjamd_counter *c,
                        const tjamd_site *d_sites, long n_sites,
                        const int16_t *d_genotype,      /* [n_sites * n_samples], site-major: N13's or N12's */
                        int n_samples,
                        const int *d_group,             /* [n_samples]: 0 .. n_groups - 1, or -1: the sample takes no part */
                        int n_groups, int min_called,
                        tjamd_group_call *d_calls,      /* [n_sites * n_groups], site-major; may be NULL */
                        tjamd_group_site *d_site_out,   /* [n_sites]; may be NULL */
                        int *d_group_marks,             /* [n_groups]: marks per group; may be NULL */
                        tjamd_group_mark *d_marks, long mark_capacity,   /* may be NULL with capacity 0 */
                        long *h_n_marks                 /* may be NULL */);

/* the kernels of the last tjamd_group_sites on this counter, first launch to last; -1.0 for a NULL counter and after a call
 * that did not return a count */
double tjamd_last_group_sites_ms (tjamd_counter *c);

#ifdef __cplusplus
}
#endif
#endif
