/* tatajuba_linkage.h -- the step behind tatajuba_distances.h: which samples belong together.  The sample x sample matrix of N14
 * reduced to the single-linkage tree of the samples (a minimum spanning forest of the pairs under one metric) and, from that
 * tree, the clusters at a threshold: two samples are in one cluster if a chain of pairs, each within the threshold, joins them,
 * which is how an outbreak is cut.  Same conventions as tatajuba_amd.h (extern "C", plain pointers and sizes, a count or a
 * negative TJAMD_ERR_* back, tjamd_last_error for the message, which starts with the function's name).
 *
 * Reference interface replaced: none.  Neither the reference program nor its tutorial builds a tree or a clustering; the matrix
 * is on the device here, 256 MB of it at 4096 samples, and the tree is n_samples - 1 records.  N15 of DESIGN.md section 3.5.
 */
#ifndef TATAJUBA_LINKAGE_H
#define TATAJUBA_LINKAGE_H

#include "tatajuba_distances.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule of the tree (N15) ------------------------------------------------------------------------------------------
 * Input: d_dist[a * n_samples + b] as tjamd_sample_distances wrote it: full, symmetric, the diagonal included.
 * Edges: a pair (a, b), a < b, is an edge if and only if n_both >= min_both.  Two samples with too little in common are not
 *   near each other, whatever their counts say.  The diagonal makes no edge.
 * Key of an edge, by the metric:
 *     TJAMD_LINK_DIFFER       n_differ
 *     TJAMD_LINK_LENGTH       length_diff
 *     TJAMD_LINK_DIFFER_RATE  floor (n_differ * 2^32 / n_both), formed exactly in 64 bits (n_differ <= n_both < 2^31: the
 *                             product is below 2^63; min_both >= 1: the divisor is not 0)
 *   Every key is in 0 .. 2^63 - 1.
 * Order: edges are totally ordered by (key, a, b).  Under a total order the minimum spanning forest is unique.
 * Output: d_links holds that forest's edges, ascending in (key, a, b): the order in which single linkage merges.  Returns
 *   n_links = n_samples - (components of the edge graph).  Entries of d_links from n_links on are not written.
 * Refused with TJAMD_ERR_ARG, from an error flag raised on the device by a first pass that reads every cell and writes nothing
 *   of the caller's (N13's idiom: d_links is untouched by a refused call, and the timer reads -1.0 after one): a cell, the
 *   diagonal included, with n_both < 0, n_differ < 0, n_differ > n_both or length_diff < 0; a cell (a, b) one of whose three
 *   values differs from the same value of (b, a).
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter; a null d_dist; a null d_links with
 *   n_samples > 1; n_samples outside 1 .. 4096; a metric outside the three; min_both < 1.  Then, without a device,
 *   TJAMD_ERR_NO_DEVICE.
 * n_samples == 1 returns 0 and launches nothing but the wait.  Changes none of its inputs nor the counter's finalised state.
 *   Waits once, at the end.  Two runs give the same bytes: every minimum is one of integers under the total order, which does
 *   not depend on the order in which it is taken, and the links are sorted at the end.
 * Scratch, from the counter's block (it grows to the largest call and is kept): 8 bytes per cell of the matrix for the keys
 *   (128 MB at 4096 samples) and 36 bytes per sample; at 64 samples and fewer neither, the call is one workgroup in one launch
 *   with the keys in LDS.  A call whose scratch cannot be had returns TJAMD_ERR_HIP.
 *
 * ---- the rule of the clusters ----------------------------------------------------------------------------------------------
 * Graph: n_samples vertices and those of the n_links links whose key <= threshold.
 * Output: d_cluster[s] is the dense id of s's connected component; components are numbered from 0 in the order of their
 *   smallest member, so d_cluster[0] == 0 always.  Returns the number of components.
 * Any list of links is accepted: unsorted, cyclic, with duplicates, with more than n_samples - 1 links, up to 2^24.  A caller
 *   may cut a list it has filtered or concatenated.  With tjamd_sample_linkage's own output the result equals the components
 *   of the graph of all pairs with n_both >= min_both and key <= threshold: that is the point of the tree.
 * n_links == 0, or a threshold below 0, gives every sample its own cluster.
 * Refused with TJAMD_ERR_ARG on the device (d_cluster untouched, the timer reads -1.0): a link with a < 0, a >= b,
 *   b >= n_samples or key < 0.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter; a null d_cluster; n_links < 0 or
 *   above 2^24; a null d_links with n_links > 0; n_samples outside 1 .. 4096.  Then, without a device, TJAMD_ERR_NO_DEVICE.
 * Changes none of its inputs.  Waits once.  The labels are minima of integers: two runs give the same bytes.
 *
 * Not built: other linkages (complete, average, Ward); neighbour joining; a Newick writer; length_diff per site; a cophenetic
 *   matrix; bootstrap. */
enum { TJAMD_LINK_DIFFER = 0, TJAMD_LINK_LENGTH = 1, TJAMD_LINK_DIFFER_RATE = 2 };
typedef struct { int a, b; long long key; } tjamd_link;            /* 16 bytes; a < b */

long tjamd_sample_linkage (tjamd_counter *c,
                           const tjamd_sample_distance *d_dist,  /* [n_samples * n_samples], as tjamd_sample_distances wrote it */
                           int n_samples, int metric, int min_both,
                           tjamd_link *d_links                   /* [n_samples - 1] */);

long tjamd_linkage_clusters (tjamd_counter *c, const tjamd_link *d_links, long n_links, int n_samples, long long threshold,
                             int *d_cluster                      /* [n_samples] */);

/* the kernels of the last call of either entry on this counter, first launch to last; -1.0 for a NULL counter and after a
 * refused call */
double tjamd_last_sample_linkage_ms (tjamd_counter *c);
double tjamd_last_linkage_clusters_ms (tjamd_counter *c);

#ifdef __cplusplus
}
#endif
#endif
