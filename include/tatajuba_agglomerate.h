/* tatajuba_agglomerate.h -- a second builder of the sample tree beside tatajuba_linkage.h: complete and average linkage.  The
 * sample x sample matrix of N14 agglomerated into a list of links that tjamd_linkage_clusters, tjamd_group_sites,
 * tjamd_linkage_tree and tjamd_clade_sites take as they take single linkage's.  Single linkage chains: one sample in between
 * joins two groups that are far apart, and the clades of such a tree are the chain's prefixes.  Under complete linkage two
 * groups are as far apart as their farthest pair, under average linkage as the mean of their pairs.  Same conventions as
 * tatajuba_amd.h (extern "C", plain pointers and sizes, a count or a negative TJAMD_ERR_* back, tjamd_last_error for the message,
 * which starts with the function's name).
 *
 * Reference interface replaced: none.  Neither the reference program nor its tutorial builds a tree.  N18 of DESIGN.md section
 * 3.5.
 */
#ifndef TATAJUBA_AGGLOMERATE_H
#define TATAJUBA_AGGLOMERATE_H

#include "tatajuba_linkage.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule of the tree (N18) ------------------------------------------------------------------------------------------
 * Input, edges and keys of pairs of samples: N15's (tatajuba_linkage.h), all of it.  d_dist[a * n_samples + b] as
 *   tjamd_sample_distances wrote it; a pair is an edge if and only if n_both >= min_both; the key of an edge by the metric
 *   (TJAMD_LINK_DIFFER, TJAMD_LINK_LENGTH, TJAMD_LINK_DIFFER_RATE) is the same 64-bit integer.
 * Clusters: at the start every sample is a cluster.  A cluster's id is its smallest member, its size the number of its members.
 * Distance of two clusters X != Y, with P (X, Y) the keys of all pairs (x in X, y in Y):
 *     if any of those pairs is no edge, X and Y have no edge: two groups join only if every pair across them has enough in
 *       common;
 *     otherwise, TJAMD_AGGL_COMPLETE  D (X, Y) = max P
 *                TJAMD_AGGL_AVERAGE   D (X, Y) = floor (sum P / (|X| * |Y|)); the sum is kept exactly in 64 bits, and the division
 *                                     is taken only where two distances are compared or a link is written, never stored.
 *   Under AVERAGE the key of a pair of samples stays below 2^40 (a larger one is refused): a sum over at most 2^22 pairs is then
 *   below 2^62.  The keys of DIFFER and DIFFER_RATE are 2^32 at most by construction.
 * A round: every live cluster X that has an edge to a live cluster picks nn (X), the live Y != X that minimises
 *   (D (X, Y), id (Y)); for one X that is the order of (D, smaller id, larger id) over the pairs of clusters, a strict total
 *   order.  All pairs with nn (X) = Y and nn (Y) = X merge in that round, all at once; the union keeps the smaller id.  The
 *   smallest pair under the total order is always mutual, so a round with an edge left merges at least one pair.  The rounds
 *   end when no live cluster has an edge.
 * Links: a merge is one tjamd_link: a the smaller of the two ids, b the larger (both are samples, members of the two
 *   clusters), key = D at the time of the merge.  d_links holds them ascending in (key, round, a, b); the round is not stored.
 *   Returns n_links; entries of d_links from n_links on are not written.  *h_n_rounds, if given, is the number of rounds that
 *   merged something.
 * Two properties:
 *   Keys ascend with the rounds.  Both linkages are reducible, D (X u Y, Z) >= min (D (X, Z), D (Y, Z)), and the floor keeps
 *     that, since the mean over the union lies between the two means: no later round merges below an earlier one's key.
 *   A cluster's own link comes before any link the cluster takes part in: by the key, and among equal keys by the round.
 *     tjamd_linkage_tree on the list therefore gives the dendrogram, and tjamd_linkage_clusters at a threshold T the
 *     dendrogram cut at T.  Ordering by (key, a, b) alone would be wrong under AVERAGE, where the union of two pairs that merged
 *     at keys 0 and 1 can itself merge at 1, with a smaller a than the pair it contains.
 * Without equal distances COMPLETE gives the textbook greedy tree (the smallest pair of all merges, one at a time).  With ties
 *   it is this rule and no other: a union takes the smaller id, so parallel rounds and a greedy loop can part ways at a tie.
 * Refused with TJAMD_ERR_ARG, from an error flag raised on the device by passes that read every cell and write nothing of the
 *   caller's (N13's idiom: d_links and *h_n_rounds are untouched by a refused call, and the timer reads -1.0 after one):
 *   everything tjamd_sample_linkage refuses (a cell, the diagonal included, with n_both < 0, n_differ < 0, n_differ > n_both or
 *   length_diff < 0; a cell one of whose three values differs from its mirror's); under AVERAGE a key of 2^40 or more.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter; a null d_dist; a null d_links with
 *   n_samples > 1; n_samples outside 1 .. 4096; a metric outside the three; min_both < 1; a linkage outside the two.  Then,
 *   without a device, TJAMD_ERR_NO_DEVICE.
 * n_samples == 1 returns 0 and launches nothing but the wait.  Changes none of its inputs nor the counter's finalised state.
 *   Two runs give the same bytes: every value is an integer maximum, sum, quotient or minimum under a total order, and the
 *   links are sorted at the end under an order that no two of them share.
 * The number of rounds depends on the data: a few dozen for keys without many ties, n_samples - 1 when all keys are equal
 *   (everyone's nearest neighbour is cluster 0, and one pair merges a round).  The rounds are launched without a look at the
 *   device; the call waits once per batch of 32 rounds, and at 64 samples and fewer, one workgroup in one launch, once.
 * Scratch, from the counter's block (it grows to the largest call and is kept): 8 bytes per cell of the matrix (128 MB at
 *   4096 samples), rewritten in place as clusters merge, and 44 bytes per sample; at 64 samples and fewer neither, the matrix
 *   is in LDS.  A call whose scratch cannot be had returns TJAMD_ERR_HIP.
 *
 * Not built: Ward; neighbour joining; a cache of nearest neighbours across rounds (every round reads the live matrix again);
 *   compaction of retired rows; averaging over the edges only; a tie rule that merges stars of equal keys in fewer rounds;
 *   bootstrap. */
enum { TJAMD_AGGL_COMPLETE = 1, TJAMD_AGGL_AVERAGE = 2 };

long tjamd_sample_agglomerate (tjamd_counter *c,
                               const tjamd_sample_distance *d_dist,  /* [n_samples * n_samples], as tjamd_sample_distances wrote it */
                               int n_samples, int metric, int min_both, int linkage,
                               tjamd_link *d_links,                  /* [n_samples - 1] */
                               int *h_n_rounds                       /* may be NULL: the rounds that merged */);

/* the kernels of the last call on this counter, first launch to last (the waits between batches included); -1.0 for a NULL
 * counter and after a refused call */
double tjamd_last_sample_agglomerate_ms (tjamd_counter *c);

#ifdef __cplusplus
}
#endif
#endif
