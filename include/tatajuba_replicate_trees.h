/* tatajuba_replicate_trees.h -- the step between tjamd_sample_distances_weighted and tjamd_clade_support of
 * tatajuba_bootstrap.h: the trees of all bootstrap replicates in one call.  tatajuba_bootstrap.h lists "a batched tree builder"
 * as not built and tells the caller to run the tree entries per replicate; it is built here, and that header stays as it was
 * written.  Same conventions as tatajuba_amd.h (extern "C", plain pointers and sizes, a count or a negative TJAMD_ERR_* back,
 * tjamd_last_error for the message, which starts with the function's name).
 *
 * Reference interface replaced: none.  Neither the reference program nor its tutorial builds a tree or resamples anything.
 * N20 of DESIGN.md section 3.5.
 */
#ifndef TATAJUBA_REPLICATE_TREES_H
#define TATAJUBA_REPLICATE_TREES_H

#include "tatajuba_bootstrap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the third linkage, beside TJAMD_AGGL_COMPLETE = 1 and TJAMD_AGGL_AVERAGE = 2 of tatajuba_agglomerate.h: the single-linkage
 * forest of tatajuba_linkage.h */
enum { TJAMD_TREE_SINGLE = 0 };

/* ---- the rule of the replicate trees (N20) ---------------------------------------------------------------------------------
 * Input: d_dist[(r * n_samples + a) * n_samples + b], the matrices of n_replicates replicates as
 *   tjamd_sample_distances_weighted wrote them; metric and min_both as tjamd_sample_linkage takes them; linkage one of
 *   TJAMD_TREE_SINGLE, TJAMD_AGGL_COMPLETE, TJAMD_AGGL_AVERAGE.
 * For every replicate r the call gives what the per-replicate loop of the existing entries gives, byte for byte:
 *   d_rep_links[r * (n_samples - 1) ..] and h_rep_n_nodes[r] are the links and the return value of the builder on replicate
 *     r's slice of d_dist: tjamd_sample_linkage under TJAMD_TREE_SINGLE, tjamd_sample_agglomerate under the other two.
 *     d_rep_links may be NULL: the links are then not handed out.
 *   h_rep_n_rounds[r] is what that builder returns through *h_n_rounds; under TJAMD_TREE_SINGLE it is 0.  May be NULL.
 *   d_rep_nodes[r * (n_samples - 1) ..] and d_rep_order[r * n_samples ..] are the nodes and the leaf order that
 *     tjamd_linkage_tree gives on those links.
 *   Entries past a replicate's n_nodes are not written: replicates that are forests of different sizes share one call.
 * The outputs are the arrays tjamd_clade_support takes, as they stand.
 * Single linkage's forest is unique under the total order (key, a, b), and it is stored sorted by that order.  The two
 *   agglomerative linkages are the round rule of tatajuba_agglomerate.h and no other: (key, round, a, b).
 * Returns n_replicates.  n_samples == 1 writes the identity orders (one 0 per replicate) and zero counts with one memset and
 *   no kernel, and returns n_replicates.
 * Refused with TJAMD_ERR_ARG, from an error word raised on the device by a check pass over all replicates that runs before
 *   anything of the caller's is stored: a bad cell in any replicate refuses the whole call.  A bad cell is anything
 *   tjamd_sample_linkage refuses on the device (a cell's values; a cell that differs from its mirror) and, under
 *   TJAMD_AGGL_AVERAGE, a key of 2^40 or more.  Nothing of the caller's is written then, on the device or the host, for the
 *   replicates before the bad one either, and the timer reads -1.0.  The message carries the text of tjamd_sample_linkage /
 *   tjamd_sample_agglomerate for the first broken rule in their order, and names the smallest refused replicate.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter, d_dist, d_rep_order or
 *   h_rep_n_nodes; a null d_rep_nodes with n_samples > 1; n_samples outside 1 .. 4096; n_replicates outside 1 .. 4096; a
 *   metric outside the three; min_both < 1; a linkage outside 0 .. 2.  Then, without a device, TJAMD_ERR_NO_DEVICE.
 * Changes none of its inputs nor the counter's finalised state.  Two runs give the same bytes.
 * Launches and waits: up to 64 samples a check pass and one kernel, a workgroup per replicate that does the rounds, the sort,
 *   the tree and the leaf order in LDS: two launches and one wait, whatever n_replicates is.  Beyond, the kernels of
 *   tjamd_sample_linkage and tjamd_sample_agglomerate take the replicate from the grid, and a workgroup per replicate builds
 *   the tree behind them: the launches of one replicate, not n_replicates times as many; under the agglomerative linkages
 *   the call waits once per batch of rounds, for all replicates together, and enqueues the rounds of the slowest replicate.
 * Replicate groups: the replicates go through in groups of as many as 1 GiB of scratch holds (8 bytes a cell of a key
 *   matrix: 128 MB a replicate at 4096 samples), at least one.
 * Scratch, from the counter's block (it grows to the largest call and is kept): per replicate of a group what
 *   tjamd_sample_linkage or tjamd_sample_agglomerate cuts, and its links; 32 bytes of flag words per replicate of the call.
 *   A call whose scratch cannot be had returns TJAMD_ERR_HIP.
 *
 * Not built: a parallel walk of one replicate's tree (one lane steps through a replicate's links, as in tjamd_linkage_tree;
 *   the replicates run side by side); replicates of different n_samples in one call; the base tree in the same call (it is
 *   one more replicate with weights of 1); support written into the Newick file; Ward and neighbour joining. */
long tjamd_replicate_trees (tjamd_counter *c,
                            const tjamd_sample_distance *d_dist    /* [n_replicates * n_samples * n_samples] */,
                            int n_samples, int n_replicates, int metric, int min_both, int linkage,
                            tjamd_link *d_rep_links                /* [n_replicates * (n_samples - 1)]; may be NULL */,
                            tjamd_tree_node *d_rep_nodes           /* [n_replicates * (n_samples - 1)] */,
                            int *d_rep_order                       /* [n_replicates * n_samples] */,
                            int *h_rep_n_nodes                     /* host, [n_replicates] */,
                            int *h_rep_n_rounds                    /* host, [n_replicates]; may be NULL */);

/* the kernels of the last call on this counter, first launch to last; -1.0 for a NULL counter and after a refused call */
double tjamd_last_replicate_trees_ms (tjamd_counter *c);

#ifdef __cplusplus
}
#endif
#endif
