/* tatajuba_bootstrap.h -- the step behind tatajuba_agglomerate.h and tatajuba_clades.h: how far each clade of the sample tree is
 * to be believed.  The bootstrap over sites: integer weights per site drawn with replacement, the sample x sample matrix of N14
 * under every replicate's weights in one call, and, once the caller has built every replicate's tree with the entries that
 * exist, the number of replicates in which each clade of the tree appears again.  The headers before this one list "bootstrap"
 * and "a site list or mask; weights" as not built; they are built here, and those headers stay as they were written.  A site
 * mask is the weighted matrix under weights of 0 and 1.  Same conventions as tatajuba_amd.h (extern "C", plain pointers and
 * sizes, a count or a negative TJAMD_ERR_* back, tjamd_last_error for the message, which starts with the function's name).
 *
 * Reference interface replaced: none.  Neither the reference program nor its tutorial builds a tree or resamples anything.
 * N19 of DESIGN.md section 3.5.
 */
#ifndef TATAJUBA_BOOTSTRAP_H
#define TATAJUBA_BOOTSTRAP_H

#include "tatajuba_agglomerate.h"
#include "tatajuba_clades.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule of the weights (N19) ---------------------------------------------------------------------------------------
 * All arithmetic is unsigned 64-bit and wraps.
 *     mix (z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *     base_r = mix (seed + 0x9E3779B97F4A7C15 * (r + 1))                  for replicate r
 *     h      = mix (base_r + j)                                           for its draw j = 0 .. n_sites - 1
 *     the draw picks site ((h >> 32) * n_sites) >> 32
 *   d_weights[r * n_sites + i] is the number of draws of replicate r that picked site i.
 * Every replicate sums to n_sites, and replicate r does not depend on n_replicates: a longer call has a shorter one as its
 *   prefix.  With n_sites = 7 and seed = 1 the replicates 0 .. 2 are 3 0 1 0 1 0 2, 2 0 1 1 1 1 1 and 1 0 1 3 1 1 0.
 * Returns n_replicates.  One memset and one kernel that counts with integer atomic adds: the sums do not depend on their
 *   order, and two runs give the same bytes.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter; a null d_weights; n_sites < 1 or
 *   n_sites >= 2^31; n_replicates outside 1 .. 4096; n_replicates * n_sites >= 2^31.  Then, without a device,
 *   TJAMD_ERR_NO_DEVICE.  Nothing is refused on the device.
 *
 * ---- the rule of the weighted distances ------------------------------------------------------------------------------------
 * Inputs: those of tjamd_sample_distances (tatajuba_distances.h), all of them, and d_weights[r * n_sites + i], the weight of
 *   site i in replicate r: that of tjamd_bootstrap_weights, or any the caller writes (0 and 1: a site mask; a jackknife).
 * For replicate r this is N14's rule with every site's contribution multiplied by w = d_weights[r * n_sites + i]:
 *     n_both       the sum of w over the sites where g_a >= 0 and g_b >= 0
 *     n_differ     the sum of w over those of them where g_a != g_b
 *     length_diff  the sum of w * |L(g_a) - L(g_b)| over them, formed exactly in 64 bits
 * Output: d_out[(r * n_samples + a) * n_samples + b].  Each replicate's matrix is full and symmetric, with N14's diagonal
 *   (n_both the weighted number of sites at which the sample is called): it is valid input to tjamd_sample_linkage and
 *   tjamd_sample_agglomerate as it stands.  With one replicate whose weights are all 1 the bytes are tjamd_sample_distances'.
 * Returns n_sites.  n_sites == 0 zeroes all of d_out with a memset, launches no kernel and returns 0.
 * Refused with TJAMD_ERR_ARG, from an error flag raised on the device by first passes that read everything and write nothing
 *   of the caller's (N13's idiom: d_out is untouched by a refused call, and the timer reads -1.0 after one): everything
 *   tjamd_sample_distances refuses, whatever the weights (a bad cell in a site of weight 0 is still refused: the check reads
 *   every cell); a weight below 0; a replicate whose weights sum to 2^31 or more.  Below that sum n_both fits an int and
 *   length_diff stays under 2^62.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: what tjamd_sample_distances refuses there; a null
 *   d_weights with n_sites > 0; n_replicates outside 1 .. 4096; n_replicates * n_sites >= 2^31.  Then, without a device,
 *   TJAMD_ERR_NO_DEVICE.
 * Changes none of its inputs nor the counter's finalised state.  Waits once, at the end.  No atomic reaches global memory but
 *   the error flag's, and where the sites are split over workgroups their partial tiles are summed in a fixed order, as in
 *   N14: two runs give the same bytes.
 * A workgroup stages a chunk of genotypes once and walks it for two replicates; the replicates beyond two lie in the grid.
 * Scratch, from the counter's block (it grows to the largest call and is kept): N14's 4 bytes per genotype cell; and, only
 *   where the sites are split, one tile of 16-byte sums per workgroup and replicate (128 MB at most on 256 compute units).
 *   A call whose scratch cannot be had returns TJAMD_ERR_HIP.
 *
 * ---- the rule of the clade support -----------------------------------------------------------------------------------------
 * Input: the tree whose clades are asked about, d_nodes / n_nodes over d_order, as tjamd_clade_sites takes it; and per
 *   replicate r the nodes d_rep_nodes[r * (n_samples - 1) + k] for k < h_rep_n_nodes[r], which lie over the order
 *   d_rep_order[r * n_samples ..].  h_rep_n_nodes is host memory.  Of a node only first and size are read: node j's clade is
 *   the set d_order[first .. first + size).  Any intervals over any permutation are valid, nested or not: forests are fine.
 * d_support[j] is the number of replicates in which some node's set equals node j's set.  A replicate with two equal nodes
 *   counts once.  A set equals an interval of a replicate's order exactly when the positions of its members in that order
 *   span `size` and the replicate has a node at that (first, size).
 * Returns n_nodes.  n_nodes == 0 returns 0 and launches no kernel.
 * The trees of the replicates come from the entries that exist: tjamd_sample_linkage or tjamd_sample_agglomerate on a
 *   replicate's slice of the weighted matrices, then tjamd_linkage_tree, per replicate.
 * Refused with TJAMD_ERR_ARG, from an error flag raised on the device by a first pass that writes nothing of the caller's
 *   (d_support is untouched by a refused call, and the timer reads -1.0 after one): an order, the base's or a replicate's,
 *   that is not a permutation of 0 .. n_samples - 1; a node, of the base or among a replicate's first h_rep_n_nodes[r], with
 *   size < 2, first < 0 or first + size > n_samples.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter; null d_order, d_rep_order or
 *   h_rep_n_nodes; null d_nodes or d_support with n_nodes > 0; a null d_rep_nodes while some replicate has a node;
 *   n_samples outside 1 .. 4096; n_nodes outside 0 .. 4096; n_replicates outside 1 .. 4096; a count in h_rep_n_nodes
 *   outside 0 .. n_samples - 1.  Then, without a device, TJAMD_ERR_NO_DEVICE.
 * Changes none of its inputs nor the counter's finalised state.  Waits once, at the end.  The counts are integer sums: two
 *   runs give the same bytes.
 * Scratch, from the counter's block: one int per node and per replicate, and the flag words.
 *
 * Not built: a batched tree builder (the caller runs the tree entries per replicate); jackknife or other resampling schemes
 *   as entries of their own (a caller writes such weights itself); real-valued weights; support written into the Newick file;
 *   MFMA for the 0/1 quantities. */
long tjamd_bootstrap_weights (tjamd_counter *c, long n_sites, int n_replicates, unsigned long long seed,
                              int *d_weights                      /* [n_replicates * n_sites] */);

long tjamd_sample_distances_weighted (tjamd_counter *c,
                                      const tjamd_site *d_sites, long n_sites, const tjamd_allele *d_alleles, long n_alleles,
                                      const int16_t *d_genotype,  /* [n_sites * n_samples], site-major */
                                      int n_samples,
                                      tjamd_sample_distance *d_out /* [n_replicates * n_samples * n_samples] */,
                                      const int *d_weights        /* [n_replicates * n_sites] */,
                                      int n_replicates);

long tjamd_clade_support (tjamd_counter *c,
                          const tjamd_tree_node *d_nodes, int n_nodes,
                          const int *d_order,                     /* [n_samples] */
                          int n_samples,
                          const tjamd_tree_node *d_rep_nodes      /* [n_replicates * (n_samples - 1)] */,
                          const int *d_rep_order                  /* [n_replicates * n_samples] */,
                          const int *h_rep_n_nodes                /* host, [n_replicates] */,
                          int n_replicates,
                          int *d_support                          /* [n_nodes] */);

/* the kernels of the last call of each entry on this counter, first launch to last; -1.0 for a NULL counter and after a
 * refused call */
double tjamd_last_bootstrap_weights_ms (tjamd_counter *c);
double tjamd_last_sample_distances_weighted_ms (tjamd_counter *c);
double tjamd_last_clade_support_ms (tjamd_counter *c);

#ifdef __cplusplus
}
#endif
#endif
