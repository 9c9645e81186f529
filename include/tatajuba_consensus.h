/* tatajuba_consensus.h -- the step behind tatajuba_replicate_trees.h: what the bootstrap replicates agree on among themselves.
 * tjamd_clade_support counts the replicates that hold each clade of a tree it is handed; here every clade of every replicate is
 * put into its class of equal sets, every class is counted, and the classes that a majority of the replicates hold are
 * assembled into the majority-rule consensus tree, each inner node with its count.  tatajuba_bootstrap.h and
 * tatajuba_replicate_trees.h list "support written into the Newick file" as not built; the consensus tree carries it
 * (examples/merged_vcf.c -K), and those headers stay as they were written.  Same conventions as tatajuba_amd.h (extern "C",
 * plain pointers and sizes, a count or a negative TJAMD_ERR_* back, tjamd_last_error for the message, which starts with the
 * function's name).
 *
 * Reference interface replaced: none.  Neither the reference program nor its tutorial builds a tree or resamples anything.
 * N21 of DESIGN.md section 3.5.
 */
#ifndef TATAJUBA_CONSENSUS_H
#define TATAJUBA_CONSENSUS_H

#include "tatajuba_replicate_trees.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A node of the consensus tree.  first and size sit where tjamd_tree_node has them, and tjamd_clade_sites and
 * tjamd_clade_support read nothing else of a node: the consensus nodes, cast to tjamd_tree_node, are valid input to both as
 * they stand, over d_order. */
typedef struct { int parent, count, first, size; } tjamd_consensus_node;   /* 16 bytes */

/* ---- the rule of the consensus tree (N21) -----------------------------------------------------------------------------------
 * All of it is integer work: the result is fixed to the byte.
 * Input: exactly what tjamd_clade_support takes for the replicates, which is what tjamd_replicate_trees writes: per replicate r
 *   the nodes d_rep_nodes[r * (n_samples - 1) + k] for k < h_rep_n_nodes[r] over the order d_rep_order[r * n_samples ..].
 *   h_rep_n_nodes is host memory.  Of a node only first and size are read.  The clade of node k of replicate r is the set
 *   d_rep_order[r * n_samples + first .. + size).  Forests are fine, so are replicates with 0 nodes and nodes of size n_samples.
 * Classes: two clades are equal if and only if they are the same set of samples; the replicate, the position and the order
 *   they lie in do not matter.  A class is one distinct set.  A class's count is the number of replicates that have at least one
 *   node with that set: two equal nodes of one replicate count once.  *h_n_classes is the number of classes.
 *   d_rep_count[r * (n_samples - 1) + k], for k < h_rep_n_nodes[r], is the count of the class of that node; entries past a
 *   replicate's count are not written.  d_rep_count is the all-against-all form of tjamd_clade_support: what n_replicates
 *   calls of it give, each with another replicate as the base.
 * Consensus: a class is kept if and only if count >= min_count.  The host requires 2 * min_count > n_replicates and
 *   min_count <= n_replicates.  Every replicate's nodes are required to be laminar (below); two kept classes then share a
 *   replicate, so they are nested or disjoint, and there are at most n_samples - 1 of them.  min_count == n_replicates gives
 *   the strict consensus.
 * Nodes: the kept classes, ascending in (size, smallest member): a total order, and a child always comes before its parent.
 *   The call returns their number.  parent is the index of the smallest kept class that strictly contains the node, or -1;
 *   count is the class's count.  Entries of d_nodes from the return value on are not written.
 * Leaf order: the children of a node are its child nodes and those of its samples that lie in no child; the roots are the
 *   nodes with parent == -1 together with the samples that lie in no node.  Children are laid out ascending by smallest member,
 *   roots the same way.  d_order[p] is the sample at position p, and node j's clade is d_order[first .. first + size).  It
 *   follows that d_order[first] is the clade's smallest member and that d_order[0] == 0.
 * Degenerate cases: n_samples == 1 writes d_order[0] = 0 and *h_n_classes = 0, returns 0 and launches no kernel (the timer
 *   reads -1.0).  If no replicate has a node, the call writes the identity order, returns 0, and *h_n_classes = 0.
 * Exactness: equality of clades is set equality and rests on no hash.  A clade's key is (size, the low 51 bits of the wrapping
 *   64-bit sum of mix (salt + sample) over its members), mix being that of tatajuba_bootstrap.h; the sum comes from a prefix sum
 *   over the replicate's order.  The clades are sorted by that key.  Inside a run of equal keys every clade is compared with
 *   the run's leader as a set, by the test tjamd_clade_support uses: a set equals an interval of replicate r's order exactly
 *   when the positions of its members in that order span `size`.  The clades that differ from the leader stay behind, the
 *   first of them leads the next round, until none is left: they form further classes of the same run.
 *   TATAJUBA_AMD_CONSENSUS_KEY_BITS = b (0 .. 51, read when the counter is made, for tests) keeps only the low b bits of the
 *   sum: with b = 0 every clade of a size lies in one run and everything is decided by comparison.  Every output is the same
 *   bytes under any b.
 * Refused with TJAMD_ERR_ARG, from error words raised on the device by a first pass that writes nothing of the caller's (N13's
 *   idiom: no output is touched by a refused call, *h_n_classes is left alone and the timer reads -1.0 after one): a
 *   replicate's order that is not a permutation of 0 .. n_samples - 1; a node among a replicate's first h_rep_n_nodes[r] with
 *   size < 2, first < 0 or first + size > n_samples; two nodes of one replicate that cross, meaning their intervals overlap
 *   and neither contains the other.  The message names the smallest refused replicate and the first broken rule in this order.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter, d_rep_order, h_rep_n_nodes or
 *   d_order; a null d_nodes with n_samples > 1; a null d_rep_nodes while some replicate has a node; n_samples or n_replicates
 *   outside 1 .. 4096; a count in h_rep_n_nodes outside 0 .. n_samples - 1; min_count outside the range above.  Then, without
 *   a device, TJAMD_ERR_NO_DEVICE.
 * Changes none of its inputs nor the counter's finalised state.  Two runs give the same bytes: no output depends on the order
 *   in which an atomic operation lands (they are integer minima, sums and ORs), and the kept classes are ordered by a total
 *   order.
 * Launches and waits: a workgroup per replicate checks it, stores the positions of its samples and emits a (key, index) pair per
 *   node; the shared key-value sort (eight passes); the runs; per round a wavefront per unsettled clade compares it with its
 *   run's leader, and the host looks at one word: one round and one wait where no two different sets share a key, one more per
 *   further class of the fullest run; the counts; then the kept classes, at most n_samples - 1: a wavefront each finds its
 *   smallest member and its parent, one workgroup orders them, and one workgroup lays the leaves out in LDS (one lane walks
 *   the samples once and the nodes once, as in tjamd_linkage_tree).  One more wait at the end.
 * Cost of the exact comparison: a clade that is not its run's leader costs `size` loads.  Balanced trees of n samples cost
 *   n log2 n per replicate; a caterpillar, the worst case, n * n / 2.
 * Scratch, from the counter's block (it grows to the largest call and is kept): 44 bytes per clade of the call (two halves of
 *   8-byte keys and 4-byte indices for the sort, five words for the runs, the classes and the counts) and the sort's
 *   histograms (1 KB per 1024 clades); per replicate 2 bytes per sample (positions) and 12 bytes; 56 bytes per sample for
 *   the kept classes.  A call whose scratch cannot be had returns TJAMD_ERR_HIP.
 *
 * Not built: extended (greedy) consensus below 50 %; branch lengths on the consensus; Robinson-Foulds distances between
 *   replicates; the base tree inside the same call; Ward and neighbour joining; any change to an existing entry. */
long tjamd_consensus_tree (tjamd_counter *c,
                           const tjamd_tree_node *d_rep_nodes   /* [n_replicates * (n_samples - 1)] */,
                           const int *d_rep_order               /* [n_replicates * n_samples] */,
                           const int *h_rep_n_nodes             /* host, [n_replicates] */,
                           int n_samples, int n_replicates, int min_count,
                           tjamd_consensus_node *d_nodes        /* [n_samples - 1] */,
                           int *d_order                         /* [n_samples] */,
                           int *d_rep_count                     /* [n_replicates * (n_samples - 1)]; may be NULL */,
                           long *h_n_classes                    /* may be NULL */);

/* the kernels of the last call on this counter, first launch to last; -1.0 for a NULL counter and after a refused call */
double tjamd_last_consensus_tree_ms (tjamd_counter *c);

#ifdef __cplusplus
}
#endif
#endif
