/* tatajuba_clades.h -- the step behind tatajuba_groups.h: which sites hold each branch of the sample tree together, without a
 * cut.  The links of N15 become a tree with nodes, children and a leaf order, and the site x sample genotype matrix of N13 (or
 * N12) is read once by every inner node of that tree: per site and node whether the called samples of the node's clade all
 * carry one genotype, how many called samples outside the clade carry it too, and the short list of (site, node) pairs where
 * nobody outside does: the sites that support the branch.  Same conventions as tatajuba_amd.h (extern "C", plain pointers and
 * sizes, a count or a negative TJAMD_ERR_* back, tjamd_last_error for the message, which starts with the function's name).
 *
 * Reference interface replaced: none.  The reference program ends at per-sample VCFs and builds no tree; here the tree and the
 * matrix are on the device, the clades of a tree of 4096 samples cover a sample up to 4095 times, and the answer is a short
 * list.  N17 of DESIGN.md section 3.5.
 */
#ifndef TATAJUBA_CLADES_H
#define TATAJUBA_CLADES_H

#include "tatajuba_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule of the tree (N17) ------------------------------------------------------------------------------------------
 * Input: n_links links over n_samples samples, in the order given: tjamd_sample_linkage's output as it stands, or any list
 *   without a cycle.  Of a link a and b are read; key is not read.
 * Nodes: link j joins the component that holds a and the one that holds b, as the links 0 .. j - 1 left them.  Node j is
 *   that union: there are n_links nodes, and a later node is never a child of an earlier one.
 * Children: a child >= 0 is the earlier node that was that component; a child < 0 is the single sample -1 - child.  left is
 *   the child whose smallest member is smaller, whichever of a and b it holds.
 * Leaf order: the roots -- the nodes that no later link joins, and the samples in no link -- are laid out ascending by
 *   smallest member; inside a node the order is left, then right.  d_order[p] is the sample at position p.
 * Intervals: first and size say that node j's clade is d_order[first .. first + size).  It follows that d_order[first] is the
 *   clade's smallest member, that d_order[0] == 0, and that the intervals of two nodes are disjoint or nested.
 * Returns n_links.  n_links == 0 writes the identity order and no node.
 * Refused with TJAMD_ERR_ARG, from an error flag raised on the device before anything of the caller's is written (N13's
 *   idiom: d_nodes and d_order are untouched by a refused call, and the timer reads -1.0 after one): a link with a < 0,
 *   a >= b or b >= n_samples; a link whose ends are already joined by the links before it, which is a cycle.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter; a null d_order; null d_links or
 *   d_nodes with n_links > 0; n_links < 0 or n_links > n_samples - 1; n_samples outside 1 .. 4096.  Then, without a device,
 *   TJAMD_ERR_NO_DEVICE.
 * Changes none of its inputs nor the counter's finalised state.  Waits once, at the end.  Every value is an index, a count or
 *   a minimum of integers, formed in the order of the list: two runs give the same bytes.
 *
 * ---- the rule of the clade sites -------------------------------------------------------------------------------------------
 * Input: d_sites and d_genotype[site * n_samples + s] as tjamd_merge_variants or tjamd_site_depths wrote them (-1: not called;
 *   0: the genome's own length; a > 0: the site's a-th allele); of a site only n_alleles is read.  d_order is a permutation
 *   of 0 .. n_samples - 1.  Of a node only first and size are read: its clade is the samples d_order[first .. first + size).
 *   Any set of intervals over any permutation is valid input, nested or not; d_nodes and d_order of tjamd_linkage_tree, with
 *   its return value as n_nodes, are valid as they stand.  Every sample takes part.
 * Per site i and node j (d_calls[i * n_nodes + j]): the called members are the samples of j's clade with a genotype g >= 0
 *   at i.
 *     n_called   the number of called members
 *     fixed      the one genotype they all carry; -1 if none is called, -2 if they carry more than one
 *     n_outside  the number of called samples outside the clade that carry `fixed`; 0 when fixed < 0
 *     mark       1 if and only if fixed >= 0, n_called >= min_called, n_outside == 0 and at least one sample outside the
 *                clade is called at i; otherwise 0.  A node that covers every sample is therefore never marked.
 * Per site (d_site_out[i]): n_called counts the called samples, n_genotypes the distinct genotypes among them, n_marks the
 *   nodes marked there, first_group the smallest such node or -1.
 * d_node_marks[j] is the number of sites at which node j is marked.
 * d_marks holds the marked (site, node) pairs, ascending in (site, node), each with the fixed genotype and the clade's
 *   n_called.  The three records are N16's: the field `group` holds the node, `first_group` the first marked node.
 * Returns the number of marks and sets *h_n_marks.  More marks than mark_capacity is -TJAMD_ERR_CAPACITY: nothing is written
 *   at or beyond the capacity, what lies below it is in its place, the other three outputs are complete and *h_n_marks is set,
 *   so that a caller may size with capacity 0 and call again.
 * Refused with TJAMD_ERR_ARG, from an error flag raised on the device by a first pass that reads everything and writes nothing
 *   of the caller's (no output is touched by a refused call, *h_n_marks is left alone, and the timer reads -1.0 after one):
 *   d_order is not a permutation of 0 .. n_samples - 1; a node with size < 2, first < 0 or first + size > n_samples; a site
 *   with n_alleles < 1 or n_alleles > n_samples; a genotype cell below -1 or above its site's n_alleles.
 * Refused on the host, before a device is looked for, with TJAMD_ERR_ARG: a null counter; n_sites < 0; null d_sites or
 *   d_genotype with n_sites > 0; a null d_order; a null d_nodes with n_nodes > 0; n_samples outside 1 .. 4096; n_nodes
 *   outside 0 .. 4096; min_called < 1; mark_capacity < 0; a null d_marks with a capacity above 0; n_sites * n_samples >= 2^31;
 *   with d_calls given, n_sites * n_nodes >= 2^31.  Then, without a device, TJAMD_ERR_NO_DEVICE.
 * n_sites == 0 or n_nodes == 0 returns 0, sets *h_n_marks to 0, zeroes d_node_marks with a memset and launches no kernel.
 * Changes none of its inputs nor the counter's finalised state.  Waits once, at the end.  Every value is a count or a minimum
 *   of integers and the list's places come from a scan: two runs give the same bytes.  The cost of a node does not depend on
 *   the tree's depth: a clade is an interval of the leaf order, and its record comes from prefix counts over that order.
 * Scratch, from the counter's block (it grows to the largest call and is kept): the error and count words (one per node
 *   among them) and one int per site (its marks, then their offsets).  A call whose scratch cannot be had returns TJAMD_ERR_HIP.
 *
 * Not built: leaves as nodes (a sample's private alleles are N16 with the identity labelling); samples left out; weights;
 *   marks that allow a share of exceptions; read depths; bootstrap support; other linkages. */
typedef struct { int left, right, first, size; } tjamd_tree_node;   /* 16 bytes, per link */

long tjamd_linkage_tree (tjamd_counter *c, const tjamd_link *d_links, long n_links, int n_samples,
                         tjamd_tree_node *d_nodes        /* [n_links] */,
                         int *d_order                    /* [n_samples] */);

long tjamd_clade_sites (tjamd_counter *c,
                        const tjamd_site *d_sites, long n_sites,
                        const int16_t *d_genotype,      /* [n_sites * n_samples], site-major: N13's or N12's */
                        int n_samples,
                        const tjamd_tree_node *d_nodes, int n_nodes,
                        const int *d_order,             /* [n_samples]: the sample at each leaf position */
                        int min_called,
                        tjamd_group_call *d_calls,      /* [n_sites * n_nodes], site-major; may be NULL */
                        tjamd_group_site *d_site_out,   /* [n_sites]; may be NULL */
                        int *d_node_marks,              /* [n_nodes]: marks per node; may be NULL */
                        tjamd_group_mark *d_marks, long mark_capacity,   /* may be NULL with capacity 0 */
                        long *h_n_marks                 /* may be NULL */);

/* the kernels of the last call of either entry on this counter, first launch to last; -1.0 for a NULL counter and after a
 * call that did not return a count */
double tjamd_last_linkage_tree_ms (tjamd_counter *c);
double tjamd_last_clade_sites_ms (tjamd_counter *c);

#ifdef __cplusplus
}
#endif
#endif
