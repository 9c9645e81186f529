/* tatajuba_locate.h -- the second pass of the lookup on top of tatajuba_amd.h: rows that tjamd_locate left unlocated because
 * a flank differs from the genome by an indel, or because both flanks differ, are placed by a banded edit distance (N10).
 * Same conventions as tatajuba_amd.h (extern "C", plain pointers and sizes, a count or a negative TJAMD_ERR_* back,
 * tjamd_last_error for the message, which starts with the entry's name).
 *
 * Reference interface replaced:
 *   tjamd_locate_gapped       : find_reference_location_and_sort_hopo_counter (BWA, mismatch = nm)   src/hopo_counter.c:495-572
 *   tjamd_flank_edit_distance : distance_between_context_kmer_pair_with_edit_shift                   src/hopo_counter.c:81-113
 */
#ifndef TATAJUBA_LOCATE_H
#define TATAJUBA_LOCATE_H

#include "tatajuba_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TJAMD_MAX_SHIFT 3      /* the widest band: a flank may be shifted by up to three bases, as in the reference's rescan */

/* The distance.  The inner-first sequence of a packed flank starts at the base next to the tract: side = 0 is the ctx0
 * packing (inner base i at bits 2 (k - 1 - i)), side = 1 the ctx1 packing (inner base i at bits 2i).  For two inner-first
 * sequences q, r of length k and a band B = max_shift (0 ... TJAMD_MAX_SHIFT):
 *   D[0][0] = 0, D[i][0] = i, D[0][j] = j
 *   D[i][j] = min (D[i-1][j-1] + (q[i-1] != r[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)      over the cells with |i - j| <= B
 *   d_B (q, r) = the smallest D over the last row (D[k][j]) and the last column (D[i][k]) inside the band:
 * the unit-cost edit distance, anchored at the tract and free at the outer end.  The alignment uses up one of the two
 * flanks; the other may keep up to B unexplained outer bases, which stand for genome or read bases beyond the k stored.
 * d_0 is the number of differing positions (the distance of tjamd_locate); d_B is symmetric, does not grow with B and never
 * exceeds d_0; a flank made from a genome flank by one substitution, or by an insertion or deletion of s <= B bases, and cut
 * back to k bases with the genome's next bases, has d_B <= 1 or <= s.
 * A host function without a device call: it runs the arithmetic of the lookup kernel.  Bits of a and b above 2k are not
 * read.  k outside 1 ... 32, side outside 0 ... 1 or max_shift outside 0 ... TJAMD_MAX_SHIFT: -TJAMD_ERR_ARG. */
int tjamd_flank_edit_distance (uint64_t a, uint64_t b, int k, int side, int max_shift);

/* The seed order: a third order of the index, sorted by (base, ctx1 with its base order reversed, no complement), in which the
 * entries that share the inner bases of a row's ctx1 (its low bits) are a contiguous range, as those that share the inner
 * bases of ctx0 (its high bits) are in the order tjamd_reference_create builds.  Built on the device from the entries
 * already there (one kernel, one sort); 24 bytes per entry in a block of its own, freed by tjamd_reference_destroy.
 * tjamd_reference_create does not build it.  Returns the number of entries; a second call returns at once.  A counter of
 * another k or device is refused (TJAMD_ERR_ARG).  Waits once.  tjamd_reference_has_seeds: 1 once it is there, else 0. */
long tjamd_reference_add_seeds (tjamd_counter *c, tjamd_reference *ref);
int  tjamd_reference_has_seeds (const tjamd_reference *ref);

/* The lookup.  d_keys, n as in tjamd_locate.  d_loc (device tjamd_location[n]) is in and out: a row with flat >= 0 is left
 * byte for byte as it is, a row with flat < 0 (what tjamd_locate writes for a row without a hit) is tried.  With the seed
 * length h = (k + 1) / 2, an entry r is a hit for a row q when
 *   r.base == q.base,
 *   the inner h bases of ctx0 are equal or the inner h bases of ctx1 are equal (the seed), and
 *   d_B (q.ctx0, r.ctx0) + d_B (q.ctx1, r.ctx1) <= max_edits, B = max_shift.
 * The run length is free.  The row's location is the hit with the fewest total edits, then the smallest flat; mismatches =
 * that total; n_hits = distinct hit entries (one that passes both seeds counts once); ref_length, neg_strand, contig, pos are
 * that entry's.  No hit leaves the row as it was.  The minimum decides a value, never a place: the output is the same from
 * run to run.
 *   d_how (device int32[n], may be NULL): 0 for a row located before the call, 1 for one located by it, -1 for one still
 *   unlocated.
 * Returns the number of rows located by this call.  Refused with TJAMD_ERR_ARG: a null counter or reference, a reference of
 * another k or device, a reference without seeds, max_shift outside 0 ... TJAMD_MAX_SHIFT, max_edits outside 0 ... k, null
 * buffers with n > 0.  n = 0 returns 0 without a launch.  One launch, one wait.  Changes neither d_keys nor the reference
 * nor the counter's finalised state.
 * Out of scope: the seed is part of the rule, as "one flank exact" is part of tjamd_locate's -- an entry with an edit in
 * the inner half of both flanks is not a hit; the signed shift is not an output (the reference's best_shift has no consumer
 * here); tjamd_tract_variants compares the flanks of a row located with a shifted flank as it already does for rows joined
 * by the indel retry of tjamd_union_tracts. */
long tjamd_locate_gapped (tjamd_counter *c, const tjamd_reference *ref, const void *d_keys, long n, int max_edits, int max_shift,
                          tjamd_location *d_loc, int *d_how);

double tjamd_last_seed_order_ms (tjamd_counter *c);        /* kernels of the last tjamd_reference_add_seeds that built an order (-1.0 for a NULL counter) */
double tjamd_last_locate_gapped_ms (tjamd_counter *c);     /* the lookup kernel of the last tjamd_locate_gapped (-1.0 for a NULL counter) */

#ifdef __cplusplus
}
#endif
#endif
