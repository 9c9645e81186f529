/* tatajuba_features.h -- the annotation step on top of tatajuba_amd.h: the features of a GFF3 file, the feature each located
 * tract lies in, and the longest modal tract length over the samples.  Same conventions as tatajuba_amd.h (extern "C",
 * plain pointers and sizes, a count or a negative TJAMD_ERR_* back, tjamd_last_error for the message, which starts with
 * the function's name).
 *
 * Reference interface replaced:
 *   tjamd_tract_features : genomic_context_find_features()                               src/context_histogram.c:331-351
 *                          max_length of create_tract_in_reference_structure()           src/genome_set.c:492,502-503
 */
#ifndef TATAJUBA_FEATURES_H
#define TATAJUBA_FEATURES_H

#include "tatajuba_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the GFF3 reader (host only) ---------------------------------------------------------------------------------------
 * One tjamd_feature per feature line of a GFF3 file, plain, gzip or BGZF (decoded by tj_inflate.c, the decoder of the
 * feeder; no zlib).
 *   Lines: a line that starts with '#' is skipped, but "##FASTA", like a line that starts with '>', ends the features; blank
 *     lines are skipped; one trailing '\r' is dropped; a last line without '\n' counts.
 *   Columns: nine, separated by tabs.  contig = the index of column 1 among contig_names, compared byte for byte;
 *     contig_names is what tjamd_read_file_names writes: n_contigs names, each followed by '\n'.  start, end = columns 4 and 5,
 *     decimal, 1-based inclusive.  cls = TJAMD_FEATURE_REGION or TJAMD_FEATURE_CDS if column 3 equals "region" or "cds"
 *     without regard to ASCII case, else TJAMD_FEATURE_OTHER.  strand = 0 for "+", 1 for "-", 2 for anything else.
 *     line = the 1-based number of the line in the file.  type_off, id_off = offsets in `strings` of two NUL-terminated
 *     strings: column 3, and the value of ID= in column 9 -- the bytes behind "ID=" at the start of the column or right behind
 *     a ';', up to the next ';' or the end of the column, percent escapes left as they are; empty if there is no ID=.
 *     A feature of several lines (the parts of one CDS) is one feature per line.
 *   Skipped and counted in *n_skipped, not refused: a line of fewer than nine columns, a seqid that is not among the names,
 *     a start or an end that is not a decimal number (or is beyond 2^31 - 1), start < 1, end < start.
 *   Not built: the sequences of an embedded ##FASTA section are not extracted; the caller has the FASTA file.
 * Returns the number of features; -1 if the file cannot be opened or is not what its gzip header says.  Two calls, as with
 * tjamd_read_file_names: out = NULL or strings = NULL only sizes (the count back, *strings_bytes = the bytes the strings need);
 * otherwise records and strings are written when BOTH capacities suffice and nothing is written when one does not.
 * strings_bytes and n_skipped may be NULL. */
enum { TJAMD_FEATURE_REGION = 0, TJAMD_FEATURE_CDS = 1, TJAMD_FEATURE_OTHER = 2 };
typedef struct { int contig, start, end, cls, strand, line, type_off, id_off; } tjamd_feature;     /* 32 bytes */
long tjamd_gff3_read (const char *path, const char *contig_names, long n_contigs, tjamd_feature *out, long capacity,
                      char *strings, long strings_capacity, long *strings_bytes, long *n_skipped);

/* ---- the annotation (N9; reference: genomic_context_find_features, src/context_histogram.c:331-351) ---------------------
 * For each located histogram the reference asks biomcmc-lib's find_gff3_fields_within_position for the features that contain
 * the tract's first base (loc2d[1] + kmer_size, :341), walks them, skips `region` features, keeps the last one seen and
 * stops at the first CDS (:343-347).  biomcmc-lib is absent from the reference tree; the reading built here, which the tests
 * pin, takes the containing features in file order:
 *   Containment: feature f contains a tract located at (contig, pos) when f.contig == contig and f.start <= pos + 1 <= f.end
 *     (pos is the 0-based first base of the run, as tjamd_locate writes it; start and end are 1-based inclusive).
 *   Winner: the first CDS (in file order) that contains the tract; if no CDS contains it, the last feature that is not a
 *     region and contains it; region features never count.  -1: an unlocated tract (flat < 0), or one that nothing contains.
 *
 * tjamd_annotation is an elementary-interval table on the device.  Every feature that is not a region gives two points,
 * (contig << 32) | start and (contig << 32) | (end + 1); the points are sorted ascending, duplicates kept; index e stands
 * for [point[e], point[e + 1]).  A feature covers the indices [lower_bound (its start point), lower_bound (its end + 1
 * point)) and leaves on each of them the maximum of a 32-bit priority: 1u << 31 | (0x7fffffff - i) for a CDS of file index
 * i, i + 1 for any other feature, 0 for nothing -- the maximum is the winner of the rule, and a maximum does not depend on the
 * order it is taken in, so the table is the same from run to run.  A lookup is one binary search:
 * e = upper_bound (points, (contig << 32) | (pos + 1)) - 1; e = -1 or a priority of 0 gives -1.
 *   tjamd_annotation_create copies the features to the counter's device and builds the table on its stream; one wait, at the
 *     end.  NULL with TJAMD_ERR_ARG for a contig outside [0, tjamd_reference_contigs (ref)), start < 1, end < start, a cls
 *     outside 0 ... 2, more than 2^30 features, a reference of another device; an end beyond the contig's length is accepted; n_features = 0 is valid (every lookup gives -1).  NULL with TJAMD_ERR_NO_DEVICE without a
 *     device.  The annotation keeps nothing of the caller's and does not need the reference afterwards.
 *   tjamd_annotation_features: n_features (-1 for NULL).
 *   tjamd_annotation_download: returns the number of points; h_points[e] and h_winner[e] (the file index of the winner on
 *     index e, or -1) are written when capacity suffices, otherwise nothing is written. */
typedef struct tjamd_annotation tjamd_annotation;
tjamd_annotation *tjamd_annotation_create (tjamd_counter *c, const tjamd_reference *ref, const tjamd_feature *h_features, long n_features);
void tjamd_annotation_destroy (tjamd_annotation *a);
long tjamd_annotation_features (const tjamd_annotation *a);
long tjamd_annotation_download (const tjamd_annotation *a, uint64_t *h_points, int *h_winner, long capacity);

/* One record per tract of a tiling (the tracts and tract locations tjamd_located_tracts writes, or a caller's own):
 *   feature: the winner of the rule above for d_tract_loc[t], a file index or -1.
 *   max_length: the max_tract_length column of the reference's tract_list.tsv (src/genome_set.c:492,502-503): the maximum,
 *     over the samples that have a count above 0 in the tract's rows, of the length field of the sample's modal row -- the row
 *     of the tract with the highest count for that sample, the first in union order on a tie; the length is read signed
 *     (10 bits), so this is the maximum of the "sample's allele" of tjamd_tract_variants.  0 when no sample has a count.
 *     With d_keys or d_counts NULL max_length is 0 and n_union, n_samples and d_tracts are not read.
 * Returns n_tracts and writes exactly n_tracts records (n_tracts = 0: returns 0, writes nothing).  Refused with
 * TJAMD_ERR_ARG: when a union is given, tracts that do not tile it (from an error flag raised on the device) and n_samples
 * outside 1 ... 4096; an annotation of another device; null buffers.  Without a device, TJAMD_ERR_NO_DEVICE.  A refused call
 * writes nothing to d_out (the tiling is checked by a launch of its own, in front of the lookup).  Changes none of its inputs
 * nor the counter's finalised state.  One launch without a union, two with one; waits once, at the end. */
typedef struct { int feature, max_length; } tjamd_tract_feature;                                   /* 8 bytes */
long tjamd_tract_features (tjamd_counter *c, const tjamd_annotation *a, const void *d_keys, const void *d_counts, long n_union,
                           int n_samples, const tjamd_union_tract *d_tracts, long n_tracts, const tjamd_location *d_tract_loc,
                           tjamd_tract_feature *d_out);

/* -1.0 for a NULL counter and after a refused call */
double tjamd_last_annotation_ms (tjamd_counter *c);        /* the kernels of the last tjamd_annotation_create on this counter (the copy to the device not included) */
double tjamd_last_tract_features_ms (tjamd_counter *c);    /* the kernel of the last tjamd_tract_features */

#ifdef __cplusplus
}
#endif
#endif
