/* gff3_reader.h -- the feature lines of a GFF3 file (plain, gzip, BGZF) as tjamd_feature records; see gff3_reader.c and
 * include/tatajuba_features.h, which has the rules above tjamd_gff3_read. */
#ifndef TATAJUBA_AMD_GFF3_READER_H
#define TATAJUBA_AMD_GFF3_READER_H
#include "../../include/tatajuba_features.h"

/* what tjamd_gff3_read returns and writes (it is this function behind the C ABI's name) */
long tjg_read (const char *path, const char *contig_names, long n_contigs, tjamd_feature *out, long capacity,
               char *strings, long strings_capacity, long *strings_bytes, long *n_skipped);

/* what tjamd_gff3_read_phase (include/tatajuba_effects.h) returns and writes: column 8 of the lines tjg_read keeps */
long tjg_read_phase (const char *path, const char *contig_names, long n_contigs, signed char *out, long capacity);

#endif
