/* tatajuba_amd.h -- C-ABI extension of the drop-in boundary (tatajuba_hopo.h) for callers that hold their reads in
 * device memory, drive several GPUs, or want to inspect the device-side state.  Everything is extern "C", plain
 * pointers and sizes; `void *hip_stream` is a hipStream_t (NULL = the counter's own stream).
 *
 * A "stream of reads" (the batch format of the device path) is a byte buffer in which every read is followed by one
 * '\n' (0x0A) -- the one byte tatajuba's parser can never deliver inside a sequence (reference: src/kseq.h:105,189-192).
 * It carries read boundaries in-band, so the scan kernel needs no offset table.
 *
 * Reference interfaces replaced:
 *   tjamd_scan_*      : the loop `while (kseq_read) update_hopo_counter_from_seq(...)`   src/hopo_counter.c:153,219-258,285-307
 *   tjamd_finalise    : finalise_hopo_counter() steps 1-4 + coverage                     src/hopo_counter.c:339-415,419-438
 *   tjamd_download_*  : the caller's direct reads of hc->elem / idx_* / coverage          src/context_histogram.c:231-256
 */
#ifndef TATAJUBA_AMD_H
#define TATAJUBA_AMD_H

#include "tatajuba_hopo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bit positions inside the 64-bit word of hopo_element / of a device record (see tatajuba_hopo.h) */
#define TJ_META_BASE_SHIFT   0
#define TJ_META_LEN_SHIFT    2
#define TJ_META_COUNT_SHIFT  12
#define TJ_META_MISM_SHIFT   32
#define TJ_META_FLAG_SHIFT   49
#define TJ_META_RAW_CONST    ((1ULL << TJ_META_COUNT_SHIFT) | (0xffeULL << TJ_META_MISM_SHIFT)) /* count=1, mismatches=0xffe */

typedef struct tjamd_counter tjamd_counter;      /* device-side per-sample accumulator (opaque) */

/* 24-byte device record: context[0], context[1], bitfield word.  32-byte "located" record adds the global byte
 * position of the tract's first base in the scanned stream (test / CPU-entry aid; gives emission order and read_offset). */
typedef struct { uint64_t ctx0, ctx1, meta; } tjamd_record;
typedef struct { uint64_t ctx0, ctx1, meta, pos; } tjamd_located_record;

/* error codes (0 = ok) */
enum { TJAMD_OK = 0, TJAMD_ERR_NO_DEVICE = 1, TJAMD_ERR_HIP = 2, TJAMD_ERR_ARG = 3, TJAMD_ERR_CAPACITY = 4, TJAMD_ERR_STATE = 5 };

int  tjamd_device_count (void);                   /* number of visible HIP devices (0 => every entry below fails loudly) */
const char *tjamd_last_error (void);              /* thread-local message of the last failure */
const char *tjamd_version (void);        /* name, version and the hash of the sources the library was built from */
const char *tjamd_source_hash (void);    /* that hash alone (tatajuba_amd/build.py computes the same over the tree) */

tjamd_counter *tjamd_counter_create (int device, int kmer_size);   /* NULL on failure (see tjamd_last_error) */
void tjamd_counter_destroy (tjamd_counter *c);
int  tjamd_counter_reset (tjamd_counter *c);      /* forget raw and finalised records, keep buffers */
int  tjamd_counter_set_stream (tjamd_counter *c, void *hip_stream); /* run on the caller's stream (e.g. torch's) */
int  tjamd_counter_device (const tjamd_counter *c);

/* Scan a stream of reads already resident in this counter's device memory.  d_stream must be 16-byte aligned.
 * Asynchronous; appends to the counter's raw records. */
int  tjamd_scan_device (tjamd_counter *c, const void *d_stream, size_t n_bytes, int min_tract_size);
/* Same from host memory (copied to HBM first). */
int  tjamd_scan_host (tjamd_counter *c, const void *h_stream, size_t n_bytes, int min_tract_size);
/* Located variant: records go to a separate list with positions, sorted by position (emission order) on download.
 * min_tract_size == 0 selects the all-monomers scan (reference: src/hopo_counter.c:260-283). */
long tjamd_scan_host_located (tjamd_counter *c, const void *h_stream, size_t n_bytes, int min_tract_size,
                              tjamd_located_record *out, long capacity);

/* Plain FASTQ text parsed on the device (the three memchr and one memcpy per record of the host reader, as a line count and a
 * compaction in HBM): text in, the stream of reads out, scanned at once or kept.  A session is tjamd_fastq_begin, any number
 * of pushes, tjamd_fastq_end; the text is the concatenation of all pushes of the session, in order.
 *
 * The rule.  A regular record starting at offset p is four lines L0..L3, each ended by '\n', of which all of these hold:
 *   L0[0] == '@';   len (L1) >= 1 and L1[0] is none of '>' '+' '@';   L2[0] == '+';   len (L3) == len (L1);
 *   none of the record's bytes is '\r'.
 * Line parity decides what is a header, the byte alone does not: a quality line may start with '@'.  On the push marked
 * `final`, the end of the text ends a non-empty L3 that has no '\n'.  The consumed prefix is the longest run of regular
 * records from offset 0; its stream is L1 + '\n' for each record, in order: what tjamd_read_file_stream makes of the same
 * bytes.  Everything from the first irregular record on is left to the caller (tjamd_fastq_end says where it starts):
 * FASTA and multi-line records, CRLF, a blank line, a quality line of another length, after `final` a record cut short,
 * and the reference's stop at a bad quality string, which stays where it is, in the host reader.
 *
 * Pushes may cut the text anywhere, mid-line, mid-record, one byte at a time: the incomplete tail of a push is carried on
 * the device (never through the host) in front of the next push's text.  The carry is at most TJAMD_FASTQ_CARRY_MAX bytes
 * (TATAJUBA_AMD_FASTQ_CARRY in the environment when the counter is created shortens it: tests): a record that a push
 * boundary cuts must end within that many bytes of its start, or the session stops with code 2 at its start.  After a
 * stop the later pushes of the session do nothing.  A push does not wait for the device (growing a buffer, and a
 * staging buffer of tjamd_fastq_push_host still in flight, may); tjamd_fastq_end is the one wait of a session.  d_text
 * must stay as it is until then (or until a mark taken behind the push has been waited for); h_text is free again when
 * tjamd_fastq_push_host returns unless it is pinned memory (tjamd_host_alloc), which is copied from where it lies and is
 * free after such a mark.  No byte at or beyond d_text + n_bytes, rounded up to 16, is read.
 *
 * tjamd_fastq_begin: min_tract_size >= 0 scans every push's stream into the counter's raw records exactly as
 * tjamd_scan_device would with that value -- which, like tjamd_scan_device, takes 1 ... 32 and refuses 0: the all-monomers
 * scan exists for located records only (tjamd_scan_host_located) --, small pushes gathered into one scan launch, so the
 * records are all there when tjamd_fastq_end has returned; -1 parses only and keeps the session's whole stream
 * for tjamd_fastq_stream.  Refused with TJAMD_ERR_ARG: a push without begin, begin inside a session, a push after `final`;
 * and, before a device is looked for: a null counter, null text with n_bytes > 0, n_bytes above 1 GiB, a d_text that is
 * not 16-byte aligned, min_tract_size < -1.  Without a device: TJAMD_ERR_NO_DEVICE.  n_bytes == 0 is valid (how a caller
 * says `final` late).  A session ended without a final push reports an incomplete record as stop 1.
 * Not built: gzip or BGZF on the device, FASTA or multi-line records on the device, paired files in one session, read names. */
enum { TJAMD_FASTQ_CARRY_MAX = 1 << 20 };
int  tjamd_fastq_begin (tjamd_counter *c, int min_tract_size);
int  tjamd_fastq_push_device (tjamd_counter *c, const void *d_text, size_t n_bytes, int final);   /* 16-byte aligned */
int  tjamd_fastq_push_host   (tjamd_counter *c, const void *h_text, size_t n_bytes, int final);   /* staged copy, then the same */
long tjamd_fastq_end (tjamd_counter *c);          /* waits; bytes of text consumed since begin, or a negative TJAMD_ERR_* */
long tjamd_fastq_reads (const tjamd_counter *c);  /* records consumed by the last ended session */
int  tjamd_fastq_stop (const tjamd_counter *c);   /* 0: all text consumed; 1: irregular record at the consumed offset;
                                                     2: a record did not end within the carry */
const void *tjamd_fastq_stream (const tjamd_counter *c);   /* device pointer, 16-byte aligned; parse-only sessions, else NULL */
long tjamd_fastq_stream_bytes (const tjamd_counter *c);
int  tjamd_fastq_tile_bytes (void);               /* text bytes one workgroup takes per step: what the edge tests aim at */

/* Many short strings in one launch: what the reference does with one counter and one update_hopo_counter_from_seq call per
 * reference window (src/genome_set.c:525-577), batched.  seqs[i] / lens[i]: the windows; min_tract_size as in
 * update_hopo_counter_from_seq (0: the all-monomers scan).  out: hopo_element[capacity] in window order, then read order,
 * with read_offset relative to the window; window_of[i] (may be NULL) = window of record i.  Uses the calling thread's
 * shared device context.  Returns the number of records, -1 on error (tjamd_last_error) or if capacity is too small. */
long tjamd_scan_windows (int kmer_size, const char *const *seqs, const int *lens, int n_windows, int min_tract_size,
                         hopo_element *out, int *window_of, long capacity);

/* Host-only: parse a FASTA/FASTQ file (plain or gzip; same record semantics as the reference's reader, src/kseq.h:172-212
 * as looped at src/hopo_counter.c:153) into a stream of reads.  Returns the stream's size in bytes and writes it to out
 * when capacity suffices (call with out = NULL to size); *n_reads = records parsed; -1 if the file cannot be opened. */
long tjamd_read_file_stream (const char *path, unsigned char *out, long capacity, long *n_reads);

/* The same through the multi-threaded feeder (tatajuba_amd/csrc/feeder.c): n_threads readers over window_bytes of
 * file bytes at a time (0 = default), their outputs accepted only where each reader ended exactly on the next one's
 * first record -- so the result is byte-identical to tjamd_read_file_stream.  A plain file is mapped; a gzip file is
 * inflated one window ahead of the parse, BGZF (bgzip) members by all threads side by side, any other gzip stream by
 * one thread.  new_or_append_hopo_counter_from_file takes this path for plain files of 32 MiB and gzip files of 4 MiB
 * and more (TATAJUBA_AMD_FEEDER_THREADS, default min(8, cores); 1 = the single reader). */
long tjamd_read_file_stream_mt (const char *path, unsigned char *out, long capacity, long *n_reads, int n_threads, long window_bytes);

/* pinned host memory, so that tjamd_scan_host overlaps the copy with the caller's parsing; tjamd_sync waits for
 * everything queued on the counter's stream */
void *tjamd_host_alloc (size_t bytes);
void tjamd_host_free (void *p);
int  tjamd_sync (tjamd_counter *c);

/* device memory on the counter's device for callers without HIP headers of their own (buffers for tjamd_merge_samples,
 * tjamd_tract_ids); tjamd_device_download waits for the counter's stream, then copies to the host */
void *tjamd_device_alloc (tjamd_counter *c, size_t bytes);
void tjamd_device_free (tjamd_counter *c, void *p);
int  tjamd_device_download (tjamd_counter *c, void *host, const void *dev, size_t bytes);

/* Hint: reads of about stream_bytes in total are coming.  Allocates the raw-record storage for them in one piece (up to
 * 4 GB) instead of by repeated growth. */
int  tjamd_reserve (tjamd_counter *c, size_t stream_bytes, int min_tract_size);

/* A mark is a point in the counter's stream: tjamd_mark() returns a small handle (>= 0; < 0 on error), tjamd_wait_mark()
 * returns once everything queued before the mark has finished -- without waiting for what was queued after it (how the
 * feeder re-uses a pinned batch buffer while later batches are in flight).  Eight marks are live at a time. */
int  tjamd_mark (tjamd_counter *c);
int  tjamd_wait_mark (tjamd_counter *c, int mark);

long tjamd_raw_count (tjamd_counter *c);          /* synchronises; number of raw records so far; <0 on error */
long tjamd_download_raw (tjamd_counter *c, tjamd_record *out, long capacity); /* unordered multiset */
long tjamd_undefined_runs (tjamd_counter *c);     /* qualifying non-ACGTU runs with no earlier tract in the read (dropped) */
/* append host-produced raw records (hopo_element array) to the device raw list */
int  tjamd_upload_raw (tjamd_counter *c, const hopo_element *elems, long n);

/* steps 1-4 + coverage on the device.  status: 0 ok, 1 no raw records, 2 nothing after filter, 3 nothing reaches
 * min_coverage (reference: src/hopo_counter.c:345-349,376-381,406-411). */
int  tjamd_finalise (tjamd_counter *c, int remove_biased, int min_coverage, int *status);
/* The same in two calls, for a caller with more samples than GPUs: _begin queues the whole device finalise on the counter's
 * stream and returns; _end waits until THIS counter's counts have reached the host (an event, not the stream: the next
 * sample's scan, queued on another counter of the same stream in between, runs on) and returns what tjamd_finalise
 * returns.  Between the two calls the counter must not be touched. */
int  tjamd_finalise_begin (tjamd_counter *c, int remove_biased, int min_coverage);
/* The HIP stream for the ordering step (bin partition, sort, index, coverage: six small launches whose time is latency)
 * of a finalise begun with tjamd_finalise_begin: the step runs there behind an event, beside whatever the counter's own
 * stream does next -- the next sample's scan on another counter; its kernels are sized to start on a CU that the
 * scan's workgroups fill (DESIGN.md sections 3.4 and 5).  A stream handle means that stream; NULL means none
 * (everything on the counter's stream).  A counter on which this was never called uses a side stream that the library
 * owns: one per device for the whole process, made when first needed and released with the last counter that used it.
 * TATAJUBA_AMD_ORDER=main in the environment when a counter is created gives that counter none instead (A/B runs,
 * tests); a later call of this function still decides.  tjamd_finalise and a step that has to be run again with the
 * count in hand stay on the counter's stream whatever is set here. */
int  tjamd_counter_set_order_stream (tjamd_counter *c, void *hip_stream);
int  tjamd_finalise_end (tjamd_counter *c, int *status);
long tjamd_kept_count (tjamd_counter *c);
int  tjamd_n_idx (tjamd_counter *c);
int  tjamd_coverage (tjamd_counter *c);
long tjamd_download_kept (tjamd_counter *c, hopo_element *out, long capacity);      /* widened to 40-byte elements */
long tjamd_download_idx (tjamd_counter *c, int *idx_initial, int *idx_final, long capacity);
const void *tjamd_kept_device_ptr (tjamd_counter *c);   /* tjamd_record[kept_count] in HBM (for collectives) */

/* cross-sample merge on one device (reference precursor of src/genome_set.c:250-289, keyed by context instead of
 * BWA location): concatenation of n_samples kept arrays (d_records, counts[]) -> sorted union with per-sample counts.
 * out_keys: tjamd_record[n_union] (count field = total over the samples, canon_flag = OR of the samples' flags),
 * out_counts: int32[n_union * n_samples].  Returns n_union. */
long tjamd_merge_samples (tjamd_counter *c, const void *d_records, const long *counts, int n_samples,
                          void *d_out_keys, void *d_out_counts, long capacity);

/* The exchange of that merge for a caller that, like the reference, runs its samples as threads of one process
 * (reference: src/genome_set.c:66-94 OpenMP loop, merge at :195-229): the kept records of the finalised counters
 * `samples`, whatever devices they live on, copied back to back into a buffer on dst's device (peer copies over xGMI).
 * counts[i] = records of sample i, *d_records = the buffer (owned by dst until its next gather).  Returns the total. */
long tjamd_gather_histograms (tjamd_counter *dst, tjamd_counter *const *samples, int n_samples, const void **d_records, long *counts);

/* which device pairs the gathers of this process have used, and how: "dst<-src:direct" (peer access, xGMI) or
 * "dst<-src:staged" (peer access refused: the runtime copies through host memory).  Returns the number of staged pairs. */
int tjamd_peer_access_report (char *out, int capacity);

/* The same exchange between PROCESSES, one per GPU (north_star: "an RCCL all-gatherv over xGMI of the per-sample
 * histograms"; reference attach point src/genome_set.c:195-229, where the samples are threads and nothing moves): every
 * rank contributes its finalised counter's kept records and receives every rank's, in rank order, back to back in a device
 * buffer the communicator owns (valid until its next exchange), ready for tjamd_merge_samples.  Two calls set it up:
 *   rank 0:      tjamd_comm_unique_id (id)            -> TJAMD_COMM_ID_BYTES bytes to hand to the other ranks (MPI_Bcast, a file, ...)
 *   every rank:  tjamd_comm_create (c, id, rank, world)   collective; the communicator is bound to c's device
 * and tjamd_allgather_histograms (c, comm, &d_records, counts[world]) is the exchange: ncclAllGather on c's stream, one
 * block per rank (its count, then its records), block size agreed from the counts of the exchange before; returns the total
 * number of records, counts[r] = records of rank r.  Collective: every rank calls it, in the same order. */
#define TJAMD_COMM_ID_BYTES 128
typedef struct tjamd_comm tjamd_comm;
int  tjamd_comm_unique_id (void *id_bytes);
tjamd_comm *tjamd_comm_create (tjamd_counter *c, const void *id_bytes, int rank, int world);
void tjamd_comm_destroy (tjamd_comm *comm);
/* run the exchanges on this HIP stream instead of the exchanged counter's (null: back to the counter's): a finalised
 * sample's exchange then runs beside the next sample's scan.  The caller must have seen the counter's finalise end. */
int  tjamd_comm_set_stream (tjamd_comm *comm, void *hip_stream);
int  tjamd_comm_rank (const tjamd_comm *comm);
int  tjamd_comm_world (const tjamd_comm *comm);
int  tjamd_comm_count (const tjamd_comm *comm);            /* ranks RCCL itself reports for the communicator (ncclCommCount); -1 on failure */
/* the last exchange on this communicator: device milliseconds from the first pack to the last unpack (HIP events on the
 * exchange's stream), bytes the data collective delivered to this rank, collectives it took; any pointer may be NULL;
 * non-zero before the first exchange */
int  tjamd_comm_last_exchange (const tjamd_comm *comm, double *ms, long *bytes, long *collectives);
long tjamd_comm_collectives (const tjamd_comm *comm);    /* RCCL calls issued so far (diagnostic: one per exchange once the block size has settled) */
long tjamd_allgather_histograms (tjamd_counter *c, tjamd_comm *comm, const void **d_records, long *counts);

/* tract ids on a merged union (reference: src/genome_set.c:207-221, context-keyed: the id goes up wherever
 * (base, ctx0, ctx1) changes between neighbours of d_keys = tjamd_record[n] in the reference's descending order).
 * d_tract_id (device, may be NULL) and / or h_tract_id (host, may be NULL) receive int32[n].  Returns the number of ids. */
long tjamd_tract_ids (tjamd_counter *c, const void *d_keys, long n, int *d_tract_id, int *h_tract_id);

/* Per-tract statistics across the samples of a merged union, and the tracts that vary between them (reference:
 * describe_statistics_for_genome_set, src/genome_set.c:619-678, with descriptive_stats_of_histogram :738-766,
 * relative_difference_of_vector :768-779 and update_descriptive_stats_for_this_trait :692-710).
 * A tract is a run of union rows with one tract id; a sample's histogram in it is the tract's rows as (signed 10-bit length,
 * the sample's count), one bar per row; the sample is present if any of them has a non-zero count.  Per (tract, present
 * sample), in this order (absent samples: 0 in all five):
 *   avg length = sum count * length / integral       modal freq = max count / integral      prop coverage = integral / coverage
 *   coverage per context = integral / n_context      entropy = -sum p ln p, p = count / integral
 * integral = the sample's summed count; n_context = distinct contexts (base, ctx0, ctx1) among its non-zero rows (1 for the
 * ids of tjamd_tract_ids), counted as changes of context from one non-zero row to the next: the rows of one context must be
 * contiguous within a tract, as they are in the sorted union of tjamd_merge_samples; modal length = the length of the
 * highest count, the larger length on a tie.  For tracts of several contexts (the grouped ids of tjamd_union_tracts),
 * tjamd_union_tract_stats gives the reference's histogram h instead: one bar per length, summed over the contexts. */
#define TJAMD_N_TRACT_STATS 5
enum { TJAMD_STAT_AVG_LENGTH, TJAMD_STAT_MODAL_FREQ, TJAMD_STAT_PROP_COVERAGE, TJAMD_STAT_COVERAGE_PER_CONTEXT, TJAMD_STAT_ENTROPY };
/* one tract: its rows [first, first + n_rows) of the union, present samples, the variable flag, and per statistic the
 * max - min over the present samples (0 if that max <= DBL_MIN).  56 bytes. */
typedef struct { int first, n_rows, n_present, variable; double reldiff[TJAMD_N_TRACT_STATS]; } tjamd_tract_summary;

/* Summaries of all tracts and the ascending ids of the variable ones.  A tract is variable if n_present < n_samples, or if
 * reldiff[avg length] + reldiff[modal freq] + reldiff[entropy] > 1e-5, or if a reference length > 0 was given for it and a
 * present sample's modal length differs from it.
 *   d_keys        device tjamd_record[n_union], d_counts device int32[n_union * n_samples] (as tjamd_merge_samples writes them)
 *   n_samples     1 ... 4096
 *   d_tract_id    device int32[n_union]: caller's tract ids (0 on the first row, up by 0 or 1 per row; refused otherwise);
 *                 NULL = the context-keyed ids of tjamd_tract_ids, computed here
 *   coverage      host int32[n_samples]: each sample's coverage (tjamd_coverage of its counter)
 *   d_ref_length  device int32[n_tracts]: a reference tract length per tract (<= 0: none), or NULL (no such test)
 *   d_summary     device tjamd_tract_summary[capacity]; d_var device int32[capacity] (may be NULL): variable tract ids
 *   n_var         host (may be NULL): number of variable tracts
 * Runs on the counter's stream, synchronises at the end.  Returns n_tracts, or a negative TJAMD_ERR_* (tjamd_last_error). */
long tjamd_tract_stats (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                        const int *d_tract_id, const int *coverage, const int *d_ref_length,
                        tjamd_tract_summary *d_summary, int *d_var, long capacity, long *n_var);
/* The per-sample values of a list of tracts (typically d_var), in the reference's samples_per_trait layout
 * (src/genome_set.c:696-698), recomputed from the union without a table of all tracts:
 *   d_summary     device tjamd_tract_summary[n_tracts] from tjamd_tract_stats (first and n_rows are read)
 *   d_list        device int32[n_list]: tract ids, each in [0, n_tracts) (refused otherwise)
 *   d_values      device double[n_list][TJAMD_N_TRACT_STATS][n_samples]
 *   d_modal_len   device int32[n_list][n_samples] (may be NULL): modal length, 0 if absent
 *   d_n_context   device int32[n_list][n_samples] (may be NULL): n_context, 0 if absent
 * Other arguments as for tjamd_tract_stats.  Synchronises at the end.  Returns n_list, or a negative TJAMD_ERR_*. */
long tjamd_tract_sample_stats (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                               const int *coverage, const tjamd_tract_summary *d_summary, long n_tracts, const int *d_list, long n_list,
                               double *d_values, int *d_modal_len, int *d_n_context);

/* Tracts across samples by grouping near-identical contexts of the union (N6; reference: the context histograms of
 * new_genomic_context_list, src/context_histogram.c:245-286, as the tracts of new_g_tract_vector_from_genomic_context_list,
 * src/genome_set.c:195-229, summarised by update_g_tract_summary_from_context_histogram / fill_g_tract_summary_tables
 * :291-378 and selected by print_selected_g_tract_vector :380-434).
 *   Grouping: the tracts are the context histograms that new_genomic_context_list's grouping forms on the union rows taken
 *     in union order as one sample's finalised array: the max_distance_per_flank / levenshtein_distance rule of
 *     tjamd_context_histograms, with the same edit-distance readings (TATAJUBA_AMD_EDIT_DISTANCE, read per call).
 *   Row counts: a row's count is its exact total over the samples (the int64 sum of its d_counts row; the union key's
 *     20-bit count field wraps and is not read).  The modal row (highest total, the first on a tie) carries the tract's
 *     name in the indel retry.
 *   Contiguity: a tract is a run of rows, so the ids start at 0 and go up by 0 or 1 per row (tjamd_tract_stats accepts them).
 *   lev_distance: the largest edit distance that admitted a row through the retry (join type 2), measured between the row's
 *     name and the modal name at that moment; 0 if no row joined that way (the reference's lev_distance).
 *   A sample's histogram in a tract: its non-zero rows summed per length into bars, ordered by count (highest first), then
 *     length (larger first): the reference's h.  The five values are descriptive_stats_of_histogram's (:738-766), its sums
 *     taken bar by bar in h order; n_context = distinct contexts among the sample's non-zero rows; modal length = h's first.
 *     reldiff is relative_difference_of_vector (:768-779) over the present samples.
 *   variable: the rule of tjamd_tract_stats (d_ref_length included).  selected: the rule of print_selected_g_tract_vector:
 *     n_present < n_samples, or lev_distance > 0, or reldiff of modal freq, avg length or entropy > 1e-6.
 *   Known limitation: only rows that are neighbours in the sort order can join, as within a sample.  That covers variants in
 *     the right flank and variants of the left flank far from the tract; a left-flank SNP next to the tract usually has
 *     unrelated rows between its two alleles, and its two tracts stay apart.  With a reference genome, tjamd_locate and
 *     tjamd_located_tracts (N7, below) join them: two tracts located at one place become one.
 * Names use the counter's k.  Every entry runs on the counter's stream, changes neither d_keys nor d_counts nor the
 * counter's finalised state, and returns a count or a negative TJAMD_ERR_* (tjamd_last_error starts with its name). */
typedef struct { int first, n_rows, n_context, mode, indel, lev_distance; long long integral; } tjamd_union_tract;   /* 32 bytes */
/* one tract: rows [first, first + n_rows), present samples, both flags, lev_distance, and per statistic (TJAMD_STAT_*
 * order) the max - min over the present samples (0 if that max <= DBL_MIN).  64 bytes. */
typedef struct { int first, n_rows, n_present, variable, selected, lev_distance; double reldiff[TJAMD_N_TRACT_STATS]; } tjamd_union_tract_summary;

/* Groups the union (d_keys / d_counts as tjamd_merge_samples writes them, n_samples 1 ... 4096):
 *   d_tract_id   device int32[n_union]: each row's tract
 *   d_join_type  device int32[n_union] (may be NULL): 0 opened its tract, 1 joined within the flank distance, 2 through the retry
 *   d_tracts     device tjamd_union_tract[capacity]: first and n_rows, n_context (as tjamd_context_histograms counts them), mode
 *                (the modal row, by totals), indel (a row joined through the retry), lev_distance, integral (summed totals)
 * Distances must be >= 0; a capacity below the tracts found is refused (TJAMD_ERR_CAPACITY).  Waits twice: for the retry
 * candidates and for the tract count, as tjamd_context_histograms does.  Returns n_tracts. */
long tjamd_union_tracts (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                         int max_distance_per_flank, int levenshtein_distance,
                         int *d_tract_id, int *d_join_type, tjamd_union_tract *d_tracts, long capacity);
/* Summaries of the tracts of tjamd_union_tracts, the ascending ids of the variable ones (d_var, may be NULL; their number in
 * *n_var) and of the selected ones (d_sel, may be NULL; *n_sel).  d_tracts must tile the union (first 0, each tract starting
 * where the one before ends, the last ending at n_union): refused otherwise, from an error flag raised on the device.
 * coverage and d_ref_length as for tjamd_tract_stats; d_summary, d_var, d_sel hold n_tracts entries.  Waits once, at the
 * end.  Returns n_tracts. */
long tjamd_union_tract_stats (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                              const tjamd_union_tract *d_tracts, long n_tracts, const int *coverage, const int *d_ref_length,
                              tjamd_union_tract_summary *d_summary, int *d_var, long *n_var, int *d_sel, long *n_sel);
/* The per-sample values of a list of tracts, as tjamd_tract_sample_stats lays them out ([n_list][TJAMD_N_TRACT_STATS]
 * [n_samples]); d_modal_len, d_n_context and d_n_len (bars of h, 0 if absent) are int32[n_list][n_samples] and may be NULL.
 * Waits once, at the end.  Returns n_list. */
long tjamd_union_tract_sample_stats (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                                     const int *coverage, const tjamd_union_tract_summary *d_summary, long n_tracts,
                                     const int *d_list, long n_list, double *d_values, int *d_modal_len, int *d_n_context, int *d_n_len);

/* within-sample grouping of near-identical contexts on a finalised counter (reference: new_genomic_context_list,
 * src/context_histogram.c:245-270 with the Hamming distance of :25-48, on the finalised array's own order; no
 * Levenshtein retry).  group_of: int32[kept_count] (host, may be NULL); groups: one entry per group (host, may be NULL):
 * first element, elements, distinct contexts, element with the modal count, summed count.  Returns the number of groups. */
typedef struct { int first, n_elem, n_context, mode; long long integral; } tjamd_group;
long tjamd_group_contexts (tjamd_counter *c, int max_distance_per_flank, int *group_of, tjamd_group *groups, long capacity);

/* The whole grouping step (reference: new_genomic_context_list, src/context_histogram.c:245-270 and :278-286): the flank
 * distance test as above, then, for an element of the histogram's base that fails it, the retry with an edit distance
 * between the "left.B.right" names of the histogram's modal context and of the element (:19-23,255-261: joins if it is below
 * levenshtein_distance and marks the histogram `indel`), then every histogram's tract lengths weighted by count, highest
 * count first (:282 new_empfreq_from_int_weighted; modal_len / modal_freq = its first entry).  The edit distance stands
 * for biomcmc_levenshtein_distance (.., 1, 1, true) of biomcmc-lib, absent from the reference tree: unit-cost global edit
 * distance; likewise the order among equal counts (larger length first).
 *   group_of   int32[kept_count]   histogram of each element (host, may be NULL)
 *   join_type  int32[kept_count]   0 = the element opened its histogram, 1 = joined within the flank distance, 2 = by the retry
 *   groups     one entry per histogram (host, may be NULL; `capacity` entries)
 *   hist       tjamd_length_freq[kept_count]: histogram g's entries at [groups[g].first, groups[g].first + groups[g].n_len)
 * Returns the number of histograms. */
typedef struct { int first, n_elem, n_context, mode, indel, n_len, modal_len, modal_freq; long long integral; } tjamd_context_group;
typedef struct { int length, freq; } tjamd_length_freq;
long tjamd_context_histograms (tjamd_counter *c, int max_distance_per_flank, int levenshtein_distance, int *group_of, int *join_type,
                               tjamd_context_group *groups, tjamd_length_freq *hist, long capacity);

/* Tracts located on a reference genome by flank matching (N7; reference: find_reference_location_and_sort_hopo_counter,
 * src/hopo_counter.c:495-572, which maps the contexts with BWA, and find_best_context_name_for_reference,
 * src/genome_set.c:525-577, which rescans the reference around the location; BWA is not part of this library).  The genome is
 * scanned as a stream of reads: a tract seen in a read and the same tract seen in the genome give the same canonical (base,
 * ctx0, ctx1), so a location is found by joining keys against an index of the genome's own runs.
 *
 * The index.  tjamd_reference_create builds it on the counter's device and stream from the contigs as a stream of reads
 * (every contig followed by '\n', as tjamd_read_file_stream makes of a FASTA file), with the counter's k; one wait, at
 * the end.  One entry per maximal run of one base (A, C, G, T or U, either case counting as the same base; length >= 1)
 * whose k bytes on each side lie in the same contig and are all A, C, G, T or U by the scan's classification: a run or a
 * flank touching any other byte is left out (it would pack as A and give false matches), and so is a run closer than k to
 * a contig end.  An entry holds ctx0, ctx1 and base as the scan makes them (A and C as read; T and G reverse-complemented,
 * neg_strand = 1), the run length as a plain int (no 10-bit field), the 0-based contig, pos = the 0-based position in the
 * contig of the run's first base in forward coordinates on either strand, and flat = pos + the lengths of all earlier
 * contigs, delimiters not counted (the reference's refseq_offset, src/genome_set.c:527-529,537).  n_contigs counts the
 * delimiters, plus one for a last contig without one.  tjamd_reference_download returns the entries in ascending flat. */
typedef struct tjamd_reference tjamd_reference;
typedef struct { uint64_t ctx0, ctx1; long long flat; int contig, pos, length, base, neg_strand, pad; } tjamd_ref_entry;   /* 48 bytes */
tjamd_reference *tjamd_reference_create (tjamd_counter *c, const void *h_stream, size_t n_bytes);   /* NULL on failure (tjamd_last_error) */
void tjamd_reference_destroy (tjamd_reference *ref);
long tjamd_reference_entries (const tjamd_reference *ref);
long tjamd_reference_contigs (const tjamd_reference *ref);
long tjamd_reference_download (const tjamd_reference *ref, tjamd_ref_entry *out, long capacity);

/* The lookup.  d_keys: device tjamd_record[n], a union as tjamd_merge_samples writes it or a counter's kept array
 * (tjamd_kept_device_ptr); only base, ctx0 and ctx1 are read.  d_loc: device tjamd_location[n].  With d (x, y) = the number of
 * the k base positions at which two packed flanks differ (the distance of the grouping), an entry r is a hit for a row q when
 *   r.base == q.base, and either r.ctx0 == q.ctx0 and d (r.ctx1, q.ctx1) <= max_mismatches
 *                           or r.ctx1 == q.ctx1 and d (r.ctx0, q.ctx0) <= max_mismatches:
 * one flank matches exactly, the other within the limit; the run length is free.  mismatches = the distance in the inexact
 * flank; the row's location is the hit with the fewest mismatches, then the smallest flat (the reference's best and leftmost
 * match, src/genome_set.c:540-542); n_hits = distinct hit entries (one that is exact in both flanks counts once); ref_length
 * and neg_strand are that entry's.  No hit: flat = contig = pos = -1, the rest 0.  Rows of one context get one result.
 * A reference built with another k or on another device is refused, as is max_mismatches outside 0 ... k.  Waits once, at
 * the end.  Returns the number of located rows.
 * Out of scope here: a row whose flank differs from the genome by an indel, or that has mismatches in both flanks, stays
 * unlocated by this call; tjamd_locate_gapped (N10, tatajuba_locate.h) is the second pass that tries those rows by a banded
 * edit distance.  GFF3 features are read in tatajuba_features.h; the
 * drop-in gets no find_reference_location_and_sort_hopo_counter of its own (the weak hook stays as it is: a host program
 * fills loc_* from this call on tjamd_kept_device_ptr). */
typedef struct { long long flat; int contig, pos, ref_length, mismatches, neg_strand, n_hits; } tjamd_location;   /* 32 bytes */
long tjamd_locate (tjamd_counter *c, const tjamd_reference *ref, const void *d_keys, long n, int max_mismatches, tjamd_location *d_loc);

/* Tracts by location (reference: context_histograms_overlap, genomic_context_merge_histograms_at_same_location,
 * src/context_histogram.c:88-110,364-385: two histograms mapped to one place are one tract).
 *   d_tracts      device tjamd_union_tract[n_tracts] that tile the union (from tjamd_union_tracts; refused otherwise, as in
 *                 tjamd_union_tract_stats), or NULL: the context-keyed tracts of tjamd_tract_ids (n_tracts is not read)
 *   d_loc         device tjamd_location[n_union] from tjamd_locate on the same union (or the caller's own places: flat < 0
 *                 means unlocated, and a flat of 2^45 or more is refused: the order is a sort on 48 bits of (flat + 1, base))
 * A tract's location is that of its located row with the highest exact int64 total over the samples, the first such row
 * on a tie; a tract without a located row is unlocated.  Tracts with the same base and the same flat become one tract.
 * The reference's further rule for nearby but unequal locations (within mode_context_length - 1, joined by edit distance,
 * src/context_histogram.c:98-108) makes up for alignment starts that move with the flank; here the location is the tract's
 * own first base, the same number for every allele of one genomic tract, so the rule is not needed and not built.
 * Output order: the unlocated tracts first, in input order (the reference puts unknown locations first,
 * src/hopo_counter.c:561-564), then the located ones ascending by (flat, base); inside a merged tract the member tracts
 * keep input order and rows keep union order, so the rows of one context stay contiguous.
 *   d_perm        device int32[n_union]: output row i is input row d_perm[i]
 *   d_out_keys    device tjamd_record[n_union], d_out_counts device int32[n_union * n_samples]: the gathered union (each may be NULL)
 *   d_out_tracts  device tjamd_union_tract[capacity] of the new tiling: first, n_rows; n_context, integral = sums over the
 *                 members; indel = OR, lev_distance = max of the members'; mode = the output row with the highest total, the
 *                 first on a tie
 *   d_tract_loc   device tjamd_location[capacity] (may be NULL): the tract's location, by the rule above on its output rows
 *   d_ref_length  device int32[capacity] (may be NULL): that location's ref_length, 0 if unlocated
 * The output tiles the permuted union: tjamd_union_tract_stats and tjamd_union_tract_sample_stats run on (d_out_keys,
 * d_out_counts, d_out_tracts), and d_ref_length feeds their reference-length test.  Changes neither d_keys nor d_counts nor
 * the counter's finalised state.  Waits once, at the end (twice with d_tracts NULL).  Returns the number of tracts; a
 * capacity below it is TJAMD_ERR_CAPACITY. */
long tjamd_located_tracts (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                           const tjamd_union_tract *d_tracts, long n_tracts, const tjamd_location *d_loc,
                           int *d_perm, void *d_out_keys, void *d_out_counts,
                           tjamd_union_tract *d_out_tracts, tjamd_location *d_tract_loc, int *d_ref_length, long capacity);

/* Per-sample tract variants against the reference as the fields of VCF records (N8: tjamd_tract_variants), and the contig
 * names of a FASTA file (tjamd_read_file_names), are declared in tatajuba_variants.h, which includes this header; their
 * timer is tjamd_last_tract_variants_ms below. */

/* The second pass of the lookup for rows whose flanks differ from the genome by indels or in both flanks (N10: the seed
 * order of the index, the banded flank distance and the gapped lookup) is declared, with its timers, in tatajuba_locate.h,
 * which includes this header. */

/* The GFF3 feature a located tract lies in and its longest modal length (N9: tjamd_gff3_read, tjamd_annotation_create and
 * its kin, tjamd_tract_features) are declared, with their timers, in tatajuba_features.h, which includes this header. */

/* The coding effect of a variant record (N11: tjamd_translate, tjamd_gff3_read_phase, tjamd_coding_create and its kin,
 * tjamd_variant_effects) is declared, with its timers, in tatajuba_effects.h, which includes this header. */

/* The per-sample variant records merged into multi-sample sites, their distinct alleles and a genotype per sample (N12:
 * tjamd_merge_variants, tjamd_site_ref_alt) are declared, with their timer, in tatajuba_sites.h, which includes
 * tatajuba_variants.h and through it this header. */

/* The read depths of the merged sites and the genotype that tells a reference sample from an unseen one (N13:
 * tjamd_site_depths) are declared, with their timer, in tatajuba_depths.h, which includes tatajuba_sites.h and through it this
 * header. */

/* The pairwise distances of the samples over the merged sites (N14: tjamd_sample_distances) are declared, with their timer,
 * in tatajuba_distances.h, which includes tatajuba_depths.h and through it this header. */

/* The single-linkage tree of the samples over that matrix and its clusters at a threshold (N15: tjamd_sample_linkage,
 * tjamd_linkage_clusters) are declared, with their timers, in tatajuba_linkage.h, which includes tatajuba_distances.h and
 * through it this header. */

/* The sites that set a group of samples apart from the rest (N16: tjamd_group_sites) are declared, with their timer, in
 * tatajuba_groups.h, which includes tatajuba_linkage.h and through it this header. */

/* The links of that tree as nodes with children and a leaf order, and the sites that support each of its clades without a
 * cut (N17: tjamd_linkage_tree, tjamd_clade_sites), are declared, with their timers, in tatajuba_clades.h, which includes
 * tatajuba_groups.h and through it this header. */

/* release the calling thread's shared device contexts of the synchronous string scans (update_hopo_counter_from_seq on a
 * counter that never read a file, tjamd_scan_windows) now; they are released by themselves when the thread ends */
void tjamd_thread_cleanup (void);

/* timing of the last operations on this counter, from HIP events on its stream (milliseconds) */
double tjamd_last_scan_ms (tjamd_counter *c);       /* scan kernel(s) of the last tjamd_scan_* call */
int    tjamd_counter_uses_log (const tjamd_counter *c);  /* 1: k <= 12 and the scan writes a record log that partition_log_kernel distributes (default); 0: the scan kernels partition by themselves (k > 12, or TATAJUBA_AMD_SINK=fused) */
double tjamd_last_partition_ms (tjamd_counter *c);  /* partition_log_kernel behind the last scan launch (k <= 12); 0 if the scan kernel partitioned by itself */
/* whole device finalise of the last tjamd_finalise call, or tjamd_finalise_begin / _end pair.  After a pair whose ordering
 * step went to another stream (tjamd_counter_set_order_stream; the default) the interval begins on the counter's stream
 * and ends on that one: it includes the time the step spent sharing CUs with the next sample's scan and is no measure
 * of what the finalise costs the pipeline -- that is the time per sample, bench.py's ms_per_step. */
double tjamd_last_finalise_ms (tjamd_counter *c);
double tjamd_last_merge_ms (tjamd_counter *c);      /* kernels of the last tjamd_merge_samples on this counter */
double tjamd_last_tract_stats_ms (tjamd_counter *c); /* the last tjamd_tract_stats on this counter, first launch to last (host waits included) */
double tjamd_last_union_tracts_ms (tjamd_counter *c);      /* the last tjamd_union_tracts, first launch to last (host waits included) */
double tjamd_last_union_tract_stats_ms (tjamd_counter *c); /* the last tjamd_union_tract_stats, first launch to last */
long   tjamd_last_union_tract_candidates (tjamd_counter *c); /* rows of the last tjamd_union_tracts that the indel retry was tried on first (-1: none yet) */
double tjamd_last_reference_ms (tjamd_counter *c);         /* kernels of the last tjamd_reference_create on this counter (the copy to the device not included) */
double tjamd_last_locate_ms (tjamd_counter *c);            /* the lookup kernel of the last tjamd_locate */
double tjamd_last_located_tracts_ms (tjamd_counter *c);    /* the last tjamd_located_tracts, first launch to last (host waits included) */
double tjamd_last_tract_variants_ms (tjamd_counter *c);    /* the last tjamd_tract_variants, first launch to last */
double tjamd_last_fastq_ms (tjamd_counter *c);    /* parse kernels of the last ended session; -1.0 for NULL / after a refusal */
long   tjamd_last_scan_launches (tjamd_counter *c);
/* finalises of this counter whose device-side sizing of the ordering step had read a stale kept count (checked against the
 * count at the next kernel boundary and repaired; expected to stay 0) */
long   tjamd_plan_mismatches (tjamd_counter *c);

/* synthetic inputs: genome of `genome_len` i.i.d. bases from splitmix64(seed_genome); n_reads reads of
 * length read_len (or uniform in [read_len, read_len_max] when read_len_max > read_len), uniform start, strand by coin,
 * no N, written as a stream of reads into out (capacity bytes).  variant_seed != 0 lengthens/shortens 1% of the
 * genome's tracts >= 4 by one base first.  Returns bytes written, or -(bytes needed) if capacity is too small. */
long tjamd_synth_stream (uint64_t seed_genome, uint64_t seed_reads, uint64_t variant_seed, long genome_len,
                         long n_reads, int read_len, int read_len_max, unsigned char *out, long capacity, int n_threads);

#ifdef __cplusplus
}
#endif
#endif
