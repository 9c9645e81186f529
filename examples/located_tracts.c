/* located_tracts.c -- tatajuba's main table with its location column filled (src/genome_set.c:380-434,
 * print_selected_g_tract_vector, on tracts placed as find_reference_location_and_sort_hopo_counter, src/hopo_counter.c:495-572,
 * places them), through the C ABI and nothing else.  The samples are scanned, finalised, gathered, merged and grouped as in
 * selected_tracts.c; then the reference FASTA becomes an index of its own runs (tjamd_reference_create), every union row is
 * looked up in it by its flanks (tjamd_locate), tracts at one place become one tract, ordered by place
 * (tjamd_located_tracts), and tjamd_union_tract_stats summarises and selects them on the permuted union, the reference's
 * tract length feeding its variable rule:
 *   DIR/selected_tracts_unknown.tsv    the selected tracts in the reference's layout (:404-412); begin_context = the flat
 *                                      location (position + lengths of the earlier contigs), -1 for an unlocated tract
 *   DIR/tract_locations.tsv            every tract: contig, position, strand (+, -, or . if unlocated), the reference's tract
 *                                      length, mismatches of the best hit, number of hits
 * -x is the number of mismatches allowed in the inexact flank (1); the other options are selected_tracts.c's.
 * -g max_edits adds the second pass (tatajuba_locate.h): the rows tjamd_locate left unlocated are tried by a banded edit
 * distance of up to max_edits edits in both flanks together, each flank shifted by up to -s max_shift bases (3); one more
 * line on the standard output gives the rows it located.  Without -g nothing changes.
 *
 *   gcc -O2 -I include examples/located_tracts.c -L tatajuba_amd -ltatajuba_amd -Wl,-rpath,$PWD/tatajuba_amd -o located_tracts
 *   ./located_tracts -r reference.fa [-x 1] [-g G] [-s 3] [-k 10] [-m 3] [-c 5] [-d 1] [-l -1] [-o .] sample1.fastq[.gz] sample2.fastq[.gz] ...   */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tatajuba_amd.h>
#include <tatajuba_locate.h>

#define MAX_SAMPLES 64

static int
fail (const char *what)
{
  fprintf (stderr, "%s: %s\n", what, tjamd_last_error ());
  return 1;
}

static FILE *
open_output (const char *outdir, const char *name)
{
  size_t len = strlen (outdir) + strlen (name) + 2;
  char *path = (char *) malloc (len);
  FILE *f;
  snprintf (path, len, "%s/%s", outdir, name);
  f = fopen (path, "w");
  if (!f) fprintf (stderr, "cannot write %s\n", path);
  free (path);
  return f;
}

int
main (int argc, char **argv)
{
  tjamd_counter *ctr[MAX_SAMPLES];
  const char *files[MAX_SAMPLES], *outdir = ".", *reference = NULL;
  long counts[MAX_SAMPLES], total, n_union, n_grouped, n_tracts, n_located, n_gapped = 0, n_sel = 0, i, cap, ref_bytes, n_contigs = 0;
  int n = 0, k = 10, m = 3, cov = 5, maxd = 1, lev = -1, mism = 1, max_edits = -1, max_shift = TJAMD_MAX_SHIFT, coverage[MAX_SAMPLES], a, j, ndev = tjamd_device_count (), status;
  const void *d_records = NULL;
  void *d_keys, *d_counts, *d_ids, *d_grouped, *d_loc, *d_perm, *d_pkeys, *d_pcounts, *d_tracts, *d_tloc, *d_reflen, *d_summary, *d_sel;
  unsigned char *ref_stream;
  int *h_sel;
  tjamd_reference *ref;
  tjamd_union_tract_summary *h_summary;
  tjamd_location *h_tloc;
  FILE *fout;

  for (a = 1; a < argc; a++) {
    if (!strcmp (argv[a], "-k") && a + 1 < argc) k = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-m") && a + 1 < argc) m = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-c") && a + 1 < argc) cov = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-d") && a + 1 < argc) maxd = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-l") && a + 1 < argc) lev = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-x") && a + 1 < argc) mism = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-g") && a + 1 < argc) max_edits = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-s") && a + 1 < argc) max_shift = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-r") && a + 1 < argc) reference = argv[++a];
    else if (!strcmp (argv[a], "-o") && a + 1 < argc) outdir = argv[++a];
    else if (n < MAX_SAMPLES) files[n++] = argv[a];
  }
  if (n < 1 || !reference) { fprintf (stderr, "usage: %s -r reference.fa [-x X] [-g G] [-s S] [-k K] [-m M] [-c C] [-d D] [-l L] [-o DIR] sample.fastq[.gz] ...\n", argv[0]); return 2; }
  if (ndev < 1) { fprintf (stderr, "tatajuba_amd error: no HIP device is visible (there is no CPU fallback)\n"); return 1; }
  if (maxd < 0) maxd = 0;                                 /* src/main.c:190-192 */
  if (maxd > k / 2) maxd = k / 2;
  if (lev < 0) lev = maxd + 1;

  for (a = 0; a < n; a++) {
    long n_reads = 0, bytes = tjamd_read_file_stream (files[a], NULL, 0, &n_reads);
    unsigned char *buf;
    if (bytes < 0) { fprintf (stderr, "cannot read %s\n", files[a]); return 1; }
    buf = (unsigned char *) malloc ((size_t) bytes + 1);
    tjamd_read_file_stream (files[a], buf, bytes, &n_reads);
    ctr[a] = tjamd_counter_create (a % ndev, k);
    if (!ctr[a] || tjamd_scan_host (ctr[a], buf, (size_t) bytes, m) || tjamd_finalise (ctr[a], 1, cov, &status)) return fail (files[a]);
    coverage[a] = tjamd_coverage (ctr[a]);
    free (buf);
  }

  total = tjamd_gather_histograms (ctr[0], ctr, n, &d_records, counts);
  if (total < 0) return fail ("gather");
  d_keys = tjamd_device_alloc (ctr[0], (size_t) (total ? total : 1) * 24);
  d_counts = tjamd_device_alloc (ctr[0], (size_t) (total ? total : 1) * (size_t) n * 4);
  n_union = tjamd_merge_samples (ctr[0], d_records, counts, n, d_keys, d_counts, total);
  if (n_union < 0) return fail ("merge");

  /* the tracts by grouping, as in selected_tracts.c (a union of n_union rows has at most n_union of them) */
  cap = n_union ? n_union : 1;
  d_ids = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (int));
  d_grouped = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_union_tract));
  n_grouped = tjamd_union_tracts (ctr[0], d_keys, d_counts, n_union, n, maxd, lev, (int *) d_ids, NULL, (tjamd_union_tract *) d_grouped, cap);
  if (n_grouped < 0) return fail ("union tracts");

  /* the reference: its contigs as a stream of reads -> the index of its runs; every union row -> its place */
  ref_bytes = tjamd_read_file_stream (reference, NULL, 0, &n_contigs);
  if (ref_bytes < 0) { fprintf (stderr, "cannot read %s\n", reference); return 1; }
  ref_stream = (unsigned char *) malloc ((size_t) ref_bytes + 1);
  tjamd_read_file_stream (reference, ref_stream, ref_bytes, &n_contigs);
  ref = tjamd_reference_create (ctr[0], ref_stream, (size_t) ref_bytes);
  if (!ref) return fail (reference);
  free (ref_stream);
  d_loc = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_location));
  n_located = tjamd_locate (ctr[0], ref, d_keys, n_union, mism, (tjamd_location *) d_loc);
  if (n_located < 0) return fail ("locate");
  if (max_edits >= 0) {                                   /* the second pass, on the rows left unlocated */
    if (tjamd_reference_add_seeds (ctr[0], ref) < 0) return fail ("seed order");
    n_gapped = tjamd_locate_gapped (ctr[0], ref, d_keys, n_union, max_edits, max_shift, (tjamd_location *) d_loc, NULL);
    if (n_gapped < 0) return fail ("gapped locate");
  }

  /* tracts at one place become one; the union permuted into the order of the places; then summaries and the selected ids */
  d_perm = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (int));
  d_pkeys = tjamd_device_alloc (ctr[0], (size_t) cap * 24);
  d_pcounts = tjamd_device_alloc (ctr[0], (size_t) cap * (size_t) n * 4);
  d_tracts = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_union_tract));
  d_tloc = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_location));
  d_reflen = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (int));
  n_tracts = tjamd_located_tracts (ctr[0], d_keys, d_counts, n_union, n, (const tjamd_union_tract *) d_grouped, n_grouped, (const tjamd_location *) d_loc,
                                   (int *) d_perm, d_pkeys, d_pcounts, (tjamd_union_tract *) d_tracts, (tjamd_location *) d_tloc, (int *) d_reflen, cap);
  if (n_tracts < 0) return fail ("located tracts");
  d_summary = tjamd_device_alloc (ctr[0], (size_t) (n_tracts ? n_tracts : 1) * sizeof (tjamd_union_tract_summary));
  d_sel = tjamd_device_alloc (ctr[0], (size_t) (n_tracts ? n_tracts : 1) * sizeof (int));
  if (tjamd_union_tract_stats (ctr[0], d_pkeys, d_pcounts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, coverage, (const int *) d_reflen,
                               (tjamd_union_tract_summary *) d_summary, NULL, NULL, (int *) d_sel, &n_sel) < 0) return fail ("tract statistics");
  h_summary = (tjamd_union_tract_summary *) malloc ((size_t) (n_tracts ? n_tracts : 1) * sizeof (tjamd_union_tract_summary));
  h_tloc = (tjamd_location *) malloc ((size_t) (n_tracts ? n_tracts : 1) * sizeof (tjamd_location));
  h_sel = (int *) malloc ((size_t) (n_sel ? n_sel : 1) * sizeof (int));
  if (tjamd_device_download (ctr[0], h_summary, d_summary, (size_t) n_tracts * sizeof (tjamd_union_tract_summary)) ||
      tjamd_device_download (ctr[0], h_tloc, d_tloc, (size_t) n_tracts * sizeof (tjamd_location)) ||
      tjamd_device_download (ctr[0], h_sel, d_sel, (size_t) n_sel * sizeof (int))) return fail ("download");
  printf ("%ld contigs, %ld runs indexed; %ld of %ld union rows located; %ld grouped tracts -> %ld tracts by location\n", n_contigs,
          tjamd_reference_entries (ref), n_located, n_union, n_grouped, n_tracts);
  if (max_edits >= 0) printf ("%ld more union rows located within %d edits and a shift of %d\n", n_gapped, max_edits, max_shift);

  /* :398: no GFF3, so every selected tract is "not annotated" */
  printf ("From %d tracts, %d interesting ones are annotated and %d interesting ones are not annotated\n", (int) n_tracts, 0, (int) n_sel);
  if (!(fout = open_output (outdir, "selected_tracts_unknown.tsv"))) return 1;
  fprintf (fout, "tract_id\tbegin_context\tn_genomes\tlev_distance\t|\trd_frequency\trd_avge_tract_length\trd_coverage\trd_context_covge\trd_entropy\n");
  for (i = 0; i < n_sel; i++) {                          /* :406-411, the reldiffs in the reference's order (gentab, :351-370) */
    const tjamd_union_tract_summary *t = h_summary + h_sel[i];
    const int order[TJAMD_N_TRACT_STATS] = {TJAMD_STAT_MODAL_FREQ, TJAMD_STAT_AVG_LENGTH, TJAMD_STAT_PROP_COVERAGE, TJAMD_STAT_COVERAGE_PER_CONTEXT,
                                            TJAMD_STAT_ENTROPY};
    fprintf (fout, "tid_%06d\t%8lld\t%5d\t%5d\t|\t", h_sel[i], h_tloc[h_sel[i]].flat, t->n_present, t->lev_distance);
    for (j = 0; j < TJAMD_N_TRACT_STATS; j++) fprintf (fout, "%8.6lf\t", t->reldiff[order[j]]);
    fprintf (fout, "\n");
  }
  fclose (fout);
  if (!(fout = open_output (outdir, "tract_locations.tsv"))) return 1;
  fprintf (fout, "tract_id\tcontig\tposition\tstrand\treference_length\tmismatches\tn_hits\n");
  for (i = 0; i < n_tracts; i++) {
    const tjamd_location *l = h_tloc + i;
    fprintf (fout, "tid_%06ld\t%d\t%d\t%s\t%d\t%d\t%d\n", i, l->contig, l->pos, l->flat < 0 ? "." : l->neg_strand ? "-" : "+", l->ref_length, l->mismatches,
             l->n_hits);
  }
  fclose (fout);

  tjamd_reference_destroy (ref);
  tjamd_device_free (ctr[0], d_keys); tjamd_device_free (ctr[0], d_counts); tjamd_device_free (ctr[0], d_ids); tjamd_device_free (ctr[0], d_grouped);
  tjamd_device_free (ctr[0], d_loc); tjamd_device_free (ctr[0], d_perm); tjamd_device_free (ctr[0], d_pkeys); tjamd_device_free (ctr[0], d_pcounts);
  tjamd_device_free (ctr[0], d_tracts); tjamd_device_free (ctr[0], d_tloc); tjamd_device_free (ctr[0], d_reflen);
  tjamd_device_free (ctr[0], d_summary); tjamd_device_free (ctr[0], d_sel);
  free (h_summary); free (h_tloc); free (h_sel);
  for (a = 0; a < n; a++) tjamd_counter_destroy (ctr[a]);
  return 0;
}
