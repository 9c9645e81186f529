/* selected_tracts.c -- tatajuba's main table (src/genome_set.c:380-434, print_selected_g_tract_vector): the tracts that
 * differ between samples once near-identical contexts are grouped across them, through the C ABI and nothing else.
 * Every sample is scanned and finalised on a counter of its own (sample mod devices); tjamd_gather_histograms brings the
 * histograms to the first counter's device, tjamd_merge_samples builds the union, tjamd_union_tracts groups its rows into
 * tracts (new_genomic_context_list's rule on the pooled union) and tjamd_union_tract_stats summarises and selects them:
 *   DIR/selected_tracts_unknown.tsv    the selected tracts, in the reference's layout (:404-412)
 *   DIR/selected_tracts_annotated.tsv  its header only: there is no GFF3 here, so no tract is annotated
 * Without a mapper the location (begin_context) is -1.  Options as the reference's (src/main.c:59-60,190-192): -d is
 * max_distance_per_flank (1, clamped to [0, k/2]), -l the levenshtein_distance (below 0: d + 1).
 *
 *   gcc -O2 -I include examples/selected_tracts.c -L tatajuba_amd -ltatajuba_amd -Wl,-rpath,$PWD/tatajuba_amd -o selected_tracts
 *   ./selected_tracts [-k 10] [-m 3] [-c 5] [-d 1] [-l -1] [-o .] sample1.fastq[.gz] sample2.fastq[.gz] ...              */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tatajuba_amd.h>

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
  const char *files[MAX_SAMPLES], *outdir = ".";
  long counts[MAX_SAMPLES], total, n_union, n_tracts, n_sel = 0, i;
  int n = 0, k = 10, m = 3, cov = 5, maxd = 1, lev = -1, coverage[MAX_SAMPLES], a, j, ndev = tjamd_device_count (), status;
  const void *d_records = NULL;
  void *d_keys, *d_counts, *d_ids, *d_tracts, *d_summary, *d_sel;
  int *h_sel;
  tjamd_union_tract_summary *h_summary;
  FILE *fout;

  for (a = 1; a < argc; a++) {
    if (!strcmp (argv[a], "-k") && a + 1 < argc) k = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-m") && a + 1 < argc) m = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-c") && a + 1 < argc) cov = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-d") && a + 1 < argc) maxd = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-l") && a + 1 < argc) lev = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-o") && a + 1 < argc) outdir = argv[++a];
    else if (n < MAX_SAMPLES) files[n++] = argv[a];
  }
  if (n < 1) { fprintf (stderr, "usage: %s [-k K] [-m M] [-c C] [-d D] [-l L] [-o DIR] sample.fastq[.gz] ...\n", argv[0]); return 2; }
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

  /* the tracts (a union of n_union rows has at most n_union of them), then their summaries and the selected ids */
  d_ids = tjamd_device_alloc (ctr[0], (size_t) (n_union ? n_union : 1) * sizeof (int));
  d_tracts = tjamd_device_alloc (ctr[0], (size_t) (n_union ? n_union : 1) * sizeof (tjamd_union_tract));
  n_tracts = tjamd_union_tracts (ctr[0], d_keys, d_counts, n_union, n, maxd, lev, (int *) d_ids, NULL, (tjamd_union_tract *) d_tracts,
                                 n_union ? n_union : 1);
  if (n_tracts < 0) return fail ("union tracts");
  d_summary = tjamd_device_alloc (ctr[0], (size_t) (n_tracts ? n_tracts : 1) * sizeof (tjamd_union_tract_summary));
  d_sel = tjamd_device_alloc (ctr[0], (size_t) (n_tracts ? n_tracts : 1) * sizeof (int));
  if (tjamd_union_tract_stats (ctr[0], d_keys, d_counts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, coverage, NULL,
                               (tjamd_union_tract_summary *) d_summary, NULL, NULL, (int *) d_sel, &n_sel) < 0) return fail ("tract statistics");
  h_summary = (tjamd_union_tract_summary *) malloc ((size_t) (n_tracts ? n_tracts : 1) * sizeof (tjamd_union_tract_summary));
  h_sel = (int *) malloc ((size_t) (n_sel ? n_sel : 1) * sizeof (int));
  if (tjamd_device_download (ctr[0], h_summary, d_summary, (size_t) n_tracts * sizeof (tjamd_union_tract_summary)) ||
      tjamd_device_download (ctr[0], h_sel, d_sel, (size_t) n_sel * sizeof (int))) return fail ("download");

  /* :398: no GFF3, so every selected tract is "not annotated" */
  printf ("From %d tracts, %d interesting ones are annotated and %d interesting ones are not annotated\n", (int) n_tracts, 0, (int) n_sel);
  if (!(fout = open_output (outdir, "selected_tracts_unknown.tsv"))) return 1;
  fprintf (fout, "tract_id\tbegin_context\tn_genomes\tlev_distance\t|\trd_frequency\trd_avge_tract_length\trd_coverage\trd_context_covge\trd_entropy\n");
  for (i = 0; i < n_sel; i++) {                          /* :406-411, the reldiffs in the reference's order (gentab, :351-370) */
    const tjamd_union_tract_summary *t = h_summary + h_sel[i];
    const int order[TJAMD_N_TRACT_STATS] = {TJAMD_STAT_MODAL_FREQ, TJAMD_STAT_AVG_LENGTH, TJAMD_STAT_PROP_COVERAGE, TJAMD_STAT_COVERAGE_PER_CONTEXT,
                                            TJAMD_STAT_ENTROPY};
    fprintf (fout, "tid_%06d\t%8d\t%5d\t%5d\t|\t", h_sel[i], -1, t->n_present, t->lev_distance);
    for (j = 0; j < TJAMD_N_TRACT_STATS; j++) fprintf (fout, "%8.6lf\t", t->reldiff[order[j]]);
    fprintf (fout, "\n");
  }
  fclose (fout);
  if (!(fout = open_output (outdir, "selected_tracts_annotated.tsv"))) return 1;
  fprintf (fout, "tract_id\tGFF3_info\tbegin_context\tn_genomes\tlev_distance\t|\trd_frequency\trd_avge_tract_length\trd_coverage\trd_context_covge\trd_entropy\n");
  fclose (fout);

  tjamd_device_free (ctr[0], d_keys); tjamd_device_free (ctr[0], d_counts); tjamd_device_free (ctr[0], d_ids);
  tjamd_device_free (ctr[0], d_tracts); tjamd_device_free (ctr[0], d_summary); tjamd_device_free (ctr[0], d_sel);
  free (h_summary); free (h_sel);
  for (a = 0; a < n; a++) tjamd_counter_destroy (ctr[a]);
  return 0;
}
