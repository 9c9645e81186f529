/* variable_tracts.c -- the last step of tatajuba (src/genome_set.c:619-736, describe_statistics_for_genome_set): the tracts
 * that vary between samples and the three per-sample tables that describe them, through the C ABI and nothing else.
 * Every sample is scanned and finalised on a counter of its own (sample mod devices); tjamd_gather_histograms brings the
 * histograms to the first counter's device, tjamd_merge_samples builds the union, tjamd_tract_stats finds the variable
 * tracts and tjamd_tract_sample_stats computes their per-sample values, written as
 *   DIR/per_sample_average_length.tsv  DIR/per_sample_modal_frequency.tsv  DIR/per_sample_proportional_coverage.tsv
 * in the reference's layout (:680-736).  Without a mapper the location is -1, the feature "unannotated" and the reference
 * column empty (1 in the modal-frequency table, as the reference prints); sample names are the paths as given.
 *
 *   gcc -O2 -I include examples/variable_tracts.c -L tatajuba_amd -ltatajuba_amd -Wl,-rpath,$PWD/tatajuba_amd -o variable_tracts
 *   ./variable_tracts [-k 10] [-m 3] [-c 5] [-o .] sample1.fastq[.gz] sample2.fastq[.gz] ...                                */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tatajuba_amd.h>

#define MAX_SAMPLES 64
#define N_FNAME_SAMPLE 3

static const char *fname[N_FNAME_SAMPLE] = {"per_sample_average_length.tsv", "per_sample_modal_frequency.tsv", "per_sample_proportional_coverage.tsv"};
static const int precision[N_FNAME_SAMPLE] = {2, 2, 5};                  /* sample_print_precision (src/genome_set.c:17) */
static const char *reference_value[N_FNAME_SAMPLE] = {"", "1", ""};

static int
fail (const char *what)
{
  fprintf (stderr, "%s: %s\n", what, tjamd_last_error ());
  return 1;
}

int
main (int argc, char **argv)
{
  tjamd_counter *ctr[MAX_SAMPLES];
  const char *files[MAX_SAMPLES], *outdir = ".";
  long counts[MAX_SAMPLES], total, n_union, n_tracts, n_var = 0, i;
  int n = 0, k = 10, m = 3, cov = 5, coverage[MAX_SAMPLES], a, j, ndev = tjamd_device_count (), status;
  const void *d_records = NULL;
  void *d_keys, *d_counts, *d_summary, *d_var, *d_values;
  int *h_var;
  double *h_values;
  FILE *fout[N_FNAME_SAMPLE];

  for (a = 1; a < argc; a++) {
    if (!strcmp (argv[a], "-k") && a + 1 < argc) k = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-m") && a + 1 < argc) m = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-c") && a + 1 < argc) cov = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-o") && a + 1 < argc) outdir = argv[++a];
    else if (n < MAX_SAMPLES) files[n++] = argv[a];
  }
  if (n < 1) { fprintf (stderr, "usage: %s [-k K] [-m M] [-c C] [-o DIR] sample.fastq[.gz] ...\n", argv[0]); return 2; }
  if (ndev < 1) { fprintf (stderr, "tatajuba_amd error: no HIP device is visible (there is no CPU fallback)\n"); return 1; }

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

  /* every tract's summary, the variable ones' ids (a union of n_union rows has at most n_union tracts) */
  d_summary = tjamd_device_alloc (ctr[0], (size_t) (n_union ? n_union : 1) * sizeof (tjamd_tract_summary));
  d_var = tjamd_device_alloc (ctr[0], (size_t) (n_union ? n_union : 1) * sizeof (int));
  n_tracts = tjamd_tract_stats (ctr[0], d_keys, d_counts, n_union, n, NULL, coverage, NULL, (tjamd_tract_summary *) d_summary, (int *) d_var,
                                n_union ? n_union : 1, &n_var);
  if (n_tracts < 0) return fail ("tract statistics");
  /* per-sample values of the variable tracts only: [n_var][5][n] */
  d_values = tjamd_device_alloc (ctr[0], (size_t) (n_var ? n_var : 1) * TJAMD_N_TRACT_STATS * (size_t) n * sizeof (double));
  if (tjamd_tract_sample_stats (ctr[0], d_keys, d_counts, n_union, n, coverage, (const tjamd_tract_summary *) d_summary, n_tracts, (const int *) d_var,
                                n_var, (double *) d_values, NULL, NULL) < 0) return fail ("per-sample statistics");
  h_var = (int *) malloc ((size_t) (n_var ? n_var : 1) * sizeof (int));
  h_values = (double *) malloc ((size_t) (n_var ? n_var : 1) * TJAMD_N_TRACT_STATS * (size_t) n * sizeof (double));
  if (tjamd_device_download (ctr[0], h_var, d_var, (size_t) n_var * sizeof (int)) ||
      tjamd_device_download (ctr[0], h_values, d_values, (size_t) n_var * TJAMD_N_TRACT_STATS * (size_t) n * sizeof (double))) return fail ("download");

  for (j = 0; j < N_FNAME_SAMPLE; j++) {                  /* initialise_files_descriptive_stats (:680-690) */
    size_t len = strlen (outdir) + strlen (fname[j]) + 2;
    char *path = (char *) malloc (len);
    snprintf (path, len, "%s/%s", outdir, fname[j]);
    fout[j] = fopen (path, "w");
    if (!fout[j]) { fprintf (stderr, "cannot write %s\n", path); return 1; }
    free (path);
    fprintf (fout[j], "tract_id\tlocation\tfeature\treference");
    for (a = 0; a < n; a++) fprintf (fout[j], "\t%s", files[a]);
    fprintf (fout[j], "\n");
  }
  for (i = 0; i < n_var; i++)                             /* print_descriptive_stats_per_sample (:712-736) */
    for (j = 0; j < N_FNAME_SAMPLE; j++) {               /* (the tables are the first three statistics, in their order) */
      const double *v = h_values + ((size_t) i * TJAMD_N_TRACT_STATS + (size_t) j) * (size_t) n;
      fprintf (fout[j], "tid_%06d\t%d\t%s\t%s", h_var[i], -1, "unannotated", reference_value[j]);
      for (a = 0; a < n; a++) {
        if (v[a] > 0.) fprintf (fout[j], "\t%.*lf", precision[j], v[a]);
        else           fprintf (fout[j], "\t");
      }
      fprintf (fout[j], "\n");
    }
  for (j = 0; j < N_FNAME_SAMPLE; j++) fclose (fout[j]);

  printf ("From %ld tracts, %ld are variable\n", n_tracts, n_var);
  tjamd_device_free (ctr[0], d_keys); tjamd_device_free (ctr[0], d_counts); tjamd_device_free (ctr[0], d_summary);
  tjamd_device_free (ctr[0], d_var); tjamd_device_free (ctr[0], d_values);
  free (h_var); free (h_values);
  for (a = 0; a < n; a++) tjamd_counter_destroy (ctr[a]);
  return 0;
}
