/* annotated_tracts.c -- the pipeline of located_tracts.c with a GFF3 annotation (-g), through the C ABI and nothing else: the
 * feature each located tract lies in (genomic_context_find_features, src/context_histogram.c:331-351) splits the selected
 * tracts into the reference's two tables, and the tract list and the BED file of the variable tracts are written as
 * src/genome_set.c:380-434,591-614,646-648 writes them:
 *   DIR/selected_tracts_annotated.tsv  the selected tracts that lie in a feature, the feature's ID in GFF3_info (:418-428)
 *   DIR/selected_tracts_unknown.tsv    the selected tracts that lie in none (:406-415); begin_context = the flat location
 *   DIR/tract_list.tsv                 every located tract (:598-611): contig name, feature type and ID (nc, unannotated if
 *                                      none), position in the contig, the longest modal length over the samples, the
 *                                      reference's length, the tract's modal context and the reference's as left.B.right
 *   DIR/variable_tracts.bed            the variable located tracts (:646-648): contig, first base, one past the last, tid
 * Options are located_tracts.c's, and -g annotation.gff3[.gz].
 *
 *   gcc -O2 -I include examples/annotated_tracts.c -L tatajuba_amd -ltatajuba_amd -Wl,-rpath,$PWD/tatajuba_amd -o annotated_tracts
 *   ./annotated_tracts -r reference.fa -g annotation.gff3 [-x 1] [-k 10] [-m 3] [-c 5] [-d 1] [-l -1] [-o .] sample1.fastq[.gz] ...   */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tatajuba_features.h>
#include <tatajuba_variants.h>
#include <tatajuba_hopo.h>

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

/* :406-411 / :420-425, the reldiffs in the reference's order (gentab, :351-370); info = NULL: the table without GFF3_info */
static void
selected_line (FILE *fout, int tid, const char *info, long long flat, const tjamd_union_tract_summary *t)
{
  const int order[TJAMD_N_TRACT_STATS] = {TJAMD_STAT_MODAL_FREQ, TJAMD_STAT_AVG_LENGTH, TJAMD_STAT_PROP_COVERAGE, TJAMD_STAT_COVERAGE_PER_CONTEXT,
                                          TJAMD_STAT_ENTROPY};
  int j;
  if (info) fprintf (fout, "tid_%06d\t%s\t%8lld\t%5d\t%5d\t|\t", tid, info, flat, t->n_present, t->lev_distance);
  else fprintf (fout, "tid_%06d\t%8lld\t%5d\t%5d\t|\t", tid, flat, t->n_present, t->lev_distance);
  for (j = 0; j < TJAMD_N_TRACT_STATS; j++) fprintf (fout, "%8.6lf\t", t->reldiff[order[j]]);
  fprintf (fout, "\n");
}

int
main (int argc, char **argv)
{
  tjamd_counter *ctr[MAX_SAMPLES];
  const char *files[MAX_SAMPLES], *outdir = ".", *reference = NULL, *gff = NULL;
  long counts[MAX_SAMPLES], total, n_union, n_grouped, n_tracts, n_located, n_sel = 0, n_var = 0, i, cap, ref_bytes, n_contigs = 0, n_names = 0, name_bytes,
       n_features, string_bytes = 0, n_skipped = 0, n_entries, n_yes = 0, n_no = 0, nt1;
  int n = 0, k = 10, m = 3, cov = 5, maxd = 1, lev = -1, mism = 1, coverage[MAX_SAMPLES], a, ndev = tjamd_device_count (), status;
  const void *d_records = NULL;
  void *d_keys, *d_counts, *d_ids, *d_grouped, *d_loc, *d_perm, *d_pkeys, *d_pcounts, *d_tracts, *d_tloc, *d_reflen, *d_summary, *d_sel, *d_var, *d_tf;
  unsigned char *ref_stream;
  char *names, **contig_name, *strings;
  int *h_sel, *h_var;
  tjamd_reference *ref;
  tjamd_annotation *ann;
  tjamd_feature *features;
  tjamd_union_tract_summary *h_summary;
  tjamd_union_tract *h_tracts;
  tjamd_location *h_tloc;
  tjamd_tract_feature *h_tf;
  tjamd_record *h_keys;
  tjamd_ref_entry *entries;
  FILE *fyes, *fno, *fout;

  for (a = 1; a < argc; a++) {
    if (!strcmp (argv[a], "-k") && a + 1 < argc) k = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-m") && a + 1 < argc) m = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-c") && a + 1 < argc) cov = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-d") && a + 1 < argc) maxd = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-l") && a + 1 < argc) lev = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-x") && a + 1 < argc) mism = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-r") && a + 1 < argc) reference = argv[++a];
    else if (!strcmp (argv[a], "-g") && a + 1 < argc) gff = argv[++a];
    else if (!strcmp (argv[a], "-o") && a + 1 < argc) outdir = argv[++a];
    else if (n < MAX_SAMPLES) files[n++] = argv[a];
  }
  if (n < 1 || !reference || !gff) {
    fprintf (stderr, "usage: %s -r reference.fa -g annotation.gff3 [-x X] [-k K] [-m M] [-c C] [-d D] [-l L] [-o DIR] sample.fastq[.gz] ...\n", argv[0]);
    return 2;
  }
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
  cap = n_union ? n_union : 1;
  d_ids = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (int));
  d_grouped = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_union_tract));
  n_grouped = tjamd_union_tracts (ctr[0], d_keys, d_counts, n_union, n, maxd, lev, (int *) d_ids, NULL, (tjamd_union_tract *) d_grouped, cap);
  if (n_grouped < 0) return fail ("union tracts");

  /* the reference: the index of its runs and the names of its contigs; the annotation: its features on those contigs */
  ref_bytes = tjamd_read_file_stream (reference, NULL, 0, &n_contigs);
  if (ref_bytes < 0) { fprintf (stderr, "cannot read %s\n", reference); return 1; }
  ref_stream = (unsigned char *) malloc ((size_t) ref_bytes + 1);
  tjamd_read_file_stream (reference, ref_stream, ref_bytes, &n_contigs);
  ref = tjamd_reference_create (ctr[0], ref_stream, (size_t) ref_bytes);
  if (!ref) return fail (reference);
  free (ref_stream);
  name_bytes = tjamd_read_file_names (reference, NULL, 0, &n_names);
  names = (char *) malloc ((size_t) name_bytes + 1);
  contig_name = (char **) malloc ((size_t) (n_names ? n_names : 1) * sizeof (char *));
  tjamd_read_file_names (reference, names, name_bytes, &n_names);
  n_features = tjamd_gff3_read (gff, names, n_names, NULL, 0, NULL, 0, &string_bytes, &n_skipped);
  if (n_features < 0) { fprintf (stderr, "cannot read %s\n", gff); return 1; }
  features = (tjamd_feature *) malloc ((size_t) (n_features ? n_features : 1) * sizeof (tjamd_feature));
  strings = (char *) malloc ((size_t) string_bytes + 1);
  tjamd_gff3_read (gff, names, n_names, features, n_features, strings, string_bytes, &string_bytes, &n_skipped);
  for (i = 0, a = 0; i < n_names; i++) {                  /* (after the GFF3 is read: the names become C strings) */
    contig_name[i] = names + a;
    while (names[a] != '\n') a++;
    names[a++] = '\0';
  }
  ann = tjamd_annotation_create (ctr[0], ref, features, n_features);
  if (!ann) return fail (gff);
  d_loc = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_location));
  n_located = tjamd_locate (ctr[0], ref, d_keys, n_union, mism, (tjamd_location *) d_loc);
  if (n_located < 0) return fail ("locate");

  /* tracts by location, their summaries, the variable and the selected ones, and each tract's feature and longest length */
  d_perm = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (int));
  d_pkeys = tjamd_device_alloc (ctr[0], (size_t) cap * 24);
  d_pcounts = tjamd_device_alloc (ctr[0], (size_t) cap * (size_t) n * 4);
  d_tracts = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_union_tract));
  d_tloc = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_location));
  d_reflen = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (int));
  n_tracts = tjamd_located_tracts (ctr[0], d_keys, d_counts, n_union, n, (const tjamd_union_tract *) d_grouped, n_grouped, (const tjamd_location *) d_loc,
                                   (int *) d_perm, d_pkeys, d_pcounts, (tjamd_union_tract *) d_tracts, (tjamd_location *) d_tloc, (int *) d_reflen, cap);
  if (n_tracts < 0) return fail ("located tracts");
  nt1 = n_tracts ? n_tracts : 1;
  d_summary = tjamd_device_alloc (ctr[0], (size_t) nt1 * sizeof (tjamd_union_tract_summary));
  d_sel = tjamd_device_alloc (ctr[0], (size_t) nt1 * sizeof (int));
  d_var = tjamd_device_alloc (ctr[0], (size_t) nt1 * sizeof (int));
  d_tf = tjamd_device_alloc (ctr[0], (size_t) nt1 * sizeof (tjamd_tract_feature));
  if (tjamd_union_tract_stats (ctr[0], d_pkeys, d_pcounts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, coverage, (const int *) d_reflen,
                               (tjamd_union_tract_summary *) d_summary, (int *) d_var, &n_var, (int *) d_sel, &n_sel) < 0) return fail ("tract statistics");
  if (tjamd_tract_features (ctr[0], ann, d_pkeys, d_pcounts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, (const tjamd_location *) d_tloc,
                            (tjamd_tract_feature *) d_tf) < 0) return fail ("tract features");
  h_summary = (tjamd_union_tract_summary *) malloc ((size_t) nt1 * sizeof (tjamd_union_tract_summary));
  h_tracts = (tjamd_union_tract *) malloc ((size_t) nt1 * sizeof (tjamd_union_tract));
  h_tloc = (tjamd_location *) malloc ((size_t) nt1 * sizeof (tjamd_location));
  h_tf = (tjamd_tract_feature *) malloc ((size_t) nt1 * sizeof (tjamd_tract_feature));
  h_keys = (tjamd_record *) malloc ((size_t) cap * sizeof (tjamd_record));
  h_sel = (int *) malloc ((size_t) (n_sel ? n_sel : 1) * sizeof (int));
  h_var = (int *) malloc ((size_t) (n_var ? n_var : 1) * sizeof (int));
  if (tjamd_device_download (ctr[0], h_summary, d_summary, (size_t) n_tracts * sizeof (tjamd_union_tract_summary)) ||
      tjamd_device_download (ctr[0], h_tracts, d_tracts, (size_t) n_tracts * sizeof (tjamd_union_tract)) ||
      tjamd_device_download (ctr[0], h_tloc, d_tloc, (size_t) n_tracts * sizeof (tjamd_location)) ||
      tjamd_device_download (ctr[0], h_tf, d_tf, (size_t) n_tracts * sizeof (tjamd_tract_feature)) ||
      tjamd_device_download (ctr[0], h_keys, d_pkeys, (size_t) n_union * sizeof (tjamd_record)) ||
      tjamd_device_download (ctr[0], h_sel, d_sel, (size_t) n_sel * sizeof (int)) ||
      tjamd_device_download (ctr[0], h_var, d_var, (size_t) n_var * sizeof (int))) return fail ("download");
  n_entries = tjamd_reference_entries (ref);
  entries = (tjamd_ref_entry *) malloc ((size_t) (n_entries ? n_entries : 1) * sizeof (tjamd_ref_entry));
  if (tjamd_reference_download (ref, entries, n_entries) < 0) return fail ("reference entries");
  printf ("%ld contigs, %ld runs indexed; %ld features read, %ld lines skipped; %ld of %ld union rows located; %ld grouped tracts -> %ld tracts by location\n",
          n_contigs, n_entries, n_features, n_skipped, n_located, n_union, n_grouped, n_tracts);

  /* :391-428: the selected tracts, those with a feature and those without */
  if (!(fno = open_output (outdir, "selected_tracts_unknown.tsv")) || !(fyes = open_output (outdir, "selected_tracts_annotated.tsv"))) return 1;
  fprintf (fno, "tract_id\tbegin_context\tn_genomes\tlev_distance\t|\trd_frequency\trd_avge_tract_length\trd_coverage\trd_context_covge\trd_entropy\n");
  fprintf (fyes, "tract_id\tGFF3_info\tbegin_context\tn_genomes\tlev_distance\t|\trd_frequency\trd_avge_tract_length\trd_coverage\trd_context_covge\trd_entropy\n");
  for (i = 0; i < n_sel; i++) {
    const int t = h_sel[i], f = h_tf[t].feature;
    if (f >= 0) { selected_line (fyes, t, strings + features[f].id_off, h_tloc[t].flat, h_summary + t); n_yes++; }
    else { selected_line (fno, t, NULL, h_tloc[t].flat, h_summary + t); n_no++; }
  }
  fclose (fno); fclose (fyes);
  printf ("From %d tracts, %d interesting ones are annotated and %d interesting ones are not annotated\n", (int) n_tracts, (int) n_yes, (int) n_no);

  /* :598-611: the located tracts, ascending; the reference's own tract is the index entry at the tract's flat */
  if (!(fout = open_output (outdir, "tract_list.tsv"))) return 1;
  fprintf (fout, "tract_id\tcontig_name\tfeature_type\tfeature\tlocation_in_contig\tmax_tract_length\tref_tract_length\ttract\tref_tract\n");
  for (i = 0; i < n_tracts; i++) {
    const tjamd_location *l = h_tloc + i;
    const int f = h_tf[i].feature;
    long lo = 0, hi = n_entries;
    char *tract, *ref_tract;
    tjamd_record *mode;
    if (l->flat < 0) continue;
    while (lo < hi) { const long mid = (lo + hi) / 2; if (entries[mid].flat < l->flat) lo = mid + 1; else hi = mid; }
    if (lo >= n_entries || entries[lo].flat != l->flat) continue;          /* (a caller's own location; tjamd_locate writes an entry's) */
    mode = h_keys + h_tracts[i].mode;
    tract = generate_name_from_flanking_contexts (&mode->ctx0, (int8_t) (mode->meta & 3), k, l->neg_strand != 0);
    ref_tract = generate_name_from_flanking_contexts (&entries[lo].ctx0, (int8_t) entries[lo].base, k, entries[lo].neg_strand != 0);
    fprintf (fout, "tid_%06ld\t%s\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n", i, contig_name[l->contig], f >= 0 ? strings + features[f].type_off : "nc",
             f >= 0 ? strings + features[f].id_off : "unannotated", l->pos, h_tf[i].max_length, entries[lo].length, tract, ref_tract);
    free (tract); free (ref_tract);
  }
  fclose (fout);

  /* :646-648: the variable tracts that have a place, from the tract's first base to one past its last on the genome */
  if (!(fout = open_output (outdir, "variable_tracts.bed"))) return 1;
  for (i = 0; i < n_var; i++) {
    const tjamd_location *l = h_tloc + h_var[i];
    if (l->flat >= 0) fprintf (fout, "%s\t%d\t%d\ttid_%06d\n", contig_name[l->contig], l->pos, l->pos + l->ref_length, h_var[i]);
  }
  fclose (fout);

  tjamd_annotation_destroy (ann);
  tjamd_reference_destroy (ref);
  tjamd_device_free (ctr[0], d_keys); tjamd_device_free (ctr[0], d_counts); tjamd_device_free (ctr[0], d_ids); tjamd_device_free (ctr[0], d_grouped);
  tjamd_device_free (ctr[0], d_loc); tjamd_device_free (ctr[0], d_perm); tjamd_device_free (ctr[0], d_pkeys); tjamd_device_free (ctr[0], d_pcounts);
  tjamd_device_free (ctr[0], d_tracts); tjamd_device_free (ctr[0], d_tloc); tjamd_device_free (ctr[0], d_reflen);
  tjamd_device_free (ctr[0], d_summary); tjamd_device_free (ctr[0], d_sel); tjamd_device_free (ctr[0], d_var); tjamd_device_free (ctr[0], d_tf);
  free (h_summary); free (h_tracts); free (h_tloc); free (h_tf); free (h_keys); free (h_sel); free (h_var); free (entries);
  free (features); free (strings); free (names); free (contig_name);
  for (a = 0; a < n; a++) tjamd_counter_destroy (ctr[a]);
  return 0;
}
