/* sample_vcfs.c -- one VCF per sample with that sample's tract-length variants against the reference genome (tatajuba's
 * generate_vcf_files, src/analyse_variable_tracts.c:13-33, with initialise_vcf_file :35-73 and
 * update_vcf_file_from_context_histogram :147-190), through the C ABI and nothing else.  The pipeline of located_tracts.c --
 * scan, finalise, gather, merge, group, index the reference, locate, tracts by location, statistics on the permuted union --
 * then tjamd_tract_variants on the variable tracts (the list the reference walks, :28) and, per sample,
 *   DIR/<sample>.vcf    the reference's header (:57-69: fileformat, FORMAT=GT, INFO=TID, a ##contig line per contig of the
 *                       FASTA with its name and length, #CHROM ... <sample>) and one row per record (:183):
 *                       contig  POS  .  REF  ALT  .  .  TID=tid_%06d  GT  1
 * <sample> is the file's basename with / " ' space and \ replaced by _ (:53).  The files are written plain; the reference
 * gzips them when it has zlib.  The options are located_tracts.c's.
 *
 *   gcc -O2 -I include examples/sample_vcfs.c -L tatajuba_amd -ltatajuba_amd -Wl,-rpath,$PWD/tatajuba_amd -o sample_vcfs
 *   ./sample_vcfs -r reference.fa [-x 1] [-g G] [-s 3] [-k 10] [-m 3] [-c 5] [-d 1] [-l -1] [-o .] sample1.fastq[.gz] sample2.fastq[.gz] ...   */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tatajuba_variants.h>
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
  long counts[MAX_SAMPLES], total, n_union, n_grouped, n_tracts, n_located, n_gapped = 0, n_var = 0, n_rec, i, cap, ref_bytes, n_contigs = 0, n_names = 0, name_bytes;
  long offsets[MAX_SAMPLES + 1], *contig_len, var_cap;
  int n = 0, k = 10, m = 3, cov = 5, maxd = 1, lev = -1, mism = 1, max_edits = -1, max_shift = TJAMD_MAX_SHIFT, coverage[MAX_SAMPLES], a, ndev = tjamd_device_count (), status;
  const void *d_records = NULL;
  void *d_keys, *d_counts, *d_ids, *d_grouped, *d_loc, *d_perm, *d_pkeys, *d_pcounts, *d_tracts, *d_tloc, *d_reflen, *d_summary, *d_var, *d_variants;
  unsigned char *ref_stream;
  char *names, **contig_name;
  tjamd_reference *ref;
  tjamd_variant *h_variants;
  FILE *fout;

  for (a = 1; a < argc; a++) {
    if (!strcmp (argv[a], "-k") && a + 1 < argc) k = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-m") && a + 1 < argc) m = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-c") && a + 1 < argc) cov = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-d") && a + 1 < argc) maxd = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-l") && a + 1 < argc) lev = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-x") && a + 1 < argc) mism = atoi (argv[++a]);
    else if (!strcmp (argv[a], "-g") && a + 1 < argc) max_edits = atoi (argv[++a]);      /* the second pass of the lookup, as in located_tracts.c */
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
  /* contig names from the FASTA's headers, contig lengths from the delimiters of its stream */
  name_bytes = tjamd_read_file_names (reference, NULL, 0, &n_names);
  if (name_bytes < 0 || n_names != n_contigs) { fprintf (stderr, "cannot read the contig names of %s\n", reference); return 1; }
  names = (char *) malloc ((size_t) name_bytes + 1);
  tjamd_read_file_names (reference, names, name_bytes, &n_names);
  contig_name = (char **) malloc ((size_t) (n_contigs ? n_contigs : 1) * sizeof (char *));
  contig_len = (long *) malloc ((size_t) (n_contigs ? n_contigs : 1) * sizeof (long));
  {
    char *p = names;
    long from = 0, at, c = 0;
    for (i = 0; i < n_contigs; i++) { contig_name[i] = p; p = strchr (p, '\n'); *p++ = '\0'; }
    for (at = 0; at < ref_bytes && c < n_contigs; at++) if (ref_stream[at] == '\n') { contig_len[c++] = at - from; from = at + 1; }
  }
  free (ref_stream);
  d_loc = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_location));
  n_located = tjamd_locate (ctr[0], ref, d_keys, n_union, mism, (tjamd_location *) d_loc);
  if (n_located < 0) return fail ("locate");
  if (max_edits >= 0) {
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
  d_var = tjamd_device_alloc (ctr[0], (size_t) (n_tracts ? n_tracts : 1) * sizeof (int));
  if (tjamd_union_tract_stats (ctr[0], d_pkeys, d_pcounts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, coverage, (const int *) d_reflen,
                               (tjamd_union_tract_summary *) d_summary, (int *) d_var, &n_var, NULL, NULL) < 0) return fail ("tract statistics");

  /* the variants of the variable tracts: at most one record per (variable tract, sample), sample by sample */
  var_cap = n_var > 0 ? n_var * n : 1;
  d_variants = tjamd_device_alloc (ctr[0], (size_t) var_cap * sizeof (tjamd_variant));
  n_rec = tjamd_tract_variants (ctr[0], ref, d_pkeys, d_pcounts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, (const tjamd_location *) d_tloc,
                                (const int *) d_var, n_var, (tjamd_variant *) d_variants, var_cap, offsets);
  if (n_rec < 0) return fail ("tract variants");
  h_variants = (tjamd_variant *) malloc ((size_t) (n_rec ? n_rec : 1) * sizeof (tjamd_variant));
  if (tjamd_device_download (ctr[0], h_variants, d_variants, (size_t) n_rec * sizeof (tjamd_variant))) return fail ("download");
  printf ("%ld contigs, %ld runs indexed; %ld of %ld union rows located; %ld tracts by location, %ld variable; %ld variants in %d samples\n", n_contigs,
          tjamd_reference_entries (ref), n_located, n_union, n_tracts, n_var, n_rec, n);
  if (max_edits >= 0) printf ("%ld more union rows located within %d edits and a shift of %d\n", n_gapped, max_edits, max_shift);

  for (a = 0; a < n; a++) {
    const char *slash = strrchr (files[a], '/'), *base = slash ? slash + 1 : files[a];
    size_t len = strlen (base) + 5;
    char *sample = (char *) malloc (len), *file = (char *) malloc (len), *p;
    snprintf (sample, len, "%s", base);
    for (p = sample; *p; p++) if (*p == '/' || *p == '"' || *p == '\'' || *p == ' ' || *p == '\\') *p = '_';      /* :53 */
    snprintf (file, len, "%s.vcf", sample);
    if (!(fout = open_output (outdir, file))) return 1;
    fprintf (fout, "##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
                   "##INFO=<ID=TID,Number=A,Type=String,Description=\"tract ID\">\n");                             /* :57 */
    for (i = 0; i < n_contigs; i++) fprintf (fout, "##contig=<ID=%s,length=%ld>\n", contig_name[i], contig_len[i]);   /* :61-65 */
    fprintf (fout, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n", sample);                   /* :68 */
    for (i = offsets[a]; i < offsets[a + 1]; i++) {
      const tjamd_variant *v = h_variants + i;
      const char B = "ACGT"[v->base];
      int j, n_ref = (v->ref_length > v->alt_length ? v->ref_length - v->alt_length : 0) + 1,
             n_alt = (v->alt_length > v->ref_length ? v->alt_length - v->ref_length : 0) + 1;
      fprintf (fout, "%s\t%d\t.\t", contig_name[v->contig], v->pos);
      for (j = 0; j < n_ref; j++) fputc (B, fout);
      for (j = 0; j < v->n_flank; j++) fputc ("ACGT"[(v->ref_flank >> (2 * j)) & 3], fout);
      fputc ('\t', fout);
      for (j = 0; j < n_alt; j++) fputc (B, fout);
      for (j = 0; j < v->n_flank; j++) fputc ("ACGT"[(v->alt_flank >> (2 * j)) & 3], fout);
      fprintf (fout, "\t.\t.\tTID=tid_%06d\tGT\t1\n", v->tract);                                                  /* :183 */
    }
    fclose (fout);
    free (sample); free (file);
  }

  tjamd_reference_destroy (ref);
  tjamd_device_free (ctr[0], d_keys); tjamd_device_free (ctr[0], d_counts); tjamd_device_free (ctr[0], d_ids); tjamd_device_free (ctr[0], d_grouped);
  tjamd_device_free (ctr[0], d_loc); tjamd_device_free (ctr[0], d_perm); tjamd_device_free (ctr[0], d_pkeys); tjamd_device_free (ctr[0], d_pcounts);
  tjamd_device_free (ctr[0], d_tracts); tjamd_device_free (ctr[0], d_tloc); tjamd_device_free (ctr[0], d_reflen);
  tjamd_device_free (ctr[0], d_summary); tjamd_device_free (ctr[0], d_var); tjamd_device_free (ctr[0], d_variants);
  free (h_variants); free (names); free (contig_name); free (contig_len);
  for (a = 0; a < n; a++) tjamd_counter_destroy (ctr[a]);
  return 0;
}
