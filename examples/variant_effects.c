/* variant_effects.c -- what each sample's tract-length variants do to the proteins of a GFF3 annotation, through the C ABI and
 * nothing else: the pipeline of annotated_tracts.c (scan, finalise, gather, merge, group, index the reference, locate, tracts by
 * location, statistics, the feature of every tract) and of sample_vcfs.c (tjamd_tract_variants on the variable tracts), then
 * the coding table of the genome and the annotation's CDS lines (tjamd_coding_create, with the phase column) and
 * tjamd_variant_effects on the variant records.  The reference program stops at the VCF files and sends the user to snpEff,
 * VEP or bcftools for this.
 *   DIR/variant_effects.tsv   one line per variant record, sample by sample: sample (as sample_vcfs.c names it), tid_%06d,
 *                             contig, POS, REF, ALT, the feature's ID (unannotated if none), the class (NONE, BOUNDARY, IDENTICAL,
 *                             INFRAME, FRAMESHIFT), cds_pos, the 1-based first amino acid that differs (0 if none), the up to
 *                             eight amino acids from there on in the reference and in the sample ("." if none), and the two
 *                             protein lengths
 * Options are annotated_tracts.c's.
 *
 *   gcc -O2 -I include examples/variant_effects.c -L tatajuba_amd -ltatajuba_amd -Wl,-rpath,$PWD/tatajuba_amd -o variant_effects
 *   ./variant_effects -r reference.fa -g annotation.gff3 [-x 1] [-k 10] [-m 3] [-c 5] [-d 1] [-l -1] [-o .] sample1.fastq[.gz] ...   */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tatajuba_effects.h>

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

/* the up to eight symbols of a window, "." if it is empty */
static const char *
window_text (uint64_t w, char *buf)
{
  int j;
  for (j = 0; j < 8 && ((w >> (8 * j)) & 0xff); j++) buf[j] = (char) ((w >> (8 * j)) & 0xff);
  buf[j] = '\0';
  return j ? buf : ".";
}

int
main (int argc, char **argv)
{
  static const char *class_name[5] = {"NONE", "BOUNDARY", "IDENTICAL", "INFRAME", "FRAMESHIFT"};
  tjamd_counter *ctr[MAX_SAMPLES];
  const char *files[MAX_SAMPLES], *outdir = ".", *reference = NULL, *gff = NULL;
  long counts[MAX_SAMPLES], offsets[MAX_SAMPLES + 1], total, n_union, n_grouped, n_tracts, n_located, n_var = 0, n_rec, i, cap, ref_bytes, n_contigs = 0, n_names = 0,
       name_bytes, n_features, string_bytes = 0, n_skipped = 0, nt1, var_cap, n_class[5] = {0, 0, 0, 0, 0};
  int n = 0, k = 10, m = 3, cov = 5, maxd = 1, lev = -1, mism = 1, coverage[MAX_SAMPLES], a, ndev = tjamd_device_count (), status;
  const void *d_records = NULL;
  void *d_keys, *d_counts, *d_ids, *d_grouped, *d_loc, *d_perm, *d_pkeys, *d_pcounts, *d_tracts, *d_tloc, *d_reflen, *d_summary, *d_var, *d_tf, *d_variants, *d_effects;
  unsigned char *ref_stream;
  char *names, **contig_name, *strings;
  signed char *phase;
  tjamd_reference *ref;
  tjamd_annotation *ann;
  tjamd_coding *cod;
  tjamd_feature *features;
  tjamd_variant *h_variants;
  tjamd_effect *h_effects;
  FILE *fout;

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

  /* the reference: the index of its runs and the names of its contigs; the annotation: its features and their phases; the
   * coding table: the genome's bases and where each CDS line's protein ends */
  ref_bytes = tjamd_read_file_stream (reference, NULL, 0, &n_contigs);
  if (ref_bytes < 0) { fprintf (stderr, "cannot read %s\n", reference); return 1; }
  ref_stream = (unsigned char *) malloc ((size_t) ref_bytes + 1);
  tjamd_read_file_stream (reference, ref_stream, ref_bytes, &n_contigs);
  ref = tjamd_reference_create (ctr[0], ref_stream, (size_t) ref_bytes);
  if (!ref) return fail (reference);
  name_bytes = tjamd_read_file_names (reference, NULL, 0, &n_names);
  if (name_bytes < 0 || n_names != n_contigs) { fprintf (stderr, "cannot read the contig names of %s\n", reference); return 1; }
  names = (char *) malloc ((size_t) name_bytes + 1);
  contig_name = (char **) malloc ((size_t) (n_names ? n_names : 1) * sizeof (char *));
  tjamd_read_file_names (reference, names, name_bytes, &n_names);
  n_features = tjamd_gff3_read (gff, names, n_names, NULL, 0, NULL, 0, &string_bytes, &n_skipped);
  if (n_features < 0) { fprintf (stderr, "cannot read %s\n", gff); return 1; }
  features = (tjamd_feature *) malloc ((size_t) (n_features ? n_features : 1) * sizeof (tjamd_feature));
  strings = (char *) malloc ((size_t) string_bytes + 1);
  phase = (signed char *) malloc ((size_t) (n_features ? n_features : 1));
  tjamd_gff3_read (gff, names, n_names, features, n_features, strings, string_bytes, &string_bytes, &n_skipped);
  if (tjamd_gff3_read_phase (gff, names, n_names, phase, n_features) != n_features) { fprintf (stderr, "cannot read the phases of %s\n", gff); return 1; }
  for (i = 0, a = 0; i < n_names; i++) {                  /* (after the GFF3 is read: the names become C strings) */
    contig_name[i] = names + a;
    while (names[a] != '\n') a++;
    names[a++] = '\0';
  }
  ann = tjamd_annotation_create (ctr[0], ref, features, n_features);
  if (!ann) return fail (gff);
  cod = tjamd_coding_create (ctr[0], ref_stream, (size_t) ref_bytes, features, n_features, phase);
  if (!cod) return fail ("coding table");
  free (ref_stream);
  d_loc = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_location));
  n_located = tjamd_locate (ctr[0], ref, d_keys, n_union, mism, (tjamd_location *) d_loc);
  if (n_located < 0) return fail ("locate");

  /* tracts by location, the variable ones, each tract's feature, the variants of the variable tracts and their effects */
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
  d_var = tjamd_device_alloc (ctr[0], (size_t) nt1 * sizeof (int));
  d_tf = tjamd_device_alloc (ctr[0], (size_t) nt1 * sizeof (tjamd_tract_feature));
  if (tjamd_union_tract_stats (ctr[0], d_pkeys, d_pcounts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, coverage, (const int *) d_reflen,
                               (tjamd_union_tract_summary *) d_summary, (int *) d_var, &n_var, NULL, NULL) < 0) return fail ("tract statistics");
  if (tjamd_tract_features (ctr[0], ann, d_pkeys, d_pcounts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, (const tjamd_location *) d_tloc,
                            (tjamd_tract_feature *) d_tf) < 0) return fail ("tract features");
  var_cap = n_var > 0 ? n_var * n : 1;
  d_variants = tjamd_device_alloc (ctr[0], (size_t) var_cap * sizeof (tjamd_variant));
  d_effects = tjamd_device_alloc (ctr[0], (size_t) var_cap * sizeof (tjamd_effect));
  n_rec = tjamd_tract_variants (ctr[0], ref, d_pkeys, d_pcounts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, (const tjamd_location *) d_tloc,
                                (const int *) d_var, n_var, (tjamd_variant *) d_variants, var_cap, offsets);
  if (n_rec < 0) return fail ("tract variants");
  if (tjamd_variant_effects (ctr[0], cod, (const tjamd_variant *) d_variants, n_rec, (const tjamd_tract_feature *) d_tf, n_tracts, (tjamd_effect *) d_effects) < 0)
    return fail ("variant effects");
  h_variants = (tjamd_variant *) malloc ((size_t) (n_rec ? n_rec : 1) * sizeof (tjamd_variant));
  h_effects = (tjamd_effect *) malloc ((size_t) (n_rec ? n_rec : 1) * sizeof (tjamd_effect));
  if (tjamd_device_download (ctr[0], h_variants, d_variants, (size_t) n_rec * sizeof (tjamd_variant)) ||
      tjamd_device_download (ctr[0], h_effects, d_effects, (size_t) n_rec * sizeof (tjamd_effect))) return fail ("download");
  printf ("%ld contigs, %ld runs indexed; %ld features read, %ld lines skipped; %ld of %ld union rows located; %ld tracts by location, %ld variable\n",
          n_contigs, tjamd_reference_entries (ref), n_features, n_skipped, n_located, n_union, n_tracts, n_var);

  if (!(fout = open_output (outdir, "variant_effects.tsv"))) return 1;
  fprintf (fout, "sample\ttract_id\tcontig_name\tpos\tref\talt\tfeature\teffect\tcds_pos\tfirst_diff\tref_aa\talt_aa\tref_aa_len\talt_aa_len\n");
  for (a = 0; a < n; a++) {
    const char *slash = strrchr (files[a], '/'), *base = slash ? slash + 1 : files[a];
    size_t len = strlen (base) + 1;
    char *sample = (char *) malloc (len), *p;
    snprintf (sample, len, "%s", base);
    for (p = sample; *p; p++) if (*p == '/' || *p == '"' || *p == '\'' || *p == ' ' || *p == '\\') *p = '_';      /* as sample_vcfs.c names it */
    for (i = offsets[a]; i < offsets[a + 1]; i++) {
      const tjamd_variant *v = h_variants + i;
      const tjamd_effect *e = h_effects + i;
      const char B = "ACGT"[v->base & 3];
      char wr[9], wa[9];
      int j, n_ref = (v->ref_length > v->alt_length ? v->ref_length - v->alt_length : 0) + 1,
             n_alt = (v->alt_length > v->ref_length ? v->alt_length - v->ref_length : 0) + 1;
      fprintf (fout, "%s\ttid_%06d\t%s\t%d\t", sample, v->tract, contig_name[v->contig], v->pos);
      for (j = 0; j < n_ref; j++) fputc (B, fout);
      for (j = 0; j < v->n_flank; j++) fputc ("ACGT"[(v->ref_flank >> (2 * j)) & 3], fout);
      fputc ('\t', fout);
      for (j = 0; j < n_alt; j++) fputc (B, fout);
      for (j = 0; j < v->n_flank; j++) fputc ("ACGT"[(v->alt_flank >> (2 * j)) & 3], fout);
      fprintf (fout, "\t%s\t%s\t%d\t%d\t%s\t%s\t%d\t%d\n", e->feature >= 0 ? strings + features[e->feature].id_off : "unannotated", class_name[e->cls], e->cds_pos,
               e->first_diff + 1, window_text (e->ref_aa, wr), window_text (e->alt_aa, wa), e->ref_aa_len, e->alt_aa_len);
      n_class[e->cls]++;
    }
    free (sample);
  }
  fclose (fout);
  printf ("%ld variants in %d samples: %ld outside coding features, %ld across a boundary, %ld identical, %ld in frame, %ld frameshifts\n", n_rec, n,
          n_class[TJAMD_EFFECT_NONE], n_class[TJAMD_EFFECT_BOUNDARY], n_class[TJAMD_EFFECT_IDENTICAL], n_class[TJAMD_EFFECT_INFRAME], n_class[TJAMD_EFFECT_FRAMESHIFT]);

  tjamd_coding_destroy (cod);
  tjamd_annotation_destroy (ann);
  tjamd_reference_destroy (ref);
  tjamd_device_free (ctr[0], d_keys); tjamd_device_free (ctr[0], d_counts); tjamd_device_free (ctr[0], d_ids); tjamd_device_free (ctr[0], d_grouped);
  tjamd_device_free (ctr[0], d_loc); tjamd_device_free (ctr[0], d_perm); tjamd_device_free (ctr[0], d_pkeys); tjamd_device_free (ctr[0], d_pcounts);
  tjamd_device_free (ctr[0], d_tracts); tjamd_device_free (ctr[0], d_tloc); tjamd_device_free (ctr[0], d_reflen);
  tjamd_device_free (ctr[0], d_summary); tjamd_device_free (ctr[0], d_var); tjamd_device_free (ctr[0], d_tf);
  tjamd_device_free (ctr[0], d_variants); tjamd_device_free (ctr[0], d_effects);
  free (h_variants); free (h_effects); free (features); free (strings); free (phase); free (names); free (contig_name);
  for (a = 0; a < n; a++) tjamd_counter_destroy (ctr[a]);
  return 0;
}
