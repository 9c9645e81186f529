/* merged_vcf.c -- one multi-sample VCF with every sample's tract-length variants against the reference genome, through the C
 * ABI and nothing else.  The reference program writes one VCF per sample and leaves the rest to its user (docs/tutorial.md,
 * "Downstream analyses": sort | uniq over the files, or bcftools norm, index and merge); here the pipeline of sample_vcfs.c
 * (scan, finalise, gather, merge, group, index the reference, locate, tracts by location, statistics, tjamd_tract_variants on
 * the variable tracts) is followed by tjamd_merge_variants on the records where they are, on the device:
 *   DIR/merged.vcf            sample_vcfs.c's header with ##INFO lines for AC and AN and one column per sample; one row per
 *                             site, ALT comma-separated in allele order, haploid GT 1, 2, ... or "." where the sample has no record:
 *                             contig  POS  .  REF  ALT1,ALT2  .  .  AC=n1,n2;AN=n_called;TID=tid_%06d  GT  g0  g1 ...
 *                             with -D: tjamd_site_depths after the merge; FORMAT is GT:DP:AD, GT is 0 where the sample's reads
 *                             show the genome's own length and "." only where it was not seen, AN counts the reference samples too
 *   DIR/sample_distances.tsv  with -M: tjamd_sample_distances on the genotype matrix the run has (that of the depths with -D, that of
 *                             the merge without, where samples that equal the reference count as not called), one row per pair
 *                             of samples a <= b: sample_a  sample_b  n_both  n_differ  length_diff
 *   DIR/sample_linkage.tsv    with -C T (which implies -M): tjamd_sample_linkage on that matrix, by n_differ over the pairs with at
 *                             least one site in common; one line per link, in the order single linkage merges: sample_a  sample_b  key
 *                             with -L complete or -L average (only together with -C T; -L single is the default): the links of
 *                             tjamd_sample_agglomerate under that linkage instead, in the order (key, round, a, b), and the clusters, the
 *                             cluster sites, the tree and the clade sites below are built from them
 *   DIR/sample_clusters.tsv   with -C T: tjamd_linkage_clusters at threshold T, one line per sample: sample  cluster
 *   DIR/cluster_sites.tsv     with -G (only together with -C T): tjamd_group_sites on that genotype matrix with the clusters as the groups and a
 *                             min_called of 1: the sites at which every called sample of a cluster carries one genotype that no called
 *                             sample outside it carries, one line per (site, cluster) in that order: cluster  contig  POS  REF  the
 *                             genotype's text (REF again for genotype 0)  the cluster's called samples
 *   DIR/sample_tree.nwk       with -N (only together with -C T): tjamd_linkage_tree on the links and tjamd_clade_sites on that genotype matrix with a
 *                             min_called of 1; one Newick line per root of the tree, the roots in the order of their smallest sample:
 *                             (left,right)label:length; with a sample's name for a leaf, the number of sites that support the clade
 *                             (d_node_marks) as an inner node's label, and as a branch's length the key of the parent's link minus the key of
 *                             the child's own (0 for a leaf); a root's branch has length 0
 *   DIR/clade_sites.tsv       with -N: the sites at which every called sample of a node's clade carries one genotype that no called sample
 *                             outside it carries, one line per (site, node) in that order: node  contig  POS  REF  the genotype's text
 *                             (REF again for genotype 0)  the clade's called samples
 *   DIR/clade_support.tsv     with -B R[:seed] (only together with -C T -N): the bootstrap over sites.  tjamd_bootstrap_weights draws R rows of site
 *                             weights (seed 1 unless given), tjamd_sample_distances_weighted gives the R matrices in one call, tjamd_replicate_trees
 *                             builds every replicate's tree as the tree above was (the linkage -L chose) in one call, and tjamd_clade_support counts the
 *                             replicates that hold each clade; one line per node of the tree: node  size  the name of its smallest sample  the
 *                             key of its link  the sites that support it (the label in sample_tree.nwk)  the replicates that hold it  R
 *   DIR/consensus_tree.nwk    with -K [percent] (only together with -C T -N -B R): tjamd_consensus_tree on the R replicate trees, the clades that
 *                             more than half of the replicates hold (with a percentage above 50: at least ceil (percent * R / 100) of them), in Newick
 *                             with several children per node where the replicates disagree; the label of an inner node is the number of
 *                             replicates that hold its clade, and there are no branch lengths; a root per line
 *   DIR/consensus_clades.tsv  with -K: one line per node of the consensus tree: node  parent (-1: a root)  size  the replicates that hold it  R
 *                             its samples, separated by commas, in the order of the tree's leaves
 *   DIR/unique_variants.vcf   with -u: the tutorial's concatenation, one row per distinct allele in N8's own form (the record
 *                             d_unique holds), one column all_samples
 *   DIR/variant_effects.tsv   with -e annotation.gff3: tjamd_variant_effects on d_unique only, one line per allele: variant_effects.c's
 *                             columns without the sample, then the number of samples that carry the allele
 * The other options are sample_vcfs.c's.
 *
 *   gcc -O2 -I include examples/merged_vcf.c -L tatajuba_amd -ltatajuba_amd -Wl,-rpath,$PWD/tatajuba_amd -o merged_vcf
 *   ./merged_vcf -r reference.fa [-u] [-D] [-M] [-C T [-G] [-N [-B R[:seed] [-K [percent]]]] [-L single|complete|average]] [-e annotation.gff3] [-x 1] [-g G] [-s 3] [-k 10] [-m 3] [-c 5] [-d 1] [-l -1] [-o .] sample1.fastq[.gz] ...   */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tatajuba_consensus.h>
#include <tatajuba_effects.h>
#include <tatajuba_locate.h>

#define MAX_SAMPLES 64

static int
fail (const char *what)
{
  fprintf (stderr, "%s: %s\n", what, tjamd_last_error ());
  return 1;
}

/* the up to eight symbols of a window, "." if it is empty (variant_effects.c) */
static const char *
window_text (uint64_t w, char *buf)
{
  int j;
  for (j = 0; j < 8 && ((w >> (8 * j)) & 0xff); j++) buf[j] = (char) ((w >> (8 * j)) & 0xff);
  buf[j] = '\0';
  return j ? buf : ".";
}

/* REF and ALT of a variant record in N8's own form (sample_vcfs.c) */
static void
print_ref_alt (FILE *fout, const tjamd_variant *v)
{
  const char B = "ACGT"[v->base & 3];
  int j, n_ref = (v->ref_length > v->alt_length ? v->ref_length - v->alt_length : 0) + 1,
         n_alt = (v->alt_length > v->ref_length ? v->alt_length - v->ref_length : 0) + 1;
  for (j = 0; j < n_ref; j++) fputc (B, fout);
  for (j = 0; j < v->n_flank; j++) fputc ("ACGT"[(v->ref_flank >> (2 * j)) & 3], fout);
  fputc ('\t', fout);
  for (j = 0; j < n_alt; j++) fputc (B, fout);
  for (j = 0; j < v->n_flank; j++) fputc ("ACGT"[(v->alt_flank >> (2 * j)) & 3], fout);
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

/* a child of the tree in Newick: a sample's name, or (left,right) and the node's marks; then the branch to its parent */
static void
print_clade (FILE *fout, int child, long long parent_key, const tjamd_tree_node *nodes, const tjamd_link *links, const int *node_marks, char **sample_name)
{
  if (child < 0) { fprintf (fout, "%s:%lld", sample_name[-1 - child], parent_key); return; }
  fputc ('(', fout);
  print_clade (fout, nodes[child].left, links[child].key, nodes, links, node_marks, sample_name);
  fputc (',', fout);
  print_clade (fout, nodes[child].right, links[child].key, nodes, links, node_marks, sample_name);
  fprintf (fout, ")%d:%lld", node_marks[child], parent_key - links[child].key);
}

/* node j of the consensus tree in Newick, or with j == -1 its roots, one per line: a node's children are the nodes under it
 * and the samples of its interval that lie in none of them, in the order of the leaves; the label is the node's count */
static void
print_consensus (FILE *fout, int j, const tjamd_consensus_node *nodes, int n_nodes, const int *order, int n, char **sample_name)
{
  int p = j < 0 ? 0 : nodes[j].first, i;
  const int end = j < 0 ? n : p + nodes[j].size;
  if (j >= 0) fputc ('(', fout);
  while (p < end) {
    int child = -1;
    for (i = 0; i < n_nodes; i++) if (nodes[i].parent == j && nodes[i].first == p) child = i;
    if (j >= 0 && p > nodes[j].first) fputc (',', fout);
    if (child >= 0) { print_consensus (fout, child, nodes, n_nodes, order, n, sample_name); p += nodes[child].size; }
    else fprintf (fout, "%s", sample_name[order[p++]]);
    if (j < 0) fprintf (fout, ";\n");
  }
  if (j >= 0) fprintf (fout, ")%d", nodes[j].count);
}

int
main (int argc, char **argv)
{
  tjamd_counter *ctr[MAX_SAMPLES];
  const char *files[MAX_SAMPLES], *outdir = ".", *reference = NULL, *gff = NULL;
  static const char *class_name[5] = {"NONE", "BOUNDARY", "IDENTICAL", "INFRAME", "FRAMESHIFT"};
  long counts[MAX_SAMPLES], total, n_union, n_grouped, n_tracts, n_located, n_gapped = 0, n_var = 0, n_rec, i, cap, ref_bytes, n_contigs = 0, n_names = 0, name_bytes;
  long offsets[MAX_SAMPLES + 1], *contig_len, var_cap, n_sites, n_alleles = 0, s, text_cap = 0;
  int with_unique = 0, with_depths = 0, with_distances = 0, with_clusters = 0, with_groups = 0, with_clades = 0, with_linkage = 0, linkage = 0;
  long long cut = 0;
  long n_links = 0, n_clusters = 0, n_marks = 0;
  tjamd_link *h_links = NULL;
  int *h_cluster = NULL;
  tjamd_group_mark *h_marks = NULL, *h_clade_marks = NULL;
  tjamd_tree_node *h_nodes = NULL;
  int *h_order = NULL, *h_node_marks = NULL;
  long n_clade_marks = 0;
  int n_boot = 0, *h_support = NULL;                      /* -B: the replicates, and per node of the tree those that hold its clade */
  unsigned long long boot_seed = 1;
  int with_consensus = 0, cons_min = 0, *h_cons_order = NULL; /* -K: the consensus of the replicates; the replicates a kept clade needs */
  double cons_percent = 0;                                /* 0: more than half */
  long n_cons = 0;
  tjamd_consensus_node *h_cons = NULL;
  int n = 0, k = 10, m = 3, cov = 5, maxd = 1, lev = -1, mism = 1, max_edits = -1, max_shift = TJAMD_MAX_SHIFT, coverage[MAX_SAMPLES], a, ndev = tjamd_device_count (), status;
  const void *d_records = NULL;
  void *d_keys, *d_counts, *d_ids, *d_grouped, *d_loc, *d_perm, *d_pkeys, *d_pcounts, *d_tracts, *d_tloc, *d_reflen, *d_summary, *d_var, *d_variants, *d_sites, *d_alleles, *d_genotype, *d_unique,
       *d_dp = NULL, *d_ad = NULL, *d_sd = NULL;
  unsigned char *ref_stream;
  char *names, **contig_name;
  tjamd_reference *ref;
  tjamd_variant *h_unique;
  tjamd_site *h_sites;
  tjamd_allele *h_alleles;
  int16_t *h_genotype;
  int *h_dp = NULL, *h_ad = NULL;
  tjamd_site_depth *h_sd = NULL;
  tjamd_sample_distance *h_dist = NULL;
  char *text, **sample_name;
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
    else if (!strcmp (argv[a], "-e") && a + 1 < argc) gff = argv[++a];
    else if (!strcmp (argv[a], "-u")) with_unique = 1;
    else if (!strcmp (argv[a], "-D")) with_depths = 1;
    else if (!strcmp (argv[a], "-M")) with_distances = 1;
    else if (!strcmp (argv[a], "-C") && a + 1 < argc) { cut = atoll (argv[++a]); with_clusters = with_distances = 1; }
    else if (!strcmp (argv[a], "-G")) with_groups = 1;
    else if (!strcmp (argv[a], "-N")) with_clades = 1;
    else if (!strcmp (argv[a], "-B") && a + 1 < argc) {   /* R or R:seed */
      const char *colon = strchr (argv[++a], ':');
      n_boot = atoi (argv[a]);
      if (colon) boot_seed = strtoull (colon + 1, NULL, 10);
      if (n_boot < 1 || n_boot > 4096) n_boot = -1;
    }
    else if (!strcmp (argv[a], "-K")) {                   /* alone, or with a percentage above 50 */
      char *end = NULL;
      with_consensus = 1;
      if (a + 1 < argc && argv[a + 1][0] >= '0' && argv[a + 1][0] <= '9' && (cons_percent = strtod (argv[a + 1], &end), end && !*end)) {
        a++;
        if (!(cons_percent > 50 && cons_percent <= 100)) with_consensus = -1;
      } else cons_percent = 0;
    }
    else if (!strcmp (argv[a], "-L") && a + 1 < argc) {   /* which tree: 0 single linkage (tjamd_sample_linkage), else TJAMD_AGGL_* */
      a++; with_linkage = 1;
      if (!strcmp (argv[a], "single")) linkage = 0;
      else if (!strcmp (argv[a], "complete")) linkage = TJAMD_AGGL_COMPLETE;
      else if (!strcmp (argv[a], "average")) linkage = TJAMD_AGGL_AVERAGE;
      else linkage = -1;
    }
    else if (n < MAX_SAMPLES) files[n++] = argv[a];
  }
  if (n < 1 || !reference || ((with_groups || with_clades || with_linkage) && !with_clusters) || linkage < 0 || n_boot < 0 || (n_boot && !with_clades) || with_consensus < 0 || (with_consensus && !n_boot)) { fprintf (stderr, "usage: %s -r reference.fa [-u] [-D] [-M] [-C T [-G] [-N [-B R[:seed] [-K [percent]]]] [-L single|complete|average]] [-e annotation.gff3] [-x X] [-g G] [-s S] [-k K] [-m M] [-c C] [-d D] [-l L] [-o DIR] sample.fastq[.gz] ...\n", argv[0]); return 2; }
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

  /* the records of all samples -> sites, their alleles, a genotype per (site, sample), one record per allele */
  cap = n_rec ? n_rec : 1;
  d_sites = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_site));
  d_alleles = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_allele));
  d_genotype = tjamd_device_alloc (ctr[0], (size_t) cap * (size_t) n * sizeof (int16_t));
  d_unique = tjamd_device_alloc (ctr[0], (size_t) cap * sizeof (tjamd_variant));
  n_sites = tjamd_merge_variants (ctr[0], k, (const tjamd_variant *) d_variants, n_rec, n, n_tracts, (tjamd_site *) d_sites, cap, (tjamd_allele *) d_alleles, cap,
                                  (int16_t *) d_genotype, NULL, (tjamd_variant *) d_unique, &n_alleles);
  if (n_sites < 0) return fail ("merge variants");
  if (with_depths) {                                      /* the same union and tiling once more: depths, and 0 or -1 where N12 has -1 */
    const size_t cells = (size_t) (n_sites ? n_sites : 1) * (size_t) n, ad_cells = (size_t) (n_sites + n_alleles ? n_sites + n_alleles : 1) * (size_t) n;
    d_dp = tjamd_device_alloc (ctr[0], cells * sizeof (int));
    d_ad = tjamd_device_alloc (ctr[0], ad_cells * sizeof (int));
    d_sd = tjamd_device_alloc (ctr[0], (size_t) (n_sites ? n_sites : 1) * sizeof (tjamd_site_depth));
    if (tjamd_site_depths (ctr[0], ref, d_pkeys, d_pcounts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, (const tjamd_location *) d_tloc,
                           (const tjamd_site *) d_sites, n_sites, (const tjamd_allele *) d_alleles, n_alleles, (int16_t *) d_genotype, (int *) d_dp, (int *) d_ad,
                           (tjamd_site_depth *) d_sd) < 0) return fail ("site depths");
    h_dp = (int *) malloc (cells * sizeof (int));
    h_ad = (int *) malloc (ad_cells * sizeof (int));
    h_sd = (tjamd_site_depth *) malloc ((size_t) (n_sites ? n_sites : 1) * sizeof (tjamd_site_depth));
    if (tjamd_device_download (ctr[0], h_dp, d_dp, (size_t) n_sites * (size_t) n * sizeof (int)) ||
        tjamd_device_download (ctr[0], h_ad, d_ad, (size_t) (n_sites + n_alleles) * (size_t) n * sizeof (int)) ||
        tjamd_device_download (ctr[0], h_sd, d_sd, (size_t) n_sites * sizeof (tjamd_site_depth))) return fail ("download");
  }
  if (with_distances) {                                   /* how far apart the samples are, on the genotypes the run has by now */
    void *d_dist = tjamd_device_alloc (ctr[0], (size_t) n * (size_t) n * sizeof (tjamd_sample_distance));
    if (tjamd_sample_distances (ctr[0], (const tjamd_site *) d_sites, n_sites, (const tjamd_allele *) d_alleles, n_alleles, (const int16_t *) d_genotype, n,
                                (tjamd_sample_distance *) d_dist) < 0) return fail ("sample distances");
    h_dist = (tjamd_sample_distance *) malloc ((size_t) n * (size_t) n * sizeof (tjamd_sample_distance));
    if (tjamd_device_download (ctr[0], h_dist, d_dist, (size_t) n * (size_t) n * sizeof (tjamd_sample_distance))) return fail ("download");
    if (with_clusters) {                                  /* the tree of the samples from the matrix where it is, and its cut at T */
      void *d_links = tjamd_device_alloc (ctr[0], (size_t) n * sizeof (tjamd_link)), *d_cluster = tjamd_device_alloc (ctr[0], (size_t) n * sizeof (int));
      n_links = linkage ? tjamd_sample_agglomerate (ctr[0], (const tjamd_sample_distance *) d_dist, n, TJAMD_LINK_DIFFER, 1, linkage, (tjamd_link *) d_links, NULL)
                        : tjamd_sample_linkage (ctr[0], (const tjamd_sample_distance *) d_dist, n, TJAMD_LINK_DIFFER, 1, (tjamd_link *) d_links);
      if (n_links < 0) return fail ("sample linkage");
      n_clusters = tjamd_linkage_clusters (ctr[0], (const tjamd_link *) d_links, n_links, n, cut, (int *) d_cluster);
      if (n_clusters < 0) return fail ("linkage clusters");
      h_links = (tjamd_link *) malloc ((size_t) n * sizeof (tjamd_link));
      h_cluster = (int *) malloc ((size_t) n * sizeof (int));
      if (tjamd_device_download (ctr[0], h_links, d_links, (size_t) n_links * sizeof (tjamd_link)) ||
          tjamd_device_download (ctr[0], h_cluster, d_cluster, (size_t) n * sizeof (int))) return fail ("download");
      if (with_groups) {                                  /* what sets each cluster apart: the genotypes and the labels where they are; sized first, the list is short */
        void *d_marks;
        long rc = tjamd_group_sites (ctr[0], (const tjamd_site *) d_sites, n_sites, (const int16_t *) d_genotype, n, (const int *) d_cluster, (int) n_clusters, 1,
                                     NULL, NULL, NULL, NULL, 0, &n_marks);
        if (rc < 0 && rc != -TJAMD_ERR_CAPACITY) return fail ("group sites");
        d_marks = tjamd_device_alloc (ctr[0], (size_t) (n_marks ? n_marks : 1) * sizeof (tjamd_group_mark));
        if (tjamd_group_sites (ctr[0], (const tjamd_site *) d_sites, n_sites, (const int16_t *) d_genotype, n, (const int *) d_cluster, (int) n_clusters, 1,
                               NULL, NULL, NULL, (tjamd_group_mark *) d_marks, n_marks, &n_marks) < 0) return fail ("group sites");
        h_marks = (tjamd_group_mark *) malloc ((size_t) (n_marks ? n_marks : 1) * sizeof (tjamd_group_mark));
        if (tjamd_device_download (ctr[0], h_marks, d_marks, (size_t) n_marks * sizeof (tjamd_group_mark))) return fail ("download");
        tjamd_device_free (ctr[0], d_marks);
      }
      if (with_clades) {                                  /* the links as a tree, and what supports each of its clades: no threshold; sized first, the list is short */
        void *d_nodes = tjamd_device_alloc (ctr[0], (size_t) n * sizeof (tjamd_tree_node)), *d_order = tjamd_device_alloc (ctr[0], (size_t) n * sizeof (int)),
             *d_node_marks = tjamd_device_alloc (ctr[0], (size_t) n * sizeof (int)), *d_marks;
        long rc;
        if (tjamd_linkage_tree (ctr[0], (const tjamd_link *) d_links, n_links, n, (tjamd_tree_node *) d_nodes, (int *) d_order) < 0) return fail ("linkage tree");
        rc = tjamd_clade_sites (ctr[0], (const tjamd_site *) d_sites, n_sites, (const int16_t *) d_genotype, n, (const tjamd_tree_node *) d_nodes, (int) n_links, (const int *) d_order, 1,
                                NULL, NULL, NULL, NULL, 0, &n_clade_marks);
        if (rc < 0 && rc != -TJAMD_ERR_CAPACITY) return fail ("clade sites");
        d_marks = tjamd_device_alloc (ctr[0], (size_t) (n_clade_marks ? n_clade_marks : 1) * sizeof (tjamd_group_mark));
        if (tjamd_clade_sites (ctr[0], (const tjamd_site *) d_sites, n_sites, (const int16_t *) d_genotype, n, (const tjamd_tree_node *) d_nodes, (int) n_links, (const int *) d_order, 1,
                               NULL, NULL, (int *) d_node_marks, (tjamd_group_mark *) d_marks, n_clade_marks, &n_clade_marks) < 0) return fail ("clade sites");
        h_nodes = (tjamd_tree_node *) malloc ((size_t) n * sizeof (tjamd_tree_node));
        h_order = (int *) malloc ((size_t) n * sizeof (int));
        h_node_marks = (int *) malloc ((size_t) n * sizeof (int));
        h_clade_marks = (tjamd_group_mark *) malloc ((size_t) (n_clade_marks ? n_clade_marks : 1) * sizeof (tjamd_group_mark));
        if (tjamd_device_download (ctr[0], h_nodes, d_nodes, (size_t) n_links * sizeof (tjamd_tree_node)) ||
            tjamd_device_download (ctr[0], h_order, d_order, (size_t) n * sizeof (int)) ||
            tjamd_device_download (ctr[0], h_node_marks, d_node_marks, (size_t) n_links * sizeof (int)) ||
            tjamd_device_download (ctr[0], h_clade_marks, d_marks, (size_t) n_clade_marks * sizeof (tjamd_group_mark))) return fail ("download");
        if (n_boot) {                                     /* how many of R trees over resampled sites hold each clade of this one */
          const size_t R = (size_t) n_boot;
          void *d_weights = tjamd_device_alloc (ctr[0], R * (size_t) (n_sites ? n_sites : 1) * sizeof (int)),
               *d_rep_dist = tjamd_device_alloc (ctr[0], R * (size_t) n * (size_t) n * sizeof (tjamd_sample_distance)),
               *d_rep_nodes = tjamd_device_alloc (ctr[0], R * (size_t) n * sizeof (tjamd_tree_node)), *d_rep_order = tjamd_device_alloc (ctr[0], R * (size_t) n * sizeof (int)),
               *d_support = tjamd_device_alloc (ctr[0], (size_t) n * sizeof (int));
          int *rep_n_nodes = (int *) malloc (R * sizeof (int));
          h_support = (int *) calloc ((size_t) n, sizeof (int));
          if (n_sites > 0 && tjamd_bootstrap_weights (ctr[0], n_sites, n_boot, boot_seed, (int *) d_weights) < 0) return fail ("bootstrap weights");
          if (tjamd_sample_distances_weighted (ctr[0], (const tjamd_site *) d_sites, n_sites, (const tjamd_allele *) d_alleles, n_alleles, (const int16_t *) d_genotype, n,
                                               (tjamd_sample_distance *) d_rep_dist, (const int *) d_weights, n_boot) < 0) return fail ("weighted sample distances");
          /* every replicate's tree, built as the tree was (linkage: 0 is TJAMD_TREE_SINGLE, else TJAMD_AGGL_*); the links are not kept */
          if (tjamd_replicate_trees (ctr[0], (const tjamd_sample_distance *) d_rep_dist, n, n_boot, TJAMD_LINK_DIFFER, 1, linkage, NULL, (tjamd_tree_node *) d_rep_nodes,
                                     (int *) d_rep_order, rep_n_nodes, NULL) < 0) return fail ("replicate trees");
          if (tjamd_clade_support (ctr[0], (const tjamd_tree_node *) d_nodes, (int) n_links, (const int *) d_order, n, (const tjamd_tree_node *) d_rep_nodes,
                                   (const int *) d_rep_order, rep_n_nodes, n_boot, (int *) d_support) < 0) return fail ("clade support");
          if (tjamd_device_download (ctr[0], h_support, d_support, (size_t) n_links * sizeof (int))) return fail ("download");
          if (with_consensus) {                           /* what the replicates agree on among themselves, whatever the tree above holds */
            void *d_cons = tjamd_device_alloc (ctr[0], (size_t) n * sizeof (tjamd_consensus_node)), *d_cons_order = tjamd_device_alloc (ctr[0], (size_t) n * sizeof (int));
            cons_min = n_boot / 2 + 1;
            if (cons_percent > 0) { cons_min = (int) (cons_percent * n_boot / 100.0); if (cons_min * 100.0 < cons_percent * n_boot) cons_min++; }
            h_cons = (tjamd_consensus_node *) malloc ((size_t) n * sizeof (tjamd_consensus_node));
            h_cons_order = (int *) malloc ((size_t) n * sizeof (int));
            n_cons = tjamd_consensus_tree (ctr[0], (const tjamd_tree_node *) d_rep_nodes, (const int *) d_rep_order, rep_n_nodes, n, n_boot, cons_min,
                                           (tjamd_consensus_node *) d_cons, (int *) d_cons_order, NULL, NULL);
            if (n_cons < 0) return fail ("consensus tree");
            if (tjamd_device_download (ctr[0], h_cons, d_cons, (size_t) n_cons * sizeof (tjamd_consensus_node)) ||
                tjamd_device_download (ctr[0], h_cons_order, d_cons_order, (size_t) n * sizeof (int))) return fail ("download");
            tjamd_device_free (ctr[0], d_cons); tjamd_device_free (ctr[0], d_cons_order);
          }
          tjamd_device_free (ctr[0], d_weights); tjamd_device_free (ctr[0], d_rep_dist); tjamd_device_free (ctr[0], d_rep_nodes);
          tjamd_device_free (ctr[0], d_rep_order); tjamd_device_free (ctr[0], d_support);
          free (rep_n_nodes);
        }
        tjamd_device_free (ctr[0], d_nodes); tjamd_device_free (ctr[0], d_order); tjamd_device_free (ctr[0], d_node_marks); tjamd_device_free (ctr[0], d_marks);
      }
      tjamd_device_free (ctr[0], d_links); tjamd_device_free (ctr[0], d_cluster);
    }
    tjamd_device_free (ctr[0], d_dist);
  }
  h_sites = (tjamd_site *) malloc ((size_t) (n_sites ? n_sites : 1) * sizeof (tjamd_site));
  h_alleles = (tjamd_allele *) malloc ((size_t) (n_alleles ? n_alleles : 1) * sizeof (tjamd_allele));
  h_genotype = (int16_t *) malloc ((size_t) (n_sites ? n_sites : 1) * (size_t) n * sizeof (int16_t));
  h_unique = (tjamd_variant *) malloc ((size_t) (n_alleles ? n_alleles : 1) * sizeof (tjamd_variant));
  if (tjamd_device_download (ctr[0], h_sites, d_sites, (size_t) n_sites * sizeof (tjamd_site)) ||
      tjamd_device_download (ctr[0], h_alleles, d_alleles, (size_t) n_alleles * sizeof (tjamd_allele)) ||
      tjamd_device_download (ctr[0], h_genotype, d_genotype, (size_t) n_sites * (size_t) n * sizeof (int16_t)) ||
      tjamd_device_download (ctr[0], h_unique, d_unique, (size_t) n_alleles * sizeof (tjamd_variant))) return fail ("download");
  printf ("%ld contigs, %ld runs indexed; %ld of %ld union rows located; %ld tracts by location, %ld variable; %ld variants in %d samples\n", n_contigs,
          tjamd_reference_entries (ref), n_located, n_union, n_tracts, n_var, n_rec, n);
  if (max_edits >= 0) printf ("%ld more union rows located within %d edits and a shift of %d\n", n_gapped, max_edits, max_shift);
  printf ("%ld sites with %ld distinct alleles\n", n_sites, n_alleles);

  sample_name = (char **) malloc ((size_t) n * sizeof (char *));
  for (a = 0; a < n; a++) {
    const char *slash = strrchr (files[a], '/'), *base = slash ? slash + 1 : files[a];
    size_t len = strlen (base) + 1;
    char *p;
    sample_name[a] = (char *) malloc (len);
    snprintf (sample_name[a], len, "%s", base);
    for (p = sample_name[a]; *p; p++) if (*p == '/' || *p == '"' || *p == '\'' || *p == ' ' || *p == '\\') *p = '_';      /* as sample_vcfs.c names it */
  }
  for (s = 0; s < n_sites; s++) {                         /* the longest text of any site */
    long len = tjamd_site_ref_alt (h_sites + s, NULL, k, NULL, 0);
    if (len > text_cap) text_cap = len;
    for (i = 0; i < h_sites[s].n_alleles; i++) {
      len = tjamd_site_ref_alt (h_sites + s, h_alleles + h_sites[s].first_allele + i, k, NULL, 0);
      if (len > text_cap) text_cap = len;
    }
  }
  text = (char *) malloc ((size_t) text_cap + 1);

  if (!(fout = open_output (outdir, "merged.vcf"))) return 1;
  fprintf (fout, "##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n");
  if (with_depths) fprintf (fout, "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"reads on the tract\">\n"
                                  "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"reads on the reference length and on each ALT allele\">\n");
  fprintf (fout, "##INFO=<ID=AC,Number=A,Type=Integer,Description=\"samples that carry each ALT allele\">\n"
                 "##INFO=<ID=AN,Number=1,Type=Integer,Description=\"%s\">\n"
                 "##INFO=<ID=TID,Number=A,Type=String,Description=\"tract ID\">\n", with_depths ? "samples with a genotype, the reference's included" : "samples with a call");
  for (i = 0; i < n_contigs; i++) fprintf (fout, "##contig=<ID=%s,length=%ld>\n", contig_name[i], contig_len[i]);
  fprintf (fout, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT");
  for (a = 0; a < n; a++) fprintf (fout, "\t%s", sample_name[a]);
  fputc ('\n', fout);
  for (s = 0; s < n_sites; s++) {
    const tjamd_site *site = h_sites + s;
    const tjamd_allele *al = h_alleles + site->first_allele;
    if (tjamd_site_ref_alt (site, NULL, k, text, (int) text_cap + 1) < 0) { fprintf (stderr, "site %ld has no text\n", s); return 1; }
    fprintf (fout, "%s\t%d\t.\t%s\t", contig_name[site->contig], site->pos, text);
    for (i = 0; i < site->n_alleles; i++) {
      if (tjamd_site_ref_alt (site, al + i, k, text, (int) text_cap + 1) < 0) { fprintf (stderr, "site %ld has no text\n", s); return 1; }
      fprintf (fout, "%s%s", i ? "," : "", text);
    }
    fprintf (fout, "\t.\t.\tAC=");
    for (i = 0; i < site->n_alleles; i++) fprintf (fout, "%s%d", i ? "," : "", al[i].n_samples);
    fprintf (fout, ";AN=%d;TID=tid_%06d\tGT%s", with_depths ? n - h_sd[s].n_missing : site->n_called, site->tract, with_depths ? ":DP:AD" : "");
    for (a = 0; a < n; a++) {
      const int g = h_genotype[s * n + a];
      if (g < 0) fprintf (fout, "\t."); else fprintf (fout, "\t%d", g);
      if (with_depths) {                                  /* the site's AD rows: REF, then its alleles */
        fprintf (fout, ":%d:", h_dp[s * n + a]);
        for (i = 0; i <= site->n_alleles; i++) fprintf (fout, "%s%d", i ? "," : "", h_ad[(site->first_allele + s + i) * n + a]);
      }
    }
    fputc ('\n', fout);
  }
  fclose (fout);

  if (with_distances) {                                   /* the upper triangle with the diagonal, by the names of the VCF's columns */
    int b;
    if (!(fout = open_output (outdir, "sample_distances.tsv"))) return 1;
    fprintf (fout, "sample_a\tsample_b\tn_both\tn_differ\tlength_diff\n");
    for (a = 0; a < n; a++) for (b = a; b < n; b++) {
      const tjamd_sample_distance *x = h_dist + (size_t) a * (size_t) n + b;
      fprintf (fout, "%s\t%s\t%d\t%d\t%lld\n", sample_name[a], sample_name[b], x->n_both, x->n_differ, x->length_diff);
    }
    fclose (fout);
    free (h_dist);
  }
  if (with_clusters) {
    if (!(fout = open_output (outdir, "sample_linkage.tsv"))) return 1;
    for (i = 0; i < n_links; i++) fprintf (fout, "%s\t%s\t%lld\n", sample_name[h_links[i].a], sample_name[h_links[i].b], h_links[i].key);
    fclose (fout);
    if (!(fout = open_output (outdir, "sample_clusters.tsv"))) return 1;
    for (a = 0; a < n; a++) fprintf (fout, "%s\t%d\n", sample_name[a], h_cluster[a]);
    fclose (fout);
    printf ("%ld links, %ld clusters at %lld\n", n_links, n_clusters, cut);
  }
  if (with_clades) {
    long n_roots = 0;
    if (!(fout = open_output (outdir, "sample_tree.nwk"))) return 1;
    for (a = 0; a < n; n_roots++) {                       /* a root starts where the one before it ends: the last node that starts there, or a sample alone */
      int root = -1 - h_order[a], width = 1;
      for (i = 0; i < n_links; i++) if (h_nodes[i].first == a) { root = (int) i; width = h_nodes[i].size; }
      print_clade (fout, root, root >= 0 ? h_links[root].key : 0, h_nodes, h_links, h_node_marks, sample_name);
      fprintf (fout, ";\n");
      a += width;
    }
    fclose (fout);
    if (!(fout = open_output (outdir, "clade_sites.tsv"))) return 1;
    for (i = 0; i < n_clade_marks; i++) {
      const tjamd_site *site = h_sites + h_clade_marks[i].site;
      const tjamd_allele *al = h_clade_marks[i].genotype > 0 ? h_alleles + site->first_allele + h_clade_marks[i].genotype - 1 : NULL;
      if (tjamd_site_ref_alt (site, NULL, k, text, (int) text_cap + 1) < 0) { fprintf (stderr, "site %d has no text\n", h_clade_marks[i].site); return 1; }
      fprintf (fout, "%d\t%s\t%d\t%s\t", h_clade_marks[i].group, contig_name[site->contig], site->pos, text);
      if (tjamd_site_ref_alt (site, al, k, text, (int) text_cap + 1) < 0) { fprintf (stderr, "site %d has no text\n", h_clade_marks[i].site); return 1; }
      fprintf (fout, "%s\t%d\n", text, h_clade_marks[i].n_called);
    }
    fclose (fout);
    printf ("%ld marks of %ld nodes in %ld trees\n", n_clade_marks, n_links, n_roots);
    if (n_boot) {
      if (!(fout = open_output (outdir, "clade_support.tsv"))) return 1;
      for (i = 0; i < n_links; i++)
        fprintf (fout, "%ld\t%d\t%s\t%lld\t%d\t%d\t%d\n", i, h_nodes[i].size, sample_name[h_order[h_nodes[i].first]], h_links[i].key, h_node_marks[i], h_support[i], n_boot);
      fclose (fout);
      printf ("%d bootstrap replicates from seed %llu\n", n_boot, boot_seed);
      free (h_support);
      if (with_consensus) {
        if (!(fout = open_output (outdir, "consensus_tree.nwk"))) return 1;
        print_consensus (fout, -1, h_cons, (int) n_cons, h_cons_order, n, sample_name);
        fclose (fout);
        if (!(fout = open_output (outdir, "consensus_clades.tsv"))) return 1;
        for (i = 0; i < n_cons; i++) {
          fprintf (fout, "%ld\t%d\t%d\t%d\t%d\t", i, h_cons[i].parent, h_cons[i].size, h_cons[i].count, n_boot);
          for (a = 0; a < h_cons[i].size; a++) fprintf (fout, "%s%s", a ? "," : "", sample_name[h_cons_order[h_cons[i].first + a]]);
          fputc ('\n', fout);
        }
        fclose (fout);
        printf ("%ld clades in at least %d of %d replicates\n", n_cons, cons_min, n_boot);
        free (h_cons); free (h_cons_order);
      }
    }
    free (h_nodes); free (h_order); free (h_node_marks); free (h_clade_marks);
  }
  if (with_clusters) { free (h_links); free (h_cluster); }
  if (with_groups) {
    if (!(fout = open_output (outdir, "cluster_sites.tsv"))) return 1;
    for (i = 0; i < n_marks; i++) {
      const tjamd_site *site = h_sites + h_marks[i].site;
      const tjamd_allele *al = h_marks[i].genotype > 0 ? h_alleles + site->first_allele + h_marks[i].genotype - 1 : NULL;
      if (tjamd_site_ref_alt (site, NULL, k, text, (int) text_cap + 1) < 0) { fprintf (stderr, "site %d has no text\n", h_marks[i].site); return 1; }
      fprintf (fout, "%d\t%s\t%d\t%s\t", h_marks[i].group, contig_name[site->contig], site->pos, text);
      if (tjamd_site_ref_alt (site, al, k, text, (int) text_cap + 1) < 0) { fprintf (stderr, "site %d has no text\n", h_marks[i].site); return 1; }
      fprintf (fout, "%s\t%d\n", text, h_marks[i].n_called);
    }
    fclose (fout);
    printf ("%ld marks of %ld clusters\n", n_marks, n_clusters);
    free (h_marks);
  }

  if (with_unique) {                                      /* every distinct event once, as N8 wrote it for the first sample that has it */
    if (!(fout = open_output (outdir, "unique_variants.vcf"))) return 1;
    fprintf (fout, "##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
                   "##INFO=<ID=TID,Number=A,Type=String,Description=\"tract ID\">\n");
    for (i = 0; i < n_contigs; i++) fprintf (fout, "##contig=<ID=%s,length=%ld>\n", contig_name[i], contig_len[i]);
    fprintf (fout, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tall_samples\n");
    for (i = 0; i < n_alleles; i++) {
      const tjamd_variant *v = h_unique + i;
      fprintf (fout, "%s\t%d\t.\t", contig_name[v->contig], v->pos);
      print_ref_alt (fout, v);
      fprintf (fout, "\t.\t.\tTID=tid_%06d\tGT\t1\n", v->tract);
    }
    fclose (fout);
  }

  if (gff) {                                              /* the effect of every distinct allele, walked once */
    long n_features, string_bytes = 0, n_skipped = 0, n_class[5] = {0, 0, 0, 0, 0};
    tjamd_feature *features;
    tjamd_effect *h_effects;
    signed char *phase;
    char *strings, *blob = (char *) malloc ((size_t) name_bytes + 1);
    void *d_tf, *d_effects;
    tjamd_annotation *ann;
    tjamd_coding *cod;
    for (i = 0, a = 0; i < n_contigs; i++) a += sprintf (blob + a, "%s\n", contig_name[i]);      /* the names as tjamd_gff3_read takes them */
    n_features = tjamd_gff3_read (gff, blob, n_contigs, NULL, 0, NULL, 0, &string_bytes, &n_skipped);
    if (n_features < 0) { fprintf (stderr, "cannot read %s\n", gff); return 1; }
    features = (tjamd_feature *) malloc ((size_t) (n_features ? n_features : 1) * sizeof (tjamd_feature));
    strings = (char *) malloc ((size_t) string_bytes + 1);
    phase = (signed char *) malloc ((size_t) (n_features ? n_features : 1));
    tjamd_gff3_read (gff, blob, n_contigs, features, n_features, strings, string_bytes, &string_bytes, &n_skipped);
    if (tjamd_gff3_read_phase (gff, blob, n_contigs, phase, n_features) != n_features) { fprintf (stderr, "cannot read the phases of %s\n", gff); return 1; }
    ann = tjamd_annotation_create (ctr[0], ref, features, n_features);
    if (!ann) return fail (gff);
    cod = tjamd_coding_create (ctr[0], ref_stream, (size_t) ref_bytes, features, n_features, phase);
    if (!cod) return fail ("coding table");
    d_tf = tjamd_device_alloc (ctr[0], (size_t) (n_tracts ? n_tracts : 1) * sizeof (tjamd_tract_feature));
    d_effects = tjamd_device_alloc (ctr[0], (size_t) (n_alleles ? n_alleles : 1) * sizeof (tjamd_effect));
    if (tjamd_tract_features (ctr[0], ann, d_pkeys, d_pcounts, n_union, n, (const tjamd_union_tract *) d_tracts, n_tracts, (const tjamd_location *) d_tloc,
                              (tjamd_tract_feature *) d_tf) < 0) return fail ("tract features");
    if (tjamd_variant_effects (ctr[0], cod, (const tjamd_variant *) d_unique, n_alleles, (const tjamd_tract_feature *) d_tf, n_tracts, (tjamd_effect *) d_effects) < 0)
      return fail ("variant effects");
    h_effects = (tjamd_effect *) malloc ((size_t) (n_alleles ? n_alleles : 1) * sizeof (tjamd_effect));
    if (tjamd_device_download (ctr[0], h_effects, d_effects, (size_t) n_alleles * sizeof (tjamd_effect))) return fail ("download");
    if (!(fout = open_output (outdir, "variant_effects.tsv"))) return 1;
    fprintf (fout, "tract_id\tcontig_name\tpos\tref\talt\tfeature\teffect\tcds_pos\tfirst_diff\tref_aa\talt_aa\tref_aa_len\talt_aa_len\tn_samples\n");
    for (i = 0; i < n_alleles; i++) {
      const tjamd_variant *v = h_unique + i;
      const tjamd_effect *e = h_effects + i;
      char wr[9], wa[9];
      fprintf (fout, "tid_%06d\t%s\t%d\t", v->tract, contig_name[v->contig], v->pos);
      print_ref_alt (fout, v);
      fprintf (fout, "\t%s\t%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d\n", e->feature >= 0 ? strings + features[e->feature].id_off : "unannotated", class_name[e->cls], e->cds_pos,
               e->first_diff + 1, window_text (e->ref_aa, wr), window_text (e->alt_aa, wa), e->ref_aa_len, e->alt_aa_len, h_alleles[i].n_samples);
      n_class[e->cls]++;
    }
    fclose (fout);
    printf ("%ld alleles: %ld outside coding features, %ld across a boundary, %ld identical, %ld in frame, %ld frameshifts\n", n_alleles,
            n_class[TJAMD_EFFECT_NONE], n_class[TJAMD_EFFECT_BOUNDARY], n_class[TJAMD_EFFECT_IDENTICAL], n_class[TJAMD_EFFECT_INFRAME], n_class[TJAMD_EFFECT_FRAMESHIFT]);
    tjamd_coding_destroy (cod);
    tjamd_annotation_destroy (ann);
    tjamd_device_free (ctr[0], d_tf); tjamd_device_free (ctr[0], d_effects);
    free (features); free (strings); free (phase); free (blob); free (h_effects);
  }

  tjamd_reference_destroy (ref);
  tjamd_device_free (ctr[0], d_keys); tjamd_device_free (ctr[0], d_counts); tjamd_device_free (ctr[0], d_ids); tjamd_device_free (ctr[0], d_grouped);
  tjamd_device_free (ctr[0], d_loc); tjamd_device_free (ctr[0], d_perm); tjamd_device_free (ctr[0], d_pkeys); tjamd_device_free (ctr[0], d_pcounts);
  tjamd_device_free (ctr[0], d_tracts); tjamd_device_free (ctr[0], d_tloc); tjamd_device_free (ctr[0], d_reflen);
  tjamd_device_free (ctr[0], d_summary); tjamd_device_free (ctr[0], d_var); tjamd_device_free (ctr[0], d_variants);
  if (with_depths) { tjamd_device_free (ctr[0], d_dp); tjamd_device_free (ctr[0], d_ad); tjamd_device_free (ctr[0], d_sd); free (h_dp); free (h_ad); free (h_sd); }
  tjamd_device_free (ctr[0], d_sites); tjamd_device_free (ctr[0], d_alleles); tjamd_device_free (ctr[0], d_genotype); tjamd_device_free (ctr[0], d_unique);
  free (h_sites); free (h_alleles); free (h_genotype); free (h_unique); free (text); free (ref_stream);
  for (a = 0; a < n; a++) free (sample_name[a]);
  free (sample_name); free (names); free (contig_name); free (contig_len);
  for (a = 0; a < n; a++) tjamd_counter_destroy (ctr[a]);
  return 0;
}
