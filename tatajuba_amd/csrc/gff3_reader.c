/* gff3_reader.c -- see gff3_reader.h.  The file is read whole (an annotation is a few megabytes), inflated member by member
 * with tj_inflate.c if it starts with a gzip header (BGZF is a series of such members), and its lines are parsed twice:
 * once to size, once to write, so that nothing is written unless everything fits. */
#include "gff3_reader.h"
#include "tj_inflate.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct { unsigned char *p; size_t n; } tjg_text;

static int
tjg_load (const char *path, tjg_text *t)
{
  FILE *f = fopen (path, "rb");
  size_t cap = 1u << 16;
  t->p = NULL; t->n = 0;
  if (!f) return -1;
  t->p = (unsigned char *) malloc (cap);
  for (;;) {
    size_t got;
    if (t->p && t->n == cap) { unsigned char *np = (unsigned char *) realloc (t->p, cap *= 2); if (!np) free (t->p); t->p = np; }
    if (!t->p) { fclose (f); return -1; }
    got = fread (t->p + t->n, 1, cap - t->n, f);
    if (!got) break;
    t->n += got;
  }
  fclose (f);
  return 0;
}

/* length of the gzip member header at p (RFC 1952: 1f 8b, CM = 8, FLG, MTIME[4], XFL, OS, then FEXTRA / FNAME / FCOMMENT /
 * FHCRC as FLG says), 0 if it is none or cut short */
static size_t
tjg_member_header (const unsigned char *p, size_t avail)
{
  size_t x = 10;
  unsigned flg;
  if (avail < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8) return 0;
  flg = p[3];
  if (flg & 0xe0u) return 0;
  if (flg & 4u) { if (x + 2 > avail) return 0; x += 2 + ((size_t) p[x] | ((size_t) p[x + 1] << 8)); }
  if (flg & 8u) { while (x < avail && p[x]) x++; x++; }
  if (flg & 16u) { while (x < avail && p[x]) x++; x++; }
  if (flg & 2u) x += 2;
  return x < avail ? x : 0;
}

/* z: a gzip file -> its text, every member behind the other (each is checked against its own CRC-32); -1 if it is damaged */
static int
tjg_gunzip (const tjg_text *z, tjg_text *t)
{
  size_t zpos = 0, cap = z->n * 4 + 4096;
  tji_state *st = (tji_state *) malloc (sizeof (tji_state));
  int ok = st != NULL;
  t->p = (unsigned char *) malloc (cap); t->n = 0;
  if (!t->p) ok = 0;
  while (ok && zpos < z->n) {
    const size_t h = tjg_member_header (z->p + zpos, z->n - zpos), from = t->n;
    size_t in_pos, out_pos = 0;
    int rc;
    if (!h) { ok = zpos > 0 && (z->n - zpos < 2 || z->p[zpos] != 0x1f || z->p[zpos + 1] != 0x8b); break; }   /* (bytes behind the last member: ignored, as gzip does) */
    in_pos = zpos + h;
    tji_init (st);
    for (;;) {                                          /* the member's output is one stretch of t: its window is always in front */
      rc = tji_inflate (st, z->p, z->n, &in_pos, t->p + from, cap - from, &out_pos, 0);
      if (rc != TJI_OUTPUT_FULL) break;
      { unsigned char *np = (unsigned char *) realloc (t->p, cap *= 2); if (!np) { rc = TJI_ERROR; break; } t->p = np; }
    }
    if (rc != TJI_DONE || z->n - in_pos < 8) { ok = 0; break; }
    {
      const unsigned char *tr = z->p + in_pos;
      const unsigned crc = (unsigned) tr[0] | ((unsigned) tr[1] << 8) | ((unsigned) tr[2] << 16) | ((unsigned) tr[3] << 24);
      const unsigned isize = (unsigned) tr[4] | ((unsigned) tr[5] << 8) | ((unsigned) tr[6] << 16) | ((unsigned) tr[7] << 24);
      if (crc != tji_crc32 (0, t->p + from, out_pos) || isize != (unsigned) (out_pos & 0xffffffffu)) { ok = 0; break; }
    }
    t->n = from + out_pos;
    zpos = in_pos + 8;
  }
  free (st);
  if (!ok) { free (t->p); t->p = NULL; t->n = 0; return -1; }
  return 0;
}

/* the contig names, sorted by bytes, for a binary search per line */
typedef struct { const char *s; size_t len; int idx; } tjg_name;

static int
tjg_name_cmp (const void *a, const void *b)
{
  const tjg_name *x = (const tjg_name *) a, *y = (const tjg_name *) b;
  const size_t m = x->len < y->len ? x->len : y->len;
  const int c = memcmp (x->s, y->s, m);
  if (c) return c;
  if (x->len != y->len) return x->len < y->len ? -1 : 1;
  return (x->idx > y->idx) - (x->idx < y->idx);         /* a name that occurs twice: the first contig of that name */
}

static int
tjg_find_name (const tjg_name *names, long n, const char *s, size_t len)
{
  long lo = 0, hi = n;
  const tjg_name q = {s, len, -1};                      /* (sorts in front of every entry of the same name) */
  while (lo < hi) { const long mid = (lo + hi) >> 1; if (tjg_name_cmp (&names[mid], &q) < 0) lo = mid + 1; else hi = mid; }
  return (lo < n && names[lo].len == len && !memcmp (names[lo].s, s, len)) ? names[lo].idx : -1;
}

/* decimal, all of [s, s + len), at most 2^31 - 1; -1 otherwise */
static long
tjg_number (const char *s, size_t len)
{
  long v = 0;
  size_t i;
  if (!len || len > 10) return -1;
  for (i = 0; i < len; i++) { if (s[i] < '0' || s[i] > '9') return -1; v = v * 10 + (s[i] - '0'); }
  return v <= 0x7fffffffl ? v : -1;
}

static int
tjg_equals_nocase (const char *s, size_t len, const char *word)
{
  size_t i;
  if (len != strlen (word)) return 0;
  for (i = 0; i < len; i++) { const char ch = (s[i] >= 'A' && s[i] <= 'Z') ? (char) (s[i] + 32) : s[i]; if (ch != word[i]) return 0; }
  return 1;
}

/* one pass over the lines: counts always; writes records and strings if out != NULL, and column 8 of every kept line
 * (0, 1, 2; -1 for anything else) if phase != NULL */
static long
tjg_parse (const tjg_text *t, const tjg_name *names, long n_names, tjamd_feature *out, char *strings, signed char *phase, long *bytes_out, long *skipped_out)
{
  long n = 0, bytes = 0, skipped = 0, line_no = 0;
  size_t at = 0;
  while (at < t->n) {
    const char *line = (const char *) t->p + at, *nl = (const char *) memchr (line, '\n', t->n - at), *col[10];
    size_t len = nl ? (size_t) (nl - line) : t->n - at;
    int nc = 1;
    size_t i;
    at += len + (nl ? 1 : 0);
    line_no++;
    if (len && line[len - 1] == '\r') len--;
    if (!len) continue;
    if (line[0] == '>' || (len >= 7 && !memcmp (line, "##FASTA", 7))) break;
    if (line[0] == '#') continue;
    col[0] = line;
    for (i = 0; i < len && nc < 9; i++) if (line[i] == '\t') col[nc++] = line + i + 1;
    col[nc] = line + len + 1;                           /* (column j is [col[j], col[j + 1] - 1); the ninth takes the rest of the line) */
    if (nc < 9) { skipped++; continue; }
    {
#define TJG_LEN(j) ((size_t) (col[(j) + 1] - col[j] - 1))
      const int contig = tjg_find_name (names, n_names, col[0], TJG_LEN (0));
      const long start = tjg_number (col[3], TJG_LEN (3)), end = tjg_number (col[4], TJG_LEN (4));
      const char *id = NULL, *attr = col[8];
      const size_t attr_len = TJG_LEN (8), type_len = TJG_LEN (2);
      size_t id_len = 0;
      if (contig < 0 || start < 1 || end < start) { skipped++; continue; }
      for (i = 0; i + 3 <= attr_len; i++)
        if ((i == 0 || attr[i - 1] == ';') && !memcmp (attr + i, "ID=", 3)) {
          id = attr + i + 3;
          while (i + 3 + id_len < attr_len && id[id_len] != ';') id_len++;
          break;
        }
      if (out) {
        tjamd_feature f;
        f.contig = contig; f.start = (int) start; f.end = (int) end;
        f.cls = tjg_equals_nocase (col[2], type_len, "region") ? TJAMD_FEATURE_REGION : tjg_equals_nocase (col[2], type_len, "cds") ? TJAMD_FEATURE_CDS : TJAMD_FEATURE_OTHER;
        f.strand = TJG_LEN (6) == 1 && col[6][0] == '+' ? 0 : TJG_LEN (6) == 1 && col[6][0] == '-' ? 1 : 2;
        f.line = (int) line_no; f.type_off = (int) bytes; f.id_off = (int) (bytes + (long) type_len + 1);
        memcpy (strings + bytes, col[2], type_len); strings[bytes + (long) type_len] = '\0';
        if (id_len) memcpy (strings + f.id_off, id, id_len);
        strings[f.id_off + (long) id_len] = '\0';
        out[n] = f;
      }
      if (phase) phase[n] = (signed char) ((TJG_LEN (7) == 1 && col[7][0] >= '0' && col[7][0] <= '2') ? col[7][0] - '0' : -1);
#undef TJG_LEN
      bytes += (long) type_len + 1 + (long) id_len + 1;
      n++;
    }
  }
  *bytes_out = bytes; *skipped_out = skipped;
  return n;
}

/* the file's text and the sorted names; 0, or -1 if the file cannot be opened or is damaged */
static int
tjg_open (const char *path, const char *contig_names, long n_contigs, tjg_text *text, tjg_name **names_out, long *n_names_out)
{
  tjg_text raw;
  tjg_name *names = NULL;
  long i, n_names = 0;
  const char *p = contig_names;
  if (!path || tjg_load (path, &raw)) return -1;
  if (raw.n >= 2 && raw.p[0] == 0x1f && raw.p[1] == 0x8b) {
    const int rc = tjg_gunzip (&raw, text);
    free (raw.p);
    if (rc) return -1;
  } else *text = raw;
  if (n_contigs > 0 && contig_names) names = (tjg_name *) malloc ((size_t) n_contigs * sizeof (tjg_name));
  for (i = 0; names && i < n_contigs; i++) {
    const char *e = p;
    while (*e != '\n') e++;                             /* (n_contigs names, each followed by '\n': the format's promise) */
    names[n_names].s = p; names[n_names].len = (size_t) (e - p); names[n_names].idx = (int) i;
    n_names++; p = e + 1;
  }
  if (names) qsort (names, (size_t) n_names, sizeof (tjg_name), tjg_name_cmp);
  *names_out = names; *n_names_out = n_names;
  return 0;
}

long
tjg_read (const char *path, const char *contig_names, long n_contigs, tjamd_feature *out, long capacity,
          char *strings, long strings_capacity, long *strings_bytes, long *n_skipped)
{
  tjg_text text;
  tjg_name *names = NULL;
  long n, bytes = 0, skipped = 0, n_names = 0;
  if (tjg_open (path, contig_names, n_contigs, &text, &names, &n_names)) return -1;
  n = tjg_parse (&text, names, n_names, NULL, NULL, NULL, &bytes, &skipped);
  if (bytes >= 0x7fffffffl) n = -1;                     /* (the offsets are ints) */
  else if (out && strings && n <= capacity && bytes <= strings_capacity) (void) tjg_parse (&text, names, n_names, out, strings, NULL, &bytes, &skipped);
  free (names); free (text.p);
  if (strings_bytes) *strings_bytes = bytes;
  if (n_skipped) *n_skipped = skipped;
  return n;
}

long
tjg_read_phase (const char *path, const char *contig_names, long n_contigs, signed char *out, long capacity)
{
  tjg_text text;
  tjg_name *names = NULL;
  long n, bytes = 0, skipped = 0, n_names = 0;
  if (tjg_open (path, contig_names, n_contigs, &text, &names, &n_names)) return -1;
  n = tjg_parse (&text, names, n_names, NULL, NULL, NULL, &bytes, &skipped);
  if (bytes >= 0x7fffffffl) n = -1;                     /* (what tjg_read refuses) */
  else if (out && n <= capacity) (void) tjg_parse (&text, names, n_names, NULL, NULL, out, &bytes, &skipped);
  free (names); free (text.p);
  return n;
}
