"""Edge corpus of the grouping of near-identical contexts (N3: group_back_kernel, group_resolve_kernel,
group_speculate_kernel, group_repair_kernel, name_edit_distance, group_summary_kernel, group_histogram_kernel,
union_tract_kernel) and plain restatements of what those kernels walk, for tests/test_grouping_edges_corpus.py (CPU: the
corpus is what it claims) and tests/test_grouping_edges.py (GPU: the device against the oracle on it).

A corpus is a Rows: union rows in the merge's order (base, ctx0, ctx1, length, each descending by their signed values,
equal contexts adjacent) with one count per row.  The same rows feed both routes: tjamd_union_tracts takes them as they
are (the counts as the per-sample matrix, split_counts), a sample gets each row `count` times (sample_raw), finalised.

The restatements (back_of, heads_of, stretches, candidates, window_walk) are numpy / Python and never touch the device; they
use the oracle only where their arguments say so (heads_final of window_walk, orc.levenshtein in candidates).  The kernels'
constants (GR_CHUNK, the 4096 blocks of grid_for, 256 threads) are restated here and parsed against the source by
tests/test_grouping_edges_corpus.py.

Rule: a kernel that walks stretches or windows brings its constant and both neighbours into this module."""
import numpy as np

from oracle import orc
from tests.test_tract_stats_cabi import record, signed_length

GR_CHUNK = 4096          # rows per window of group_repair_kernel
GRID_CAP = 4096          # grid_for: at most this many blocks ...
BLOCK = 256              # ... of this many threads: a grid-stride loop takes a second trip from GRID_CAP * BLOCK rows on
ONE_TRIP = GRID_CAP * BLOCK
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_M55 = np.uint64(0x5555555555555555)


def pack(s):
    """a flank as the name prints it (first character = lowest two bits) -> packed word"""
    return sum(_CODE[ch] << (2 * i) for i, ch in enumerate(s))


def unpack(v, k):
    return "".join("ACGT"[(int(v) >> (2 * i)) & 3] for i in range(k))


class Rows:
    """keys uint64 [n, 3] (tests.test_tract_stats_cabi.record), counts int64 [n], marks: planted row name -> row index"""

    def __init__(self, k, rows, marks=None):
        self.k = k
        if isinstance(rows, tuple):
            self.keys, self.counts = rows
        else:
            self.keys = np.array([record(b, c0, c1, ln, cnt) for (b, c0, c1, ln, cnt) in rows], dtype=np.uint64).reshape(-1, 3)
            self.counts = np.array([r[4] for r in rows], dtype=np.int64)
        self.marks = dict(marks or {})

    def __len__(self):
        return len(self.keys)

    @property
    def bases(self):
        return (self.keys[:, 2] & np.uint64(3)).astype(np.int64)

    def name(self, i):
        return orc.name_of(self.keys[i, 0], self.keys[i, 1], int(self.keys[i, 2]) & 3, self.k)


def record_words(base, c0, c1, length, count):
    """record() on arrays"""
    n = len(c0)
    keys = np.zeros((n, 3), np.uint64)
    keys[:, 0], keys[:, 1] = c0, c1
    meta = (np.asarray(base, np.uint64) & np.uint64(3)) | ((np.asarray(length, np.int64) & 0x3FF).astype(np.uint64) << np.uint64(2))
    keys[:, 2] = meta | ((np.asarray(count, np.int64) & 0xFFFFF).astype(np.uint64) << np.uint64(12)) | np.uint64(0xffe << 32)
    return keys


def concat(k, parts):
    """Rows back to back (the caller keeps them sorted: each part under its own base or ctx0 range); marks move along"""
    keys, counts, marks, at = [], [], {}, 0
    for p in parts:
        keys.append(p.keys); counts.append(p.counts)
        marks.update({m: at + i for m, i in p.marks.items()})
        at += len(p)
    return Rows(k, (np.concatenate(keys), np.concatenate(counts)), marks)


def order_key(keys):
    """what the rows descend in: (signed base, ctx0, ctx1, signed length) per row, as Python tuples"""
    b = (keys[:, 2] & np.uint64(3)).astype(np.int64)
    b = np.where(b >= 2, b - 4, b)
    ln = signed_length(keys[:, 2])
    return [(int(b[i]), int(keys[i, 0]), int(keys[i, 1]), int(ln[i])) for i in range(len(keys))]


def strictly_descending(keys):
    keys = np.asarray(keys)
    if len(keys) < 2:
        return True
    b = (keys[:, 2] & np.uint64(3)).astype(np.int64)
    b = np.where(b >= 2, b - 4, b)
    ln = signed_length(keys[:, 2])
    c0, c1 = keys[:, 0], keys[:, 1]
    gt = lambda a: a[:-1] > a[1:]
    eq = lambda a: a[:-1] == a[1:]
    return bool((gt(b) | (eq(b) & (gt(c0) | (eq(c0) & (gt(c1) | (eq(c1) & gt(ln))))))).all())


def split_counts(counts, ns=2):
    """the per-sample matrix of the union route: a row's count spread over ns samples (the first takes the odd one out)"""
    c = np.asarray(counts, np.int64)
    mat = np.zeros((len(c), ns), np.int64)
    for s in range(ns):
        mat[:, s] = c // ns
    mat[:, 0] += c - mat.sum(axis=1)
    assert (mat.sum(axis=1) == c).all() and mat.max(initial=0) < (1 << 31)
    return mat.astype(np.int32)


def sample_raw(rows, elem_dtype):
    """the sample route: each row `count` times as raw elements of one strand, count 1 each (tests/test_gpu_parity.py)"""
    rep = np.repeat(np.arange(len(rows)), rows.counts)
    raw = np.zeros(len(rep), dtype=elem_dtype)
    raw["ctx0"], raw["ctx1"] = rows.keys[rep, 0], rows.keys[rep, 1]
    raw["meta"] = (rows.keys[rep, 2] & np.uint64(0xFFF)) | np.uint64((1 << 12) | (0xffe << 32) | (1 << 49))
    raw["read_offset"] = 0
    raw["loc_ref_id"] = raw["loc_pos"] = raw["loc_last"] = -1
    return raw


def planted(rows):
    """(ctx0, ctx1, base and length bits, count field) of every row: what a finalise (0, 0) of sample_raw must keep"""
    return np.stack([rows.keys[:, 0], rows.keys[:, 1], rows.keys[:, 2] & np.uint64(0xFFF), (rows.counts & 0xFFFFF).astype(np.uint64)], 1)


def kept_table(kept):
    return np.stack([kept["ctx0"], kept["ctx1"], kept["meta"] & np.uint64(0xFFF), (kept["meta"] >> np.uint64(12)) & np.uint64(0xFFFFF)], 1)


# ---- restatements -------------------------------------------------------------------------------------------------------

def _popcount(x):
    x = np.ascontiguousarray(x, dtype=np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def flank_distance(a0, a1, b0, b1):
    """differing flank bases of two contexts, both flanks together"""
    d0, d1 = np.asarray(a0, np.uint64) ^ np.asarray(b0, np.uint64), np.asarray(a1, np.uint64) ^ np.asarray(b1, np.uint64)
    return _popcount((d0 | (d0 >> np.uint64(1))) & _M55) + _popcount((d1 | (d1 >> np.uint64(1))) & _M55)


def back_of(keys, maxd):
    """group_back_kernel by its definition: back[i] = the nearest j < i that row i cannot share a group with -- another base, or
    maxd or more flank bases away -- or -1"""
    keys = np.asarray(keys, np.uint64).reshape(-1, 3)
    n = len(keys)
    base = keys[:, 2] & np.uint64(3)
    j = np.arange(n, dtype=np.int64) - 1
    active = np.flatnonzero(j >= 0)
    while active.size:
        jj = j[active]
        close = (base[jj] == base[active]) & (flank_distance(keys[jj, 0], keys[jj, 1], keys[active, 0], keys[active, 1]) < maxd)
        active = active[close]
        j[active] -= 1
        active = active[j[active] >= 0]
    return j


def stretches(back):
    """rows that open a group whatever came before: each starts a stretch that one thread of group_resolve_kernel walks"""
    back = np.asarray(back)
    return np.flatnonzero(back == np.arange(len(back)) - 1)


def heads_of(back):
    """the flank-only grouping from back[]: row i joins iff the group being built started after back[i]"""
    back = np.asarray(back)
    n = len(back)
    head = np.zeros(n, bool)
    ss = stretches(back)
    head[ss] = True
    rest = np.flatnonzero(~head)
    if rest.size:
        before = ss[np.searchsorted(ss, rest, "right") - 1]
        last = -1
        for i, p in zip(rest.tolist(), before.tolist()):
            if max(p, last) <= back[i]:
                head[i] = True
                last = i
    return head


def group_modes(totals, heads):
    """the row with the highest total of each group, the first of equal totals"""
    totals = np.asarray(totals, np.int64)
    starts = np.flatnonzero(heads)
    size = np.diff(np.r_[starts, len(totals)])
    mx = np.repeat(np.maximum.reduceat(totals, starts), size)
    return np.minimum.reduceat(np.where(totals == mx, np.arange(len(totals)), len(totals)), starts)


def _symbol_counts(keys, k):
    out = np.zeros((len(keys), 4), np.int64)
    for w in (0, 1):
        for t in range(k):
            d = ((keys[:, w] >> np.uint64(2 * t)) & np.uint64(3)).astype(np.int64)
            for s in range(4):
                out[:, s] += d == s
    return out


def candidates(keys, totals, heads1, k, lev, free_end=False):
    """what group_speculate_kernel flags: heads of the flank-only grouping with the base of the row before them whose name is
    less than lev edits (orc.levenshtein) from the name of the flank-only group before them -- its row with the highest
    total, the first of equal totals"""
    keys = np.asarray(keys, np.uint64).reshape(-1, 3)
    n = len(keys)
    cand = np.zeros(n, bool)
    starts = np.flatnonzero(heads1)
    if len(starts) < 2:
        return cand
    mode = group_modes(totals, heads1)
    base = keys[:, 2] & np.uint64(3)
    i, m = starts[1:], mode[:-1]
    ok = base[i] == base[i - 1]
    if not free_end:                                     # equal lengths: an edit moves the symbol counts by at most 2
        sc = _symbol_counts(keys, k)
        ok &= np.abs(sc[i] - sc[m]).sum(axis=1) < 2 * lev
    name = lambda r: orc.name_of(keys[r, 0], keys[r, 1], int(base[r]), k)
    for a, b in zip(i[ok].tolist(), m[ok].tolist()):
        cand[a] = orc.levenshtein(name(b), name(a), free_end=free_end) < lev
    return cand


def window_walk(cand, heads1, heads_final, bases, chunk=GR_CHUNK):
    """group_repair_kernel's windows: [(window start, offset of the candidate taken or None, where the next window starts)].
    A window of `chunk` rows starts where the replay before it ended.  The replay from candidate h goes on to the row behind
    the first row >= h that opens a group in both groupings, and stops in front of a row of another base, or at n."""
    n = len(cand)
    out, pos = [], 0
    while pos < n:
        end = min(n, pos + chunk)
        c = np.flatnonzero(cand[pos:end])
        if c.size == 0:
            out.append((pos, None, end))
            pos = end
            continue
        h = pos + int(c[0])
        i = h
        while i < n:
            if bases[i] != bases[h - 1]:
                break
            i += 1
            if heads1[i - 1] and heads_final[i - 1]:
                break
        out.append((pos, h - pos, i))
        pos = i
    return out


def skipped_candidates(cand, walk):
    """candidates that no window takes: they lie inside the stretch an earlier replay covered"""
    taken = {s + o for s, o, _ in walk if o is not None}
    return [int(i) for i in np.flatnonzero(cand) if int(i) not in taken]


def union_grouping(keys, mat, k, maxd, lev, free_end=False):
    """tests.test_union_tracts_cabi.oracle_union_grouping with its per-row Python loop taken out (mode and integral by numpy,
    the retry's distances only in the tracts that have a row of type 2): the same dict, for unions of a million rows"""
    from tests.test_union_tracts_cabi import count_ranks, pooled_elements
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    totals = np.asarray(mat, dtype=np.int64).sum(axis=1)
    orc.set_edit_free_end(free_end)
    r = orc.genomic_context_list(pooled_elements(keys, count_ranks(totals)), k, maxd, lev, 1)
    gof, jt = r["group_of"], r["join_type"]
    heads = np.r_[True, gof[1:] != gof[:-1]]
    first = np.flatnonzero(heads)
    mode = group_modes(totals, heads)
    integral = np.add.reduceat(totals, first)
    lev_d = np.zeros(len(first), np.int64)
    ends = np.r_[first[1:], len(keys)]
    name = lambda i: orc.name_of(keys[i, 0], keys[i, 1], int(keys[i, 2]) & 3, k)
    for g in np.unique(gof[jt == 2]).tolist():
        best = lo = int(first[g])
        for i in range(lo, int(ends[g])):
            if i > lo and jt[i] == 2:
                lev_d[g] = max(lev_d[g], orc.levenshtein(name(best), name(i), free_end=free_end))
            if totals[i] > totals[best]:
                best = i
    return {"tract_id": gof, "join_type": jt, "groups": r["groups"], "lev_distance": lev_d, "mode": mode, "integral": integral}


# ---- generators ---------------------------------------------------------------------------------------------------------

def _count(i):
    """a row's count: deterministic, 2 .. 12"""
    return 2 + (i * 7) % 11


def staircase(k, L, base=0, thin=False, hold_top=False):
    """All 2k digits of (ctx0, ctx1) start at 3; step t lowers one digit by one, the digits taken in turn from the most
    significant one of ctx0 downwards: 6k + 1 contexts, neighbours one substitution apart, contexts two steps apart two
    substitutions apart (2k steps apart: every digit differs), L lengths each.  At max_distance_per_flank 2 one stretch of
    (6k + 1) L rows with a group head every second context.  thin: every fourth context has one length only, so that a group
    head is the very row that a later row cannot join (start == back[j] in group_resolve_kernel).  hold_top: the most significant
    digit of ctx0 stays 3 (6k - 2 contexts), which leaves room for rows of the same base behind the staircase."""
    digits = [3] * (2 * k)                               # digits[0]: the most significant digit of ctx0
    word = lambda d: sum(v << (2 * (k - 1 - t)) for t, v in enumerate(d))
    rows = []
    turn = list(range(1 if hold_top else 0, 2 * k))
    for t in range(3 * len(turn) + 1):
        c0, c1 = word(digits[:k]), word(digits[k:])
        rows += [(base, c0, c1, ln, _count(t * 5 + ln)) for ln in range(1 if thin and t % 4 == 0 else L, 0, -1)]
        if t < 3 * len(turn):
            digits[turn[t % len(turn)]] -= 1
    return Rows(k, rows, {"first": 0, "last": len(rows) - 1})


FILLER_K = 10
_FILL_MASK = (1 << 14) - 1


def filler_ctx1(c0):
    """the right flank of the filler row whose left flank is c0 (k = 10): seven bases of symbol c0 mod 4, three hashed ones.
    Neighbouring fillers (ctx0 one apart) differ in those seven places and by eight in their symbol counts: 7 >= 2 maxd flank
    bases and at least 4 edits apart, so they never join, flank test or retry, at maxd <= 3 and lev <= 4"""
    c0 = np.asarray(c0, np.uint64)
    s = c0 & np.uint64(3)
    seven = s * np.uint64(0x1555)                        # 0b01 seven times
    h = ((c0 * np.uint64(2654435761)) >> np.uint64(9)) & np.uint64(63)
    return seven | (h << np.uint64(14))


def fillers(top, m, base):
    """m filler rows of k = 10 with ctx0 = top, top - 1, ..: one length, counts 2 .. 4"""
    c0 = np.uint64(top) - np.arange(m, dtype=np.uint64)
    assert m == 0 or top - (m - 1) >= 0
    keys = record_words(np.full(m, base), c0, filler_ctx1(c0), np.full(m, 5), 2 + (np.arange(m) % 3))
    return Rows(FILLER_K, (keys, 2 + (np.arange(m, dtype=np.int64) % 3)))


UNIT_RIGHT = "GATCCTGATC"                                 # k = 10: no base more than three times
UNIT_DEL = 3


def unit_rows(base, c0, kind, nlen=2):
    """A retry unit under the left flank c0 (k = 10).  A: the right flank UNIT_RIGHT with nlen lengths (7, 6, 5: counts 3, 9, 4);
    F: A's right flank with the base at UNIT_DEL deleted and a new last base, one length (6, count 5): 2 edits and 6 flank
    bases from A.  kind "FA": the new base is T, F sorts in front of A, A's first row is the candidate (unit row 1) and every
    A row is taken in by the retry (the second one as a far context a second time).  kind "AF": the new base is A, F sorts
    behind A and is the candidate (unit row nlen)."""
    a = pack(UNIT_RIGHT)
    f = pack(UNIT_RIGHT[:UNIT_DEL] + UNIT_RIGHT[UNIT_DEL + 1:] + ("T" if kind == "FA" else "A"))
    arows = [(base, c0, a, ln, cnt) for ln, cnt in zip((7, 6, 5)[:nlen], (3, 9, 4))]
    frow = [(base, c0, f, 6, 5)]
    return (frow + arows, 1) if kind == "FA" else (arows + frow, nlen)


class _Layout:
    """rows of k = 10 under one base, ctx0 descending from `top`: fillers and units, each unit under one ctx0"""

    def __init__(self, base=1, top=(1 << 20) - 1):
        self.base, self.top, self.parts, self.n, self.marks = base, top, [], 0, {}

    def fill_to(self, row):
        """fillers up to (not including) global row `row`"""
        m = row - self.n
        assert m >= 0, (row, self.n)
        if m:
            self.parts.append(fillers(self.top, m, self.base))
            self.top -= m
            self.n += m

    def unit(self, kind, nlen=2, mark=None):
        self.top -= 21                                   # three left-flank bases off the row in front: units side by side stay apart
        rows, off = unit_rows(self.base, self.top, kind, nlen)
        if mark:
            self.marks[mark] = self.n + off
        self.parts.append(Rows(FILLER_K, rows))
        self.top -= 1
        self.n += len(rows)

    def candidate_at(self, row, kind, nlen=2, mark=None):
        """a unit whose candidate lies on global row `row`, fillers in front of it"""
        self.fill_to(row - (1 if kind == "FA" else nlen))
        self.unit(kind, nlen, mark)

    def rows(self, parts):
        self.parts.extend(parts)

    def done(self):
        r = concat(FILLER_K, self.parts)
        r.marks.update(self.marks)
        return r


def retry_pair():
    """a retry unit's F and one A row as the only two rows"""
    rows, _ = unit_rows(1, 0x12345, "FA", 1)
    return Rows(FILLER_K, rows, {"cand": 1})


CASCADE_LEFT = sorted(("TTGCATTGCA", "TCCAGGTCCA", "GGATACGGAT", "GACTTAGACT", "CTAGCCCTAG", "CATGAACATG"), key=pack, reverse=True)


def _del(s, p, new_last):
    return s[:p] + s[p + 1:] + new_last


def _sub(s, p, ch):
    assert s[p] != ch
    return s[:p] + ch + s[p + 1:]


def cascade():
    """Five planted order effects of a replay (k = 10, max_distance_per_flank 2, levenshtein_distance 3), each under a left
    flank of its own, far from the others.  H: a right flank; R1: H with one base deleted (2 edits, 4 or more flank bases
    away); R2: R1 with another base deleted (2 edits from R1, 4 from H).
      new_name   H (5), R1 (9), R2 (4): R1 comes in by the retry with the highest total and becomes the name; R2 is within 3 of
                 R1 only and comes in because of that
      old_name   H (9), R1 (5), R2 (4): the name stays H; R2, within 3 of the flank-only group before it (R1), is flagged by
                 the speculation and the replay refuses it
      absorbed   H (9), R1 (5), S (4): S is R1 with one substitution -- no head in the flank-only grouping, where it joins R1.
                 R1 was absorbed by H's group, whose first context is far from S and whose name is 3 edits away: S opens a group
      tie        H (7), H' (7, one substitution: the same group), D (3): D is H with one base deleted, 2 edits from H and 3 from
                 H'.  The first of the equal totals stays the name, so D comes in
      base       the last row of base 1 and the first of base 0 with the same flanks: 1 edit apart, never joined"""
    H = "ACGTTGCAGT"
    R1 = _del(H, 2, "G")                                  # ACTTGCAGTG
    R2 = _del(R1, 6, "C")                                 # ACTTGCGTGC
    S = _sub(R1, 1, "A")
    H2 = _sub(H, 1, "A")
    D = _del(H, 5, "C")
    rows, marks = [], {}

    def case(name, left, items):
        for tag, right, cnt in items:
            marks[name + "." + tag] = len(rows)
            rows.append((1, pack(left), pack(right), 6, cnt))

    case("new_name", CASCADE_LEFT[0], [("H", H, 5), ("R1", R1, 9), ("R2", R2, 4)])
    case("old_name", CASCADE_LEFT[1], [("H", H, 9), ("R1", R1, 5), ("R2", R2, 4)])
    case("absorbed", CASCADE_LEFT[2], [("H", H, 9), ("R1", R1, 5), ("S", S, 4)])
    case("tie", CASCADE_LEFT[3], [("H", H, 7), ("H2", H2, 7), ("D", D, 3)])
    case("base", CASCADE_LEFT[4], [("last", H, 4)])
    marks["base.first"] = len(rows)
    rows.append((0, pack(CASCADE_LEFT[4]), pack(H), 6, 6))
    rows.append((0, pack(CASCADE_LEFT[5]), pack(H), 6, 3))
    return Rows(10, rows, marks)


def _pattern(k, seed):
    """k bases without long repeats"""
    out, x = [], seed
    for _ in range(k):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append("ACGT"[(x >> 16) & 3])
    return "".join(out)


def threshold_pairs(k, which="edits", lev=3):
    """Neighbouring rows of one base with nothing else under that base, so that nothing else can be the pair's name.  "edits": a
    pair exactly lev - 1 edits apart under base 1 and one exactly lev apart under base 0 (substitutions away from the names'
    ends: the same under both readings).  "shifted": a pair whose right flank is shifted by one base: 2 edits by the global
    distance, 1 with a free end.  k = 2, 10, 32: names of 7, 23 and 67 symbols."""
    assert lev == 3
    left, right = _pattern(k, 7 * k + 1), _pattern(k, 13 * k + 5)
    other = lambda ch: "ACGT"[(_CODE[ch] + 1) & 3]
    subs = lambda s, ps: "".join(other(ch) if i in ps else ch for i, ch in enumerate(s))
    pairs = {"below": ((left, right), (subs(left, {0, 1}), right)),
             "at": ((left, right), (subs(left, {0, 1}), subs(right, {0}))),
             "shifted": ((left, right), (left, right[1:] + other(right[-1])))}
    rows, marks = [], {}
    for base, name in zip((1, 0), ("below", "at") if which == "edits" else ("shifted",)):
        two = sorted(((pack(a), pack(b)) for a, b in pairs[name]), reverse=True)
        marks[name] = len(rows) + 1
        rows += [(base, two[0][0], two[0][1], 6, 5), (base, two[1][0], two[1][1], 6, 3)]
    return Rows(k, rows, marks)


def all_join(k=4, per_base=4500):
    """Two bases of per_base rows (1500 contexts of three lengths).  At levenshtein_distance 2k + 4, above any distance
    between two names, every row of a base is taken in: one tract per base, one replay over a whole base block."""
    rows = []
    n_ctx = per_base // 3
    for base in (1, 0):
        ctx = sorted({(255 - j // 6, ((j % 6) * 43 + (j // 6) * 29 + 11 * base) % 256) for j in range(n_ctx)}, reverse=True)
        assert len(ctx) == n_ctx
        for t, (c0, c1) in enumerate(ctx):
            rows += [(base, c0, c1, ln, _count(t + ln)) for ln in (9, 6, 4)]
    return Rows(k, rows)


def hist_ties():
    """one group (k = 10, max_distance_per_flank 2) of two contexts whose summed lengths tie with a negative length on
    either side: 5 -> 4 + 2, 2 -> 6, -1 -> 4, -3 -> 4 + 2: the bars are (5, 6), (2, 6), (-3, 6), (-1, 4); and a second group with
    (-2, 5), (-7, 5), (3, 2)"""
    left, x = pack("GGATACGGAT"), "ACGTTGCAGT"
    y = _sub(x, 4, "A")
    rows = [(1, left, pack(x), 5, 4), (1, left, pack(x), 2, 6), (1, left, pack(x), -1, 4), (1, left, pack(x), -3, 4),
            (1, left, pack(y), 5, 2), (1, left, pack(y), -3, 2)]
    rows = sorted(rows, key=lambda r: (-r[2], -r[3]))
    left2 = pack("CATGAACATG")
    rows += [(1, left2, pack(x), 3, 2), (1, left2, pack(x), -2, 5), (1, left2, pack(x), -7, 5)]
    return Rows(10, rows)


def count_wrap():
    """X (one substitution from Y), Y, and Z: Y with one base deleted, 2 edits from Y and 3 from X (k = 10, maxd 2, lev 3).
    Sample route: X has 2^20 + 3 copies -- a field of 3 -- and Y 5: Y is the name and Z comes in.  Union route (union_mat): X's
    total over two samples passes 2^31, X is the name and Z stays out."""
    left, y = pack("TTGCATTGCA"), "ACGTTGCAGT"
    x, z = _sub(y, 1, "T"), _del(y, 5, "C")
    rows = sorted([(1, left, pack(x), 6, (1 << 20) + 3), (1, left, pack(y), 6, 5), (1, left, pack(z), 6, 4)], key=lambda r: -r[2])
    r = Rows(10, rows)
    names = {pack(x): "X", pack(y): "Y", pack(z): "Z"}
    r.marks = {names[int(r.keys[i, 1])]: i for i in range(3)}
    return r


def count_wrap_union_mat(rows):
    mat = np.zeros((len(rows), 2), np.int32)
    mat[:, 0] = 2
    mat[:, 1] = np.minimum(rows.counts, 9) - 2
    mat[rows.marks["X"]] = [(1 << 30) + 5, (1 << 30) + 7]
    return mat


def windows():
    """The repair's windows (k = 10, maxd 1, lev 3), retry units placed by fillers; what window_walk must show is in the marks:
    a candidate on row 1; one at offset 0 of the window behind it; one at offset GR_CHUNK - 1; an empty window and a candidate
    on row 0 of the next; 260 candidates four rows apart (more than BLOCK + 1 in one window); a candidate inside an earlier
    replay (cascade's new_name rows); a replay that starts at offset GR_CHUNK - 2 and ends behind its window; a candidate on
    row n - 1."""
    lay = _Layout(base=1)
    lay.candidate_at(1, "FA", mark="row1")                       # rows 0-2, the replay ends behind row 3
    lay.unit("FA", mark="offset0")                               # F on row 3 (a head in both groupings), the candidate on row 4
    w = 7                                                        # that replay ends behind row 6 (a filler)
    lay.candidate_at(w + GR_CHUNK - 1, "FA", mark="offset_last")
    w = w + GR_CHUNK - 1 + 3                                     # A's rows, then behind the filler
    lay.marks["empty_window"] = w
    lay.candidate_at(w + GR_CHUNK, "FA", mark="after_empty")
    lay.marks["many"] = lay.n + 3
    for _ in range(BLOCK + 4):
        lay.fill_to(lay.n + 1)
        lay.unit("AF")
    lay.fill_to(lay.n + 2)
    H = "ACGTTGCAGT"
    R1 = _del(H, 2, "G")
    R2 = _del(R1, 6, "C")
    lay.marks["covered"] = lay.n + 2
    lay.top -= 21
    lay.rows([Rows(10, [(1, lay.top, pack(H), 6, 5), (1, lay.top, pack(R1), 6, 9), (1, lay.top, pack(R2), 6, 4)])])
    lay.top -= 1
    lay.n += 3
    lay.fill_to(lay.n + 1)
    w = lay.n                                                    # the covered unit's replay ends behind this filler's row
    lay.marks["past_end_window"] = w
    lay.candidate_at(w + GR_CHUNK - 2, "FA", nlen=3, mark="past_end")
    lay.fill_to(lay.n + 40)
    lay.unit("AF", mark="last_row")
    return lay.done()


def grid_stride(which):
    """n = ONE_TRIP + 300 rows of k = 10, the smallest shape at which the kernels' grid-stride loops take a second trip.
    "staircase": fillers of base 1, then under base 0 staircase (10, 5, hold_top: 290 rows, so that fillers of the same base
    fit behind it -- a sample only keeps bases 0 and 1) from row ONE_TRIP - 150, so that it straddles row ONE_TRIP, then fillers.  "retry": fillers and, on rows ONE_TRIP - 2 .. ONE_TRIP + 1, A, F1, F2, F3 (_grid_stride_retry):
    candidates on rows ONE_TRIP - 1, ONE_TRIP and ONE_TRIP + 1.  A row cannot be both inside the staircase and a candidate,
    hence two layouts of the one shape."""
    n = ONE_TRIP + 300
    if which == "staircase":
        st = staircase(10, 5, base=0, hold_top=True)
        at = ONE_TRIP - 150
        assert at <= 1 << 20
        r = concat(10, [fillers((1 << 20) - 1, at, 1), st, fillers((3 << 18) - 1, n - at - len(st), 0)])
        r.marks = {"first": at, "last": at + len(st) - 1}
        return r
    return _grid_stride_retry(n, 4096)                           # base 1 in front, the rest under base 0: ctx0 has 2^20 values


def _grid_stride_retry(n, lead):
    """three candidates on neighbouring rows: F1, F2, F3 behind one A, each a deletion of the one before it, so that each is a
    flank-only head within 3 edits of the single row in front of it"""
    a = UNIT_RIGHT
    f1 = _del(a, 3, "A")
    f2 = _del(f1, 5, "A")
    f3 = _del(f2, 2, "A")
    lay = _Layout(base=0)
    lay.n = lead
    lay.fill_to(ONE_TRIP - 2)
    c0 = lay.top
    chain = [(0, c0, pack(s), 6, cnt) for s, cnt in ((a, 9), (f1, 5), (f2, 4), (f3, 3))]
    assert [r[2] for r in chain] == sorted((r[2] for r in chain), reverse=True)
    lay.rows([Rows(10, chain)])
    lay.top -= 1
    lay.n += 4
    lay.fill_to(n)
    r = concat(10, [fillers((1 << 20) - 1, lead, 1)] + lay.parts)
    r.marks = {"cand-1": ONE_TRIP - 1, "cand0": ONE_TRIP, "cand1": ONE_TRIP + 1}
    return r


# ---- the cases both test files run ------------------------------------------------------------------------------------------

def single_row():
    return Rows(10, [(1, pack("TTGCATTGCA"), pack("ACGTTGCAGT"), 6, 3)])


def two_rows():
    """one context, two lengths"""
    return Rows(10, [(1, pack("TTGCATTGCA"), pack("ACGTTGCAGT"), 6, 3), (1, pack("TTGCATTGCA"), pack("ACGTTGCAGT"), 4, 5)])


# name -> (generator, [(max_distance_per_flank, levenshtein_distance)], both readings of the edit distance?)
CASES = {
    "windows": (windows, [(1, 3)], True),                         # (the larger problems first: the small ones meet their stale scratch)
    "all_join": (all_join, [(1, 12)], False),
    "staircase-k10-L70": (lambda: staircase(10, 70), [(2, 3), (2, 0)], False),
    "staircase-k10-L100-thin": (lambda: staircase(10, 100, thin=True), [(2, 3), (2, 0)], False),
    "staircase-k10-L5": (lambda: staircase(10, 5), [(2, 0), (2, 2), (2, 3), (1, 2), (3, 2)], False),
    "staircase-k32-L3": (lambda: staircase(32, 3), [(2, 2), (2, 3)], False),
    "cascade": (cascade, [(2, 3), (2, 0)], True),
    "threshold-k2": (lambda: threshold_pairs(2), [(1, 2), (1, 3), (1, 4)], True),
    "threshold-k10": (lambda: threshold_pairs(10), [(1, 2), (1, 3), (1, 4)], True),
    "threshold-k32": (lambda: threshold_pairs(32), [(1, 2), (1, 3), (1, 4)], True),
    "shifted-k2": (lambda: threshold_pairs(2, "shifted"), [(1, 2), (1, 3), (1, 4)], True),
    "shifted-k10": (lambda: threshold_pairs(10, "shifted"), [(1, 2), (1, 3), (1, 4)], True),
    "shifted-k32": (lambda: threshold_pairs(32, "shifted"), [(1, 2), (1, 3), (1, 4)], True),
    "hist_ties": (hist_ties, [(2, 3)], False),
    "retry_pair": (retry_pair, [(1, 3)], True),
    "two_rows": (two_rows, [(1, 2)], False),
    "single_row": (single_row, [(1, 2)], False),
}
STAIRCASE_MAXD = (2, 1, 3)                                        # tjamd_group_contexts on every staircase

_made = {}


def get(name):
    """a case's Rows, made once and not to be written to"""
    if name not in _made:
        r = CASES[name][0]()
        r.keys.setflags(write=False); r.counts.setflags(write=False)
        _made[name] = r
    return _made[name]


def with_counts(rows, count):
    """the same rows, every count (and count field) set to `count`"""
    keys = rows.keys.copy()
    keys[:, 2] = (keys[:, 2] & ~np.uint64(0xFFFFF << 12)) | np.uint64(count << 12)
    return Rows(rows.k, (keys, np.full(len(keys), count, np.int64)), rows.marks)
