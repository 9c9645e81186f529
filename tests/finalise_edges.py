"""Edge corpus for the per-sample finalise: the aggregation (aggregate1/2/4_kernel) and the ordering step (bin partition,
bin_sort_index_kernel, context index, coverage table, radix fallback).  Deterministic, seeded generators of read streams
(uint8, '\\n'-terminated).  Every read is `left flank (k) + tract + right flank (k)`: it yields exactly one record (a run
inside a flank has fewer than k bytes on one side and is not recorded), so a corpus is a table of reduction keys
(base in {A, C}, ctx0, ctx1, length) with the number of reads wanted on either strand.  No GPU and no built device library
are needed to make them; tests/test_finalise_edges_corpus.py shows on the CPU, from the oracle and the restatements below,
that each corpus is what its docstring says, and tests/test_finalise_edges.py runs them through the device finalise.
Test infrastructure.

The constants restate tatajuba_amd/csrc/hopo_device.hip; tests/test_finalise_edges_corpus.py parses the #define lines and
fails when one moves.  The restated FUNCTIONS (pack_rec1, bucket_of_rec1, bucket_of_key, bin_bits_for, bin_of_record,
cov_table_bits, cov_plan_bits, plan_cap, chunk_records) have no source to be parsed against: if the kernels' arithmetic
drifts away from them a corpus is aimed beside its edge (and the bucket counts the GPU tests compare stop matching), but
no GPU test can pass wrongly because of it -- those compare the device with the oracle, never with this module.

DEVICE_EXCLUDED: the zero_key corpora are made and checked on the CPU but not yet run on the device.  They show a bug of
aggregate1_kernel: the reduction key whose record word is 0 without its strand flag (an A tract of 1024 or 2048 bytes between
flanks that code as 0, which takes a byte outside ACGT next to the tract) is taken for an empty slot of the LDS table, its
records are added to that slot's counters and the output loop skips the slot: on an MI355X the device kept 302 records of
zero_key-k2 and of zero_key-k12 where the oracle keeps 303, under every filter and ordering path.  The change that mends it
(the table holds the word with bit 63 set) passed these corpora, but the whole suite built with it ended in a host
segmentation fault inside tjamd_finalise in tests/test_scan_variants.py, cause not found; the change and the device run of
these corpora wait for that cause."""
import numpy as np

from tests.edge_streams import NL, TJ_CH0, record_width

# ---- the kernels' geometry (hopo_device.hip) ------------------------------------------------------------------------
TJ_P = 256                           # hash buckets
AG_BLOCK = 1024                      # lanes of an aggregation workgroup: at most one more key per lane gets into a closing table
AG_NCH = 512                         # chunk ids of a bucket cached in LDS
AG1_S, AG2_S, AG4_S = 8192, 6144, 4096
AG1_CLOSE_AT, AG2_CLOSE_AT, AG4_CLOSE_AT = 4864, 2560, 2560
AG1_R, AG2_R, AG4_R = 4, 4, 2        # records in flight per lane
BS_RANK_MAX = 256                    # records of a bin that a wavefront sorts; a fuller bin: radix fallback
BS_MAXBITS = 16
R1_FLAG_SHIFT = 59

M = 2                                # minimum tract size of every corpus (tracts are two bytes or longer)
CLOSE_AT = {1: AG1_CLOSE_AT, 2: AG2_CLOSE_AT, 4: AG4_CLOSE_AT}
IN_FLIGHT = {1: AG1_R, 2: AG2_R, 4: AG4_R}
K_OF_W = {1: 10, 2: 20, 4: 31}       # one k per record width for the width-specific corpora
K_BORDERS = (2, 12, 13, 28, 29, 32)  # the small corpora also run here

_ACGT = np.frombuffer(b"ACGT", np.uint8)
KEY_DTYPE = np.dtype([("base", "u1"), ("c0", "<u8"), ("c1", "<u8"), ("length", "<i4"), ("nf", "<i8"), ("nr", "<i8"), ("nflank", "u1")])
_U = np.uint64


def max_admitted(w):
    """the most keys one round of a closing table can admit: it closes above CLOSE_AT, and every lane looks before its claim"""
    return CLOSE_AT[w] + 1 + AG_BLOCK


# ---- restatements of the device arithmetic ----------------------------------------------------------------------------

def udot4(a, b, c):
    """sum of byte_i(a) * byte_i(b), plus c, modulo 2^32 (v_dot4_u32_u8)"""
    a, b, c = (np.asarray(x, dtype=np.uint64) for x in (a, b, c))
    s = c.copy() if c.ndim else np.uint64(c)
    for i in range(4):
        s = s + ((a >> _U(8 * i)) & _U(255)) * ((b >> _U(8 * i)) & _U(255))
    return s & _U(0xFFFFFFFF)


def len10(length):
    return np.asarray(length, dtype=np.int64).astype(np.uint64) & _U(0x3FF)


def pack_rec1(c0, c1, base, l10, flag):
    """the two halves (lo, hi) of a one-word record"""
    c0, c1, base, l10, flag = (np.asarray(x, dtype=np.uint64) for x in (c0, c1, base, l10, flag))
    lo = (c1 | (l10 << _U(24))) & _U(0xFFFFFFFF)
    hi = (c0 | ((l10 >> _U(8)) << _U(24)) | (base << _U(26)) | (flag << _U(27))) & _U(0xFFFFFFFF)
    return lo, hi


def bucket_of_rec1(lo, hi):
    h = udot4(lo, 0x6D2B4F0B, 0)
    h = udot4(np.asarray(hi, dtype=np.uint64) & _U(0x07FFFFFF), 0xC5A34D17, h)
    return ((h ^ (h >> _U(8))) & _U(255)).astype(np.int64)


def bucket_of_key(c0, c1, base, l10):
    c0, c1, base, l10 = (np.asarray(x, dtype=np.uint64) for x in (c0, c1, base, l10))
    m32 = _U(0xFFFFFFFF)
    h = udot4(c0 & m32, 0x6D2B4F0B, (base | (l10 << _U(2))) & m32)
    h = udot4(c0 >> _U(32), 0x1D59A735, h)
    h = udot4(c1 & m32, 0xC5A34D17, h)
    h = udot4(c1 >> _U(32), 0x3B7F9165, h)
    return ((h ^ (h >> _U(8))) & _U(255)).astype(np.int64)


def bucket_of(k, base, c0, c1, length):
    """hash bucket of a reduction key at this k (the strand flag is no part of it)"""
    if record_width(k) == 1:
        return bucket_of_rec1(*pack_rec1(c0, c1, base, len10(length), 0))
    return bucket_of_key(c0, c1, base, len10(length))


def rec1_key_word(c0, c1, base, length):
    """the one-word record without its strand flag: the table key of aggregate1_kernel before it is marked as used"""
    lo, hi = pack_rec1(c0, c1, base, len10(length), 0)
    return (hi << _U(32)) | lo


def chunk_records(records_bound):
    """TJ_CH0 << shift of choose_chunk_size: fixed by the first scan's (or upload's) bound of its record count"""
    units = int(records_bound) // (16384 * TJ_CH0)
    sft = 3
    while (1 << sft) < units:
        sft += 1
    return TJ_CH0 << sft


def scan_bound(n_bytes):
    """the host's upper bound of the records of one scanned batch (minimum tract size M)"""
    return n_bytes // max(M, 2) + 1


def plan_cap(raw_bound):
    """kept records the ordering step is planned for on the device (finalise_impl); more: the step runs again"""
    kept_cap = raw_bound // 2 + 1
    return min(kept_cap, max(kept_cap // 8, 1 << 16))


def cov_table_bits(n1):
    b = 10
    while (1 << b) < 4 * n1 and b < 31:
        b += 1
    return b


def cov_plan_bits(n1, k):
    """(log2 of the coverage table's size, addressed by the key itself?)"""
    hb, kb = cov_table_bits(n1), min(2 * k, 31)
    return (kb, True) if kb <= hb else (hb, False)


def fine_bin_bits(k):
    return min(BS_MAXBITS, 1 + 4 * k)


def bin_bits_for(n1, k):
    nbits = 6
    while nbits < BS_MAXBITS and nbits < 1 + 4 * k and (48 << nbits) < n1:
        nbits += 1
    return min(nbits, 1 + 4 * k)


def bin_of_record(c0, c1, base, k, nbits):
    """leading nbits of [base:1][ctx0:2k][ctx1:2k], complemented"""
    c0, c1, base = (np.asarray(x, dtype=np.uint64) for x in (c0, c1, base))
    kb = nbits - 1
    if 2 * k >= kb:
        v = c0 >> _U(2 * k - kb)
    else:
        v = (c0 << _U(kb - 2 * k)) | (c1 >> _U(4 * k - kb))
    x = ((base & _U(1)) << _U(kb)) | v
    return (_U((1 << nbits) - 1) - x).astype(np.int64)


def bin_occupancy(keys, k, n1=None):
    """records per bin of the ordering step when every key of the table is kept (sorted, empty bins left out)"""
    n1 = len(keys) if n1 is None else n1
    b = bin_of_record(keys["c0"], keys["c1"], keys["base"], k, bin_bits_for(n1, k))
    return np.sort(np.bincount(b)[np.bincount(b) > 0])


def coverage_restated(elems, pool=True, cut=True):
    """numpy restatement of orc_coverage on kept elements (ctx0, ctx1, signed 20-bit count): flanks cut to 31 bits, both
    sides pooled, the largest pooled weight.  pool=False: either side on its own; cut=False: whole flanks"""
    w = ((elems["meta"] >> _U(12)) & _U(0xFFFFF)).astype(np.int64)
    w = np.where(w >= (1 << 19), w - (1 << 20), w)
    mask = _U(0x7FFFFFFF) if cut else _U(0xFFFFFFFFFFFFFFFF)
    best = None
    sides = [np.concatenate([elems["ctx0"], elems["ctx1"]])] if pool else [elems["ctx0"], elems["ctx1"]]
    for s in sides:
        ww = np.concatenate([w, w]) if pool else w
        u, inv = np.unique(s & mask, return_inverse=True)
        tot = np.bincount(inv, weights=ww.astype(np.float64)).astype(np.int64)
        best = int(tot.max()) if best is None else max(best, int(tot.max()))
    return best


# ---- keys and reads -----------------------------------------------------------------------------------------------------

def key_table(rows):
    """[(base, c0, c1, length, reads forward, reads reverse[, nflank])] -> KEY_DTYPE"""
    t = np.zeros(len(rows), KEY_DTYPE)
    for i, r in enumerate(rows):
        t[i] = tuple(r) + (0,) * (7 - len(r))
    return t


def valid_key(k, base, c0, c1):
    """the byte next to the tract differs from the tract's base on either side (or the read would hold a longer tract)"""
    c0, c1, base = (np.asarray(x, dtype=np.uint64) for x in (c0, c1, base))
    return (((c0 >> _U(2 * (k - 1))) & _U(3)) != base) & ((c1 & _U(3)) != base)


def read_for_key(k, base, c0, c1, length, reverse=False, nflank=False):
    """the read (bytes, no delimiter) whose one record has this key; bit order of oracle.orc.name_of.  reverse: its reverse
    complement, the same key seen on the other strand.  nflank: the flank bytes next to the tract, whose code must be 0 (A),
    are written as N -- a byte outside ACGT is coded as 0, which is how a key next to an A tract can hold an A there"""
    dna = "ACGT"
    left = [dna[(int(c0) >> (2 * i)) & 3] for i in range(k)]
    right = [dna[(int(c1) >> (2 * i)) & 3] for i in range(k)]
    if nflank:
        assert left[-1] == "A" and right[0] == "A"
        left[-1] = right[0] = "N"
    assert left[-1] != dna[base] and right[0] != dna[base] and base in (0, 1) and length >= M
    s = "".join(left) + dna[base] * length + "".join(right)
    if reverse:
        s = s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))
    return s.encode()


def build_stream(k, keys, seed=0, shuffle_below=400000):
    """the reads of a key table: keys['nf'] times the forward read and keys['nr'] times its reverse complement, per key.
    Reads of one length are laid down together (shuffled among themselves unless there are shuffle_below of them or more)"""
    rng = np.random.default_rng([seed, k, len(keys)])
    comp_n = np.array([3, 2, 1, 0, 4], np.uint8)
    letters = np.frombuffer(b"ACGTN", np.uint8)
    sh = (2 * np.arange(k)).astype(np.uint64)
    out = []
    for L in np.unique(keys["length"]):
        g = keys[keys["length"] == L]
        rep = g["nf"] + g["nr"]
        g, rep = g[rep > 0], rep[rep > 0]
        if len(g) == 0:
            continue
        L = int(L)
        w = 2 * k + L
        codes = np.empty((len(g), w), np.uint8)
        codes[:, :k] = (g["c0"][:, None] >> sh) & _U(3)
        codes[:, k:k + L] = g["base"][:, None]
        codes[:, k + L:] = (g["c1"][:, None] >> sh) & _U(3)
        nfl = g["nflank"] != 0
        assert (codes[nfl, k - 1] == 0).all() and (codes[nfl, k + L] == 0).all()
        codes[nfl, k - 1] = 4
        codes[nfl, k + L] = 4
        assert (codes[:, k - 1] != g["base"]).all() and (codes[:, k + L] != g["base"]).all()
        idx = np.repeat(np.arange(len(g)), rep)
        first = np.repeat(np.cumsum(rep) - rep, rep)
        rev = (np.arange(idx.size) - first) >= g["nf"][idx]
        if idx.size < shuffle_below:
            p = rng.permutation(idx.size)
            idx, rev = idx[p], rev[p]
        rows = np.empty((idx.size, w + 1), np.uint8)
        rows[:, :w] = codes[idx]
        rows[rev, :w] = comp_n[rows[rev, :w][:, ::-1]]
        rows[:, :w] = letters[rows[:, :w]]
        rows[:, w] = NL
        out.append(rows.reshape(-1))
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def expected_raw(k, keys):
    """(ctx0, ctx1, meta) and the multiplicity of every distinct raw element the oracle is to return for a key table"""
    rows = []
    for flag, col in ((1, "nf"), (2, "nr")):
        g = keys[keys[col] > 0]
        meta = g["base"].astype(np.uint64) | (len10(g["length"]) << _U(2)) | (_U(1) << _U(12)) | (_U(0xFFE) << _U(32)) | (_U(flag) << _U(49))
        rows.append((g["c0"], g["c1"], meta, g[col]))
    return tuple(np.concatenate([r[i] for r in rows]) for i in range(4))


def mix3(c0, c1, meta):
    """one 64-bit word per element (to count distinct elements of millions quickly)"""
    c0, c1, meta = (np.asarray(x, dtype=np.uint64) for x in (c0, c1, meta))
    h = c0 * _U(0x9E3779B97F4A7C15) + (c1 ^ (c1 >> _U(29))) * _U(0xBF58476D1CE4E5B9) + meta * _U(0x94D049BB133111EB)
    return h ^ (h >> _U(31))


def bucket_counts(k, keys):
    """raw records per hash bucket of a key table"""
    b = bucket_of(k, keys["base"], keys["c0"], keys["c1"], keys["length"])
    return np.bincount(b, weights=(keys["nf"] + keys["nr"]).astype(np.float64), minlength=TJ_P).astype(np.int64)


def _random_key_arrays(rng, k, c, base, lengths):
    """c random candidates, the valid ones returned as an array [n, 4] of (base, c0, c1, length); not yet distinct"""
    def flank():
        if 2 * k < 64:
            return rng.integers(0, 1 << (2 * k), c, dtype=np.uint64)
        return rng.integers(0, 1 << 63, c, dtype=np.uint64) * _U(2) + rng.integers(0, 2, c).astype(np.uint64)
    b = rng.integers(0, 2, c).astype(np.uint64) if base is None else np.full(c, base, np.uint64)
    c0, c1 = flank(), flank()
    ln = rng.integers(lengths[0], lengths[1], c).astype(np.uint64)
    ok = valid_key(k, b, c0, c1)
    return np.stack([b[ok], c0[ok], c1[ok], ln[ok]], axis=1)


def _key_space(k, lengths):
    return 2 * 9 * 16 ** (k - 1) * (lengths[1] - lengths[0])


def random_keys(rng, k, n, base=None, lengths=(2, 40)):
    """n distinct valid keys (base, c0, c1, length): random flanks, lengths in [lengths[0], lengths[1])"""
    assert n <= _key_space(k, lengths) // 4
    got, seen = [], set()
    while len(got) < n:
        for t in _random_key_arrays(rng, k, max(256, 2 * (n - len(got))), base, lengths).tolist():
            t = tuple(t)
            if t not in seen and len(got) < n:
                seen.add(t)
                got.append(t)
    return got


def keys_of_bucket(rng, k, bucket, n, lengths=(2, 40), base=None):
    """n distinct valid keys that the device hashes to this bucket: random candidates, buckets computed in numpy"""
    assert n <= _key_space(k, lengths) // (2 * TJ_P)
    got, seen = [], set()
    while len(got) < n:
        a = _random_key_arrays(rng, k, int(min(max(8192, 400 * (n - len(got))), 1 << 21)), base, lengths)
        sel = bucket_of(k, a[:, 0], a[:, 1], a[:, 2], a[:, 3].astype(np.int64)) == bucket
        for t in a[sel].tolist():
            t = tuple(t)
            if t not in seen and len(got) < n:
                seen.add(t)
                got.append(t)
    return got


def _split(rng, r):
    """a random strand split of r records with both strands seen (r >= 2)"""
    f = int(rng.integers(1, r)) if r >= 2 else r
    return f, r - f


class Corpus:
    """name, k, the key table, its own min_coverage threshold, and what the corpus claims (facts: a dict the CPU test checks)"""

    def __init__(self, name, k, keys, min_coverage, route="scan", **facts):
        self.name, self.k, self.keys, self.min_coverage, self.route, self.facts = name, k, keys, min_coverage, route, facts

    def parts(self, limit=96 << 20):
        """the stream, cut at read delimiters into parts of at most ~limit bytes (scanned one after the other)"""
        s = build_stream(self.k, self.keys, seed=len(self.name))
        out = []
        while s.size > limit:
            cut = limit - int(np.argmax(s[limit - 1::-1] == NL))
            out.append(s[:cut])
            s = s[cut:]
        out.append(s)
        return out

    @property
    def n_reads(self):
        return int((self.keys["nf"] + self.keys["nr"]).sum())


# ---- aggregation ----------------------------------------------------------------------------------------------------------

def zero_key(k):
    """k = 2 and 12 (one-word records).  The reduction key whose record word is 0 without its strand flag: base A, both flanks
    coded 0 -- the bytes next to the tract are N -- and a stored length of 0 (1024 and 2048 bytes), on both strands.  Its
    neighbours: the same with 1025 bytes, and the C tract of 1024 bytes between all-A flanks.  And 300 ordinary keys of the zero
    key's hash bucket (twice on either strand), so that other keys claim slots of the table the zero key went through."""
    assert record_width(k) == 1
    rng = np.random.default_rng([11, k])
    b = int(bucket_of(k, 0, 0, 0, 1024))
    rows = [(0, 0, 0, 1024, 3, 2, 1), (0, 0, 0, 2048, 1, 2, 1), (0, 0, 0, 1025, 2, 1, 1), (1, 0, 0, 1024, 2, 2, 0)]
    rows += [t + (2, 2, 0) for t in keys_of_bucket(rng, k, b, 300, lengths=(2, 1023) if k == 2 else (2, 60))]
    keys = key_table(rows)
    return Corpus("zero_key-k%d" % k, k, keys, 9, zero_bucket=b, zero_total=8, aliases=1)


def extreme_flanks(k):
    """flanks that are all A (packed 0), all T (all ones), and one of each, around A and C tracts of a few lengths, each key twice
    on either strand.  (An all-A flank beside an A tract, an all-T... the byte next to the tract must differ from its base: A
    tracts take all-T flanks and flanks whose last byte alone is not A; C tracts take every one.)  At k = 31 and 32 the
    C tract between all-A flanks is the "both k-mers 0: the cleared state" case of aggregate4_kernel."""
    ones = (1 << (2 * k)) - 1
    rows = []
    for base in (0, 1):
        for c0 in (0, ones):
            for c1 in (0, ones):
                if bool(valid_key(k, base, c0, c1)):
                    for ln in (2, 3, 512, 1024):
                        rows.append((base, c0, c1, ln, 2, 2, 0))
    # A tracts beside "all A but the byte next to the tract"
    near0_l, near0_r = 1 << (2 * (k - 1)), 1
    rows += [(0, near0_l, near0_r, 5, 2, 2, 0), (0, near0_l, ones, 5, 1, 1, 0), (0, ones, near0_r, 5, 3, 0, 0)]
    return Corpus("extreme_flanks-k%d" % k, k, key_table(rows), 9, n_both_zero=4)


COUNT_EDGES_FULL = [(1, "one"), (2, "one"), (2, "split"), (3, "one"), (3, "split"), ((1 << 19) - 1, "split"), (1 << 19, "one"), (1 << 19, "split"),
                    ((1 << 19) + 1, "split"), ((1 << 20) - 1, "split"), (1 << 20, "split"), ((1 << 20) + 1, "split"), ((1 << 20) + 2, "split")]
COUNT_EDGES_SHORT = [(1, "one"), (2, "split"), (3, "split"), (1 << 19, "one"), (1 << 19, "split"), (1 << 20, "split"), ((1 << 20) + 2, "split")]


def count_edges(k):
    """One key, of a context of its own, per total count and strand split of COUNT_EDGES_FULL (k = 2) or COUNT_EDGES_SHORT (other
    k): the count is a signed 20-bit field (2^19 reads count as -524288, 2^20 as 0, 2^20 + 2 as 2) that is kept under
    remove_biased = 1 when both strands were seen and under 0 only when it is above 1.  The key of 2^19 reads on both strands shares its
    context with one of 3 reads: that context's depth, -524285, is below every min_coverage."""
    rng = np.random.default_rng([13, k])
    cases = COUNT_EDGES_FULL if k == 2 else COUNT_EDGES_SHORT
    ctx = random_keys(rng, k, len(cases) + 40, lengths=(2, 3))
    seen, rows = set(), []
    for t in ctx:                                            # contexts of their own
        if (t[0], t[1], t[2]) not in seen and len(rows) < len(cases) + 1:
            seen.add((t[0], t[1], t[2]))
            rows.append(t)
    pair = rows.pop()
    out = []
    for (total, split), t in zip(cases, rows):
        nf = total if split == "one" else (total + 1) // 2
        c = pair if (total, split) == (1 << 19, "split") else t          # the context of two records: -524288 and 3
        out.append((c[0], c[1], c[2], 2, nf, total - nf, 0))
    out.append((pair[0], pair[1], pair[2], 3, 2, 1, 0))
    return Corpus("count_edges-k%d" % k, k, key_table(out), 3, cases=cases)


ONE_BUCKET_D = ("CLOSE_AT-1", "CLOSE_AT", "CLOSE_AT+1", "CLOSE_AT+2", "MAX", "MAX+1", "2MAX+1")


def one_bucket_d(w, name):
    c, mx = CLOSE_AT[w], max_admitted(w)
    return {"CLOSE_AT-1": c - 1, "CLOSE_AT": c, "CLOSE_AT+1": c + 1, "CLOSE_AT+2": c + 2, "MAX": mx, "MAX+1": mx + 1, "2MAX+1": 2 * mx + 1}[name]


def one_bucket_r(w, D):
    """records per key.  A round admits between CLOSE_AT + 1 and max_admitted keys, so its leftovers are between
    (D - max_admitted) * r and (D - CLOSE_AT - 1) * r records.  2MAX+1 keys: r makes the lower figure exceed a chunk (the second
    pool is written across a chunk boundary whatever the race admits, and a third round is certain).  MAX and MAX+1 keys: the
    lower figure is 0 or r -- it would take 72 million records to lift it over a chunk -- so r makes the upper figure, the
    leftovers of a table that closes without overshoot, exceed a chunk.  Fewer keys: 3 records each."""
    ch, mx = chunk_records(0), max_admitted(w)
    if D >= 2 * mx + 1:
        return ch // (D - mx) + 1
    if D >= mx:
        return ch // (D - CLOSE_AT[w] - 1) + 1
    return 3


def one_bucket_keys(k, d_name, bucket, others):
    """D distinct keys of one hash bucket, r records each with a random strand split (both strands seen); others: the other 255
    buckets stay empty (False) or take 600 random keys, twice on either strand (True)"""
    w = record_width(k)
    D = one_bucket_d(w, d_name)
    r = one_bucket_r(w, D)
    rng = np.random.default_rng([17, k, D, bucket])
    rows = [t + _split(rng, r) + (0,) for t in keys_of_bucket(rng, k, bucket, D)]
    if others:
        have = {t[:4] for t in rows}
        rows += [t + (2, 2, 0) for t in random_keys(rng, k, 600) if t not in have and int(bucket_of(k, t[0], t[1], t[2], t[3])) != bucket]
    return Corpus("one_bucket-k%d-%s-b%d-%s" % (k, d_name, bucket, "filled" if others else "alone"), k, key_table(rows), r,
                  bucket=bucket, D=D, r=r, others=others)


BUCKET_SIZES = ("1", "2", "64R-1", "64R", "64R+1", "chunk-1", "chunk", "chunk+1")


def bucket_size_n(w, name):
    ch, b = chunk_records(0), 64 * IN_FLIGHT[w]
    return {"1": 1, "2": 2, "64R-1": b - 1, "64R": b, "64R+1": b + 1, "chunk-1": ch - 1, "chunk": ch, "chunk+1": ch + 1}[name]


def bucket_sizes(k, name):
    """one hash bucket that holds exactly n records (three keys of it, or as many as n allows, both strands where a key has two
    records); the other buckets are empty"""
    w = record_width(k)
    n = bucket_size_n(w, name)
    rng = np.random.default_rng([19, k, n])
    nk = min(3, n)
    ks = keys_of_bucket(rng, k, 77, nk)
    share = [n // nk + (1 if i < n % nk else 0) for i in range(nk)]
    rows = [t + (_split(rng, s) if s >= 2 else (1, 0)) + (0,) for t, s in zip(ks, share)]
    return Corpus("bucket_sizes-k%d-%s" % (k, name), k, key_table(rows), 5, bucket=77, n=n)


LONG_BUCKET_K = 4


def long_bucket():
    """More than AG_NCH * chunk records of one key in one bucket (chunk ids looked up past the LDS cache), and 6000 further keys
    of the same bucket, one read on either strand: a second round behind a very long first.  k = 4, not 2: at k = 2 a bucket has
    some 1150 possible keys in all, fewer than a table admits, and no second round can happen."""
    k = LONG_BUCKET_K
    rng = np.random.default_rng([23, k])
    n_long = AG_NCH * chunk_records(0) + chunk_records(0) + 5
    big = keys_of_bucket(rng, k, 200, 1, lengths=(2, 3))[0]
    rest = [t for t in keys_of_bucket(rng, k, 200, 6001, lengths=(2, 60)) if t != big][:6000]
    rows = [big + (n_long // 2 + 1, n_long - n_long // 2 - 1, 0)] + [t + (1, 1, 0) for t in rest]
    return Corpus("long_bucket-k%d" % k, k, key_table(rows), 3, bucket=200, n_long=n_long, D=6001)


def kept_exactly_full(k, n):
    """n raw records: every key has exactly two, one per strand (n odd: one key more, with a single record).  Fed through
    Counter.upload_raw as the oracle's own raw elements, the host's bound of the raw count is exact, the kept list has
    n // 2 + 1 slots, and n // 2 records are kept: it is filled to its last slot but one."""
    rng = np.random.default_rng([29, k, n])
    rows = [t + (1, 1, 0) for t in random_keys(rng, k, n // 2)]
    if n & 1:
        have = {r[:4] for r in rows}
        extra = [t for t in random_keys(rng, k, n // 2 + 1) if t not in have][0]
        rows.append(extra + (1, 0, 0))
    return Corpus("kept_exactly_full-k%d-n%d" % (k, n), k, key_table(rows), 3, route="upload", n=n, n1=n // 2)


# ---- ordering step ----------------------------------------------------------------------------------------------------------

KEPT_COUNTS = [(10, 3072), (10, 3073), (10, 6144), (10, 6145), (10, 12288), (10, 12289), (2, 6144), (2, 6145), (2, 12288), (2, 12289),
               (6, 512), (6, 513), (10, 131072), (10, 131073)]


def kept_counts(n1, k):
    """exactly n1 kept records under either filter: n1 keys, each read once on either strand.  k = 2: all 288 contexts, as many
    lengths each as it takes; other k: random keys"""
    rng = np.random.default_rng([31, k, n1])
    if k == 2:
        ctxs = [(b, c0, c1) for b in (0, 1) for c0 in range(16) for c1 in range(16) if bool(valid_key(2, b, c0, c1))]
        assert len(ctxs) == 288
        rows = [(b, c0, c1, 2 + i // 288) for i, (b, c0, c1) in ((i, ctxs[i % 288]) for i in range(n1))]
    else:
        rows = random_keys(rng, k, n1, lengths=(2, 12))
    # (a key counts 2: at k = 2 the contexts have n1 // 288 or one more lengths, and the threshold parts them; elsewhere nearly
    # every context is one key, exactly at the threshold)
    mc = 2 * -(-n1 // 288) if k == 2 else 2
    return Corpus("kept_counts-k%d-n%d" % (k, n1), k, key_table([t + (1, 1, 0) for t in rows]), mc, n1=n1)


STAIRCASE = (1, 2, 63, 64, 65, 66, 128, 129, 255)
STAIR_LENGTHS = (511, 512, 1023, 1024, 1025)
STAIR_MIN_COVERAGE = 4               # a key is read twice: a context of two records has depth 4, one of a single record 2


def _stair_context_sizes(s, lane63):
    """context sizes of a bin of s records, in descending key order"""
    if s == 64:
        return [64] if lane63 == "whole" else ([2, 1, 2, 56, 2, 1] if lane63 == "alone" else [1, 2, 57, 2, 2])
    out, left = [], s
    for c in (65, 64, 2, 2, 1, 2, 1):
        if c <= left:
            out.append(c)
            left -= c
    while left:
        c = min(left, 1 + (left % 3))
        out.append(c)
        left -= c
    return out


def bin_staircase(k, top, lane63="alone"):
    """The bins of the ordering step hold exactly 1, 2, 63, 64, 65, 66, 128, 129, 255 and `top` records (256: every bin is
    sorted in LDS; 257: the whole sort falls back to the radix path) and every other bin is empty: 773 + top kept records make
    64 bins, a bin is the base and the leading five bits of ctx0, and a bin's records vary the rest of ctx0, ctx1 and the length.
    Inside the bins: contexts of 1, 2, 64 and 65 records (a context's records differ in length: 511, 512, 1023, 1024, 1025 -- the
    signed ten-bit order -- then 2, 3, ...); in the bin of 64 a context alone in lane 63 ("alone"), a context of two that ends
    there ("ends") or one context of 64 ("whole").  Every key is read once on either strand: a context of two records has depth
    exactly STAIR_MIN_COVERAGE, one of a single record is below it."""
    assert k >= 3
    rng = np.random.default_rng([37, k, top])
    sizes = list(STAIRCASE) + [top]
    n1 = sum(sizes)
    assert bin_bits_for(n1, k) == 6
    lengths = list(STAIR_LENGTHS) + list(range(2, 62))
    rows, ctx_sizes = [], []
    prefixes = [(b, p) for b in (0, 1) for p in range(32) if (p >> 3) != b]      # base, leading five bits of ctx0 (its first code differs from the base)
    pick = rng.permutation(len(prefixes))[:len(sizes)]
    low_bits = 2 * k - 5
    for s, pi in zip(sizes, pick):
        base, p = prefixes[pi]
        want = _stair_context_sizes(s, lane63)
        seen = set()
        while len(seen) < len(want):
            c0 = (p << low_bits) | int(rng.integers(0, 1 << min(low_bits, 62)))
            c1 = int(rng.integers(0, 1 << min(2 * k, 62)))
            if bool(valid_key(k, base, c0, c1)):
                seen.add((c0, c1))
        for c, (c0, c1) in zip(want, sorted(seen, reverse=True)):        # the bin's contexts in the order of the sorted output
            ctx_sizes.append(c)
            rows += [(base, c0, c1, ln, 1, 1, 0) for ln in lengths[:c]]
    return Corpus("bin_staircase-k%d-top%d-%s" % (k, top, lane63), k, key_table(rows), STAIR_MIN_COVERAGE, n1=n1, bins=sorted(sizes),
                  ctx_sizes=sorted(ctx_sizes))


def coverage_pools(k, negative=False):
    """The largest pooled weight is reached only by pooling a flank value that is ctx0 in some records and ctx1 in others: X is
    ctx0 of records that weigh 7 and ctx1 of records that weigh 6 (13 pooled), Y is ctx0 alone of records that weigh 10.  From
    k = 16 on half of X's records carry X with a bit at or above 31 set (X', X''): only the 31-bit cut pools them.  The flank
    values 0 (beside C tracts) and 0x7FFFFFFF (cut to 2k bits) are there with small weights.  negative: one record of 2^19
    reads (-524288) on a flank of its own and on Y, whose pool goes negative."""
    kb = 2 * k
    full = (1 << kb) - 1
    X = 0x2D2D2D2D2D2D2D2D & full & 0x7FFFFFFF
    Y = 0x1B1B1B1B1B1B1B1B & full & 0x7FFFFFFF
    Z = 0x3636363636363636 & full & 0x7FFFFFFF
    hi = [0, 0, 0] if kb <= 31 else [0, 1 << 31, 1 << (kb - 1)]
    ok = lambda b, c0, c1: bool(valid_key(k, b, c0, c1))
    base_l = lambda c: 0 if ((c >> (kb - 2)) & 3) != 0 else 1            # a base that differs from the flank's byte next to the tract
    rows = []

    def add(c0, c1, n, ln=4):
        b = [b for b in (0, 1) if ok(b, c0, c1)][0]
        rows.append((b, c0, c1, ln, n - n // 2, n // 2, 0))
    f7 = 0x7FFFFFFF & full
    o1, o2, o3, o4 = (0x0123456789ABCDEF & full) | 2, (0x0FEDCBA987654321 & full) | 2, (0x05A5A5A5A5A5A5A5 & full) | 2, (0x0C3C3C3C3C3C3C3C & full) | 2
    add(X | hi[0], o1, 3)
    add(X | hi[1], o2, 2)
    add(X | hi[2], o3, 2)                    # X as ctx0: 7
    add(o1 | (1 << (kb - 1)), X | hi[0], 2)
    add(o2 | (1 << (kb - 1)), X | hi[1], 2)
    add(o3 | (1 << (kb - 1)), X | hi[2], 2)  # X as ctx1: 6
    add(Y, o4, 10)                           # Y as ctx0 alone: 10
    add(0, Z, 2)                             # flank value 0 on the left (C tract) ...
    add(Z | (1 << (kb - 1)), 0, 2, ln=5)     # ... and on the right
    add(f7 | ((1 << (kb - 1)) if kb <= 31 else 0), o4 ^ 0x30, 2)
    add(o4 | (1 << (kb - 1)), f7, 2, ln=6)
    if negative:
        add(Y, (o3 ^ 0xC0) | 2, 1 << 19, ln=7)
    keys = key_table(rows)
    assert len({(r[0], r[1], r[2], r[3]) for r in rows}) == len(rows) and base_l(0) == 1
    return Corpus("coverage_pools-k%d%s" % (k, "-neg" if negative else ""), k, keys, 5, X=X, cut_matters=kb > 31, negative=negative)


# ---- the list -------------------------------------------------------------------------------------------------------------

def corpus_makers():
    """name -> function that makes the corpus (made when asked for: the big ones take a second)"""
    mk = {}

    def reg(name, fn):
        assert name not in mk

        def make():
            c = fn()
            c.name = name
            return c
        mk[name] = make
    for k in (2, 12):
        reg("zero_key-k%d" % k, lambda k=k: zero_key(k))
    for k in sorted(set(K_OF_W.values()) | set(K_BORDERS)):
        reg("extreme_flanks-k%d" % k, lambda k=k: extreme_flanks(k))
    for k in (2, 13, 29):
        reg("count_edges-k%d" % k, lambda k=k: count_edges(k))
    for w, k in K_OF_W.items():
        for i, d in enumerate(ONE_BUCKET_D):
            bucket, others = (0, 255, 131)[i % 3], bool(i & 1)
            reg("one_bucket-k%d-%s" % (k, d), lambda k=k, d=d, b=bucket, o=others: one_bucket_keys(k, d, b, o))
        reg("one_bucket-k%d-2MAX+1-b131-filled" % k, lambda k=k: one_bucket_keys(k, "2MAX+1", 131, True))
        reg("one_bucket-k%d-CLOSE_AT+1-b255-filled" % k, lambda k=k: one_bucket_keys(k, "CLOSE_AT+1", 255, True))
        for name in BUCKET_SIZES:
            reg("bucket_sizes-k%d-%s" % (k, name), lambda k=k, name=name: bucket_sizes(k, name))
        for n in (20000, 20001):
            reg("kept_exactly_full-k%d-n%d" % (k, n), lambda k=k, n=n: kept_exactly_full(k, n))
        for top, lane63 in ((256, "alone"), (256, "ends"), (256, "whole"), (257, "alone")):
            reg("bin_staircase-k%d-top%d-%s" % (k, top, lane63), lambda k=k, top=top, lane63=lane63: bin_staircase(k, top, lane63))
    reg("long_bucket-k%d" % LONG_BUCKET_K, long_bucket)
    for k, n1 in KEPT_COUNTS:
        reg("kept_counts-k%d-n%d" % (k, n1), lambda k=k, n1=n1: kept_counts(n1, k))
    for k in (10, 16, 17, 32):
        reg("coverage_pools-k%d" % k, lambda k=k: coverage_pools(k))
    reg("coverage_pools-k16-neg", lambda: coverage_pools(16, True))
    return mk


DEVICE_EXCLUDED = ("zero_key-k2", "zero_key-k12")

BIG = ("count_edges-", "long_bucket-", "coverage_pools-k16-neg")       # corpora of tens of megabytes


def is_big(name):
    return name.startswith(BIG)


def oracle_from_raw(k, elems):
    """an oracle counter that holds these raw elements (as if it had scanned them): one scan serves several finalises"""
    import ctypes as C
    from oracle import orc
    o = orc.Oracle(k)
    e = np.ascontiguousarray(elems, dtype=orc.ELEM_DTYPE)
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    p = libc.malloc(max(e.nbytes, 40))
    C.memmove(p, e.ctypes.data, e.nbytes)
    libc.free(o.c.elem)
    o.c.elem, o.c.n_elem, o.c.n_alloc = p, len(e), max(len(e), 1)
    return o


# ---- corpora and the oracle's answers, made once and shared by the tests ---------------------------------------------------

_MAKERS, _CORPORA, _PARTS, _REF = None, {}, {}, {}


def names():
    global _MAKERS
    if _MAKERS is None:
        _MAKERS = corpus_makers()
    return list(_MAKERS)


def get(name):
    names()
    if name not in _CORPORA:
        _CORPORA[name] = _MAKERS[name]()
    return _CORPORA[name]


def parts_of(name):
    """the corpus's stream parts; of the big corpora only the last one asked for is kept"""
    if name not in _PARTS:
        for other in [n for n in _PARTS if is_big(n)]:
            del _PARTS[other]
        _PARTS[name] = [np.ascontiguousarray(p) for p in get(name).parts()]
    return _PARTS[name]


def filters_of(c):
    """(remove_biased, min_coverage): both filters, no threshold and the corpus's own"""
    return [(0, 0), (1, 0), (0, c.min_coverage), (1, c.min_coverage)]


def reference(name, filters=None):
    """the oracle on a corpus: {"n_raw", "raw" (elements as scanned; None once a big corpus was released), "fin": {filter:
    status, n, kept bytes, idx, n_idx, coverage}, "n1": {remove_biased: kept records before the context index, None if unknown}}"""
    from oracle import orc
    c = get(name)
    filters = filters_of(c) if filters is None else filters
    ref = _REF.get(name)
    if ref is None or (ref["raw"] is None and any(f not in ref["fin"] for f in filters)):
        o = orc.Oracle(c.k)
        for p in parts_of(name):
            o.scan_stream(p, M)
        raw = o.elems()
        o.close()
        if ref is None:
            ref = _REF[name] = {"n_raw": len(raw), "fin": {}, "n1": {}}
        ref["raw"] = raw
    for f in filters:
        if f not in ref["fin"]:
            o = oracle_from_raw(c.k, ref["raw"])
            o.finalise(*f)
            st = int(o.c.status)
            ref["fin"][f] = {"status": st, "n": int(o.c.n_elem), "kept": o.elems().tobytes() if st == 0 else b"", "idx": o.idx() if st == 0 else None,
                             "n_idx": int(o.c.n_idx) if st == 0 else 0, "coverage": int(o.c.coverage) if st == 0 else 0}
            o.close()
    for rb in (0, 1):
        f = ref["fin"].get((rb, 0))
        if f is not None:
            ref["n1"][rb] = f["n"] if f["status"] == 0 else (0 if f["status"] == 2 else None)
    return ref


def release(name):
    """forget what is large about a big corpus (its stream and raw elements); the oracle's answers stay"""
    if is_big(name):
        _PARTS.pop(name, None)
        if name in _REF:
            _REF[name]["raw"] = None
