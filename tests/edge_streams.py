"""Edge corpus for the scan kernels: deterministic, seeded generators of read streams (uint8 arrays of '\\n'-terminated
reads), each built to put tracts, delimiters or record counts exactly where a kernel's arithmetic changes.  No GPU is
needed to build them; tests/test_edge_streams.py checks on the CPU that each stream is what its docstring says, and
tests/test_scan_variants.py runs them through every scan / sink variant against the oracle.  Test infrastructure.

The constants below restate tatajuba_amd/csrc/hopo_device.hip; tests/test_edge_streams.py parses the #define lines and
fails when one of them moves."""
import random

import numpy as np

# ---- the kernels' geometry (hopo_device.hip) ------------------------------------------------------------------------
FK_BLOCK = 512                       # lanes of a fast-kernel workgroup
FK_UNIT = 32                         # stream bytes per lane
FK_HL = 32                           # left halo of a fast tile
FK_HR = 64                           # right halo of a fast tile
FK_WIN = FK_BLOCK * FK_UNIT          # 16384: window of a fast tile
FK_OWN = FK_WIN - FK_HL - FK_HR      # 16288: tract starts a fast tile owns
FK_MAXCAND = 4096                    # candidates a fast tile can list; more: the tile goes to the generic kernel
TJ_HR = 192                          # right halo of the generic kernel's and the located scan's tiles
TJ_SB_TILE = 8192                    # tile of the generic kernel (scan_bins_kernel)
LOC_TILE = 4096                      # tile of the located scan (scan_list_kernel / tjamd_scan_host_located)
TJ_LOGB_SHIFT = 13                   # a log block is 2^13 words: 8192 one-word or 4096 two-word records
TJ_CH0 = 1536                        # bucket chunks are TJ_CH0 << shift records, shift >= 3
TJ_FIX_CAP = 1 << 20                 # entries of the fix list (countable runs of non-ACGTU bytes per batch)

MIN_CHUNK = TJ_CH0 << 3              # 12288 records: the smallest chunk
SEAM_TILES = {FK_OWN: FK_HR, TJ_SB_TILE: TJ_HR, LOC_TILE: TJ_HR}   # tile size -> right halo of the kernel that uses it
SEAM_KINDS = ("plain", "delim", "nocall")
DELIM_OFFSETS = ("p-k-1", "p-k", "p-1", "e+k-1", "e+k", "e+k+1")       # p: the tract's first byte, e: its last
NOCALL_BYTES = b"NnUR"

_ACGT = np.frombuffer(b"ACGT", np.uint8)
NL = 10


def record_width(k):
    """words per raw record (tjamd_counter_create)"""
    return 1 if k <= 12 else 2 if k <= 28 else 4


def log_block_records(k):
    """RB of LogSink: records per log block; four-word records never go through the log, they get the two-word figure"""
    return (1 << TJ_LOGB_SHIFT) >> (0 if record_width(k) == 1 else 1)


def mprime(m):
    return max(m, 2)


# ---- seams --------------------------------------------------------------------------------------------------------

def seam_lengths(m):
    mp = mprime(m)
    out = []
    for n in (mp - 1, mp, mp + 1, 31, 32, 33, 63, 64, 65, 96, 97, 1023, 1024, 1025, FK_OWN + 5):
        if n >= 1 and n not in out:
            out.append(n)
    return out


def seam_offsets(tile, k, length):
    """tract starts relative to a seam: the five fixed ones, then the ones that put the tract's end (e) and its right flank's
    end (e + k) on the last own byte, and e + k on the last byte of the window (WIN - 1), one past it and two past it"""
    hr = SEAM_TILES[tile]
    out = []
    for d in (-k - 1, -k, -1, 0, 1, -length, -length - k, hr - k - length, hr - k - length + 1, hr - k - length + 2):
        if d not in out:
            out.append(d)
    return out


def delim_pos(name, p, e, k):
    return {"p-k-1": p - k - 1, "p-k": p - k, "p-1": p - 1, "e+k-1": e + k - 1, "e+k": e + k, "e+k+1": e + k + 1}[name]


def seam_plan(tile, k, m, kind="plain"):
    """([(seam index t, d, length, byte, extra)], tiles in all): what seam_stream lays down, one tract per seam t * tile.
    extra: None (plain); a name of DELIM_OFFSETS (delim); (byte, where) for nocall, where in ("tract", "left", "right")."""
    plan = []
    t, i, free_from = 1, 0, 0
    for il, length in enumerate(seam_lengths(m)):
        for jd, d in enumerate(seam_offsets(tile, k, length)):
            t = max(t + 1, -((d - k - 8 - free_from) // tile))           # the first seam whose tract starts clear of the one before
            byte = int(_ACGT[i & 3])
            extra = None
            if kind == "delim":
                extra = DELIM_OFFSETS[(il + jd) % 6]                     # every offset meets every delimiter place over the lengths
            elif kind == "nocall":
                extra = (int(NOCALL_BYTES[(il + jd) & 3]), ("tract", "left", "right")[((il + jd) >> 2) % 3])
            plan.append((t, d, length, byte, extra))
            free_from = t * tile + d + length + k + 8 + SEAM_TILES[tile]  # a long tract takes the seams it runs over
            i += 1
    return plan, -(-free_from // tile) + 1


def seam_stream(tile, k, m, kind="plain", seed=1):
    """Tracts on tile seams.  Background: random ACGT reads of 150 bytes.  For every (d, length) of seam_offsets x
    seam_lengths one tract of exactly `length` bytes starts at t * tile + d on a seam t of its own, its flanks free of
    delimiters (so it is recorded unless the variant says otherwise):
      plain   nothing else
      delim   one read delimiter at start - k - 1, start - k or start - 1 (the left flank is, just is not, is not inside
              the read) or at end + k - 1, end + k, end + k + 1 (the right flank is not, is not, just is), in rotation
      nocall  the tract's byte, or one byte of its left or right flank, is N, n, U or R in rotation: runs for the fix list
              whose stale context is a tract of an earlier tile, flanks that hold a byte outside ACGT
    tile in SEAM_TILES: FK_OWN (fast kernel), TJ_SB_TILE (generic kernel), LOC_TILE (located scan)."""
    assert tile in SEAM_TILES and kind in SEAM_KINDS
    plan, n_tiles = seam_plan(tile, k, m, kind)
    rng = np.random.default_rng([seed, tile, k, m, SEAM_KINDS.index(kind)])
    n = n_tiles * tile
    s = _ACGT[rng.integers(0, 4, n)]
    s[150::151] = NL
    for (t, d, length, byte, extra) in plan:
        p = t * tile + d
        e = p + length - 1
        lo, hi = p - k - 3, e + k + 4
        fl = _ACGT[rng.integers(0, 4, hi - lo)]
        s[lo:hi] = fl                                                     # no delimiter near the tract
        s[p:e + 1] = byte
        other = [c for c in _ACGT if c != byte]
        s[p - 1] = other[int(rng.integers(0, 3))]                         # exactly `length` bytes
        s[e + 1] = other[int(rng.integers(0, 3))]
        if kind == "delim":
            s[delim_pos(extra, p, e, k)] = NL
        elif kind == "nocall":
            b, where = extra
            if where == "tract":
                s[p:e + 1] = b
            elif where == "left":
                s[p - 1 - (k // 2)] = b
            else:
                s[e + 1 + (k // 2)] = b
    s[-1] = NL
    return s


def cut_reads(stream):
    """the reads of a stream (bytes objects) and the stream position of each one's first byte"""
    b = stream.tobytes()
    reads = b.split(b"\n")
    if reads and reads[-1] == b"":
        reads.pop()
    starts = np.cumsum([0] + [len(r) + 1 for r in reads])[:len(reads)]
    return reads, starts


# ---- dense streams: the candidate limit, the record log's block ring ----------------------------------------------------

def _template_quads(n_quads, seed):
    """XXyz quadruples, X != y != z != next X: one run of two (a candidate for m' = 2) every four bytes and no other run"""
    rng = np.random.default_rng([seed, n_quads])
    q = np.zeros((n_quads, 4), np.uint8)
    x = rng.integers(0, 4, n_quads)
    y = (x + rng.integers(1, 4, n_quads)) & 3
    xn = np.roll(x, -1)
    z = np.zeros(n_quads, np.int64)
    for i in range(n_quads):                                              # z differs from y and from the next X
        c = [v for v in range(4) if v != y[i] and v != xn[i]]
        z[i] = c[int(rng.integers(0, len(c)))]
    q[:, 0] = q[:, 1] = _ACGT[x]
    q[:, 2] = _ACGT[y]
    q[:, 3] = _ACGT[z]
    return q


CAND_RANGE = tuple(range(FK_MAXCAND - 12, FK_MAXCAND + 5))


def candidate_limit_stream(seed=3, reps=2):
    """Minimum tract size 2.  A read of len(CAND_RANGE) * reps fast tiles, then its reverse complement.  Every tile is the same template of FK_OWN / 4 =
    4072 XXyz quadruples (one candidate each: a short template repeated, so that a finalise keeps its records) in which
    the first e quadruples of a fixed list are turned into XXyy (two candidates): tile j holds exactly
    CAND_RANGE[j % 17] = FK_MAXCAND - 12 ... FK_MAXCAND + 4 run starts of >= 2 bytes in its own region."""
    nq = FK_OWN // 4
    q = _template_quads(nq, seed)
    x_next = np.roll(q[:, 0], -1)
    ok = np.nonzero(q[:, 2] != x_next)[0]                                 # XXyy then still differs from the next X
    ok = ok[(ok > 40) & (ok < nq - 40)]
    spots = ok[:: max(1, len(ok) // (CAND_RANGE[-1] - nq))][: CAND_RANGE[-1] - nq]
    assert len(spots) == CAND_RANGE[-1] - nq
    tiles = []
    for j in range(len(CAND_RANGE) * reps):
        t = q.copy()
        e = CAND_RANGE[j % len(CAND_RANGE)] - nq
        t[spots[:e], 3] = t[spots[:e], 2]
        tiles.append(t.reshape(-1))
    fwd = np.concatenate(tiles)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    # a second read, the reverse complement of the first: every tract on both strands (a finalise that removes one-strand
    # tracts keeps them); its tiles are a byte out of step with the quadruples and hold FK_OWN / 4 +- 1 more candidates
    return np.concatenate([fwd, [NL], comp[fwd[::-1]], [NL]]).astype(np.uint8)


def count_candidates(stream, m, tile=FK_OWN):
    """numpy restatement: per tile, the run starts in the tile's own region [t * tile, (t + 1) * tile) that sit on a letter
    (A C G T, upper case) and begin a run of at least m' equal bytes"""
    mp = mprime(m)
    s = np.asarray(stream)
    n = s.size
    start = np.ones(n, bool)
    start[1:] = s[1:] != s[:-1]
    pos = np.nonzero(start)[0]
    runlen = np.diff(np.append(pos, n))
    letter = np.isin(s[pos], _ACGT)
    sel = pos[(runlen >= mp) & letter]
    return np.bincount(sel // tile, minlength=(n + tile - 1) // tile)


def count_records_acgt(stream, k, m):
    """numpy restatement of the record count of a stream that holds A C G T and delimiters only: runs of >= m' equal letters
    with k bytes of their read on either side"""
    mp = mprime(m)
    s = np.asarray(stream)
    n = s.size
    start = np.ones(n, bool)
    start[1:] = s[1:] != s[:-1]
    pos = np.nonzero(start)[0]
    runlen = np.diff(np.append(pos, n))
    nl = np.nonzero(s == NL)[0]
    prev_nl = np.concatenate([[-1], nl])[np.searchsorted(nl, pos, side="left")]       # delimiter before the run
    next_nl = np.append(nl, n)[np.searchsorted(nl, pos, side="left")]                 # delimiter behind it
    end = pos + runlen - 1
    ok = (s[pos] != NL) & (runlen >= mp) & (pos - prev_nl - 1 >= k) & (next_nl - end - 1 >= k)
    return int(ok.sum())


LOG_RING_J = (1, 2, 4, 5, 9)


def log_ring_stream(k, j, delta, seed=5):
    """Minimum tract size 2.  One read of XXyz quadruples (a record every four bytes but for the k bytes at either end) whose
    record count is exactly j * RB + delta, RB = log_block_records(k): with one scanning workgroup (TATAJUBA_AMD_SCAN_GRID=1)
    the record log's blocks fill to RB - 1, RB, RB + 1 records j times over, and from j = 5 on the four-slot ring wraps.
    The quadruples repeat a template of 64 (a finalise keeps them)."""
    target = j * log_block_records(k) + delta
    tpl = _template_quads(64, seed)
    nq = target + 40
    body = np.tile(tpl, ((nq + 63) // 64, 1))[:nq].reshape(-1)
    s = np.append(body, NL).astype(np.uint8)
    have = count_records_acgt(s, k, 2)
    nq -= have - target                                                   # every quadruple away from the ends is one record
    s = np.append(body[: 4 * nq], NL).astype(np.uint8)
    assert count_records_acgt(s, k, 2) == target
    return s


def sparse_stream(k, n_records=7, n_tiles=60):
    """n_tiles fast tiles of run-free reads (ACGT repeated, 150 bytes) with n_records tracts of five bytes in all: fewer records
    than scanning workgroups, so every log block is empty or nearly so"""
    n = n_tiles * FK_OWN
    s = np.tile(_ACGT, n // 4 + 1)[:n].copy()
    s[150::151] = NL
    for i in range(n_records):
        p = ((i * n_tiles // n_records) * FK_OWN // 151 + 20) * 151 + 60  # 60 bytes into a read of 150
        s[p:p + 5] = _ACGT[i & 3]
        s[p - 1] = [c for c in _ACGT if c != s[p] and c != s[p - 2]][0]   # five bytes exactly, no new run beside them
        s[p + 5] = [c for c in _ACGT if c != s[p] and c != s[p + 6]][0]
    s[-1] = NL
    return s


def delimiters_only_stream(n=50000):
    return np.full(n, NL, np.uint8)


# ---- one bucket -------------------------------------------------------------------------------------------------------

def _runfree(rng, n, first_not=None):
    out = []
    prev = first_not
    for _ in range(n):
        c = rng.choice([x for x in b"ACGT" if x != prev])
        out.append(c)
        prev = c
    return bytes(out)


def one_bucket_stream(k, n_keys=1, seed=7):
    """One read pair -- a 33-byte tract between run-free flanks of k bytes, and its reverse complement: one key, seen on both
    strands -- repeated until the key holds more than three of the smallest chunks (3 * MIN_CHUNK + 1200 records): every
    record goes to one hash bucket, whose runs cross chunk boundaries in the scan's sink and in partition_log_kernel.
    n_keys = 2: two such pairs alternating, the same number of records for each."""
    rng = random.Random(seed * 100 + k)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    pairs = []
    for i in range(n_keys):
        base = b"ACGT"[(k + i) & 3]
        left = _runfree(rng, k)
        while left[-1] == base:
            left = _runfree(rng, k)
        right = _runfree(rng, k, first_not=base)
        fwd = left + bytes([base]) * 33 + right
        pairs.append(fwd + b"\n" + fwd.translate(comp)[::-1] + b"\n")
    n_pairs = (3 * MIN_CHUNK + 1200) // 2
    return np.frombuffer(b"".join(pairs) * n_pairs, np.uint8)


# ---- fix list ---------------------------------------------------------------------------------------------------------

FIX_UNIT = b"CGTTTACGNNCA"        # one tract (TTT) and one countable run of a non-ACGTU byte (NN) per 12 bytes, nothing else for m' = 2
FIX_UNIT_CLEAN = b"CGTTTACGATCA"  # the same without the run (and without a new one)
FIX_PAD = b"ACGT" * 8             # 32 bytes in front of the units: every NN has both flanks inside the read for any k
FIX_TAIL = b"CGTA" * 8            # and 32 behind them (no run with the last unit's A)


def fix_list_stream(n_runs, clean=False):
    """Minimum tract size 2 (or 1).  One read, one batch: n_runs units of 12 bytes, each with one countable run of 'N' whose two
    flanks lie inside the read (an entry of the fix list; its stale context is the TTT five bytes before it).
    n_runs = TJ_FIX_CAP - 1, TJ_FIX_CAP: the list just holds them; TJ_FIX_CAP + 1: the scan must fail.  clean: 'NN' replaced
    by 'AT' -- the same tracts without the runs, to count the runs by difference."""
    unit = FIX_UNIT_CLEAN if clean else FIX_UNIT
    return np.frombuffer(FIX_PAD + unit * n_runs + FIX_TAIL + b"\n", np.uint8)


# ---- seeded fuzz (the generator of tools/fuzz_gpu.py) -------------------------------------------------------------------

def random_stream(rng, synth_stream):
    """One random stream and the name of its kind.  rng: random.Random; synth_stream: tatajuba_amd.synth_stream (passed in: this
    module needs no built library)."""
    mode = rng.choice(["synth", "synth", "synth_ragged", "alphabet", "lowcomplex"])
    if mode == "synth":
        n = rng.choice([50, 2000, 30000, 150000, 400000])
        L = rng.choice([36, 75, 150, 250])
        g = rng.choice([2000, 50000, 1000000, 20000000])
        return synth_stream(n, L, g, seed_reads=rng.randrange(1 << 30), variant_seed=rng.randrange(8)), mode
    if mode == "synth_ragged":
        n = rng.choice([200, 3000, 20000])
        return synth_stream(n, 100, rng.choice([50000, 3000000]), seed_reads=rng.randrange(1 << 30),
                            read_len_max=rng.choice([400, 3000, 20000])), mode
    if mode == "alphabet":
        ab = rng.choice(["ACGT", "ACGTN", "ACGTacgtUN-", "AT", "ACGTNNNN"])
        reads = []
        for _ in range(rng.choice([10, 300, 3000])):
            L = rng.randint(0, 400)
            s = []
            while len(s) < L:
                s.extend(rng.choice(ab) * rng.choice([1, 1, 1, 2, 3, 4, 6, 12, 70]))
            reads.append("".join(s[:L]))
        return np.frombuffer(("\n".join(reads) + "\n").encode("latin-1"), np.uint8), mode
    # low complexity: few distinct contexts, huge counts, long tracts (length wrap), skewed buckets
    unit = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 9)))
    reads = []
    for _ in range(rng.choice([100, 5000, 60000])):
        t = rng.choice("ACGT") * rng.choice([3, 5, 9, 30, 600, 1100])
        reads.append((unit * 12)[: rng.randint(5, 60)] + t + (unit * 12)[: rng.randint(5, 60)])
    return np.frombuffer(("\n".join(reads) + "\n").encode(), np.uint8), mode
