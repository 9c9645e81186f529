"""Edge corpus for the tract statistics: tjamd_tract_stats / tjamd_tract_sample_stats (N5) and tjamd_union_tract_stats /
tjamd_union_tract_sample_stats (N6).  Deterministic builders of hand-made unions, aimed at the decision thresholds of the
two rules (variable: the sum of three relative differences above 1e-5; selected: one of the three above 1e-6), at the
bar slots of N6 (UT_SLOTS lengths per lane in LDS, then the FULL kernel with UT_LENGTHS global slots per thread in
UT_FULL_BLOCKS blocks), at sums beyond 32 bits, at the order of tied bars and at a coverage of 0.  No GPU and no built
device library are needed to make them; tests/test_stat_edges.py shows on the CPU, from the numpy restatements of
tests/test_tract_stats_cabi.py and tests/test_union_tracts_cabi.py, that each union is what its docstring says, and
tests/test_tract_stat_edges.py runs them through the four device entries.  Test infrastructure.

Every builder returns an Edge: (keys, mat, coverage, tract_ids, lev_distance, tracts, names).  keys uint64 [n, 3] of
record (), mat int32 [n, n_samples], coverage a list, tract_ids one id per row, lev_distance one per tract (set by hand:
the grouping is not under test), tracts the same tiling as UNION_TRACT_DTYPE, names one word per tract that says what it
is there for.  Rows are in the order of the merge: tracts by descending left flank, a tract's contexts by descending right
flank, a context's rows by descending length.

The three constants restate tatajuba_amd/csrc/hopo_device.hip; tests/test_stat_edges.py parses the #define lines and fails
when one moves."""
import collections
import functools

import numpy as np

import tatajuba_amd as tj
from tests.test_tract_stats_cabi import record

UT_SLOTS = 16                        # lengths a lane of union_sample_bars<false> keeps in LDS; the next one flags the tract
UT_LENGTHS = 1024                    # slots of a thread of the FULL kernels: index length + UT_LENGTHS / 2
UT_FULL_BLOCKS = 4                   # blocks of 256 threads of the FULL kernels
LEN_MIN, LEN_MAX = -(UT_LENGTHS // 2), UT_LENGTHS // 2 - 1        # the two ends of the slot index (a signed 10-bit length)
I32 = (1 << 31) - 1

Edge = collections.namedtuple("Edge", "keys mat coverage tract_ids lev_distance tracts names")


def segment(ns):
    """S of the statistics kernels: lanes per tract"""
    s = 1
    while s < ns and s < 64:
        s <<= 1
    return s


def full_pass(ns):
    """tracts that one pass of the FULL kernels' grid-stride loop holds"""
    return UT_FULL_BLOCKS * 256 // segment(ns)


def assemble(specs, coverage):
    """specs: [(name, lev_distance, [(context, length, [count per sample]), ...])], context a small index within the tract.
    Tract t has left flank 0xFFFFF - t, its context j right flank 0xFFFFF - j (base C): descending as the merge leaves them."""
    keys, mat, ids, lev, names, first, n_ctx = [], [], [], [], [], [], []
    for t, (name, lev_distance, rows) in enumerate(specs):
        assert rows and len({(j, ln) for j, ln, _ in rows}) == len(rows), name
        first.append(len(keys))
        for j, ln, cnt in sorted(rows, key=lambda r: (r[0], -r[1])):
            assert LEN_MIN <= ln <= LEN_MAX and all(0 <= x <= I32 for x in cnt), name
            keys.append(record(1, 0xFFFFF - t, 0xFFFFF - j, ln))
            mat.append(list(cnt))
            ids.append(t)
        lev.append(lev_distance)
        names.append(name)
        n_ctx.append(len({j for j, _, _ in rows}))
    keys, mat = np.array(keys, np.uint64).reshape(-1, 3), np.array(mat, np.int64)
    assert mat.ndim == 2 and mat.shape[1] == len(coverage)
    n = len(keys)
    tr = np.zeros(len(specs), tj.UNION_TRACT_DTYPE)
    tr["first"], tr["n_rows"] = first, np.diff(first + [n])
    tr["n_context"], tr["lev_distance"] = n_ctx, lev
    totals = mat.sum(axis=1)
    for t in range(len(specs)):
        lo, hi = int(tr["first"][t]), int(tr["first"][t] + tr["n_rows"][t])
        tr["mode"][t], tr["integral"][t] = lo + int(np.argmax(totals[lo:hi])), int(totals[lo:hi].sum())
    return Edge(keys, mat.astype(np.int32), [int(c) for c in coverage], np.array(ids, np.int32), np.array(lev, np.int32), tr, names)


# ---- A. thresholds ------------------------------------------------------------------------------------------------------
# name -> (bars of sample 0, bars of sample 1, what the rules say: selected, variable, and the terms above the 1e-6 of the
# selection).  Two samples, one context per tract: N5's bar per row is N6's bar per length.  Figures: the restatement's, as
# tests/test_stat_edges.py recomputes them (avg, modal, entropy: the three relative differences the rules read).
_N24, _N27, _M20, _N4M = 1 << 24, 1 << 27, 1 << 20, 4000000
SUM_ONLY_N = 104000000               # avg 1023 / N = 9.84e-6, modal 9.2e-17 + 1 / N, entropy 1.9e-7: sum 1.004e-5


def _two(l0, n, l1, a, b):
    return [(l0, n), (l1, a)], [(l0, n), (l1, b)]


def _three(m, d):
    return [(9, m), (8, m), (7, m)], [(9, m - d), (8, m + 2 * d), (7, m - d)]


THRESHOLDS = collections.OrderedDict([
    # entropy alone on either side of 1e-6: avg 1.2e-7, modal 1.2e-7 (6e-8), entropy 1.9e-6 (9.7e-7), sum 2.1e-6 (1.09e-6)
    ("entropy-selects", (_two(8, _N24, 7, 1, 3), dict(selected=1, variable=0, over=("entropy",)))),
    ("entropy-below", (_two(8, _N24, 7, 1, 2), dict(selected=0, variable=0, over=()))),
    # average length alone, across the whole slot index: avg 7.6e-6, modal 7.5e-9, entropy 1.4e-7
    ("avg-selects", (_two(LEN_MAX, _N27, LEN_MIN, 1, 2), dict(selected=1, variable=0, over=("avg",)))),
    # modal frequency alone: 2 d / (3 M) = 6.4e-7, 1.27e-6, 1.27e-5; avg exactly 0, entropy 1e-12, 4e-12, 4e-10
    ("modal-below", (_three(_M20, 1), dict(selected=0, variable=0, over=()))),
    ("modal-selects", (_three(_M20, 2), dict(selected=1, variable=0, over=("modal",)))),
    ("modal-variable", (_three(_M20, 20), dict(selected=1, variable=1, over=("modal",)))),
    # the sum rule of variable: 8.3e-6 and 1.9e-5, nearly all of it entropy
    ("sum-below", (_two(8, _N4M, 7, 1, 3), dict(selected=1, variable=0, over=("entropy",)))),
    ("sum-variable", (_two(8, _N4M, 7, 4, 9), dict(selected=1, variable=1, over=("avg", "modal", "entropy")))),
    # the sum above 1e-5 and every term below it
    ("sum-only", (_two(LEN_MAX, SUM_ONLY_N, LEN_MIN, 1, 2), dict(selected=1, variable=1, over=("avg",)))),
])
# the runs of the threshold union: (case of CASES, reference lengths of REFS)
THRESHOLD_RUNS = collections.OrderedDict([("plain", ("thresholds", None)), ("lev", ("thresholds-lev", None)),
                                          ("ref-modal", ("thresholds", "modal")), ("ref-off", ("thresholds", "off"))])


@functools.lru_cache(None)
def thresholds(variant="plain"):
    """The nine tracts of THRESHOLDS in one union of two samples.  variant "lev": lev_distance 1 on the tracts that nothing
    else selects.  ref_lengths () gives the reference lengths of "ref-modal" and "ref-off"; the union is the same."""
    assert variant in ("plain", "lev")
    specs = []
    for name, ((b0, b1), what) in THRESHOLDS.items():
        assert [ln for ln, _ in b0] == [ln for ln, _ in b1]
        lev = 1 if variant == "lev" and not what["selected"] else 0
        specs.append((name, lev, [(0, ln, [c0, c1]) for (ln, c0), (_, c1) in zip(b0, b1)]))
    return assemble(specs, [60, 45])


def ref_lengths(modal_len, off):
    """d_ref_length for a union whose restatement gave modal_len [n_tracts, n_samples]: sample 0's modal length, or off it
    by one (a tract whose samples disagree about the modal length is off the reference either way)"""
    return (np.asarray(modal_len)[:, 0] + (1 if off else 0)).astype(np.int32)


# ---- B. the slot edge ---------------------------------------------------------------------------------------------------
SLOT_NS = (1, 3, 64, 65, 130)


def wide_positions(ns):
    """where the sample with the most lengths sits: sample 0, the last one, every one; with 130 samples also 64 and 129,
    which lanes 0 and 1 reach on their second and third round"""
    pos = [("first", [0]), ("last", [ns - 1]), ("all", list(range(ns)))]
    if ns == 130:
        pos += [("round2", [64]), ("round3", [129])]
    return pos


def _count(t, r, s):
    """a count in 1..23 that differs between neighbours in every direction"""
    return 1 + (7 * r + 3 * s + 5 * t + (r * s) % 5) % 23


def _wide_rows(t, width, wide, ns, base_len=3):
    """one context, `width` lengths: the samples in `wide` have all of them, the others the first 1 to 3"""
    rows = []
    for r in range(width):
        cnt = [_count(t, r, s) if (s in wide or r < 1 + (s + t) % 3) else 0 for s in range(ns)]
        rows.append((0, base_len + r, cnt))
    return rows


def _small_rows(t, ns):
    return [(0, 5 + r, [_count(t, r, s) for s in range(ns)]) for r in range(1 + t % 3)]


@functools.lru_cache(None)
def slot_edge(ns):
    """Tracts whose widest sample has 15, 16 and 17 lengths (UT_SLOTS - 1, UT_SLOTS, UT_SLOTS + 1), at every position of
    wide_positions (ns), each followed by a tract of 1 to 3 lengths; a tract of two contexts with the same 16 lengths (32
    rows, 16 bars: it fits) and one of two contexts with 9 + 9 distinct lengths (18 bars: it does not).  Only the tracts
    named *-17-* and shared-9+9 overflow the LDS slots."""
    specs = []
    for width in (UT_SLOTS - 1, UT_SLOTS, UT_SLOTS + 1):
        for where, wide in wide_positions(ns):
            t = len(specs)
            specs.append((f"wide-{width}-{where}", 0, _wide_rows(t, width, set(wide), ns)))
            specs.append((f"small-{t + 1}", 0, _small_rows(t + 1, ns)))
    t = len(specs)
    specs.append(("shared-16+16", 1, [(j, 3 + r, [_count(t, r + j, s) for s in range(ns)]) for j in (0, 1) for r in range(UT_SLOTS)]))
    specs.append(("shared-9+9", 0, [(j, 3 + 9 * j + r, [_count(t + 1, r + j, s) for s in range(ns)]) for j in (0, 1) for r in range(9)]))
    return assemble(specs, [30 + 7 * (s % 11) for s in range(ns)])


# ---- C. the FULL pass ---------------------------------------------------------------------------------------------------
FULL_FLAGGED = {64: 40, 1: 1100}


@functools.lru_cache(None)
def full_pass_union(ns):
    """ns = 64: 40 tracts of 17 lengths (more than two passes of the 16 segments of the FULL kernels), each followed by a
    tract of 1 to 3 lengths.  ns = 1: 1100 tracts of 17 rows (more than one pass of 1024 segments), a small tract after
    every tenth.  Flagged tract 3 spans the slot index: its lengths are -512, 511 and fifteen between; the tract named
    ends-small holds only -512 and 511 and stays in LDS.  In the flagged tracts every third sample (every tract at ns = 1)
    has all 17 lengths."""
    assert ns in FULL_FLAGGED
    specs = []
    for f in range(FULL_FLAGGED[ns]):
        t = len(specs)
        wide = {s for s in range(ns) if (s + f) % 3 == 0} if ns > 1 else {0}
        rows = _wide_rows(t, UT_SLOTS + 1, wide, ns, base_len=4 + f % 200)
        name = f"flagged-{f}"
        if f == 3:
            lens = [LEN_MAX] + list(range(20, 5, -1)) + [LEN_MIN]
            rows = [(0, lens[r], cnt) for r, (_, _, cnt) in enumerate(rows)]
            name = "flagged-ends"
        specs.append((name, 0, rows))
        if ns > 1 or f % 10 == 9:
            specs.append((f"small-{t + 1}", 0, _small_rows(t + 1, ns)))
    t = len(specs)
    specs.append(("ends-small", 0, [(0, LEN_MAX, [_count(t, 0, s) for s in range(ns)]), (0, LEN_MIN, [_count(t, 1, s) for s in range(ns)])]))
    return assemble(specs, [40 + 3 * (s % 13) for s in range(ns)])


def listed(n_tracts, n_list):
    """a caller's list for the *_sample_stats entries: out of order, with repeats (n_list > n_tracts guarantees them, and
    the first entry comes back at the end), walking flagged and unflagged tracts alike"""
    lst = [(7 + 37 * i * i + 11 * i) % n_tracts for i in range(n_list - 1)]
    return np.array(lst + lst[:1], np.int32)


# ---- D. wide sums and ties ----------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def wide_sums_and_ties():
    """Three samples.
    big-two-contexts: rows of 2^31 - 1.  Two contexts carry length 511 with 2^31 - 1 each in sample 0, so N6's bar is
      2^32 - 2; with -512 beside it every sample's sum is above 2^32 and count * length needs 64 bits (1.1e12, 2.2e12).
    big-one-context: the same in one context (N5 with context-keyed ids sees it whole): sums of 3 (2^31 - 1).
    tie-16, tie-17: 16 and 17 bars of one count per sample (5, 7, 9): the modal length is the largest length, on the LDS
      path and on the FULL path.
    tie-pairs-17: 17 bars, counts tied in pairs and rising as the length falls: the insertion sort moves every bar.
    rising, falling: 12 distinct counts rising / falling as the length falls (the sort's worst and best case)."""
    B = I32
    specs = [
        ("big-two-contexts", 0, [(0, LEN_MAX, [B, B, 1]), (0, LEN_MIN, [B, 7, B]), (1, LEN_MAX, [B, B, B]), (1, 100, [0, B, B])]),
        ("big-one-context", 0, [(0, LEN_MAX, [B, B, B]), (0, 0, [B, B - 1, B]), (0, LEN_MIN, [B, B, 3])]),
        ("tie-16", 0, [(0, 40 - r, [5, 7, 9]) for r in range(UT_SLOTS)]),
        ("tie-17", 0, [(0, 40 - r, [5, 7, 9]) for r in range(UT_SLOTS + 1)]),
        ("tie-pairs-17", 0, [(0, 60 - r, [3 + r // 2, 4 + r // 2, 3 + (r + 1) // 2]) for r in range(UT_SLOTS + 1)]),
        ("rising", 0, [(0, 30 - r, [2 + r, 3 + 2 * r, 100 + r]) for r in range(12)]),
        ("falling", 0, [(0, 30 - r, [50 - r, 90 - 2 * r, 100 - r]) for r in range(12)]),
    ]
    return assemble(specs, [I32, 1000, 77])


# ---- E. a coverage of 0 -------------------------------------------------------------------------------------------------
ZERO_COVERAGE = {"one": (1,), "all": (0, 1, 2)}


@functools.lru_cache(None)
def zero_coverage(which):
    """slot_edge (3) with the coverage of sample 1, or of every sample, 0: the proportional coverage of a sample that has
    the tract is integral / 0.0 = inf there, and so is its relative difference (the largest minus the smallest, the
    smallest staying at FLT_MAX where every value is inf); the rules read neither, so variable and selected are those of
    slot_edge (3)."""
    e = slot_edge(3)
    return e._replace(coverage=[0 if s in ZERO_COVERAGE[which] else c for s, c in enumerate(e.coverage)])


# ---- the corpus by name, and its restatements (computed once, shared, read-only) ---------------------------------------
CASES = collections.OrderedDict(
    [("thresholds", lambda: thresholds("plain")), ("thresholds-lev", lambda: thresholds("lev"))]
    + [(f"slots-{ns}", functools.partial(slot_edge, ns)) for ns in SLOT_NS]
    + [(f"full-{ns}", functools.partial(full_pass_union, ns)) for ns in FULL_FLAGGED]
    + [("sums-ties", wide_sums_and_ties)]
    + [(f"cov0-{which}", functools.partial(zero_coverage, which)) for which in ZERO_COVERAGE])
REFS = (None, "modal", "off")        # no reference lengths; sample 0's modal lengths; those plus one


def case(name):
    return CASES[name]()


def _read_only(want):
    for v in want.values():
        v.setflags(write=False)
    return want


def reference_lengths(name, ref):
    """d_ref_length of case `name`: None, or ref_lengths of its own modal lengths"""
    return None if ref is None else ref_lengths(restated_union(name)["modal_len"], ref == "off")


@functools.lru_cache(None)
def restated_union(name, ref=None):
    """restate_union_tract_stats on a case, its tracts and lev_distance as given (N6)"""
    from tests.test_union_tracts_cabi import restate_union_tract_stats
    e = case(name)
    return _read_only(restate_union_tract_stats(e.keys, e.mat, e.coverage, e.tract_ids, e.lev_distance, ref_length=reference_lengths(name, ref)))


@functools.lru_cache(None)
def restated_tracts(name, ref=None, context_keyed=False):
    """restate_tract_stats on a case (N5: a bar per row), with the case's ids or the context-keyed ones"""
    from tests.test_tract_stats_cabi import restate_tract_stats
    e = case(name)
    return _read_only(restate_tract_stats(e.keys, e.mat, e.coverage, tract_ids=None if context_keyed else e.tract_ids,
                                          ref_length=reference_lengths(name, ref)))


# ---- both summation orders ----------------------------------------------------------------------------------------------

def row_order_sums(bars):
    """the average length and the entropy of one sample's bars [(length, count)] summed in the order given (N5 sums in
    union row order) -> (avg, entropy); tests/test_stat_edges.py holds it against the reference's order"""
    integral = sum(f for _, f in bars)
    avg = ent = 0.0
    for ln, f in bars:
        avg += float(np.float64(f * ln) / np.float64(integral))
        x = float(np.float64(f) / np.float64(integral))
        ent += x * float(np.log(np.float64(x)))
    return avg, -ent
