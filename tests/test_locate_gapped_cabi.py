"""The second pass of the lookup (include/tatajuba_locate.h: tjamd_flank_edit_distance, tjamd_reference_add_seeds,
tjamd_reference_has_seeds, tjamd_locate_gapped and their timers) without a GPU: the entries are declared in their own header,
exported and prototyped, refuse bad arguments before any pointer is read, the exported distance -- the arithmetic of the
lookup kernel -- equals a plain Python DP on random and planted pairs, and the brute-force restatement that the GPU tests
(tests/test_locate_gapped.py) compare against reproduces cases worked out by hand.

Written from the rule in the header, not from the device code:
  edit_distance_plain    D[i][j] over the cells with |i - j| <= B, the minimum over the last row and the last column
  edit_distance_many     the same for many candidates at once (numpy, one DP row at a time)
  restate_locate_gapped  base equal, one seed (inner h bases of a flank) equal, d_B + d_B <= max_edits; fewest edits, then smallest
                         flat; rows located on entry stay as they are"""
import ctypes as C
import fnmatch
import os
import random
import re

import numpy as np

import tatajuba_amd as tj
from tests.test_locate_cabi import NOWHERE, flank_distance, restate_locate
from tests.test_union_tracts_cabi import pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_flank_edit_distance", "tjamd_reference_add_seeds", "tjamd_reference_has_seeds", "tjamd_locate_gapped",
               "tjamd_last_seed_order_ms", "tjamd_last_locate_gapped_ms"]
ERR_ARG, ERR_CAP = 3, 4
INF = 1 << 20


# ---- the distance, restated --------------------------------------------------------------------------------------------

def inner_first(x, k, side):
    """the k bases of a packed flank, the one next to the tract first (side 0: ctx0, side 1: ctx1)"""
    x = int(x)
    return [(x >> (2 * (k - 1 - i) if side == 0 else 2 * i)) & 3 for i in range(k)]


def pack_inner_first(seq, side):
    k = len(seq)
    return sum(b << (2 * (k - 1 - i) if side == 0 else 2 * i) for i, b in enumerate(seq))


def edit_distance_plain(q, r, B):
    """d_B of two inner-first sequences of one length"""
    k = len(q)
    assert len(r) == k
    D = {(0, 0): 0}
    for i in range(1, min(k, B) + 1):
        D[(i, 0)] = i
        D[(0, i)] = i
    for i in range(1, k + 1):
        for j in range(max(1, i - B), min(k, i + B) + 1):
            D[(i, j)] = min(D.get((i - 1, j - 1), INF) + (q[i - 1] != r[j - 1]), D.get((i - 1, j), INF) + 1, D.get((i, j - 1), INF) + 1)
    return min(min(D[(k, j)] for j in range(max(0, k - B), k + 1)), min(D[(i, k)] for i in range(max(0, k - B), k + 1)))


def edit_distance_many(x, y, k, side, B):
    """d_B (x[c], y) for an array x of packed flanks and one packed flank y -> int64 [len (x)]"""
    x = np.asarray(x, dtype=np.uint64)
    n = len(x)
    shifts = [2 * (k - 1 - i) if side == 0 else 2 * i for i in range(k)]
    q = inner_first(y, k, side)
    r = np.stack([((x >> np.uint64(s)) & np.uint64(3)).astype(np.int64) for s in shifts], axis=1) if n else np.zeros((0, k), np.int64)
    prev = np.full((n, k + 1), INF, np.int64)
    prev[:, : min(k, B) + 1] = np.arange(min(k, B) + 1)
    col = prev[:, k].copy()
    for i in range(1, k + 1):
        cur = np.full((n, k + 1), INF, np.int64)
        if i <= B:
            cur[:, 0] = i
        for j in range(max(1, i - B), min(k, i + B) + 1):
            cur[:, j] = np.minimum(np.minimum(prev[:, j - 1] + (r[:, j - 1] != q[i - 1]), prev[:, j] + 1), cur[:, j - 1] + 1)
        if i >= k - B:
            col = np.minimum(col, cur[:, k])
        prev = cur
    return np.minimum(col, prev[:, max(0, k - B):].min(axis=1))


def restate_locate_gapped(entries, keys, loc, max_edits, max_shift, k):
    """-> (LOCATION_DTYPE [n], how int32 [n]): loc with its unlocated rows tried by the gapped rule"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    out, how = np.array(loc, dtype=tj.LOCATION_DTYPE), np.zeros(len(keys), np.int32)
    h = (k + 1) // 2
    top, low = np.uint64(2 * (k - h)), np.uint64((1 << (2 * h)) - 1)
    memo = {}
    inner0, inner1 = (entries["ctx0"] >> top, entries["ctx1"] & low) if len(entries) else (None, None)
    for row, (c0, c1, meta) in enumerate(keys.tolist()):
        if out["flat"][row] >= 0:
            continue
        ctx = (c0, c1, meta & 3)
        if ctx not in memo:
            res = None
            if len(entries):
                seed0, seed1 = inner0 == (np.uint64(c0) >> top), inner1 == (np.uint64(c1) & low)
                cand = np.flatnonzero((entries["base"] == (meta & 3)) & (seed0 | seed1))             # (both seeds: once)
                if len(cand):
                    d = edit_distance_many(entries["ctx0"][cand], c0, k, 0, max_shift) + edit_distance_many(entries["ctx1"][cand], c1, k, 1, max_shift)
                    hit, d = cand[d <= max_edits], d[d <= max_edits]
                    if len(hit):
                        best = np.lexsort((entries["flat"][hit], d))[0]                               # fewest edits, then leftmost
                        e = entries[hit[best]]
                        res = (int(e["flat"]), int(e["contig"]), int(e["pos"]), int(e["length"]), int(d[best]), int(e["neg_strand"]), len(hit))
            memo[ctx] = res
        how[row] = 1 if memo[ctx] is not None else -1
        if memo[ctx] is not None:
            out[row] = memo[ctx]
    return out, how


def seed_ranges(entries, keys, k):
    """entries that share (base, inner h bases of ctx0) / (base, inner h bases of ctx1) with each row -> two int arrays"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    h = (k + 1) // 2
    out = []
    for seeds, mine in ((entries["ctx0"] >> np.uint64(2 * (k - h)), keys[:, 0] >> np.uint64(2 * (k - h))),
                        (entries["ctx1"] & np.uint64((1 << (2 * h)) - 1), keys[:, 1] & np.uint64((1 << (2 * h)) - 1))):
        # (a seed has at most 32 bits: seed * 4 + base stays below 2^63)
        val, cnt = np.unique(seeds.astype(np.int64) * 4 + entries["base"], return_counts=True)
        size = dict(zip(val.tolist(), cnt.tolist()))
        out.append(np.array([size.get(int(s) * 4 + (int(m) & 3), 0) for s, m in zip(mine, keys[:, 2])], dtype=np.int64))
    return out


# ---- planted pairs -------------------------------------------------------------------------------------------------------

def planted_pair(rng, k):
    """-> (q, r, bound per B): r the first k bases of a random inner-first genome flank, q that flank after one substitution or
    an insertion or deletion of 1 ... 3 bases at a random position, cut back to k bases with the genome's next bases"""
    g = [rng.randrange(4) for _ in range(k + 3)]
    p, s = rng.randrange(k), rng.randrange(1, 4)
    kind = rng.choice(("sub", "ins", "del"))
    if kind == "sub":
        q = list(g)
        q[p] = (q[p] + rng.randrange(1, 4)) & 3
        return q[:k], g[:k], [1, 1, 1, 1]
    if kind == "ins":
        q = g[:p] + [rng.randrange(4) for _ in range(s)] + g[p:]
    else:
        q = g[:p] + g[p + s:]
    return q[:k], g[:k], [None if B < s else s for B in range(4)]


def hamming(q, r):
    return sum(a != b for a, b in zip(q, r))


def c_distance(q, r, side, B):
    return tj.lib().tjamd_flank_edit_distance(pack_inner_first(q, side), pack_inner_first(r, side), len(q), side, B)


# ---- declarations and argument checks ------------------------------------------------------------------------------------

def test_new_entries_are_declared_in_their_header_exported_and_prototyped():
    L = tj.lib()
    inc = os.path.join(ROOT, "include")
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, name)).read(), flags=re.S)
    own = strip("tatajuba_locate.h")
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.LOCATE_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)             # the header declares these and nothing else
    others = [f for f in sorted(os.listdir(inc)) if f.endswith(".h") and f != "tatajuba_locate.h"]
    assert "tatajuba_amd.h" in others
    for s in NEW_ENTRIES:
        for f in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(f)), (s, f)                               # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert "tatajuba_locate.h" in open(os.path.join(inc, "tatajuba_amd.h")).read()
    assert re.search(r"#define\s+TJAMD_MAX_SHIFT\s+3\b", own) and tj.MAX_SHIFT == 3
    assert L.tjamd_last_seed_order_ms(None) == -1.0 and L.tjamd_last_locate_gapped_ms(None) == -1.0
    assert L.tjamd_reference_has_seeds(None) == 0
    for name in ("locate_gapped", "last_seed_order_ms", "last_locate_gapped_ms"):
        assert hasattr(tj.Counter, name)
    assert hasattr(tj.Reference, "add_seeds") and hasattr(tj.Reference, "has_seeds") and callable(tj.flank_edit_distance)


def test_entries_check_their_arguments_without_a_gpu():
    """what can be refused without reading the counter or the reference is refused first, so the pointers below are never
    dereferenced; another k or device, a reference without seeds and max_edits above k need both objects (tests/test_locate_gapped.py)"""
    L = tj.lib()
    fake = C.c_void_p(0x1000)

    def call(c=fake, ref=fake, keys=fake, n=10, edits=1, shift=1, loc=fake, how=fake):
        rc = L.tjamd_locate_gapped(c, ref, keys, n, edits, shift, loc, how)
        return rc, L.tjamd_last_error().decode()

    for kw, rc, msg in [({"c": None}, ERR_ARG, "null counter or reference"), ({"ref": None}, ERR_ARG, "null counter or reference"),
                        ({"c": None, "n": 0}, ERR_ARG, "null counter or reference"),
                        ({"shift": -1}, ERR_ARG, "max_shift -1 outside 0..3"), ({"shift": 4}, ERR_ARG, "max_shift 4 outside 0..3"),
                        ({"edits": -1}, ERR_ARG, "max_edits -1 outside 0..k"),
                        ({"n": -1}, ERR_ARG, "n -1 < 0"), ({"n": 1 << 31}, ERR_CAP, "rows"),
                        ({"keys": None}, ERR_ARG, "null key or location buffer"), ({"loc": None}, ERR_ARG, "null key or location buffer"),
                        ({"keys": None, "n": 1, "how": None}, ERR_ARG, "null key or location buffer")]:
        got, err = call(**kw)
        assert got == -rc and err.startswith("tjamd_locate_gapped") and msg in err, (kw, got, err)
    assert L.tjamd_reference_add_seeds(None, fake) == -ERR_ARG and "tjamd_reference_add_seeds: null counter or reference" in L.tjamd_last_error().decode()
    assert L.tjamd_reference_add_seeds(fake, None) == -ERR_ARG and "null counter or reference" in L.tjamd_last_error().decode()
    for args, msg in (((1, 2, 0, 0, 1), "k 0 outside 1..32"), ((1, 2, 33, 0, 1), "k 33 outside 1..32"), ((1, 2, 5, 2, 1), "side 2 outside 0..1"),
                      ((1, 2, 5, -1, 1), "side -1 outside 0..1"), ((1, 2, 5, 0, 4), "max_shift 4 outside 0..3"), ((1, 2, 5, 0, -1), "max_shift -1 outside 0..3")):
        assert L.tjamd_flank_edit_distance(*args) == -ERR_ARG and msg in L.tjamd_last_error().decode(), args
    try:
        tj.flank_edit_distance(1, 2, 5, 0, 9)
        assert False
    except tj.TatajubaAmdError as e:
        assert "max_shift 9" in str(e)
    assert tj.flank_edit_distance(pack("ACGTA"), pack("ACGTC"), 5, 1, 2) == 1


# ---- the exported distance against the plain DP ----------------------------------------------------------------------------

def test_flank_edit_distance_equals_the_plain_dp():
    """2000 pairs per k, half random and half planted, both sides, every band: no difference"""
    rng = random.Random(2025)
    for k in (2, 5, 13, 25, 31, 32):
        kinds = set()
        for n in range(2000):
            if n % 2:
                q, r, bound = planted_pair(rng, k)
                kinds.add(tuple(bound))
            else:
                q, r, bound = [rng.randrange(4) for _ in range(k)], [rng.randrange(4) for _ in range(k)], [None] * 4
            ham = hamming(q, r)
            last = None
            for B in range(4):
                want = edit_distance_plain(q, r, B)
                for side in (0, 1):
                    assert c_distance(q, r, side, B) == want, (k, q, r, side, B, want)
                assert c_distance(r, q, 0, B) == want                                             # symmetric
                assert want <= ham and (last is None or want <= last)                             # never above d_0, not growing with B
                assert bound[B] is None or want <= bound[B], (k, q, r, B, want, bound)
                if B == 0:
                    assert want == ham
                last = want
        assert len(kinds) == 4                                                                    # a substitution, and 1, 2 and 3 bases


def test_d0_is_the_flank_distance_of_the_lookup_and_the_many_candidate_dp_agrees():
    rng = random.Random(5)
    for k in (2, 7, 16, 32):
        x = np.array([rng.getrandbits(2 * k) for _ in range(300)], dtype=np.uint64)
        y = rng.getrandbits(2 * k)
        x[::3] = [int(v) ^ (rng.randrange(1, 4) << (2 * rng.randrange(k))) for v in [y] * len(x[::3])]      # near ones too
        want0 = flank_distance(x, y)
        for side in (0, 1):
            got0 = [tj.flank_edit_distance(int(v), y, k, side, 0) for v in x]
            assert got0 == want0.tolist() and edit_distance_many(x, y, k, side, 0).tolist() == got0
            for B in (1, 2, 3):
                many = edit_distance_many(x, y, k, side, B).tolist()
                assert many == [edit_distance_plain(inner_first(v, k, side), inner_first(y, k, side), B) for v in x]
                assert many == [tj.flank_edit_distance(int(v), y, k, side, B) for v in x]
    assert len(edit_distance_many(x[:0], y, 32, 0, 3)) == 0
    # bits above 2k are not read
    assert tj.flank_edit_distance(pack("ACGTA") | (0xABC << 10), pack("ACGTA"), 5, 0, 3) == 0


def test_flank_edit_distance_on_hand_built_cases():
    code = {c: i for i, c in enumerate("ACGT")}
    seq = lambda s: [code[c] for c in s]
    # k = 5, the genome flank ACGTA (inner first), one base inserted at inner position 0, 2 and 4
    r = seq("ACGTA")
    for q, d0 in (("TACGT", 5), ("ACTGT", 3), ("ACGTC", 1)):
        for side in (0, 1):
            assert c_distance(seq(q), r, side, 0) == d0 == edit_distance_plain(seq(q), r, 0)
            for B in (1, 2, 3):
                assert c_distance(seq(q), r, side, B) == 1 == edit_distance_plain(seq(q), r, B)
    # one deleted base at inner position 1: CGTA + the genome's next base
    assert [c_distance(seq("AGTAC"), r, 1, B) for B in range(4)] == [4, 1, 1, 1]
    # the packings: side 0 holds the inner base at the high end, side 1 at bit 0
    assert pack_inner_first(seq("ACGTA"), 1) == pack("ACGTA") and pack_inner_first(seq("ACGTA"), 0) == pack("ATGCA")
    assert inner_first(pack("ATGCA"), 5, 0) == r == inner_first(pack("ACGTA"), 5, 1)
    # k = 32 with all bits set: shifts by 64 bits are not taken
    L = tj.lib()
    ones = (1 << 64) - 1
    for side in (0, 1):
        for B in range(4):
            assert L.tjamd_flank_edit_distance(ones, ones, 32, side, B) == 0
            assert L.tjamd_flank_edit_distance(ones, 0, 32, side, B) == 32
            assert L.tjamd_flank_edit_distance(ones, ones ^ 1, 32, side, B) == 1 and L.tjamd_flank_edit_distance(ones, ones ^ (1 << 63), 32, side, B) == 1
        # TTTT...T against the same flank with its inner base deleted and a G pulled in at the outer end: one edit at any band
        # above 0 on either side, one substitution at band 0
        shifted = pack_inner_first([3] * 31 + [2], side)
        assert [L.tjamd_flank_edit_distance(ones, shifted, 32, side, B) for B in range(4)] == [1, 1, 1, 1]
    # a 32-base flank of period 4 against itself shifted by one base: 32 substitutions, or one deletion
    a, b = seq("ACGT" * 8), seq("CGTA" * 8)
    assert [c_distance(a, b, 0, B) for B in range(4)] == [32, 1, 1, 1] == [edit_distance_plain(a, b, B) for B in range(4)]


# ---- the rule by hand: k = 8, h = 4 ------------------------------------------------------------------------------------------
#   the entry: left flank ACGTTGCA (its inner base is the last), right flank GATCCTAT (its inner base is the first), followed
#   in the genome by GC

K = 8
LEFT, RIGHT = "ACGTTGCA", "GATCCTAT"


def _entry(c0, c1, flat, base=0):
    return (pack(c0), pack(c1), flat, 0, flat, 5, base, 0, 0)


def _gapped(entries, keys, max_edits, max_shift):
    loc = restate_locate(entries, keys, 1)
    out, how = restate_locate_gapped(entries, keys, loc, max_edits, max_shift, K)
    return loc, [tuple(x.tolist()) for x in out], how.tolist()


def test_gapped_rule_on_hand_built_cases():
    entries = np.array([_entry(LEFT, RIGHT, 100)], dtype=tj.REF_ENTRY_DTYPE)
    keys = [[pack(LEFT), pack(RIGHT), 0],                       # exact: located by the first pass
            [pack("TCGTTGCA"), pack("GATCCTAC"), 0],            # one substitution in the outer half of each flank
            [pack(LEFT), pack("GATCATGC"), 0],                  # CT deleted from the outer half of ctx1, the genome's GC pulled in
            [pack("ACGTTGCT"), pack("CATCCTAT"), 0],            # a substitution in the inner half of both flanks
            [pack("TCGTTGCA"), pack("GATCCTAC"), 1]]            # another base
    loc, got, how = _gapped(entries, keys, 2, 2)
    assert [tuple(x.tolist()) for x in loc] == [(100, 0, 100, 5, 0, 0, 1), NOWHERE, NOWHERE, NOWHERE, NOWHERE]
    assert got == [(100, 0, 100, 5, 0, 0, 1), (100, 0, 100, 5, 2, 0, 1), (100, 0, 100, 5, 2, 0, 1), NOWHERE, NOWHERE] and how == [0, 1, 1, -1, -1]
    # (row 1 passes both seeds and is counted once)
    # at one edit neither is a hit; without a shift the deletion costs its three substitutions; a band of one base is too
    # narrow for two deleted bases
    assert _gapped(entries, keys, 1, 2)[1:] == ([(100, 0, 100, 5, 0, 0, 1)] + [NOWHERE] * 4, [0, -1, -1, -1, -1])
    assert _gapped(entries, keys, 2, 0)[1][1:3] == [(100, 0, 100, 5, 2, 0, 1), NOWHERE]
    assert _gapped(entries, keys, 2, 1)[1][2] == NOWHERE and _gapped(entries, keys, 3, 1)[1][2] == (100, 0, 100, 5, 3, 0, 1)
    # the seed is part of the rule: row 3 has two edits in all, and stays unlocated at any limit
    assert _gapped(entries, keys, 8, 3)[1][3] == NOWHERE and flank_distance([pack("ACGTTGCT")], pack(LEFT)).tolist() == [1]
    # a row located on entry stays as it is, whatever it holds
    mine = np.array([(7, 3, 7, 9, 5, 1, 4), NOWHERE], dtype=tj.LOCATION_DTYPE)
    out, how = restate_locate_gapped(entries, keys[:2], mine, 2, 2, K)
    assert [tuple(x.tolist()) for x in out] == [(7, 3, 7, 9, 5, 1, 4), (100, 0, 100, 5, 2, 0, 1)] and how.tolist() == [0, 1]
    # two entries tied on edits: the smaller flat; a closer one further right (ctx1 exact, the C next to the inner base of ctx0
    # deleted: six substitutions for the first pass, one edit here) beats both; each is counted once
    three = np.array([_entry("GCGTTGCA", RIGHT, 50), _entry(LEFT, "GATCCTAG", 100), _entry("ATCGTTGA", "GATCCTAC", 200)], dtype=tj.REF_ENTRY_DTYPE)
    q = [[pack("TCGTTGCA"), pack("GATCCTAC"), 0]]
    assert _gapped(three[:2], q, 2, 1)[1] == [(50, 0, 50, 5, 2, 0, 2)]
    assert _gapped(three[1:2], q, 2, 1)[1] == [(100, 0, 100, 5, 2, 0, 1)]
    loc, got, how = _gapped(three, q, 2, 1)
    assert tuple(loc[0].tolist()) == NOWHERE and got == [(200, 0, 200, 5, 1, 0, 3)] and how == [1]
    assert _gapped(three[:0], q, 2, 1)[1:] == ([NOWHERE], [-1])
    # an entry reached by the ctx1 seed alone
    one = np.array([_entry("ACGTTCCA", RIGHT, 30)], dtype=tj.REF_ENTRY_DTYPE)
    q = [[pack("TCGTTGCA"), pack(RIGHT), 0]]
    assert _gapped(one, q, 2, 0)[1] == [(30, 0, 30, 5, 2, 0, 1)] and seed_ranges(one, q, K)[0].tolist() == [0] and seed_ranges(one, q, K)[1].tolist() == [1]
