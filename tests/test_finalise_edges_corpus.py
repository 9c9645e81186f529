"""The finalise corpus (tests/finalise_edges.py) is what it claims to be -- shown on the CPU from the oracle, the kernel
source's #define lines and the module's own restatements.  tests/test_finalise_edges.py judges the device finalise on
these corpora; if one of them missed its edge, those tests would prove less than they say.  These are conditions, not
measurements: the inputs are chosen so that they hold."""
import numpy as np
import pytest

from oracle import orc
from tests import finalise_edges as F
from tests.edge_streams import TJ_CH0, record_width
from tests.test_edge_streams import _define, _source, _value

NAMES = F.names()
MIN_CHUNK = TJ_CH0 << 3


def of_kind(kind):
    return [n for n in NAMES if n.startswith(kind + "-")]


def test_constants_are_those_of_the_kernel_source():
    src = _source()
    for name in ("TJ_P", "AG_BLOCK", "AG_NCH", "AG1_S", "AG2_S", "AG4_S", "AG1_CLOSE_AT", "AG2_CLOSE_AT", "AG4_CLOSE_AT", "AG1_R", "AG2_R", "AG4_R",
                 "BS_RANK_MAX", "BS_MAXBITS", "R1_FLAG_SHIFT", "TJ_CH0"):
        assert _value(_define(src, name)) == getattr(F, name, None if name != "TJ_CH0" else TJ_CH0), name
    # a table closes ABOVE its CLOSE_AT, every lane looks before its claim, and a bin is sorted in LDS up to BS_RANK_MAX records
    for w in (1, 2, 4):
        assert "L.n_claimed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > AG%d_CLOSE_AT;" % w in src
    assert "fin->sort_fallback = vmax > rank_max ? 1u : 0u;" in src and "u32 bin_rank_max = BS_RANK_MAX;" in src
    assert "if (s <= 64u) {" in src
    assert F.chunk_records(0) == MIN_CHUNK == 12288 and F.chunk_records(8 * 16384 * TJ_CH0) == MIN_CHUNK and F.chunk_records(9 * 16384 * TJ_CH0) == 2 * MIN_CHUNK
    assert [F.max_admitted(w) for w in (1, 2, 4)] == [5889, 3585, 3585]


def test_restatements_on_known_values():
    assert int(F.udot4(0x01020304, 0x05060708, 7)) == 1 * 5 + 2 * 6 + 3 * 7 + 4 * 8 + 7
    assert int(F.udot4(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)) == (4 * 255 * 255 + 0xFFFFFFFF) & 0xFFFFFFFF
    lo, hi = F.pack_rec1(0xABCDEF, 0x123456, 1, 0x2A5, 2)
    assert (int(lo), int(hi)) == (0x123456 | (0xA5 << 24), 0xABCDEF | (2 << 24) | (1 << 26) | (2 << 27))
    assert [F.bin_bits_for(n, 10) for n in (1, 3072, 3073, 6144, 6145, 12288, 12289)] == [6, 6, 7, 7, 8, 8, 9]
    assert [F.bin_bits_for(n, 2) for n in (6144, 6145, 12288, 12289, 10 ** 6)] == [7, 8, 8, 9, 9] and F.fine_bin_bits(2) == 9 and F.fine_bin_bits(10) == 16
    assert [F.cov_plan_bits(n, 6) for n in (512, 513)] == [(11, False), (12, True)]
    assert [F.cov_plan_bits(n, 10) for n in (131072, 131073)] == [(19, False), (20, True)]
    assert F.cov_plan_bits(10 ** 6, 16) == (22, False)
    assert F.plan_cap(100) == 51 and F.plan_cap(10 ** 6) == 65536 and F.plan_cap(10 ** 7) == 625000
    # bins: the complemented leading bits of [base][ctx0][ctx1]
    assert int(F.bin_of_record(0, 0, 0, 10, 6)) == 63 and int(F.bin_of_record((1 << 20) - 1, 0, 1, 10, 6)) == 0
    assert int(F.bin_of_record(0b1011, 0b0111, 0, 2, 9)) == 511 - 0b010110111 and int(F.bin_of_record(0b1011, 0b0111, 1, 2, 7)) == 127 - 0b1101101
    # a read for a key, in the bit order of orc.name_of, gives that key back on either strand
    for k, base, c0, c1, n in [(2, 0, 0b0110, 0b1001, 5), (10, 1, 0x2B3C4, 0x9F0E3, 1024), (20, 0, (1 << 39) | 12345, 3, 2), (32, 1, (1 << 64) - 1, 2, 33)]:
        for rev in (False, True):
            o = orc.Oracle(k)
            o.scan_seq(F.read_for_key(k, base, c0, c1, n, reverse=rev), F.M)
            e = o.elems()
            o.close()
            assert len(e) == 1 and (int(e["ctx0"][0]), int(e["ctx1"][0])) == (c0, c1)
            d = orc.decode_meta(e["meta"])
            assert (int(d["base"][0]), int(d["length"][0]) & 0x3FF, int(d["canon_flag"][0])) == (base, n & 0x3FF, 2 if rev else 1)
            left, b, right = orc.name_of(c0, c1, base, k).split(".")
            assert F.read_for_key(k, base, c0, c1, n).decode() == left + b * n + right


# ---- every corpus: the oracle's raw elements are the intended keys, the restated buckets hold them ------------------------

def check_raw_is_the_key_table(name):
    c = F.get(name)
    ref = F.reference(name, [])
    t = c.keys
    assert len({(int(r["base"]), int(r["c0"]), int(r["c1"]), int(r["length"]) & 0x3FF) for r in t}) == len(t) - c.facts.get("aliases", 0), "keys are distinct (as stored)"
    assert F.valid_key(c.k, t["base"], t["c0"], t["c1"]).all() or t["nflank"].any()
    assert ref["n_raw"] == c.n_reads == int(F.bucket_counts(c.k, t).sum())
    c0, c1, meta, mult = F.expected_raw(c.k, t)
    raw = ref["raw"]
    got, gn = np.unique(F.mix3(raw["ctx0"], raw["ctx1"], raw["meta"]), return_counts=True)
    want, inv = np.unique(F.mix3(c0, c1, meta), return_inverse=True)      # (two lengths that are stored alike are one element)
    wn = np.bincount(inv, weights=mult.astype(np.float64)).astype(np.int64)
    assert len(got) == len(want) and (got == want).all() and (gn == wn).all(), name
    assert (raw["read_offset"] == 0).all()                                # every tract starts right behind its left flank
    chunk = F.chunk_records(F.scan_bound(F.parts_of(name)[0].size) if c.route == "scan" else c.n_reads)
    assert chunk == MIN_CHUNK
    return c, ref


@pytest.mark.parametrize("name", [n for n in NAMES if not F.is_big(n)])
def test_the_oracle_reads_the_intended_keys(name):
    check_raw_is_the_key_table(name)


@pytest.mark.parametrize("name", of_kind("zero_key"))
def test_zero_key_corpus(name):
    c = F.get(name)
    t = c.keys
    word = F.rec1_key_word(t["c0"], t["c1"], t["base"], t["length"])
    assert (word[:2] == 0).all() and (word[2:] != 0).all()                # lengths 1024 and 2048 of the A tract between N: the all-zero word
    assert int(word[2]) == 1 << 24 and int(word[3]) == 1 << 58            # its neighbours: length 1025, base C
    b = F.bucket_of(c.k, t["base"], t["c0"], t["c1"], t["length"])
    assert (b == c.facts["zero_bucket"]).sum() >= 302 and (b[4:] == c.facts["zero_bucket"]).all() and len(t) == 304
    raw = F.reference(name, [])["raw"]
    z = raw[(raw["ctx0"] == 0) & (raw["ctx1"] == 0) & ((raw["meta"] & np.uint64(0x3FFFFF)) == 0x1000)]
    assert len(z) == c.facts["zero_total"] and set((z["meta"] >> np.uint64(49)).tolist()) == {1, 2}
    # the reads of the issue: AN + A x 1024 + NA at k = 2, twice
    o = orc.Oracle(2)
    for _ in range(2):
        o.scan_seq(b"AN" + b"A" * 1024 + b"NA", F.M)
    e = o.elems()
    assert len(e) == 2 and (e["ctx0"] == 0).all() and (e["ctx1"] == 0).all() and ((e["meta"] & np.uint64(0x3FFFFF)) == 0x1000).all()
    o.finalise(0, 0)
    assert (o.c.status, o.c.n_elem) == (0, 1)
    o.close()
    assert F.read_for_key(2, 0, 0, 0, 1024, nflank=True) == b"AN" + b"A" * 1024 + b"NA"
    # under either filter the oracle keeps the zero key with a count of 8
    for f in F.filters_of(c):
        fin = F.reference(name)["fin"][f]
        kept = np.frombuffer(fin["kept"], orc.ELEM_DTYPE)
        zk = kept[(kept["ctx0"] == 0) & (kept["ctx1"] == 0) & ((kept["meta"] & np.uint64(0xFFF)) == 0)]
        assert fin["status"] == 0 and len(zk) == 1 and int(orc.decode_meta(zk["meta"])["count"][0]) == 8


@pytest.mark.parametrize("name", of_kind("extreme_flanks"))
def test_extreme_flanks_corpus(name):
    c = F.get(name)
    t, ones = c.keys, (1 << (2 * c.k)) - 1
    pairs = {(int(r["base"]), int(r["c0"]), int(r["c1"])) for r in t}
    assert {(1, 0, 0), (1, ones, ones), (1, 0, ones), (1, ones, 0), (0, ones, ones)} <= pairs
    assert ((t["c0"] == 0) & (t["c1"] == 0)).sum() == c.facts["n_both_zero"] == 4
    assert F.reference(name)["fin"][(1, 0)]["n"] == len(t) - 1                # all but the key seen on one strand only
    assert F.reference(name)["fin"][(0, 0)]["n"] == len(t)


@pytest.mark.parametrize("name", of_kind("count_edges"))
def test_count_edges_corpus(name):
    c, ref = check_raw_is_the_key_table(name)
    assert sum(p.size for p in F.parts_of(name)) < (210 << 20) and max(p.size for p in F.parts_of(name)) <= (96 << 20) + 1
    ref = F.reference(name, [(0, 0), (1, 0), (1, c.min_coverage)])
    cases = c.facts["cases"]
    assert {t for t, _ in cases} >= {1 << 19, 1 << 20, (1 << 20) + 2} and ((1 << 19, "one") in cases and (1 << 19, "split") in cases)
    if c.k == 2:
        assert {t for t, _ in cases} == {1, 2, 3, (1 << 19) - 1, 1 << 19, (1 << 19) + 1, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 2}
    sx = lambda v: ((v + (1 << 19)) & 0xFFFFF) - (1 << 19)
    for rb in (0, 1):
        fin = ref["fin"][(rb, 0)]
        kept = np.frombuffer(fin["kept"], orc.ELEM_DTYPE)
        d = orc.decode_meta(kept["meta"])
        got = sorted(zip(d["count"].tolist(), d["canon_flag"].tolist()))
        want = [(sx(int(r["nf"] + r["nr"])), (1 if r["nf"] else 0) | (2 if r["nr"] else 0)) for r in c.keys]
        want = sorted(w for w in want if (w[1] == 3 if rb else w[0] > 1))
        assert fin["status"] == 0 and got == want, (name, rb)
    assert (-524288, 3) in want and (-524288, 1) not in want                  # 2^19 reads count as -524288: kept when both strands were seen
    # a context whose depth is negative has no index range even at min_coverage 0 (one of depth 0 has): among them the
    # context that pairs the record of 2^19 reads with one of 3
    depth = {}
    for r in c.keys:
        if r["nf"] and r["nr"]:
            key = (int(r["base"]), int(r["c0"]), int(r["c1"]))
            depth[key] = depth.get(key, 0) + sx(int(r["nf"] + r["nr"]))
    assert -524288 + 3 in depth.values() and (c.k != 2 or 0 in depth.values())
    assert ref["fin"][(1, 0)]["n_idx"] == sum(1 for d in depth.values() if d >= 0) < len(depth)
    assert ref["fin"][(1, c.min_coverage)]["n_idx"] == sum(1 for d in depth.values() if d >= c.min_coverage) < ref["fin"][(1, 0)]["n_idx"]
    F.release(name)


@pytest.mark.parametrize("name", of_kind("one_bucket"))
def test_one_bucket_corpus(name):
    c = F.get(name)
    w = record_width(c.k)
    D, r, bucket = c.facts["D"], c.facts["r"], c.facts["bucket"]
    b = F.bucket_of(c.k, c.keys["base"], c.keys["c0"], c.keys["c1"], c.keys["length"])
    counts = F.bucket_counts(c.k, c.keys)
    assert (b == bucket).sum() == D and counts[bucket] == D * r
    assert ((c.keys["nf"] > 0) & (c.keys["nr"] > 0)).all()
    rest = np.delete(counts, bucket)
    assert (rest.sum() == 0) if not c.facts["others"] else (rest.sum() > 2000 and (rest > 0).sum() > 200 and rest.max() < 64)
    lo, hi = max(0, D - F.max_admitted(w)) * r, max(0, D - F.CLOSE_AT[w] - 1) * r       # leftovers of the first round: at least, at most
    if D >= 2 * F.max_admitted(w) + 1:
        assert lo > MIN_CHUNK and D - 2 * F.max_admitted(w) >= 1                          # whatever the race admits: over a chunk, and a third round
    elif D >= F.max_admitted(w):
        assert hi > MIN_CHUNK and lo == (D - F.max_admitted(w)) * r
    elif D > F.CLOSE_AT[w] + 1:
        assert 0 < hi < MIN_CHUNK and lo == 0
    else:
        assert hi == 0                                                                     # every key gets in: the table closes at most behind the last
    ref = F.reference(name)
    assert ref["fin"][(1, 0)]["n"] == len(c.keys) == ref["fin"][(0, 0)]["n"]
    assert 0 < ref["fin"][(0, c.min_coverage)]["n_idx"] <= len(c.keys)


def test_one_bucket_corpora_cover_what_was_asked():
    for k in F.K_OF_W.values():
        mine = [F.get(n) for n in of_kind("one_bucket") if "-k%d-" % k in n]
        w = record_width(k)
        c, mx = F.CLOSE_AT[w], F.max_admitted(w)
        assert {x.facts["D"] for x in mine} == {c - 1, c, c + 1, c + 2, mx, mx + 1, 2 * mx + 1}
        assert {x.facts["bucket"] for x in mine} == {0, 255, 131} and {x.facts["others"] for x in mine} == {False, True}
        assert {(x.facts["D"], x.facts["others"]) for x in mine} >= {(2 * mx + 1, False), (2 * mx + 1, True), (c + 1, False), (c + 1, True)}


@pytest.mark.parametrize("name", of_kind("bucket_sizes"))
def test_bucket_sizes_corpus(name):
    c = F.get(name)
    w = record_width(c.k)
    counts = F.bucket_counts(c.k, c.keys)
    assert counts[77] == c.facts["n"] == c.n_reads and counts.sum() == c.n_reads
    assert sorted(F.bucket_size_n(w, s) for s in F.BUCKET_SIZES) == [1, 2, 64 * F.IN_FLIGHT[w] - 1, 64 * F.IN_FLIGHT[w], 64 * F.IN_FLIGHT[w] + 1, 12287, 12288, 12289]


def test_long_bucket_corpus():
    name = of_kind("long_bucket")[0]
    c, ref = check_raw_is_the_key_table(name)
    counts = F.bucket_counts(c.k, c.keys)
    b = c.facts["bucket"]
    assert counts[b] == c.n_reads == c.facts["n_long"] + 12000 and counts[b] > (F.AG_NCH + 1) * MIN_CHUNK
    assert int((c.keys["nf"] + c.keys["nr"]).max()) == c.facts["n_long"] > F.AG_NCH * MIN_CHUNK
    assert len(c.keys) == 6001 > F.max_admitted(1)                            # more keys than a round admits: a second round behind the long first
    assert record_width(c.k) == 1 and ref["n_raw"] < 2 ** 23                  # (one scan, the smallest chunk)
    ref = F.reference(name, [(1, 0)])
    assert ref["fin"][(1, 0)]["n"] == 6001
    F.release(name)


@pytest.mark.parametrize("name", of_kind("kept_exactly_full"))
def test_kept_exactly_full_corpus(name):
    c = F.get(name)
    ref = F.reference(name)
    n = c.facts["n"]
    assert c.route == "upload" and ref["n_raw"] == n
    kept_cap = n // 2 + 1                                                     # finalise_impl: raw_bound / 2 + 1, and upload_raw's bound is exact
    assert ref["fin"][(1, 0)]["n"] == ref["fin"][(0, 0)]["n"] == n // 2 == kept_cap - 1
    assert F.plan_cap(n) == kept_cap


@pytest.mark.parametrize("name", of_kind("kept_counts"))
def test_kept_counts_corpus(name):
    c = F.get(name)
    ref = F.reference(name)
    n1, k = c.facts["n1"], c.k
    for f in F.filters_of(c):
        assert ref["fin"][f]["status"] == 0 and ref["fin"][f]["n"] == n1, (name, f)
    assert 0 < ref["fin"][(1, c.min_coverage)]["n_idx"] and (k != 2 or ref["fin"][(1, c.min_coverage)]["n_idx"] < ref["fin"][(1, 0)]["n_idx"] or n1 % 288 == 0)
    occ = F.bin_occupancy(c.keys, k)
    assert occ.sum() == n1 and occ.max() <= F.BS_RANK_MAX                    # no fallback
    raw_bound = sum(F.scan_bound(p.size) for p in F.parts_of(name))
    assert F.plan_cap(raw_bound) > n1 + 1                                    # the device's plan holds unless TATAJUBA_AMD_PLAN_CAP lowers it


def test_kept_counts_pairs_sit_on_either_side_of_their_threshold():
    pairs = {}
    for n in of_kind("kept_counts"):
        c = F.get(n)
        pairs.setdefault(c.k, []).append(c.facts["n1"])
    for k, lo in [(10, 3072), (10, 6144), (10, 12288), (2, 6144), (2, 12288)]:
        assert lo in pairs[k] and lo + 1 in pairs[k] and F.bin_bits_for(lo + 1, k) == F.bin_bits_for(lo, k) + 1
    assert [F.fine_bin_bits(2) - F.bin_bits_for(n, 2) for n in sorted(pairs[2])] == [2, 1, 1, 0]     # the fold of clear_buckets_kernel: uint4 loop, scalar loop, no fold
    for k, lo in [(6, 512), (10, 131072)]:
        assert lo in pairs[k] and lo + 1 in pairs[k]
        assert (F.cov_plan_bits(lo, k)[1], F.cov_plan_bits(lo + 1, k)[1]) == (False, True)              # hashed, then addressed by the key


@pytest.mark.parametrize("name", of_kind("bin_staircase"))
def test_bin_staircase_corpus(name):
    c = F.get(name)
    ref = F.reference(name)
    n1, k = c.facts["n1"], c.k
    top = max(c.facts["bins"])
    occ = F.bin_occupancy(c.keys, k)
    assert occ.tolist() == c.facts["bins"] == sorted([1, 2, 63, 64, 65, 66, 128, 129, 255, top]) and occ.sum() == n1 == len(c.keys)
    assert (top == 256 and occ.max() <= F.BS_RANK_MAX) or (top == 257 and occ.max() == F.BS_RANK_MAX + 1)    # which sort runs: LDS / radix fallback
    assert {1, 2, 64, 65} <= set(c.facts["ctx_sizes"])
    for f in F.filters_of(c):
        assert ref["fin"][f]["status"] == 0 and ref["fin"][f]["n"] == n1
    # from the oracle's sorted output: the bin of 64 records and what its last lane holds; the lengths' signed order
    kept = np.frombuffer(ref["fin"][(1, 0)]["kept"], orc.ELEM_DTYPE)
    base = (kept["meta"] & np.uint64(3)).astype(np.uint64)
    bins = F.bin_of_record(kept["ctx0"], kept["ctx1"], base, k, 6)
    assert (np.diff(bins) >= 0).all()                                         # ascending bins are the sorted order
    b64 = kept[bins == np.nonzero(np.bincount(bins) == 64)[0][0]]
    same_as_last = int(((b64["ctx0"] == b64["ctx0"][-1]) & (b64["ctx1"] == b64["ctx1"][-1])).sum())
    assert same_as_last == {"alone": 1, "ends": 2, "whole": 64}[name.rsplit("-", 1)[1]]
    ctx = {}
    for e, ln in zip(kept, orc.decode_meta(kept["meta"])["length"].tolist()):
        ctx.setdefault((int(e["ctx0"]), int(e["ctx1"])), []).append(ln)
    longest = max(ctx.values(), key=len)
    assert len(longest) == 65
    assert longest == sorted(longest, reverse=True) and {511, 1, 0, -1, -512} <= set(longest)       # 511 > ... > 1025 (1) > 1024 (0) > 1023 (-1) > 512 (-512)
    # depth: a context of two records is exactly at the threshold, one of a single record below it
    sizes = np.array([len(v) for v in ctx.values()])
    assert ref["fin"][(1, c.min_coverage)]["n_idx"] == int((sizes >= 2).sum()) < len(sizes) == ref["fin"][(1, 0)]["n_idx"]
    assert (sizes == 2).sum() >= 2 and c.min_coverage == 4


@pytest.mark.parametrize("name", of_kind("coverage_pools"))
def test_coverage_pools_corpus(name):
    c = F.get(name)
    ref = F.reference(name)
    for f in F.filters_of(c):
        fin = ref["fin"][f]
        kept = np.frombuffer(fin["kept"], orc.ELEM_DTYPE)
        assert fin["status"] == 0 and fin["coverage"] == F.coverage_restated(kept) == 13
        assert F.coverage_restated(kept, pool=False) != 13                    # only the pooling of both sides reaches it
        if c.facts["cut_matters"]:
            assert F.coverage_restated(kept, cut=False) != 13                 # and, from k = 16 on, only the 31-bit cut
        assert {0, 0x7FFFFFFF & ((1 << (2 * c.k)) - 1)} <= set((kept["ctx0"] & np.uint64(0x7FFFFFFF)).tolist()) & set((kept["ctx1"] & np.uint64(0x7FFFFFFF)).tolist())
        if c.facts["negative"] and f[0] == 1:
            assert (orc.decode_meta(kept["meta"])["count"] == -524288).sum() == 1
    F.release(name)


def test_the_corpus_list_covers_the_widths_and_borders():
    assert [int(n.split("-k")[1]) for n in of_kind("zero_key")] == [2, 12]
    assert [int(n.split("-k")[1]) for n in of_kind("extreme_flanks")] == [2, 10, 12, 13, 20, 28, 29, 31, 32]
    assert [int(n.split("-k")[1]) for n in of_kind("count_edges")] == [2, 13, 29]
    for kind in ("one_bucket", "bucket_sizes", "kept_exactly_full", "bin_staircase"):
        assert sorted({int(n.split("-k")[1].split("-")[0]) for n in of_kind(kind)}) == [10, 20, 31], kind
    assert sorted({int(n.split("-k")[1].split("-")[0]) for n in of_kind("coverage_pools")}) == [10, 16, 17, 32]
