"""The grouping corpus (tests/grouping_edges.py) is what it claims to be -- shown on the CPU from the oracle, the kernel
source's constants and the module's own restatements.  tests/test_grouping_edges.py judges the device's grouping on these
rows; if a planted row missed its place, those tests would prove less than they say.  These are conditions, not
measurements: the rows are chosen so that they hold.  Nothing here touches the device, and nothing skips."""
import re

import numpy as np
import pytest

from oracle import orc
from tests import grouping_edges as G
from tests.test_edge_streams import _define, _source, _value
from tests.test_union_tracts_cabi import oracle_union_grouping, pooled_elements

ALL = list(G.CASES)


def analyse(r, maxd, lev, free_end=False):
    """restatements and oracle on one corpus: back, flank-only heads, candidates, the oracle's grouping, final heads, windows"""
    back = G.back_of(r.keys, maxd)
    h1 = G.heads_of(back)
    cand = G.candidates(r.keys, r.counts, h1, r.k, lev, free_end)
    want = G.union_grouping(r.keys, r.counts[:, None], r.k, maxd, lev, free_end)
    orc.set_edit_free_end(False)
    hf = want["join_type"] == 0
    return {"back": back, "h1": h1, "cand": cand, "want": want, "hf": hf, "jt": want["join_type"], "gof": want["tract_id"],
            "walk": G.window_walk(cand, h1, hf, r.bases)}


def replay_cover(n, walk):
    """rows inside some replay"""
    inside = np.zeros(n, bool)
    for s, o, e in walk:
        if o is not None:
            inside[s + o:e] = True
    return inside


def test_constants_are_those_of_the_kernel_source():
    src = _source()
    assert _value(_define(src, "GR_CHUNK")) == G.GR_CHUNK
    m = re.search(r"static unsigned grid_for \(long n\) \{ return \(unsigned\) std::max<long> \(1, std::min<long> \(\(n \+ 255\) / (\d+), (\d+)\)\); \}", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (G.BLOCK, G.GRID_CAP) and G.ONE_TRIP == 1 << 20
    for kern in ("group_back_kernel", "group_resolve_kernel", "group_speculate_kernel<CountOf>", "group_summary_kernel", "group_histogram_kernel",
                 "union_tract_kernel"):
        assert "hipLaunchKernelGGL (%s, dim3 (grid_for (n)), dim3 (%d)" % (kern, G.BLOCK) in src, kern
    assert "hipLaunchKernelGGL (group_repair_kernel<CountOf>, dim3 (1), dim3 (%d)" % G.BLOCK in src
    assert "unsigned char row[2 * 32 + 4];" in src                     # name_edit_distance: 2k + 4 entries at k = 32


@pytest.mark.parametrize("name", ALL + ["count_wrap", "grid-staircase", "grid-retry"])
def test_rows_descend_and_counts_fit_the_field(name):
    r = {"count_wrap": G.count_wrap, "grid-staircase": lambda: G.grid_stride("staircase"), "grid-retry": lambda: G.grid_stride("retry")}.get(name, lambda: G.get(name))()
    assert G.strictly_descending(r.keys) and len(r) == len(r.counts) and set(r.bases.tolist()) <= {0, 1}   # (a sample keeps no other base)
    if len(r) < 20000:
        key = G.order_key(r.keys)
        assert key == sorted(key, reverse=True) and len(set(key)) == len(key)
    assert ((signed := G.signed_length(r.keys[:, 2])) != 0).all() and signed.min() >= -512   # (a stored length of 0: the zero key of tests/finalise_edges.py)
    if name == "count_wrap":
        assert sorted(r.counts.tolist()) == [4, 5, (1 << 20) + 3]
    else:
        assert r.counts.min() >= 2 and r.counts.max() < 1 << 19          # a finalise drops what it saw once; the oracle's field is 20 bits, signed
    assert ((r.keys[:, 2] >> np.uint64(12)) & np.uint64(0xFFFFF) == (r.counts & 0xFFFFF).astype(np.uint64)).all()


@pytest.mark.parametrize("name", ALL)
def test_restatements_agree_with_the_oracle(name):
    """back_of / heads_of give the oracle's flank-only grouping; union_grouping is oracle_union_grouping; every row taken in by
    the retry and every row whose head flag differs between the two groupings lies inside a replay of window_walk; a candidate
    that no window takes lies inside one too"""
    r = G.get(name)
    for maxd, lev in G.CASES[name][1]:
        for fe in ((False, True) if G.CASES[name][2] else (False,)):
            a = analyse(r, maxd, lev, fe)
            ogof = orc.group_contexts(pooled_elements(r.keys, np.minimum(r.counts, 1000)), maxd)[0]
            assert (a["h1"] == np.r_[True, ogof[1:] != ogof[:-1]]).all(), (maxd, lev)
            if len(r) <= 5000:
                slow = oracle_union_grouping(r.keys, r.counts[:, None], r.k, maxd, lev, free_end=fe)
                orc.set_edit_free_end(False)
                for f in ("tract_id", "join_type", "lev_distance", "mode", "integral"):
                    assert (slow[f] == a["want"][f]).all(), f
            inside = replay_cover(len(r), a["walk"])
            assert inside[a["jt"] == 2].all() and inside[a["h1"] != a["hf"]].all()
            assert all(inside[i] for i in G.skipped_candidates(a["cand"], a["walk"]))
            assert (a["cand"] <= a["h1"]).all() and (lev > 0 or not a["cand"].any())


@pytest.mark.parametrize("k,L,thin", [(10, 5, False), (10, 70, False), (32, 3, False), (10, 100, True)])
def test_staircase_is_one_long_stretch_with_heads_deep_inside(k, L, thin):
    r = G.staircase(k, L, thin=thin)
    n_ctx = 6 * k + 1
    thin_ctx = (n_ctx + 3) // 4 if thin else 0
    assert len(r) == (n_ctx - thin_ctx) * L + thin_ctx
    if (k, L, thin) == (10, 70, False):
        assert len(r) == 4270 > G.GR_CHUNK and len(r) > 16 * G.BLOCK
    ctx = np.r_[True, (r.keys[1:, :2] != r.keys[:-1, :2]).any(axis=1)]
    first = np.flatnonzero(ctx)
    assert len(first) == n_ctx
    d = lambda a, b: int(G.flank_distance(r.keys[a, 0], r.keys[a, 1], r.keys[b, 0], r.keys[b, 1])[0]) if np.ndim(a) else int(
        G.flank_distance(r.keys[a:a + 1, 0], r.keys[a:a + 1, 1], r.keys[b:b + 1, 0], r.keys[b:b + 1, 1])[0])
    assert all(d(first[t], first[t + 1]) == 1 for t in range(n_ctx - 1)) and all(d(first[t], first[t + 2]) == 2 for t in range(n_ctx - 2))
    assert d(first[0], first[2 * k]) == 2 * k
    back = G.back_of(r.keys, 2)
    heads = G.heads_of(back)
    assert G.stretches(back).tolist() == [0]                             # one stretch: one thread of group_resolve_kernel walks it all
    deep = np.flatnonzero(heads)[1:]
    assert heads.sum() == (n_ctx + 1) // 2 and (heads[first[::2]]).all() and len(deep) >= 10 and deep.max() >= G.BLOCK
    # the walk back of a row two contexts down ends on the last row of the context two up: L rows or more behind
    assert (np.arange(len(r)) - back)[first[2]:].min() >= min(L, 2) and (np.arange(len(r)) - back).max() >= L
    if thin:                                                             # a head that is itself back[j] of the rows two contexts on
        start_is_back = [h for h in deep if (back[h + 1:] == h).any()]
        assert len(start_is_back) >= 10 and max(start_is_back) >= G.BLOCK
    else:
        assert not any((back[h + 1:] == h).any() for h in deep) or L == 1
    for maxd, n_heads in ((1, n_ctx), (3, (n_ctx + 2) // 3)):
        assert G.heads_of(G.back_of(r.keys, maxd)).sum() == n_heads


def test_cascade_cases_do_what_their_names_say():
    r = G.cascade()
    m = r.marks
    a, a0 = analyse(r, 2, 3), analyse(r, 2, 0)
    jt, gof, h1, cand = a["jt"], a["gof"], a["h1"], a["cand"]
    ed = lambda x, y: orc.levenshtein(r.name(m[x]), r.name(m[y]))
    assert not (a0["jt"] == 2).any() and (a0["hf"] == h1).all() and (a["hf"] != a0["hf"]).any()      # at lev 0 the flank-only grouping
    # new_name: R1 comes in with the highest total, R2 is within 3 of R1 and not of H
    assert [jt[m["new_name." + t]] for t in ("H", "R1", "R2")] == [0, 2, 2] and r.counts[m["new_name.R1"]] > r.counts[m["new_name.H"]]
    assert ed("new_name.R1", "new_name.R2") < 3 <= ed("new_name.H", "new_name.R2") and a["want"]["mode"][gof[m["new_name.H"]]] == m["new_name.R1"]
    # old_name: the speculation flags R2, the replay refuses it
    assert [jt[m["old_name." + t]] for t in ("H", "R1", "R2")] == [0, 2, 0] and cand[m["old_name.R2"]] and a["hf"][m["old_name.R2"]]
    assert ed("old_name.R1", "old_name.R2") < 3 <= ed("old_name.H", "old_name.R2") and r.counts[m["old_name.R1"]] < r.counts[m["old_name.H"]]
    assert m["old_name.R2"] in G.skipped_candidates(cand, a["walk"])
    # absorbed: no head without the retry, a head with it; exactly lev edits from the name
    s = m["absorbed.S"]
    assert not h1[s] and a["hf"][s] and jt[m["absorbed.R1"]] == 2 and gof[m["absorbed.R1"]] == gof[m["absorbed.H"]] and ed("absorbed.H", "absorbed.S") == 3
    assert int(G.flank_distance(r.keys[[s], 0], r.keys[[s], 1], r.keys[[m["absorbed.H"]], 0], r.keys[[m["absorbed.H"]], 1])[0]) >= 4
    # tie: equal totals, the first is the name: D is within 3 of H and not of H2
    assert r.counts[m["tie.H"]] == r.counts[m["tie.H2"]] and [jt[m["tie." + t]] for t in ("H", "H2", "D")] == [0, 1, 2]
    assert ed("tie.H", "tie.D") < 3 <= ed("tie.H2", "tie.D") and a["want"]["mode"][gof[m["tie.H"]]] == m["tie.H"] and cand[m["tie.D"]]
    # base: one edit apart, another base
    lo, hi = m["base.last"], m["base.first"]
    assert hi == lo + 1 and (r.keys[lo, :2] == r.keys[hi, :2]).all() and r.bases[lo] != r.bases[hi] and ed("base.last", "base.first") == 1
    assert a["hf"][hi] and not cand[hi]


def test_window_cases_are_on_their_rows():
    r = G.windows()
    m, n = r.marks, len(r)
    a = analyse(r, 1, 3)
    cand, walk = a["cand"], a["walk"]
    taken = {s: (o, e) for s, o, e in walk}
    where = np.flatnonzero(cand)
    assert where[0] == m["row1"] == 1 and where[-1] == m["last_row"] == n - 1
    assert (0, 1) == (walk[0][0], walk[0][1])                                    # a candidate on row 1
    s = walk[1][0]
    assert taken[s][0] == 0 and s == m["offset0"]                                # the next window's first row
    s = walk[2][0]
    assert taken[s][0] == G.GR_CHUNK - 1 and s + G.GR_CHUNK - 1 == m["offset_last"]   # a window's last row
    s = m["empty_window"]
    assert taken[s] == (None, s + G.GR_CHUNK) and taken[s + G.GR_CHUNK][0] == 0 and s + G.GR_CHUNK == m["after_empty"]   # empty, then row 0
    s = m["after_empty"] + 3
    assert s in taken and cand[s:s + G.GR_CHUNK].sum() >= G.BLOCK + 1             # a thread sees several, several threads see one
    assert taken[s][0] == m["many"] - s and np.flatnonzero(cand[s:s + G.GR_CHUNK])[1] < G.BLOCK
    assert G.skipped_candidates(cand, walk) == [m["covered"]]                    # inside the stretch an earlier replay covered
    s = m["past_end_window"]
    assert taken[s][0] == G.GR_CHUNK - 2 and taken[s][1] == s + G.GR_CHUNK + 2 and s + G.GR_CHUNK - 2 == m["past_end"]   # the replay ends behind its window
    assert walk[-1][0] + walk[-1][1] == n - 1 and walk[-1][2] == n               # the last row
    # a far context taken in a second time: the unit's second A row, n_context counts it twice
    g = a["want"]["groups"][a["gof"][m["row1"]]]
    assert a["jt"][m["row1"]:m["row1"] + 2].tolist() == [2, 2] and (g["n_elem"], g["n_context"]) == (3, 3)
    assert (r.keys[m["row1"], :2] == r.keys[m["row1"] + 1, :2]).all()
    # the fillers stay alone under both readings
    for fe in (False, True):
        b = analyse(r, 1, 3, fe)
        assert b["cand"].sum() == 4 + G.BLOCK + 4 + 3 + 1 and (b["cand"] == cand).all()


@pytest.mark.parametrize("k", [2, 10, 32])
def test_threshold_pairs_are_exactly_at_and_below(k):
    r, sh = G.threshold_pairs(k), G.threshold_pairs(k, "shifted")
    assert len(r.name(0)) == 2 * k + 3 and r.bases.tolist() == [1, 1, 0, 0] and sh.bases.tolist() == [1, 1]   # a pair per base: nothing else can be its name
    ed = lambda r, i, fe=False: orc.levenshtein(r.name(i - 1), r.name(i), free_end=fe)
    assert ed(r, r.marks["below"]) == 2 == ed(r, r.marks["below"], True) and ed(r, r.marks["at"]) == 3 == ed(r, r.marks["at"], True)
    assert ed(sh, sh.marks["shifted"]) == 2 and ed(sh, sh.marks["shifted"], True) == 1     # the readings part here
    joined = lambda lev, fe: [int(analyse(r, 1, lev, fe)["jt"][r.marks[x]]) for x in ("below", "at")] + [int(analyse(sh, 1, lev, fe)["jt"][1])]
    assert joined(2, False) == [0, 0, 0] and joined(2, True) == [0, 0, 2]
    assert joined(3, False) == [2, 0, 2] == joined(3, True)
    assert joined(4, False) == [2, 2, 2] == joined(4, True)


def test_all_join_is_one_tract_per_base_under_one_replay_each():
    r = G.all_join()
    lev = 2 * r.k + 4
    a = analyse(r, 1, lev)
    assert len(r) == 9000 and a["hf"].sum() == 2 and np.flatnonzero(a["hf"]).tolist() == [0, 4500]
    replays = [(s + o, e) for s, o, e in a["walk"] if o is not None]
    assert [e for _, e in replays] == [4500, 9000] and all(h - h // 4500 * 4500 <= 3 for h, _ in replays)
    assert all(h < s + G.GR_CHUNK < e for (s, _, _), (h, e) in zip(a["walk"], replays))   # a window's end inside each replay
    assert max(orc.levenshtein(r.name(i), r.name(j)) for i in range(0, 4500, 97) for j in range(1, 4500, 89)) < lev


def test_hist_ties_and_count_wrap():
    r = G.hist_ties()
    g = orc.genomic_context_list(pooled_elements(r.keys, r.counts), r.k, 2, 3, 1)
    assert g["groups"]["n_len"].tolist() == [4, 3]
    assert list(zip(g["hist_len"][:4].tolist(), g["hist_freq"][:4].tolist())) == [(5, 6), (2, 6), (-3, 6), (-1, 4)]
    assert list(zip(g["hist_len"][6:9].tolist(), g["hist_freq"][6:9].tolist())) == [(-2, 5), (-7, 5), (3, 2)]
    w = G.count_wrap()
    m = w.marks
    ed = lambda x, y: orc.levenshtein(w.name(m[x]), w.name(m[y]))
    assert (m["X"], m["Y"], m["Z"]) == (0, 1, 2) and ed("Y", "Z") == 2 and ed("X", "Z") == 3 and ed("X", "Y") == 1
    field = orc.genomic_context_list(pooled_elements(w.keys, w.counts & 0xFFFFF), w.k, 2, 3, 1)          # the sample route: the field
    assert field["join_type"].tolist() == [0, 1, 2] and field["groups"]["mode"].tolist() == [1]
    mat = G.count_wrap_union_mat(w)
    assert mat[0].astype(np.int64).sum() > 1 << 31 and mat.min() >= 0
    exact = G.union_grouping(w.keys, mat, w.k, 2, 3)                                                      # the union route: exact totals
    assert exact["join_type"].tolist() == [0, 1, 0] and exact["mode"].tolist() == [0, 2]


@pytest.mark.parametrize("which", ["staircase", "retry"])
def test_grid_stride_rows_reach_the_second_trip(which):
    r = G.with_counts(G.grid_stride(which), 2)                  # (as tests/test_grouping_edges.py runs it)
    n, m = len(r), r.marks
    assert n == G.GRID_CAP * G.BLOCK + 300 and n > G.ONE_TRIP and set(r.bases.tolist()) == {0, 1}
    a = analyse(r, 2, 3)
    if which == "staircase":
        assert m["first"] < G.ONE_TRIP - 100 and m["last"] > G.ONE_TRIP + 100 and m["last"] - m["first"] + 1 == 290
        st = G.stretches(a["back"])
        assert m["first"] in st and not ((st > m["first"]) & (st <= m["last"])).any()          # one stretch across the boundary
        inner = np.flatnonzero(a["h1"][m["first"] + 1:m["last"] + 1]) + m["first"] + 1
        assert (inner < G.ONE_TRIP).sum() >= 10 and (inner >= G.ONE_TRIP).sum() >= 10
        assert (np.flatnonzero(a["cand"]) >= G.ONE_TRIP).sum() >= 10 and (a["jt"][G.ONE_TRIP:] == 2).any()
        assert (a["jt"][:m["first"]] == 0).all() and (a["jt"][m["last"] + 1:] == 0).all()      # the fillers stay alone
    else:
        assert np.flatnonzero(a["cand"]).tolist() == [G.ONE_TRIP - 1, G.ONE_TRIP, G.ONE_TRIP + 1] == [m["cand-1"], m["cand0"], m["cand1"]]
        assert np.flatnonzero(a["jt"]).tolist() == [G.ONE_TRIP - 1, G.ONE_TRIP + 1] and (a["jt"][a["jt"] != 0] == 2).all()
        assert G.skipped_candidates(a["cand"], a["walk"]) == [G.ONE_TRIP]
