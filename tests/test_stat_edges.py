"""The statistics corpus (tests/stat_edges.py) is what it claims to be -- checked on the CPU, from the unions themselves, the
kernel source and the numpy restatements.  tests/test_tract_stat_edges.py judges the kernels on these unions; if a union
missed its edge, those tests would prove nothing."""
import os
import re

import numpy as np
import pytest

from tests import stat_edges as E
from tests.test_tract_stats_cabi import signed_length
from tests.test_union_tracts_cabi import AVG, ENT, MODAL, PROP, restate_union_tract_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = (AVG, MODAL, ENT)                                 # the relative differences both rules read


def _source():
    with open(os.path.join(ROOT, "tatajuba_amd", "csrc", "hopo_device.hip")) as fh:
        return fh.read()


def test_constants_are_those_of_the_kernel_source():
    src = _source()
    for name in ("UT_SLOTS", "UT_LENGTHS", "UT_FULL_BLOCKS"):
        m = re.findall(r"^#define %s (\d+)$" % name, src, re.M)
        assert len(m) == 1 and int(m[0]) == getattr(E, name), (name, m)
    # what the corpus takes from them: the slot index of a length, the grid of the FULL kernels, the two thresholds
    assert "cnt[(l + UT_LENGTHS / 2) * stride] += x;" in src and "if (nb == UT_SLOTS) return -1;" in src
    assert src.count("(unsigned) UT_FULL_BLOCKS);") == 2
    assert src.count("difference > 1.e-5") == 1 and src.count("> 1e-6") == 3
    assert (E.LEN_MIN, E.LEN_MAX) == (-512, 511) and [E.segment(ns) for ns in (1, 2, 3, 64, 65, 130)] == [1, 2, 4, 64, 64, 64]
    assert E.full_pass(64) == 16 and E.full_pass(1) == 1024


@pytest.mark.parametrize("name", list(E.CASES))
def test_unions_are_well_formed_and_away_from_the_thresholds(name):
    """merge order, tracts that tile the union, and for every input of the corpus (every reference-length variant): no tract
    within 1e-9 of the 1e-5 of `variable` (the band in which the shared checks do not ask for the same side), no term
    that `selected` reads within 1e-8 of 1e-6; N5 on the same ids agrees with N6 wherever a length has one row"""
    e = E.case(name)
    n, nt = len(e.keys), len(e.tracts)
    assert e.mat.shape == (n, len(e.coverage)) and e.mat.dtype == np.int32 and len(e.tract_ids) == n and len(e.lev_distance) == nt == len(e.names)
    order = [(-int(b & 3), -int(a), -int(c), -int(signed_length(b))) for a, c, b in e.keys]
    assert order == sorted(order) and len(set(order)) == n
    tr = e.tracts
    assert tr["first"][0] == 0 and (tr["first"][1:] == tr["first"][:-1] + tr["n_rows"][:-1]).all() and tr["first"][-1] + tr["n_rows"][-1] == n
    assert (np.repeat(np.arange(nt), tr["n_rows"]) == e.tract_ids).all() and (tr["lev_distance"] == e.lev_distance).all()
    assert (e.mat.astype(np.int64).sum(axis=1) > 0).all()
    for ref in E.REFS:
        w6, w5 = E.restated_union(name, ref), E.restated_tracts(name, ref)
        for w in (w6, w5):
            assert (np.abs(w["difference"] - 1e-5) > 1e-9).all()
            assert (np.abs(w["reldiff"][:, RULE] - 1e-6) >= 1e-8).all()
            assert (w["first"] == tr["first"]).all() and (w["n_rows"] == tr["n_rows"]).all()
        same = (w6["n_len"] == w6["n_rows"][:, None]).all(axis=1)          # every sample has every row, one per length
        assert (w5["variable"][same] == w6["variable"][same]).all() and (w5["modal_len"][same] == w6["modal_len"][same]).all()


# the figures of tests/stat_edges.py THRESHOLDS: (avg, modal, entropy) to two digits
FIGURES = {"entropy-selects": (1.2e-7, 1.2e-7, 1.9e-6), "entropy-below": (6.0e-8, 6.0e-8, 9.7e-7), "avg-selects": (7.6e-6, 7.5e-9, 1.37e-7),
           "modal-below": (0, 6.4e-7, 9.1e-13), "modal-selects": (0, 1.27e-6, 3.6e-12), "modal-variable": (0, 1.27e-5, 3.6e-10),
           "sum-below": (5.0e-7, 5.0e-7, 7.3e-6), "sum-variable": (1.25e-6, 1.25e-6, 1.67e-5), "sum-only": (9.84e-6, 9.6e-9, 1.74e-7)}


def test_threshold_tracts_sit_where_they_say():
    e = E.thresholds()
    assert e.names == list(E.THRESHOLDS) == list(FIGURES) and e.mat.shape[1] == 2 and (e.tracts["n_context"] == 1).all()
    w6, w5, w5c = E.restated_union("thresholds"), E.restated_tracts("thresholds"), E.restated_tracts("thresholds", context_keyed=True)
    # one context per tract: the context-keyed tracts are these, and N5's bar per row is N6's bar per length, to the bit
    for f in ("first", "n_rows", "reldiff", "values", "variable", "difference"):
        assert (w5[f] == w6[f]).all() and (w5c[f] == w6[f]).all(), f
    for t, name in enumerate(e.names):
        what = E.THRESHOLDS[name][1]
        rd = w6["reldiff"][t]
        for j, fig in zip(RULE, FIGURES[name]):
            assert rd[j] == fig == 0 or abs(rd[j] / fig - 1) < 0.02, (name, j, rd[j], fig)
        assert (w6["selected"][t], w6["variable"][t], w6["n_present"][t]) == (what["selected"], what["variable"], 2), name
        over = {term for term, j in (("avg", AVG), ("modal", MODAL), ("entropy", ENT)) if rd[j] > 1e-6}
        assert over == set(what["over"]), (name, over)
        assert what["selected"] == int(bool(over)) and what["variable"] == int(w6["difference"][t] > 1e-5)
    d = dict(zip(e.names, w6["difference"]))
    rd = dict(zip(e.names, w6["reldiff"]))
    assert 8.2e-6 < d["sum-below"] < 8.4e-6 and 1.9e-5 < d["sum-variable"] < 1.95e-5
    # neither 1e-4 nor 1e-6 in place of 1e-5, and no term left out of the sum, gives the same lists
    assert d["modal-variable"] < 1e-4 and d["sum-variable"] < 1e-4 and d["sum-below"] > 1e-6
    assert d["sum-variable"] - rd["sum-variable"][ENT] < 1e-5 and d["sum-variable"] - rd["sum-variable"][AVG] > 1e-5
    # the sum alone: above 1e-5 by 2e-8, every term below it, so a per-term test says "not variable"
    assert d["sum-only"] > 1e-5 + 1e-8 and (rd["sum-only"][list(RULE)] < 1e-5 - 1e-8).all()
    assert d["sum-only"] - rd["sum-only"][ENT] < 1e-5 - 1e-7            # ... and so does the sum without the entropy
    # neither 1e-5 in place of 1e-6 (the three *-selects are below it) nor the two swapped
    for name in ("entropy-selects", "avg-selects", "modal-selects"):
        assert d[name] < 1e-5 - 1e-6 and rd[name][list(RULE)].max() > 1e-6 + 2e-7
    for name in ("entropy-below", "modal-below"):
        assert rd[name][list(RULE)].max() < 1e-6 - 3e-8 and d[name] > 6e-7
    assert d["entropy-below"] > 1e-6                      # the sum is above 1e-6, no term is: a sum in the selection would select it
    # reference lengths: on sample 0's modal length nothing changes but the tracts whose samples disagree about it (the
    # modal-* tracts: sample 0 ties at 9, sample 1 has 8); off it every tract is variable; selection reads neither
    assert w6["modal_len"].tolist() == [[8, 8]] * 2 + [[511, 511]] + [[9, 8]] * 3 + [[8, 8]] * 2 + [[511, 511]]
    on, off = E.restated_union("thresholds", "modal"), E.restated_union("thresholds", "off")
    disagree = w6["modal_len"][:, 0] != w6["modal_len"][:, 1]
    assert (on["variable"] == (w6["variable"] | disagree)).all() and (off["variable"] == 1).all() and off["variable"].sum() > w6["variable"].sum()
    assert (on["selected"] == w6["selected"]).all() and (off["selected"] == w6["selected"]).all()
    # lev_distance 1 where nothing else selects: every tract selected, variable as before
    lev = E.restated_union("thresholds-lev")
    assert E.thresholds("lev").lev_distance.tolist() == [1 - s for s in w6["selected"]] and 0 < w6["selected"].sum() < len(e.names)
    assert (lev["selected"] == 1).all() and (lev["variable"] == w6["variable"]).all()


@pytest.mark.parametrize("ns", E.SLOT_NS)
def test_slot_edge_tracts_overflow_where_they_say(ns):
    e = E.slot_edge(ns)
    w = E.restated_union(f"slots-{ns}")
    widest = dict(zip(e.names, w["n_len"].max(axis=1)))
    seen = set()
    for t, name in enumerate(e.names):
        part = name.split("-")
        if part[0] == "wide":
            width, wide = int(part[1]), dict(E.wide_positions(ns))[part[2]]
            assert widest[name] == width == e.tracts["n_rows"][t] and np.flatnonzero(w["n_len"][t] == width).tolist() == wide
            others = np.delete(w["n_len"][t], wide)
            assert ((others >= 1) & (others <= 3)).all() and (w["n_context"][t] == 1).all()
            seen.add((width, part[2]))
        elif part[0] == "small":
            assert 1 <= widest[name] <= 3 and (w["n_len"][t] == widest[name]).all()
    assert seen == {(width, where) for width in (15, 16, 17) for where, _ in E.wide_positions(ns)}
    if ns == 130:                                        # lanes 0 and 1 of the segment of 64 reach these on their second and third round
        (r2,), (r3,) = dict(E.wide_positions(130))["round2"], dict(E.wide_positions(130))["round3"]
        assert E.segment(130) == 64 and (r2 % 64, r2 // 64) == (0, 1) and (r3 % 64, r3 // 64) == (1, 2)
    t16, t99 = e.names.index("shared-16+16"), e.names.index("shared-9+9")
    assert e.tracts["n_rows"][t16] == 32 and (w["n_len"][t16] == 16).all() and (w["n_context"][t16] == 2).all() and e.lev_distance[t16] == 1
    assert e.tracts["n_rows"][t99] == 18 and (w["n_len"][t99] == 18).all() and (w["n_context"][t99] == 2).all()
    over = {name for name in e.names if widest[name] > E.UT_SLOTS}
    assert over == {name for name in e.names if name.startswith("wide-17-")} | {"shared-9+9"}
    assert len(e.keys) < 400


@pytest.mark.parametrize("ns", list(E.FULL_FLAGGED))
def test_full_pass_unions_hold_more_flagged_tracts_than_a_pass(ns):
    e = E.full_pass_union(ns)
    w = E.restated_union(f"full-{ns}")
    flagged = w["n_len"].max(axis=1) > E.UT_SLOTS
    assert flagged.sum() == E.FULL_FLAGGED[ns] and [n for n, f in zip(e.names, flagged) if not f] == [n for n in e.names if "small" in n]
    assert (e.tracts["n_rows"][flagged] == E.UT_SLOTS + 1).all() and (w["n_len"].max(axis=1)[flagged] == E.UT_SLOTS + 1).all()
    passes = {64: 2, 1: 1}[ns]
    assert flagged.sum() > passes * E.full_pass(ns) and len(e.keys) < 20000
    where = np.flatnonzero(flagged)
    assert (np.diff(where) > 1).sum() >= {64: 39, 1: 100}[ns]              # unflagged tracts between them
    lengths = signed_length(e.keys[:, 2])
    for name, n_len, is_flagged in (("flagged-ends", 17, True), ("ends-small", 2, False)):
        t = e.names.index(name)
        own = lengths[e.tract_ids == t]
        assert own.max() == E.LEN_MAX == 511 and own.min() == E.LEN_MIN == -512 and len(own) == n_len and flagged[t] == is_flagged
        assert (w["n_len"][t].max() == n_len) and (w["modal_len"][t] != 0).all()
    # the list of the *_sample_stats calls
    n_list = {64: 100, 1: 1300}[ns]
    lst = E.listed(len(e.tracts), n_list)
    assert len(lst) == n_list > E.full_pass(ns) and flagged[lst].sum() > E.full_pass(ns) and 0 < (~flagged[lst]).sum()
    assert len(set(lst.tolist())) < n_list and lst[0] == lst[-1] and (np.diff(lst) < 0).sum() > n_list // 4
    assert 0 <= lst.min() and lst.max() < len(e.tracts)


def test_wide_sums_and_ties_are_what_they_say():
    e = E.wide_sums_and_ties()
    w6, w5 = E.restated_union("sums-ties"), E.restated_tracts("sums-ties")
    mat, lengths = e.mat.astype(np.int64), signed_length(e.keys[:, 2])
    B = (1 << 31) - 1
    for name in ("big-two-contexts", "big-one-context"):
        rows = e.tract_ids == e.names.index(name)
        assert (mat[rows].sum(axis=0) > 1 << 32).all()                         # every sample's sum needs 64 bits
        assert (np.abs(mat[rows] * lengths[rows][:, None]).max(axis=0) > 1 << 32).all()   # and so does count * length
    t = e.names.index("big-two-contexts")
    rows = np.flatnonzero(e.tract_ids == t)
    top = rows[lengths[rows] == E.LEN_MAX]
    assert len(top) == 2 and mat[top, 0].tolist() == [B, B] and mat[top, 0].sum() == (1 << 32) - 2    # one bar of N6 above 32 bits
    assert w6["n_len"][t].tolist() == [2, 3, 3] and w6["n_context"][t].tolist() == [2, 2, 2] and w6["modal_len"][t, 0] == E.LEN_MAX
    assert w6["values"][t, MODAL, 0] == ((1 << 32) - 2) / (3 * B) and w5["values"][t, MODAL, 0] == B / (3 * B)
    assert np.isfinite(w6["values"]).all() and np.isfinite(w5["values"]).all()
    for name, n in (("tie-16", 16), ("tie-17", 17)):
        t = e.names.index(name)
        rows = e.tract_ids == t
        assert (mat[rows] == [5, 7, 9]).all() and (w6["n_len"][t] == n).all() and lengths[rows].max() == 40 and (w6["modal_len"][t] == 40).all()
        assert (w6["reldiff"][t][list(RULE)] == 0).all() and (w6["values"][t, MODAL] == 1 / n).all()
    t = e.names.index("tie-pairs-17")
    rows = np.flatnonzero(e.tract_ids == t)
    assert (np.diff(mat[rows], axis=0) >= 0).all() and (np.diff(lengths[rows]) == -1).all()
    assert w6["modal_len"][t].tolist() == [int(lengths[rows[-1]])] * 2 + [int(lengths[rows[-2]])]    # sample 2: the last two rows tie, the larger length
    for name, sign in (("rising", 1), ("falling", -1)):
        rows = np.flatnonzero(e.tract_ids == e.names.index(name))
        assert len(rows) == 12 and (np.sign(np.diff(mat[rows], axis=0)) == sign).all() and (np.diff(lengths[rows]) == -1).all()
    # the values do not depend on the order of a tract's rows: the same union with every tract's rows reversed
    back = np.concatenate([np.flatnonzero(e.tract_ids == t)[::-1] for t in range(len(e.tracts))])
    again = restate_union_tract_stats(e.keys[back], e.mat[back], e.coverage, e.tract_ids, e.lev_distance)
    for t in [e.names.index(n) for n in e.names if "two-contexts" not in n]:       # (reversing a tract of two contexts keeps them contiguous too)
        assert (again["values"][t] == w6["values"][t]).all() and (again["modal_len"][t] == w6["modal_len"][t]).all()
    assert (again["values"] == w6["values"]).all()


@pytest.mark.parametrize("which", list(E.ZERO_COVERAGE))
def test_a_coverage_of_zero_gives_inf_where_it_says(which):
    """integral / 0.0 is inf; relative_difference_of_vector keeps x_min at FLT_MAX where every value is inf and gives
    inf - FLT_MAX = inf: no NaN comes out of the reference's comparisons, and none may come out of the device's"""
    zero = list(E.ZERO_COVERAGE[which])
    e = E.zero_coverage(which)
    base = E.restated_union("slots-3")
    assert [c == 0 for c in e.coverage] == [s in zero for s in range(3)] and (e.mat == E.slot_edge(3).mat).all()
    for w in (E.restated_union(f"cov0-{which}"), E.restated_tracts(f"cov0-{which}")):
        present = w["n_context"] > 0
        inf = np.isinf(w["values"])
        want_inf = np.zeros_like(inf)
        want_inf[:, PROP, zero] = present[:, zero]
        assert (inf == want_inf).all() and not np.isnan(w["values"]).any() and not np.isnan(w["reldiff"]).any()
        assert (np.isinf(w["reldiff"][:, PROP]) == present[:, zero].any(axis=1)).all() and not np.isinf(np.delete(w["reldiff"], PROP, axis=1)).any()
        assert np.isinf(w["reldiff"][:, PROP]).sum() > 10 and (w["values"][inf] > 0).all()
        assert np.isfinite(w["difference"]).all()
    w = E.restated_union(f"cov0-{which}")
    assert (w["variable"] == base["variable"]).all() and (w["selected"] == base["selected"]).all()
    rest = np.delete(np.arange(5), PROP)
    assert (w["values"][:, rest] == base["values"][:, rest]).all()


@pytest.mark.parametrize("name", list(E.CASES))
def test_row_order_summation_stays_inside_the_tolerance(name):
    """N5 sums a sample's bars in union row order, the restatement in the reference's order (count descending).  On every
    union of the corpus the two orders differ by less than a quarter of what the shared checks allow (rtol and atol
    1e-12), so no case needs a tolerance of its own; on the threshold union they do not differ at all (two bars, or
    three of which the first two swap: the same sum)."""
    e = E.case(name)
    w = E.restated_tracts(name)
    lengths, cols = signed_length(e.keys[:, 2]).tolist(), e.mat.astype(np.int64)
    worst = 0.0
    for t in range(len(e.tracts)):
        lo, hi = int(e.tracts["first"][t]), int(e.tracts["first"][t] + e.tracts["n_rows"][t])
        for s in range(e.mat.shape[1]):
            bars = [(lengths[r], int(cols[r, s])) for r in range(lo, hi) if cols[r, s]]
            if not bars:
                continue
            avg, ent = E.row_order_sums(bars)
            for j, v in ((AVG, avg), (ENT, ent)):
                want = w["values"][t, j, s]
                worst = max(worst, abs(v - want) / (1e-12 + 1e-12 * abs(want)))
    assert worst < 0.25, worst
    if name.startswith("thresholds"):
        assert worst == 0.0
