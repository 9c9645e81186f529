"""tjamd_tract_stats / tjamd_tract_sample_stats (N5) and tjamd_union_tract_stats / tjamd_union_tract_sample_stats (N6) on the
GPU, on the edge corpus of tests/stat_edges.py, against the numpy restatements: the thresholds of `variable` and `selected`,
the 16 LDS bar slots and the FULL kernels behind them, sums beyond 32 bits, tied bars and a coverage of 0.  Every call goes
through tests/bounds_calls.py, so every output sits between guards; the comparisons are those of tests/test_tract_stats.py
and tests/test_union_tracts.py, at their tolerances.  tests/test_stat_edges.py shows on the CPU that each union holds the
edge it is named for."""
import numpy as np
import pytest

import tatajuba_amd as tj
from tests import bounds_calls as bc
from tests import stat_edges as E
from tests.test_tract_stats import check_against_restatement
from tests.test_union_tracts import check_stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(10)
    yield c
    c.close()


def _ref(name, ref):
    r = E.reference_lengths(name, ref)
    return None if r is None else bc.dev(r, np.int32)


def union_stats(counter, name, ref=None):
    """N6 on a case of the corpus, the tracts as the case gives them -> (Union, dict for check_stats)"""
    e = E.case(name)
    u = bc.Union(e.keys, e.mat, e.coverage)
    return u, bc.union_stats_of(counter, u, bc.dev(e.tracts), len(e.tracts), ref=_ref(name, ref))


def tract_stats(counter, name, ref=None, context_keyed=False):
    """N5 on a case, with the case's tract ids or the context-keyed ones -> (Union, dict for check_against_restatement)"""
    e = E.case(name)
    u = bc.Union(e.keys, e.mat, e.coverage)
    nt, got = bc.tract_stats_of(counter, u, len(e.tracts), ids=None if context_keyed else bc.dev(e.tract_ids, np.int32), ref=_ref(name, ref))
    assert nt == len(e.tracts), got
    return u, got


def check_both(counter, name, ref=None):
    _, got6 = union_stats(counter, name, ref)
    check_stats(got6, E.restated_union(name, ref))
    _, got5 = tract_stats(counter, name, ref)
    assert check_against_restatement(got5, E.restated_tracts(name, ref)) == 0
    return got5, got6


@pytest.mark.parametrize("run", list(E.THRESHOLD_RUNS))
def test_thresholds(counter, run):
    """both rules on either side of their constants, by each term alone and by the sum alone; with reference lengths on
    and off the modal length; with lev_distance 1 where nothing else selects"""
    name, ref = E.THRESHOLD_RUNS[run]
    got5, got6 = check_both(counter, name, ref)
    _, ctx = tract_stats(counter, name, ref, context_keyed=True)         # one context per tract: tjamd_tract_ids' tracts are these
    assert check_against_restatement(ctx, E.restated_tracts(name, ref, context_keyed=True)) == 0
    what = list(E.THRESHOLDS.values())
    s = got6["summary"]
    if run == "plain":
        assert s["selected"].tolist() == [w["selected"] for _, w in what] and s["variable"].tolist() == [w["variable"] for _, w in what]
        assert got5["summary"]["variable"].tolist() == s["variable"].tolist() == ctx["summary"]["variable"].tolist()
        assert got6["selected"].tolist() == [0, 2, 4, 5, 6, 7, 8] and got6["variable"].tolist() == [5, 7, 8]
    elif run == "lev":
        assert (s["selected"] == 1).all() and s["variable"].tolist() == [w["variable"] for _, w in what]
    elif run == "ref-off":
        assert (s["variable"] == 1).all() and (got5["summary"]["variable"] == 1).all()


@pytest.mark.parametrize("ns", E.SLOT_NS)
def test_slot_edge(counter, ns):
    """15, 16 and 17 lengths in the widest sample, which is sample 0, the last, every one, or (130 samples) one that a lane
    reaches on its second or third round; two contexts sharing 16 lengths, and 9 + 9"""
    name = f"slots-{ns}"
    _, got6 = check_both(counter, name)
    e, want = E.case(name), E.restated_union(name)
    t = e.names.index("shared-9+9")
    assert got6["n_len"][t].tolist() == [18] * ns and got6["n_context"][t].tolist() == [2] * ns
    assert int(got6["n_len"].max()) == 18 and (got6["n_len"].max(axis=1) == want["n_len"].max(axis=1)).all()
    check_both(counter, name, "off")


def listed_like(want, lst):
    """a restatement's tracts as a caller's list names them: what the shared checks hold a listed call against"""
    return {f: v[lst] for f, v in want.items()}


@pytest.mark.parametrize("ns", list(E.FULL_FLAGGED))
def test_full_pass(counter, ns):
    """more flagged tracts than the FULL kernels hold in one pass of their grid (two passes at 64 samples), the lengths
    -512 and 511 on both paths; then the listed entries on a list that repeats tracts, is out of order, mixes flagged and
    unflagged tracts and is longer than a pass, once with every optional output and once with none"""
    name = f"full-{ns}"
    e = E.case(name)
    u, got6 = union_stats(counter, name)
    want6 = E.restated_union(name)
    check_stats(got6, want6)
    u5, got5 = tract_stats(counter, name)
    want5 = E.restated_tracts(name)
    assert check_against_restatement(got5, want5) == 0
    assert got6["n_len"][e.names.index("flagged-ends")].max() == E.UT_SLOTS + 1 and (got6["n_len"][e.names.index("ends-small")] == 2).all()
    nt = len(e.tracts)
    lst = E.listed(nt, {64: 100, 1: 1300}[ns])
    ld, n_list = bc.dev(lst, np.int32), len(lst)
    # N6
    summary = got6["raw"][0]["d_summary"].payload
    v = bc.call_union_tract_sample_stats(counter, u, summary, nt, ld)
    assert v.rc == n_list, v.err
    per = lambda r, f: r[f].view(np.int32).reshape(n_list, ns)
    listed = {"summary": got6["summary"][lst], "values": v["d_values"].view(np.float64).reshape(n_list, bc.N_STATS, ns),
              "modal_len": per(v, "d_modal_len"), "n_context": per(v, "d_n_context"), "n_len": per(v, "d_n_len")}
    listed["variable"], listed["selected"] = np.flatnonzero(listed["summary"]["variable"]), np.flatnonzero(listed["summary"]["selected"])
    check_stats(listed, listed_like(want6, lst))
    assert listed["values"].tobytes() == got6["values"][lst].tobytes()         # an entry's values do not depend on its place in the list
    bare = bc.call_union_tract_sample_stats(counter, u, summary, nt, ld, null=("d_modal_len", "d_n_context", "d_n_len"))
    assert bare.rc == n_list and bare.bytes_of("d_values") == v.bytes_of("d_values")
    # N5
    summary5 = got5["raw"][0]["d_summary"].payload
    v5 = bc.call_tract_sample_stats(counter, u5, summary5, nt, ld)
    assert v5.rc == n_list, v5.err
    listed5 = {"summary": got5["summary"][lst], "values": v5["d_values"].view(np.float64).reshape(n_list, bc.N_STATS, ns),
               "modal_len": per(v5, "d_modal_len"), "n_context": per(v5, "d_n_context")}
    listed5["variable"] = np.flatnonzero(listed5["summary"]["variable"])
    assert check_against_restatement(listed5, listed_like(want5, lst)) == 0
    bare5 = bc.call_tract_sample_stats(counter, u5, summary5, nt, ld, null=("d_modal_len", "d_n_context"))
    assert bare5.rc == n_list and bare5.bytes_of("d_values") == v5.bytes_of("d_values")


def test_wide_sums_and_ties(counter):
    """sums and count * length beyond 32 bits, one bar of 2^32 - 2; 16 and 17 tied bars (the largest length is modal, in
    LDS and in the FULL kernel); counts rising and falling against the order of the rows"""
    got5, got6 = check_both(counter, "sums-ties")
    e = E.case("sums-ties")
    t = e.names.index("big-two-contexts")
    assert got6["values"][t, 1, 0] == ((1 << 32) - 2) / (3 * ((1 << 31) - 1)) and got6["modal_len"][t, 0] == E.LEN_MAX
    for name in ("tie-16", "tie-17"):
        assert got6["modal_len"][e.names.index(name)].tolist() == [40] * 3 == got5["modal_len"][e.names.index(name)].tolist()
    check_both(counter, "sums-ties", "modal")


def check_with_infinities(got, want, union):
    """check_stats / check_against_restatement where the restatement holds inf or NaN (which allclose refuses): the same
    fields, inf and NaN exactly where the restatement has them (inf with its sign), everything finite within rtol and atol
    1e-12; variable and selected as the restatement says"""
    s = got["summary"]
    for f in ("first", "n_rows", "n_present", "variable") + (("lev_distance", "selected") if union else ()):
        assert (s[f] == want[f]).all(), f
    for g, w in ((s["reldiff"], want["reldiff"]), (got["values"], want["values"])):
        assert (np.isnan(g) == np.isnan(w)).all() and (np.isinf(g) == np.isinf(w)).all()
        inf, fin = np.isinf(w), np.isfinite(w)
        assert (g[inf] == w[inf]).all() and np.allclose(g[fin], w[fin], rtol=1e-12, atol=1e-12)
    for f in ("modal_len", "n_context") + (("n_len",) if union else ()):
        assert (got[f] == want[f]).all(), f
    assert (np.abs(want["difference"] - 1e-5) > 1e-9).all()
    assert list(got["variable"]) == list(np.flatnonzero(want["variable"]))
    if union:
        assert list(got["selected"]) == list(np.flatnonzero(want["selected"]))
    return int(np.isinf(want["values"]).sum()), int(np.isinf(want["reldiff"]).sum())


@pytest.mark.parametrize("which", list(E.ZERO_COVERAGE))
def test_a_coverage_of_zero(counter, which):
    """the coverage of one sample, and of all three, is 0: the proportional coverage of a sample that has the tract is inf,
    and so is its relative difference; nothing else changes, neither list among it"""
    name = f"cov0-{which}"
    n_tracts, n_zero = len(E.case(name).tracts), len(E.ZERO_COVERAGE[which])
    _, got6 = union_stats(counter, name)
    n_inf, n_rd = check_with_infinities(got6, E.restated_union(name), union=True)
    assert n_inf == n_tracts * n_zero and n_rd == n_tracts            # (every sample has every tract of slot_edge (3))
    _, got5 = tract_stats(counter, name)
    n_inf, n_rd = check_with_infinities(got5, E.restated_tracts(name), union=False)
    assert n_inf == n_tracts * n_zero and n_rd == n_tracts
    base = E.restated_union("slots-3")
    assert (got6["summary"]["variable"] == base["variable"]).all() and (got6["summary"]["selected"] == base["selected"]).all()
