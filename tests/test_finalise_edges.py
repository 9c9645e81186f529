"""The per-sample finalise of the device -- the aggregation (aggregate1/2/4_kernel) and the ordering step (bin partition,
bin_sort_index_kernel, context index, coverage table, radix fallback) -- against the CPU oracle on the finalise corpus
(tests/finalise_edges.py), whose streams sit where the kernels' arithmetic changes: tests/test_finalise_edges_corpus.py shows
on the CPU that each of them does, and so which path a sample takes.

Integer work, no tolerances: status, all 40 bytes of every kept element, both index arrays, n_idx and the coverage equal
the oracle's, the records per hash bucket equal the restated hash, and a second run on a fresh counter gives the same bytes
(which keys a closing table admits is a race; the result must not be one).  Every corpus runs under remove_biased 0 and 1 and
min_coverage 0 and its own threshold, and under every ordering path: the default, TATAJUBA_AMD_NO_FUSED_BINS,
TATAJUBA_AMD_NO_PLAN, and TATAJUBA_AMD_PLAN_CAP at one below, at and one above the oracle's kept count.  The corpora of tens of
megabytes (finalise_edges.BIG) keep a kept set of a dozen records: they take the four filters on the default path and the
other paths under their own filter.  Nothing in this file skips."""
import numpy as np
import pytest

import tatajuba_amd as tj
from tests import finalise_edges as F

pytestmark = pytest.mark.gpu

PATHS = ("default", "nofused", "noplan", "cap-1", "cap", "cap+1")
# The zero_key corpora (the reduction key whose one-word record is 0: aggregate1_kernel takes it for an empty table slot and
# loses the tract -- the device keeps 302 records where the oracle keeps 303, at k = 2 and at k = 12, on every ordering path)
# are not run here: see DEVICE_EXCLUDED in the module docstring of tests/finalise_edges.py.
NAMES = [n for n in F.names() if n not in F.DEVICE_EXCLUDED]
TWO_CALLS = ("one_bucket-k10-2MAX+1", "one_bucket-k31-MAX+1", "bin_staircase-k20-top256-ends", "bin_staircase-k10-top257-alone",
             "kept_counts-k2-n12289", "kept_counts-k6-n513", "kept_exactly_full-k31-n20001", "coverage_pools-k32")


def set_path(monkeypatch, path, n1):
    """the ordering path of the next finalise (read from the environment when it is queued).  Returns False when the path needs a
    kept count and the sample has none"""
    for name in ("TATAJUBA_AMD_NO_FUSED_BINS", "TATAJUBA_AMD_NO_PLAN", "TATAJUBA_AMD_PLAN_CAP"):
        monkeypatch.delenv(name, raising=False)
    if path == "nofused":
        monkeypatch.setenv("TATAJUBA_AMD_NO_FUSED_BINS", "1")
    elif path == "noplan":
        monkeypatch.setenv("TATAJUBA_AMD_NO_PLAN", "1")
    elif path.startswith("cap"):
        if n1 is None:
            return False
        monkeypatch.setenv("TATAJUBA_AMD_PLAN_CAP", str(max(1, n1 + {"cap-1": -1, "cap": 0, "cap+1": 1}[path])))
    return True


def fill(c, name, ref, what):
    """the corpus into a counter by its route; the records per hash bucket are those of the restated hash"""
    corpus = F.get(name)
    if corpus.route == "upload":
        c.upload_raw(ref["raw"])
    else:
        for p in F.parts_of(name):
            c.scan_host(p, F.M)
    assert c.raw_count() == ref["n_raw"], (what, c.raw_count(), ref["n_raw"])
    assert (c.bucket_counts().astype(np.int64) == F.bucket_counts(corpus.k, corpus.keys)).all(), what + ": records per hash bucket"


def finalised(c, f, two_calls):
    if two_calls:
        c.finalise_begin(*f)
        st = c.finalise_end()
    else:
        st = c.finalise(*f)
    out = {"status": st, "n": 0, "kept": b"", "idx": (np.zeros(0, np.int32), np.zeros(0, np.int32)), "n_idx": 0, "coverage": 0}
    if st == 0:
        out.update(n=c.n_kept, kept=c.download_kept().tobytes(), idx=c.download_idx(), n_idx=c.n_idx, coverage=c.coverage)
    assert c.plan_mismatches() == 0
    return out


def compare(got, exp, what):
    assert got["status"] == exp["status"], (what, "status", got["status"], exp["status"])
    if exp["status"] != 0:
        return
    assert got["n"] == exp["n"], (what, "kept records", got["n"], exp["n"])
    if got["kept"] != exp["kept"]:
        g, e = (np.frombuffer(x["kept"], tj.ELEM_DTYPE) for x in (got, exp))
        bad = np.nonzero(g != e)[0]
        raise AssertionError("%s: %d of %d kept elements differ, first at %d: got %s, expected %s" % (what, bad.size, len(e), bad[0], g[bad[0]], e[bad[0]]))
    assert got["n_idx"] == exp["n_idx"], (what, "n_idx", got["n_idx"], exp["n_idx"])
    assert (got["idx"][0] == exp["idx"][0]).all() and (got["idx"][1] == exp["idx"][1]).all(), what + ": index ranges"
    assert got["coverage"] == exp["coverage"], (what, "coverage", got["coverage"], exp["coverage"])


def check_corpus(monkeypatch, name, path, filters=None, two_calls=False, counter=None):
    """the helper beside test_gpu_parity.check_finalise: one corpus, one ordering path, every filter, twice (or once on the
    counter given).  On the default path every filter gets a fresh pair of counters; on the others one fresh pair serves the
    test's filters one after the other, so that the whole file creates some two thousand counters, not five thousand."""
    corpus = F.get(name)
    filters = F.filters_of(corpus) if filters is None else filters
    ref = F.reference(name, sorted(set(filters) | {(f[0], 0) for f in filters}))
    ran, pair = 0, []
    for f in filters:
        if not set_path(monkeypatch, path, ref["n1"].get(f[0])):
            continue
        what = "%s %s filter=%s%s" % (name, path, f, " (two calls)" if two_calls else "")
        first = None
        if counter is None and (path == "default" or not pair):
            for c in pair:
                c.close()
            pair = [tj.Counter(corpus.k), tj.Counter(corpus.k)]
        for run in range(1 if counter is not None else 2):
            c = counter if counter is not None else pair[run]
            fill(c, name, ref, what)
            got = finalised(c, f, two_calls)
            compare(got, ref["fin"][f], what + " run %d" % run)
            if first is not None:
                assert (got["kept"], got["n_idx"], got["coverage"]) == (first["kept"], first["n_idx"], first["coverage"]), what + ": two runs differ"
                assert (got["idx"][0] == first["idx"][0]).all() and (got["idx"][1] == first["idx"][1]).all(), what + ": two runs differ"
            first = got
        ran += 1
    for c in pair:
        c.close()
    return ran


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", [n for n in NAMES if not F.is_big(n)])
def test_finalise_on_the_edge_corpus(monkeypatch, name, path):
    assert check_corpus(monkeypatch, name, path) == 4


@pytest.mark.parametrize("name", [n for n in NAMES if F.is_big(n)])
def test_finalise_on_the_big_corpora(monkeypatch, name):
    corpus = F.get(name)
    assert check_corpus(monkeypatch, name, "default") == 4
    for path in PATHS[1:]:
        assert check_corpus(monkeypatch, name, path, [(1, corpus.min_coverage)]) == 1
    F.release(name)


@pytest.mark.parametrize("path", ["default", "cap", "noplan"])
@pytest.mark.parametrize("name", TWO_CALLS)
def test_finalise_begin_and_end_on_the_edge_corpus(monkeypatch, name, path):
    corpus = F.get(name)
    assert check_corpus(monkeypatch, name, path, [(0, 0), (1, corpus.min_coverage)], two_calls=True) == 2


def test_one_counter_through_fallback_small_three_rounds_nothing_kept_and_small_again(monkeypatch):
    """what a finalise leaves in the counter -- the fine bins, the zeroed bins, the sort_fallback flag, the second pool -- must
    not reach the next sample: a staircase that falls back to the radix sort, a small kept set, a bucket of three rounds, a sample
    of which nothing is kept (status 2), and the small kept set again, on one counter and on every ordering path"""
    seq = ["bin_staircase-k10-top257-alone", "kept_counts-k10-n3073", "one_bucket-k10-2MAX+1", "bucket_sizes-k10-1", "kept_counts-k10-n3073",
           "bin_staircase-k10-top256-alone"]
    assert F.reference("bucket_sizes-k10-1", [(0, 0)])["fin"][(0, 0)]["status"] == 2
    for path in PATHS:
        c = tj.Counter(10)
        for name in seq:
            f = (0, 0) if name.startswith("bucket_sizes") else (1, F.get(name).min_coverage)
            assert check_corpus(monkeypatch, name, path, [f], counter=c) == 1
        c.close()


def test_one_counter_through_every_outcome_of_begin_and_end(monkeypatch):
    """tjamd_finalise_begin / tjamd_finalise_end on one counter through status 0, status 2 (nothing kept) and status 3 (no
    context deep enough), with the small kept set again at the end: the same bytes as the first time, so nothing of the two in
    between is left in the counter.  An end without a begin raises, before the first begin and after an end.  On the planned
    paths the end waits for the event of the begin; without the plan the begin has waited for the stream and the end has
    nothing left to wait for."""
    small, nothing = "kept_counts-k10-n3073", "bucket_sizes-k10-1"
    own = (1, F.get(small).min_coverage)
    # (3073 keys, each read twice: the depths of all contexts together are 6146, so none of them reaches 6147)
    unreached = (1, 2 * 3073 + 1)
    assert F.reference(nothing, [(0, 0)])["fin"][(0, 0)]["status"] == 2
    assert F.reference(small, [unreached])["fin"][unreached]["status"] == 3
    ref = {small: F.reference(small, [own, unreached, (1, 0)]), nothing: F.reference(nothing, [(0, 0)])}

    def step(c, path, name, f):
        what = "%s %s filter=%s (two calls, one counter)" % (name, path, f)
        assert set_path(monkeypatch, path, ref[name]["n1"].get(f[0]))
        fill(c, name, ref[name], what)
        got = finalised(c, f, True)
        compare(got, ref[name]["fin"][f], what)
        return got

    for path in ("default", "noplan", "cap"):
        c = tj.Counter(10)
        with pytest.raises(tj.TatajubaAmdError, match="without tjamd_finalise_begin"):
            c.finalise_end()
        first = step(c, path, small, own)
        assert first["status"] == 0
        with pytest.raises(tj.TatajubaAmdError, match="without tjamd_finalise_begin"):
            c.finalise_end()
        assert step(c, path, nothing, (0, 0))["status"] == 2
        assert step(c, path, small, unreached)["status"] == 3
        again = step(c, path, small, own)
        assert (again["status"], again["kept"], again["n_idx"], again["coverage"]) == (0, first["kept"], first["n_idx"], first["coverage"]), path
        assert (again["idx"][0] == first["idx"][0]).all() and (again["idx"][1] == first["idx"][1]).all(), path
        assert c.plan_mismatches() == 0
        c.close()
