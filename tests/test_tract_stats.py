"""tjamd_tract_stats / tjamd_tract_sample_stats on the GPU against the numpy restatement of the reference's formulas
(tests/test_tract_stats_cabi.py: src/genome_set.c:692-710,738-779): hand-built unions with no scan, the eight-sample
pipeline scan -> finalise -> gather -> merge -> stats, and examples/variable_tracts.c."""
import ctypes as C
import os

import numpy as np
import pytest

import tatajuba_amd as tj
from oracle import orc
from tests.test_tract_stats_cabi import N_STATS, record, restate_tract_stats, tsv_field

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAP = 3, 4
# caller ids of five rows that tjamd_tract_stats refuses (they must start at 0 and go up by 0 or 1); tests/test_buffer_bounds.py sends them too
BAD_TRACT_IDS = ([1, 1, 1, 2, 2], [0, 2, 2, 2, 2], [0, 1, 0, 1, 1], [0, 0, -1, -1, 0], [0, 1, 2, 3, 5], [-1, 0, 0, 1, 1], [-1, -1, 0, 0, 1], [-1] * 5)


def _torch():
    return pytest.importorskip("torch")


def device_stats(counter, keys, mat, coverage, tract_ids=None, ref_length=None, capacity=None, on_device=False):
    """both calls, per-sample values for EVERY tract (list = 0 .. n_tracts-1).  keys / mat: numpy or CUDA tensors."""
    torch = _torch()
    L = tj.lib()
    dev = torch.device("cuda", 0)
    t = lambda a, dt: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    kd = t(np.asarray(keys, np.uint64), np.uint8) if not on_device else keys
    md = t(np.asarray(mat, np.int32), np.int32) if not on_device else mat
    nu, ns = int(md.shape[0]), int(md.shape[1])
    ids = t(np.asarray(tract_ids, np.int32), np.int32) if tract_ids is not None else None
    ref = t(np.asarray(ref_length, np.int32), np.int32) if ref_length is not None else None
    cap = nu if capacity is None else capacity
    summ = torch.zeros(max(cap, 1) * 56, dtype=torch.uint8, device=dev)
    var = torch.full((max(cap, 1),), -1, dtype=torch.int32, device=dev)
    cov = (C.c_int * ns)(*[int(x) for x in coverage])
    nv = C.c_long(-1)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    torch.cuda.synchronize()
    nt = L.tjamd_tract_stats(counter._h, p(kd), p(md), nu, ns, p(ids), cov, p(ref), p(summ), p(var), cap, C.byref(nv))
    if nt < 0:
        return nt, L.tjamd_last_error().decode()
    lst = torch.arange(max(nt, 1), dtype=torch.int32, device=dev)
    vals = torch.full((max(nt, 1), N_STATS, ns), -7.0, dtype=torch.float64, device=dev)
    ml = torch.full((max(nt, 1), ns), -7, dtype=torch.int32, device=dev)
    nc = torch.full((max(nt, 1), ns), -7, dtype=torch.int32, device=dev)
    got = L.tjamd_tract_sample_stats(counter._h, p(kd), p(md), nu, ns, cov, p(summ), nt, p(lst), nt, p(vals), p(ml), p(nc))
    assert got == nt, L.tjamd_last_error()
    summary = np.frombuffer(summ[: nt * 56].cpu().numpy().tobytes(), dtype=tj.TRACT_SUMMARY_DTYPE)
    return nt, {"summary": summary, "variable": var[: nv.value].cpu().numpy(), "values": vals[:nt].cpu().numpy(),
                "modal_len": ml[:nt].cpu().numpy(), "n_context": nc[:nt].cpu().numpy()}


def check_against_restatement(got, want):
    s = got["summary"]
    assert list(s["first"]) == list(want["first"]) and list(s["n_rows"]) == list(want["n_rows"])
    assert list(s["n_present"]) == list(want["n_present"])
    assert np.allclose(s["reldiff"], want["reldiff"], rtol=1e-12, atol=1e-12)
    assert np.allclose(got["values"], want["values"], rtol=1e-12, atol=1e-12)
    assert (got["modal_len"] == want["modal_len"]).all() and (got["n_context"] == want["n_context"]).all()
    near = np.abs(want["difference"] - 1e-5) <= 1e-9                    # too close to the threshold to ask for the same side
    assert (s["variable"][~near] == want["variable"][~near]).all()
    assert list(got["variable"]) == [i for i in range(len(s)) if s["variable"][i]]
    return int(near.sum())


def union_of(tracts):
    """tracts: list of (base, ctx0, ctx1, [(length, [count per sample]), ...]) -> keys, mat"""
    keys, mat = [], []
    for base, c0, c1, rows in tracts:
        for length, cnt in rows:
            keys.append(record(base, c0, c1, length))
            mat.append(cnt)
    return np.array(keys, np.uint64), np.array(mat, np.int32)


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(10)
    yield c
    c.close()


def test_hand_built_unions(counter):
    tracts = [(1, 0x111, 0x222, [(6, [3, 0]), (5, [1, 0])]),      # 0: absent from sample 1 -> variable
              (1, 0x111, 0x333, [(7, [2, 2]), (6, [5, 5])]),      # 1: identical histograms -> not variable, reldiffs exactly 0
              (0, 0x444, 0x555, [(7, [4, 9])]),                   # 2: one length (entropy exactly 0), modal length 7
              (0, 0x444, 0x666, [(9, [3, 1]), (4, [3, 2])]),      # 3: sample 0 ties 9 / 4 -> 9
              (0, 0x444, 0x777, [(-3, [0, 0])])]                  # 4: present nowhere (n_present 0)
    keys, mat = union_of(tracts)
    cov = [10, 10]
    nt, got = device_stats(counter, keys, mat, cov)
    want = restate_tract_stats(keys, mat, cov)
    assert nt == 5 and check_against_restatement(got, want) == 0
    s = got["summary"]
    assert list(s["variable"]) == [1, 0, 0, 1, 1] and list(got["variable"]) == [0, 3, 4]
    assert s[0]["n_present"] == 1 and not got["values"][0, :, 1].any() and got["modal_len"][0, 1] == 0
    assert (s[1]["reldiff"] == 0.0).all()
    assert got["values"][2, 4, 0] == 0.0 and got["values"][2, 4, 1] == 0.0 and got["values"][2, 0, 1] == 7.0
    assert (s[2]["reldiff"][[0, 1, 4]] == 0.0).all() and s[2]["reldiff"][2] == 0.5 and s[2]["reldiff"][3] == 5.0   # coverages are not in the rule
    assert got["modal_len"][3, 0] == 9 and got["modal_len"][3, 1] == 4
    assert s[4]["n_present"] == 0 and (s[4]["reldiff"] == 0.0).all()
    assert (got["n_context"][:4] == [[1, 0], [1, 1], [1, 1], [1, 1]]).all()
    k2, m2 = union_of([tracts[2]])
    # the reference tract length: equal stats, modal length 7
    for ref, var in [(None, 0), ([8], 1), ([7], 0), ([0], 0), ([-2], 0)]:
        nt, g3 = device_stats(counter, k2, m2, [10, 10], ref_length=ref)
        assert g3["summary"][0]["variable"] == var and list(g3["variable"]) == ([0] if var else []), ref


def test_caller_ids_and_bad_ids(counter):
    tracts = [(1, 0x10, 0x20, [(6, [3, 1]), (5, [1, 1])]),
              (1, 0x10, 0x30, [(6, [2, 0])]),
              (1, 0x11, 0x20, [(4, [0, 5])]),
              (0, 0x10, 0x20, [(8, [1, 1])])]
    keys, mat = union_of(tracts)
    by_base = [0, 0, 0, 0, 1]                                             # one id per base
    cov = [7, 3]
    nt, got = device_stats(counter, keys, mat, cov, tract_ids=by_base)
    want = restate_tract_stats(keys, mat, cov, tract_ids=by_base)
    assert nt == 2 and check_against_restatement(got, want) == 0
    assert list(got["n_context"][0]) == [2, 2]                            # sample 0: (0x10, 0x20), (0x10, 0x30); sample 1: (0x10, 0x20), (0x11, 0x20)
    integral = mat[:4].sum(axis=0)
    assert list(got["values"][0, 3]) == [integral[0] / 2, integral[1] / 2]
    nt, g1 = device_stats(counter, keys, mat, cov)                       # the context-keyed ids: the same as tjamd_tract_ids'
    assert nt == 4 and check_against_restatement(g1, restate_tract_stats(keys, mat, cov)) == 0
    assert (g1["n_context"] <= 1).all()
    assert counter.last_tract_stats_ms() > 0
    for bad in BAD_TRACT_IDS:
        rc, err = device_stats(counter, keys, mat, cov, tract_ids=bad)
        assert rc == -ERR_ARG and "tract ids must start at 0 and go up by 0 or 1" in err, (bad, rc, err)
        assert counter.last_tract_stats_ms() == -1.0                     # a failed call leaves no timing behind
    rc, err = device_stats(counter, keys, mat, cov, capacity=3)          # four context-keyed tracts
    assert rc == -ERR_CAP and "4 tracts, caller capacity 3" in err
    # a listed tract outside [0, n_tracts)
    torch = _torch()
    nt, _ = device_stats(counter, keys, mat, cov)
    kd = torch.from_numpy(keys.view(np.uint8).reshape(-1)).cuda()
    md = torch.from_numpy(mat).cuda()
    summ = torch.zeros(nt * 56, dtype=torch.uint8, device="cuda")
    cv = (C.c_int * 2)(*cov)
    L = tj.lib()
    assert L.tjamd_tract_stats(counter._h, C.c_void_p(kd.data_ptr()), C.c_void_p(md.data_ptr()), len(mat), 2, None, cv, None,
                               C.c_void_p(summ.data_ptr()), None, nt, None) == nt
    lst = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    vals = torch.zeros((2, N_STATS, 2), dtype=torch.float64, device="cuda")
    rc = L.tjamd_tract_sample_stats(counter._h, C.c_void_p(kd.data_ptr()), C.c_void_p(md.data_ptr()), len(mat), 2, cv, C.c_void_p(summ.data_ptr()), nt,
                                    C.c_void_p(lst.data_ptr()), 2, C.c_void_p(vals.data_ptr()), None, None)
    assert rc == -ERR_ARG and b"outside [0, 4)" in L.tjamd_last_error()


@pytest.mark.parametrize("ns", [1, 8, 70])
def test_random_unions_match_the_restatement(counter, ns):
    """n_samples 1, 8 and 70 (more than a wavefront: lanes stride over the samples)"""
    rng = np.random.default_rng(ns)
    tracts = []
    for t in range(600):
        n_len = int(rng.integers(1, 5))
        lens = sorted(rng.choice(np.arange(-4, 40), n_len, replace=False).tolist(), reverse=True)
        rows = []
        for ln in lens:
            cnt = rng.integers(1, 40, ns) * (rng.random(ns) < 0.8)
            if t % 7 == 0:
                cnt[:] = 12                                               # identical in every sample
            rows.append((ln, cnt.tolist()))
        tracts.append((int(rng.integers(0, 2)), int(rng.integers(0, 1 << 40)), t, rows))
    keys, mat = union_of(tracts)
    cov = rng.integers(1, 60, ns).tolist()
    ref = rng.integers(-1, 40, len(tracts))
    for r in (None, ref):
        nt, got = device_stats(counter, keys, mat, cov, ref_length=r)
        want = restate_tract_stats(keys, mat, cov, ref_length=r)
        assert nt == len(tracts) and check_against_restatement(got, want) == 0
        v = got["summary"]["variable"]
        assert 0 < v.sum() < nt


def _oracle_sample(stream, k, m):
    o = orc.Oracle(k)
    o.scan_stream(stream, m)
    o.finalise(1, 5)
    assert o.c.status == 0
    e = o.elems()
    rec = np.zeros(len(e), dtype=tj.RECORD_DTYPE)
    for f in ("ctx0", "ctx1", "meta"):
        rec[f] = e[f]
    cov = o.c.coverage
    o.close()
    return rec, cov


def test_eight_sample_pipeline_matches_the_restatement():
    """8 samples of one genome with per-sample tract-length variants, k = 15, m = 4: scan -> finalise -> gather -> merge ->
    stats on the GPU; the restatement on the oracle's union (orc.merge_samples of the oracle's finalised samples)"""
    torch = _torch()
    from tatajuba_amd.dist import tract_stats_device
    k, m, ns = 15, 4, 8
    counters, orecs, ocov = [], [], []
    for smp in range(ns):
        s = tj.synth_stream(150000, 150, 1000000, seed_reads=0x7A7A1000 + smp, variant_seed=smp)
        c = tj.Counter(k)
        c.scan_host(s, m)
        assert c.finalise(1, 5) == 0
        rec, cov = _oracle_sample(s, k, m)
        kept = c.download_kept()
        assert c.coverage == cov and all((kept[f] == rec[f]).all() for f in ("ctx0", "ctx1", "meta"))
        counters.append(c); orecs.append(rec); ocov.append(cov)
    L = tj.lib()
    hs = (C.c_void_p * ns)(*[c._h for c in counters])
    drec, counts = C.c_void_p(), (C.c_long * ns)()
    merger = tj.Counter(k)
    total = L.tjamd_gather_histograms(merger._h, hs, ns, C.byref(drec), counts)
    assert total == sum(len(r) for r in orecs)
    keys = torch.empty(total * 24, dtype=torch.uint8, device="cuda")
    mat = torch.empty((total, ns), dtype=torch.int32, device="cuda")
    nu = L.tjamd_merge_samples(merger._h, drec, counts, ns, C.c_void_p(keys.data_ptr()), C.c_void_p(mat.data_ptr()), total)
    merge_ms = merger.last_merge_ms()
    _, _, keys_o, mat_o = orc.merge_samples(np.frombuffer(np.concatenate(orecs).tobytes(), np.uint64).reshape(-1, 3), [len(r) for r in orecs])
    assert nu == len(keys_o)
    keys, mat = keys[: nu * 24], mat[:nu]
    want = restate_tract_stats(keys_o, mat_o, ocov)
    nt, got = device_stats(merger, keys, mat, ocov, on_device=True)
    stats_ms = merger.last_tract_stats_ms()
    assert nt == len(want["first"])
    assert check_against_restatement(got, want) == 0
    var = got["summary"]["variable"]
    assert 0 < var.sum() < nt
    assert list(got["variable"]) == list(np.flatnonzero(want["variable"]))
    # the torch-side helper: the variable tracts' per-sample values, and a second call is bitwise identical
    a = tract_stats_device(merger, keys, mat, ocov)
    b = tract_stats_device(merger, keys, mat, ocov)
    assert a["summary"].tobytes() == got["summary"].tobytes() == b["summary"].tobytes()
    assert (a["variable"] == got["variable"]).all() and (a["variable"] == b["variable"]).all()
    assert a["values"].tobytes() == got["values"][a["variable"]].tobytes() == b["values"].tobytes()
    assert (a["modal_len"] == want["modal_len"][a["variable"]]).all() and (a["n_context"] == b["n_context"]).all()
    print(f"\n[tract stats] union {nu} rows x {ns} samples ({nu * (24 + 4 * ns) / 1e6:.2f} MB), {nt} tracts, {int(var.sum())} variable: "
          f"tjamd_last_tract_stats_ms {stats_ms:.3f} ms, tjamd_last_merge_ms {merge_ms:.3f} ms")
    assert stats_ms > 0
    for c in counters + [merger]:
        c.close()


def _compile_example(tmp_path):
    import subprocess
    exe, libdir = str(tmp_path / "variable_tracts"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "variable_tracts.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


TABLES = ["per_sample_average_length.tsv", "per_sample_modal_frequency.tsv", "per_sample_proportional_coverage.tsv"]


def test_variable_tracts_c_example(tmp_path, golden_dir):
    import subprocess
    exe = _compile_example(tmp_path)
    # the same sample twice: nothing varies, three header-only tables
    g = os.path.join(golden_dir, "err1750956.fastq.gz")
    out = tmp_path / "same"
    out.mkdir()
    r = subprocess.run([exe, "-k", "10", "-m", "3", "-c", "5", "-o", str(out), g, g], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("From ") and last.endswith(" tracts, 0 are variable") and int(last.split()[1]) > 0
    for name in TABLES:
        assert (out / name).read_text() == f"tract_id\tlocation\tfeature\treference\t{g}\t{g}\n"
    # two different samples: every printed field against the restatement on the oracle's union
    files, recs, covs = [], [], []
    for smp in range(2):
        s = tj.synth_stream(20000, 150, 100000, seed_reads=0x7A7A1000 + smp, variant_seed=smp + 1)
        reads = bytes(s).split(b"\n")[:-1]
        f = str(tmp_path / f"s{smp}.fq")
        with open(f, "wb") as fh:
            fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rd, b"I" * len(rd)) for i, rd in enumerate(reads)))
        files.append(f)
        rec, cov = _oracle_sample(s, 10, 3)
        recs.append(rec); covs.append(cov)
    out = tmp_path / "two"
    out.mkdir()
    r = subprocess.run([exe, "-k", "10", "-m", "3", "-c", "5", "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    _, _, keys_o, mat_o = orc.merge_samples(np.frombuffer(np.concatenate(recs).tobytes(), np.uint64).reshape(-1, 3), [len(x) for x in recs])
    want = restate_tract_stats(keys_o, mat_o, covs)
    var = np.flatnonzero(want["variable"])
    assert r.stdout.strip().splitlines()[-1] == f"From {len(want['first'])} tracts, {len(var)} are variable"
    assert len(var) > 0
    for j, (name, prec, refcol) in enumerate(zip(TABLES, (2, 2, 5), ("", "1", ""))):
        lines = (out / name).read_text().split("\n")
        assert lines[0] == "tract_id\tlocation\tfeature\treference\t" + "\t".join(files) and lines[-1] == ""
        assert len(lines) - 2 == len(var)
        for line, t in zip(lines[1:-1], var):
            assert line.split("\t") == [f"tid_{t:06d}", "-1", "unannotated", refcol] + [tsv_field(want["values"][t, j, s], prec) for s in range(2)]
