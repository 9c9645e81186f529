"""tjamd_sample_distances on the GPU against the restatement of tests/test_distances_cabi.py, with no difference allowed:
fabricated sites, alleles and genotypes at sample counts on both sides of every tile edge (8, 16, 32, 64) and of every switch
between two edges, at site counts on both sides of every chunk (2048 / edge sites) and of the split of the sites over workgroups, the values at the limits of the
number formats, every refusal raised on the device, the eight-sample pipeline of tests/test_sites.py with N13's and with N12's
genotype matrix, and examples/merged_vcf.c -M.  d_out always sits in a guarded buffer (tests/guarded.py), every input is held
frozen, and every call is made twice and must give the same bytes."""
import os
import subprocess

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, frozen
from tests.test_depths import OUTPUTS, depth_vcf_text, dev_depths, whole_chain
from tests.test_depths_cabi import restate_site_depths
from tests.test_distances_cabi import HAND_EXPECTED, fabricate, hand_case, restate_sample_distances
from tests.test_locate import _dev, _p
from tests.test_locate_cabi import restate_reference_index
from tests.test_sites import dev_merge, pipeline  # noqa: F401  (pipeline: the module-scoped fixture, built here as there)
from tests.test_sites_cabi import merged_vcf_text, restate_merge_variants
from tests.test_variants_cabi import A_ROWS, HAND_GENOME, K, T_ROWS, canonical_row

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 3
DIST = tj.SAMPLE_DISTANCE_DTYPE


def _torch():
    return pytest.importorskip("torch")


def dev_distances(counter, sites, alleles, genotype, ns, one_buffer=False):
    """two calls of tjamd_sample_distances -> the matrix as numpy DIST [ns, ns]; or, when the call is refused, (negative code,
    message, the guarded buffer).  one_buffer: the second call writes where the first did (the largest case)"""
    torch = _torch()
    L = tj.lib()
    n_sites, n_alleles = len(sites), len(alleles)
    pad = lambda a: _dev(a) if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")
    sd, ad, gd = pad(sites), pad(alleles), pad(np.ascontiguousarray(genotype, np.int16))
    runs, buf = [], None
    for _ in range(2):
        if buf is None or not one_buffer:
            buf = GuardedDevice(ns * ns * DIST.itemsize)
        torch.cuda.synchronize()
        with frozen(sd, ad, gd):
            rc = L.tjamd_sample_distances(counter._h, _p(sd), n_sites, _p(ad), n_alleles, _p(gd), ns, buf.c)
            err = L.tjamd_last_error().decode() if rc < 0 else ""
            torch.cuda.synchronize()
        buf.check("d_out")
        if rc < 0:
            assert counter.last_sample_distances_ms() == -1.0 and err.startswith("tjamd_sample_distances")
            return rc, err, buf
        assert rc == n_sites and (n_sites == 0 or counter.last_sample_distances_ms() > 0)
        runs.append(buf.view(DIST).reshape(ns, ns))
    assert runs[0].tobytes() == runs[1].tobytes()                             # two runs: the same bytes
    return runs[0]


def check_distances(got, want):
    assert isinstance(got, np.ndarray), got[:2]
    for f in DIST.names:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, (f, bad[:5], got[f][tuple(bad[0])], want[f][tuple(bad[0])])
    assert got.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def counter():
    c = tj.Counter(15)
    yield c
    c.close()


def _counter_aiming_at(blocks):
    saved = os.environ.get("TATAJUBA_AMD_DISTANCE_BLOCKS")
    os.environ["TATAJUBA_AMD_DISTANCE_BLOCKS"] = str(blocks)
    c = tj.Counter(15)
    if saved is None:
        del os.environ["TATAJUBA_AMD_DISTANCE_BLOCKS"]
    else:
        os.environ["TATAJUBA_AMD_DISTANCE_BLOCKS"] = saved
    return c


@pytest.fixture(scope="module")
def one_block_counter():
    """a counter whose calls aim at one workgroup: beyond 16 samples the tile edge is 64 (any number of tile pairs is enough), and
    the sites are never split: one workgroup per tile pair walks all chunks"""
    c = _counter_aiming_at(1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twelve_block_counter():
    """a counter whose calls aim at twelve workgroups: 130 samples have the 6 tile pairs of edge 64 that this asks for, and two
    slices of the sites: the one way to tiles of edge 64 that are summed from scratch"""
    c = _counter_aiming_at(12)
    yield c
    c.close()


def test_hand_case(counter):
    sites, alleles, genotype = hand_case()
    got = dev_distances(counter, sites, alleles, genotype, 3)
    assert [[tuple(int(v) for v in got[a, b]) for b in range(3)] for a in range(3)] == HAND_EXPECTED
    check_distances(got, restate_sample_distances(sites, alleles, genotype))


# The tile edge is 8 up to 8 samples, 16 up to 16, and beyond that 64 where edge 64 alone gives half the workgroups a call aims
# at (four per CU: from 1 985 samples on; tests/test_the_limit_of_samples) and 32 below; a chunk has 2048 / edge sites: 256, 128,
# 64, 32.  A call splits its sites over workgroups as soon as it has more than one chunk and fewer tile pairs than it aims at:
# one site more than a chunk is the other side of that threshold (two slices, their tiles summed from scratch); 5 000 sites x 5
# samples are 20 slices.  At edge 32, 33 samples are two tile rows, 64 two full ones, 65 three, 130 five with a ragged last
# tile: diagonal and off-diagonal tiles.
@pytest.mark.parametrize("ns,n_sites", [(1, 1), (2, 255), (3, 256), (8, 257), (5, 5000), (9, 127), (16, 128), (16, 129), (17, 63), (32, 64), (32, 65),
                                        (33, 63), (63, 64), (64, 65), (65, 100), (130, 150), (130, 1)])
def test_sample_and_site_counts(counter, ns, n_sites):
    sites, alleles, g = fabricate(n_sites, ns, np.random.RandomState(1000 * ns + n_sites))
    got = dev_distances(counter, sites, alleles, g, ns)
    check_distances(got, restate_sample_distances(sites, alleles, g))
    assert ns * n_sites < 100 or (got["length_diff"] > 0).any()


@pytest.mark.parametrize("ns,n_sites", [(8, 600), (12, 300), (17, 31), (20, 200), (63, 32), (64, 33), (65, 100), (130, 100), (130, 1)])
def test_several_chunks_in_one_workgroup_and_tiles_of_edge_64(one_block_counter, ns, n_sites):
    """edge 64 beyond 16 samples: one, two and three tile rows, chunks of 32 sites; every workgroup walks all chunks of the sites"""
    sites, alleles, g = fabricate(n_sites, ns, np.random.RandomState(7 * ns + n_sites))
    check_distances(dev_distances(one_block_counter, sites, alleles, g, ns), restate_sample_distances(sites, alleles, g))


@pytest.mark.parametrize("ns,n_sites", [(130, 100), (33, 200)])
def test_slices_of_several_chunks(twelve_block_counter, ns, n_sites):
    """130 samples: edge 64, 6 tile pairs x 2 slices of 2 chunks; 33 samples: edge 32, 3 tile pairs x 4 slices of one chunk"""
    sites, alleles, g = fabricate(n_sites, ns, np.random.RandomState(3 * ns + n_sites))
    check_distances(dev_distances(twelve_block_counter, sites, alleles, g, ns), restate_sample_distances(sites, alleles, g))


@pytest.fixture(scope="module")
def default_block_counter():
    """a counter whose calls aim at 1024 workgroups, which is four per CU on the 256 CUs of an MI355X, whatever device runs the test"""
    c = _counter_aiming_at(1024)
    yield c
    c.close()


@pytest.mark.parametrize("ns", [1984, 1985, 4096])
def test_the_limit_of_samples(default_block_counter, ns):
    """4096 samples x 2 sites: the API's limit, 2080 tile pairs of edge 64, 2^24 cells of output.  1 984 samples are 31 tile rows
    of edge 64, 496 tile pairs, fewer than half of the 1024 workgroups aimed at: edge 32 (1 953 tile pairs); 1 985 are 528: edge 64"""
    sites, alleles, g = fabricate(2, ns, np.random.RandomState(4096), n_alleles=[3, 1])
    got = dev_distances(default_block_counter, sites, alleles, g, ns, one_buffer=True)
    check_distances(got, restate_sample_distances(sites, alleles, g))


def test_values(counter):
    """allele counts 1, 2, 9 and one per sample; all-missing sites and samples; alt_length 0 and 1023; lengths at the end of int"""
    ns = 9
    rng = np.random.RandomState(5)
    na = [1, 2, 9, ns] + [1] * 8 + [2, 3]
    n_sites = len(na)
    big = np.array([7, 11, 13, 5] + [2_000_000_000] * 8 + [2_147_483_647, 0])
    sites, alleles, g = fabricate(n_sites, ns, rng, n_alleles=na, ref_length=big)
    g[2] = [1, 2, 3, 4, 5, 6, 7, 8, 9]                                        # every allele of the site with nine
    g[3] = [9, 8, 7, 6, 5, 4, 3, 2, 1]
    g[4:12, 0], g[4:12, 1] = 0, 1                                             # 2 000 000 000 against alt_length 1, eight times: past 2^33
    alleles["alt_length"][sites["first_allele"][4:12]] = 1
    g[12, 0], g[12, 1], g[12, 2] = 0, 1, 2                                    # 2^31 - 1 against 0 and against 1023
    alleles["alt_length"][sites["first_allele"][12]: sites["first_allele"][12] + 2] = [0, 1023]
    g[13, :3] = [0, 1, 3]                                                     # a genome's length of 0 against 1023
    alleles["alt_length"][sites["first_allele"][13]: sites["first_allele"][13] + 3] = [1023, 0, 1023]
    g[1, :] = -1                                                              # a site where nobody is called
    g[:, 7] = -1                                                              # a sample called nowhere
    want = restate_sample_distances(sites, alleles, g)
    assert int(want["length_diff"][0, 1]) > 1 << 33 and all((want[f][7] == 0).all() and (want[f][:, 7] == 0).all() for f in DIST.names)
    check_distances(dev_distances(counter, sites, alleles, g, ns), want)
    # every sample missing everywhere; every cell the reference
    for fill in (-1, 0):
        gg = np.full_like(g, fill)
        got = dev_distances(counter, sites, alleles, gg, ns)
        check_distances(got, restate_sample_distances(sites, alleles, gg))
        assert (got["n_both"] == (0 if fill else n_sites)).all() and (got["n_differ"] == 0).all() and (got["length_diff"] == 0).all()


@pytest.mark.parametrize("ns,n_sites,ref_length", [(70, 40, 2_000_000_000), (4, 300, 2_147_483_647), (70, 40, 1_500_000_000), (20, 200, 400_000_000)])
def test_lengths_that_overflow_32_bits_inside_a_chunk(counter, ns, n_sites, ref_length):
    """the kernel sums length differences in 32 bits and flushes them into 64 before they can overflow, after floor ((2^32 - 1) /
    the chunk's largest length) sites: every 2 sites (2^31 - 1 twice is 2^32 - 2: still 2), every 2 and every 10 -- with threads
    that walk 10, 4, 10 and 16 sites of a chunk"""
    sites, alleles, g = fabricate(n_sites, ns, np.random.RandomState(ns + n_sites), p_missing=0.05, p_ref=0.5, ref_length=ref_length)
    alleles["alt_length"] = np.arange(len(alleles)) % 2                       # 0 or 1 against the genome's length
    want = restate_sample_distances(sites, alleles, g)
    assert int(want["length_diff"].max()) > 1 << 32
    check_distances(dev_distances(counter, sites, alleles, g, ns), want)


def test_zero_sites(counter):
    for ns in (1, 5, 70):
        got = dev_distances(counter, np.zeros(0, tj.SITE_DTYPE), np.zeros(0, tj.ALLELE_DTYPE), np.zeros((0, ns), np.int16), ns)
        assert got.tobytes() == bytes(ns * ns * DIST.itemsize)


def test_device_refusals(counter):
    ns = 6
    sites, alleles, g = fabricate(40, ns, np.random.RandomState(11), n_alleles=[2] * 40)
    want = restate_sample_distances(sites, alleles, g)
    check_distances(dev_distances(counter, sites, alleles, g, ns), want)
    cases = []

    def case(msg, cell=None, **change):
        s, a, gg = sites.copy(), alleles.copy(), g.copy()
        for name, (idx, value) in change.items():
            which, field = name.split("__")
            (s if which == "sites" else a)[field][idx] = value
        if cell:
            gg[cell[0], cell[1]] = cell[2]
        cases.append((msg, s, a, gg))

    case("a genotype cell is below -1 or above its site's n_alleles", cell=(0, 0, -2))
    case("a genotype cell is below -1 or above its site's n_alleles", cell=(39, 5, 3))
    case("a genotype cell is below -1 or above its site's n_alleles", cell=(17, 2, 32767))
    case("do not chain from 0 to 80", sites__first_allele=(0, 1))
    case("do not chain from 0 to 80", sites__first_allele=(20, 41))
    case("do not chain from 0 to 80", sites__n_alleles=(39, 3))
    case("do not chain from 0 to 80", sites__n_alleles=(5, 1 << 30))
    case("a site has n_alleles < 1", sites__n_alleles=(0, 0))
    case("a site has n_alleles < 1", sites__n_alleles=(9, -2))
    case("an allele's site is not the site that holds it", alleles__site=(4, 1))
    case("an allele's site is not the site that holds it", alleles__site=(79, -1))
    case("an allele's site is not the site that holds it", alleles__site=(0, 1 << 30))
    case("an allele's alt_length is outside 0..1023", alleles__alt_length=(3, 1024))
    case("an allele's alt_length is outside 0..1023", alleles__alt_length=(60, -1))
    case("a site's ref_length is below 0", sites__ref_length=(7, -1))
    for msg, s, a, gg in cases:
        with pytest.raises(ValueError):
            restate_sample_distances(s, a, gg)
        rc, err, buf = dev_distances(counter, s, a, gg, ns)
        assert rc == -ERR_ARG and msg in err, (msg, rc, err)
        assert buf.untouched(), msg                                            # nothing was written
        check_distances(dev_distances(counter, sites, alleles, g, ns), want)   # the counter serves the next good call
    # the same with the sites split over workgroups: the summing kernel must not run either
    sites, alleles, g = fabricate(3000, ns, np.random.RandomState(12))
    bad = g.copy()
    bad[2999, 5] = -5
    rc, err, buf = dev_distances(counter, sites, alleles, bad, ns)
    assert rc == -ERR_ARG and "a genotype cell" in err and buf.untouched()
    check_distances(dev_distances(counter, sites, alleles, g, ns), restate_sample_distances(sites, alleles, g))
    # host refusals with real handles; the wrapper
    torch = _torch()
    L = tj.lib()
    sd, ad, gd = _dev(sites), _dev(alleles), _dev(g)
    out = torch.zeros(ns * ns * DIST.itemsize, dtype=torch.uint8, device="cuda")
    assert L.tjamd_sample_distances(counter._h, _p(sd), len(sites), _p(ad), len(alleles), _p(gd), ns, None) == -ERR_ARG
    assert L.tjamd_sample_distances(counter._h, _p(sd), len(sites), _p(ad), len(sites) - 1, _p(gd), ns, _p(out)) == -ERR_ARG
    assert counter.sample_distances(_p(sd), len(sites), _p(ad), len(alleles), _p(gd), ns, _p(out)) == len(sites)
    assert counter.last_sample_distances_ms() > 0
    assert out.cpu().numpy().tobytes() == restate_sample_distances(sites, alleles, g).tobytes()


def test_site_depths_and_sample_distances_refuse_a_broken_allele_chain_alike():
    """one chain rule, two consumers.  Two tracts of the hand genome of tests/test_variants_cabi.py (AAA at 4, TTTTT at 11), each
    with its reference row and one longer row, two samples of which the second has the longer rows: N8, N12 and N13 on the device
    give two sites, two alleles and their genotypes.  That output with sites[1].first_allele off by one, and with
    sites[0].n_alleles = 0, goes through tjamd_site_depths and tjamd_sample_distances: the same clause behind either name, and no
    byte of any output (guarded buffers) is written"""
    ns = 2
    entries, _ = restate_reference_index(HAND_GENOME, K)
    by_flat = {int(e["flat"]): e for e in entries}
    keys, tracts, locs = [], [], []
    for flat, rows in ((4, A_ROWS[:2]), (11, T_ROWS[:2])):
        e = by_flat[flat]
        tracts.append((len(keys), 2, 1, len(keys), 0, 0, 9))
        keys += [canonical_row(*r) for r in rows]
        locs.append((int(e["flat"]), int(e["contig"]), int(e["pos"]), int(e["length"]), 0, int(e["neg_strand"]), 1))
    mat = np.array([[4, 0], [0, 5]] * 2, np.int32)                           # sample 0: the reference rows; sample 1: the longer ones
    c = tj.Counter(K)
    ref = tj.Reference(c, HAND_GENOME)
    u, m, depths, _ = whole_chain(c, ref, np.array(keys, np.uint64), mat, np.array(tracts, tj.UNION_TRACT_DTYPE), np.array(locs, tj.LOCATION_DTYPE), entries, K)
    sites, alleles, g = m["sites"], m["alleles"], depths["genotype"]
    assert len(sites) == 2 and len(alleles) == 2 and g.tolist() == [[0, 1], [0, 1]] and sites["first_allele"].tolist() == [0, 1]
    want = restate_sample_distances(sites, alleles, g)
    check_distances(dev_distances(c, sites, alleles, g, ns), want)
    for msg, field, idx, value in (("first_allele and n_alleles of the sites do not chain from 0 to 2", "first_allele", 1, 2),
                                   ("a site has n_alleles < 1", "n_alleles", 0, 0)):
        bad = sites.copy()
        bad[field][idx] = value
        said = []
        for name, (rc, err, buf) in (("tjamd_site_depths", dev_depths(c, ref, u, bad, alleles)), ("tjamd_sample_distances", dev_distances(c, bad, alleles, g, ns))):
            assert rc == -ERR_ARG and err.startswith(name + ": "), (msg, name, rc, err)
            assert all(b.untouched() for b in (buf.values() if isinstance(buf, dict) else [buf])), (msg, name)
            said.append(err[len(name):])
        assert said[0] == said[1] == ": " + msg, (msg, said)
    assert dev_depths(c, ref, u, sites, alleles)["genotype"].tobytes() == g.tobytes()      # the counter serves the next good calls
    check_distances(dev_distances(c, sites, alleles, g, ns), want)
    ref.close()
    c.close()


# ---- the pipeline ----------------------------------------------------------------------------------------------------------

def test_eight_sample_pipeline(pipeline):  # noqa: F811
    p = pipeline
    merger, ref, u, k, ns = p["merger"], p["ref"], p["u"], p["k"], p["ns"]
    want_m = restate_merge_variants(p["recs"], ns, k, n_tracts=p["nt"])
    m = dev_merge(merger, k, p["recs"], ns, p["nt"], want=want_m)
    d = dev_depths(merger, ref, u, m["sites"], m["alleles"])
    got13 = dev_distances(merger, m["sites"], m["alleles"], d["genotype"], ns)
    ms = merger.last_sample_distances_ms()
    check_distances(got13, restate_sample_distances(m["sites"], m["alleles"], d["genotype"]))
    got12 = dev_distances(merger, m["sites"], m["alleles"], m["genotype"], ns)
    check_distances(got12, restate_sample_distances(m["sites"], m["alleles"], m["genotype"]))
    assert (got12["n_both"] <= got13["n_both"]).all() and (got12["n_both"] < got13["n_both"]).any()
    assert (got13["n_differ"] > 0).any() and (got13["length_diff"] > 0).any()
    print(f"\n[distances] {len(m['sites'])} sites x {ns} samples: n_both up to {got13['n_both'].max()}, n_differ up to {got13['n_differ'].max()}, "
          f"length_diff up to {got13['length_diff'].max()}; tjamd_last_sample_distances_ms {ms:.3f} ms")


def distances_text(sample_names, d):
    out = "sample_a\tsample_b\tn_both\tn_differ\tlength_diff\n"
    for a in range(len(sample_names)):
        for b in range(a, len(sample_names)):
            out += "%s\t%s\t%d\t%d\t%d\n" % (sample_names[a], sample_names[b], d["n_both"][a, b], d["n_differ"][a, b], d["length_diff"][a, b])
    return out


def test_merged_vcf_c_example_with_distances(pipeline, tmp_path):  # noqa: F811
    p = pipeline
    exe, libdir = str(tmp_path / "merged_vcf"), os.path.join(ROOT, "tatajuba_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "merged_vcf.c"),
                           "-L", libdir, "-ltatajuba_amd", "-Wl,-rpath," + libdir, "-o", exe])
    genome = p["genome"]
    fasta = str(tmp_path / "ref.fa")
    with open(fasta, "w") as fh:
        fh.write(">genome some text\n%s\n" % "\n".join(genome[j: j + 70] for j in range(0, len(genome), 70)))
    files, samples = [], []
    for smp, s in enumerate(p["streams"]):
        f = str(tmp_path / ("s%d.fq" % smp))
        with open(f, "wb") as fh:
            fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rd, b"I" * len(rd)) for i, rd in enumerate(s.split(b"\n")[:-1])))
        files.append(f); samples.append("s%d.fq" % smp)
    m = restate_merge_variants(p["recs"], p["ns"], p["k"], n_tracts=p["nt"])
    d = restate_site_depths(p["u"].keys, p["u"].mat, p["u"].tracts, p["u"].tract_loc, p["ref"].download(), p["k"], m)
    vcf, tsv = {}, {}
    for flag in (("-M",), ("-D", "-M")):
        out = tmp_path / ("out" + "".join(flag))
        out.mkdir()
        r = subprocess.run([exe, "-r", fasta, *flag, "-x", "1", "-k", str(p["k"]), "-m", str(p["m"]), "-c", "5", "-d", "1", "-l", "2", "-o", str(out)] + files,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        vcf[flag] = (out / "merged.vcf").read_text()
        tsv[flag] = (out / "sample_distances.tsv").read_text()
    # merged.vcf: what the runs without -M write (tests/test_sites.py and tests/test_depths.py pin those to the same texts)
    assert vcf[("-M",)] == merged_vcf_text(["genome"], [len(genome)], samples, m)
    assert vcf[("-D", "-M")] == depth_vcf_text(["genome"], [len(genome)], samples, m, d)
    assert tsv[("-M",)] == distances_text(samples, restate_sample_distances(m["sites"], m["alleles"], m["genotype"]))
    assert tsv[("-D", "-M")] == distances_text(samples, restate_sample_distances(m["sites"], m["alleles"], d["genotype"]))
    assert tsv[("-M",)] != tsv[("-D", "-M")] and len(tsv[("-M",)].splitlines()) == 1 + p["ns"] * (p["ns"] + 1) // 2
