"""The distance step (include/tatajuba_distances.h: tjamd_sample_distances) without a GPU: the entries are declared in their own
header, exported and prototyped and refuse bad arguments before any device call, the record matches the header, and the
restatement that the GPU tests (tests/test_distances.py) compare against is pinned by a hand case whose expected matrix is
written out here, and by properties on a random corpus.

restate_sample_distances is written from the rule in the header: a loop over the sites, each with outer comparisons of its row
of genotypes and lengths.  The device walks tiles of sample pairs over chunks of sites staged in LDS."""
import ctypes as C
import fnmatch
import glob
import os
import re

import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedHost
from tests.test_depths_cabi import _fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tjamd_sample_distances", "tjamd_last_sample_distances_ms"]
ERR_NO_DEVICE, ERR_ARG = 1, 3
SITE, ALLELE, DIST = tj.SITE_DTYPE, tj.ALLELE_DTYPE, tj.SAMPLE_DISTANCE_DTYPE


def restate_sample_distances(sites, alleles, genotype):
    """-> SAMPLE_DISTANCE_DTYPE [ns, ns].  genotype is [n_sites, ns].  ValueError for what the entry refuses on the device."""
    genotype = np.asarray(genotype)
    n_sites, ns = genotype.shape
    assert n_sites == len(sites)
    chain = 0
    for i, s in enumerate(sites):
        if int(s["n_alleles"]) < 1:
            raise ValueError("n_alleles")
        if int(s["first_allele"]) != chain:
            raise ValueError("chain")
        chain += int(s["n_alleles"])
    if n_sites and chain != len(alleles):
        raise ValueError("chain")
    for i, s in enumerate(sites):
        for a in alleles[int(s["first_allele"]): int(s["first_allele"]) + int(s["n_alleles"])]:
            if int(a["site"]) != i:
                raise ValueError("allele site")
    if len(alleles) and not ((alleles["alt_length"] >= 0) & (alleles["alt_length"] <= 1023)).all():
        raise ValueError("alt_length")
    if n_sites and (sites["ref_length"] < 0).any():
        raise ValueError("ref_length")
    n_both = np.zeros((ns, ns), np.int64)
    n_differ = np.zeros((ns, ns), np.int64)
    length_diff = np.zeros((ns, ns), np.int64)
    for i, s in enumerate(sites):
        g = genotype[i].astype(np.int64)
        if (g < -1).any() or (g > int(s["n_alleles"])).any():
            raise ValueError("genotype")
        L = np.zeros(ns, np.int64)
        L[g == 0] = int(s["ref_length"])
        L[g > 0] = alleles["alt_length"][int(s["first_allele"]) + g[g > 0] - 1]
        both = (g >= 0)[:, None] & (g >= 0)[None, :]
        n_both += both
        n_differ += both & (g[:, None] != g[None, :])
        length_diff += np.where(both, np.abs(L[:, None] - L[None, :]), 0)
    out = np.zeros((ns, ns), DIST)
    out["n_both"], out["n_differ"], out["length_diff"] = n_both, n_differ, length_diff
    return out


def fabricate(n_sites, ns, rng, n_alleles=None, p_missing=0.15, p_ref=0.4, ref_length=None):
    """fabricated sites, alleles and genotypes, in the fields the step reads (the others stay 0): site i has n_alleles[i] alleles
    (default: 1 to 4 at random) of random alt_length, genotypes -1 with p_missing, 0 with p_ref, otherwise an allele of the site
    -> sites, alleles, genotype [n_sites, ns] int16.  rng is a numpy RandomState."""
    na = rng.randint(1, 5, n_sites) if n_alleles is None else np.asarray(n_alleles, np.int64).reshape(n_sites)
    sites = np.zeros(n_sites, SITE)
    sites["n_alleles"] = na
    sites["first_allele"] = np.cumsum(na) - na
    sites["ref_length"] = rng.randint(1, 1800, n_sites) if ref_length is None else ref_length
    sites["tract"] = np.arange(n_sites)
    alleles = np.zeros(int(na.sum()), ALLELE)
    alleles["site"] = np.repeat(np.arange(n_sites), na)
    alleles["alt_length"] = rng.randint(1, 60, len(alleles))
    r = rng.random_sample((n_sites, ns))
    g = 1 + (rng.randint(0, 1 << 30, (n_sites, ns)) % na[:, None])
    g[r < p_missing + p_ref] = 0
    g[r < p_missing] = -1
    return sites, alleles, g.astype(np.int16)


# ---- the hand case ---------------------------------------------------------------------------------------------------------
# site 0: the genome has 5, allele 1 has 6.  site 1: the genome has 3, alleles 1 and 2 both have 4 (they differ in the flank).
# site 2: the genome has 7, allele 1 has 2.
#            sample 0   sample 1   sample 2
#   site 0   0 (5)      1 (6)      -1
#   site 1   1 (4)      2 (4)      0 (3)
#   site 2   1 (2)      1 (2)      0 (7)
# (0, 1): all three sites in common; site 0 differs by 1, site 1 differs by 0 bases, site 2 is the same: (3, 2, 1)
# (0, 2) and (1, 2): sites 1 and 2 in common, both differ, by 1 and by 5: (2, 2, 6)
HAND_EXPECTED = [[(3, 0, 0), (3, 2, 1), (2, 2, 6)],
                 [(3, 2, 1), (3, 0, 0), (2, 2, 6)],
                 [(2, 2, 6), (2, 2, 6), (2, 0, 0)]]


def hand_case():
    sites = np.zeros(3, SITE)
    sites["ref_length"], sites["n_alleles"], sites["first_allele"] = [5, 3, 7], [1, 2, 1], [0, 1, 3]
    alleles = np.zeros(4, ALLELE)
    alleles["site"], alleles["alt_length"], alleles["alt_flank"], alleles["n_flank"] = [0, 1, 1, 2], [6, 4, 4, 2], [0, 0, 1, 0], [0, 1, 1, 0]
    genotype = np.array([[0, 1, -1], [1, 2, 0], [1, 1, 0]], np.int16)
    return sites, alleles, genotype


def test_the_rule_on_the_hand_case():
    sites, alleles, genotype = hand_case()
    got = restate_sample_distances(sites, alleles, genotype)
    assert [[tuple(int(v) for v in got[a, b]) for b in range(3)] for a in range(3)] == HAND_EXPECTED
    # N12's matrix of the same calls has -1 where the genome's own length was seen: those samples count as not called
    g12 = np.where(genotype == 0, -1, genotype)
    got12 = restate_sample_distances(sites, alleles, g12)
    assert [tuple(int(v) for v in got12[a, a]) for a in range(3)] == [(2, 0, 0), (3, 0, 0), (0, 0, 0)]
    assert tuple(int(v) for v in got12[0, 1]) == (2, 1, 0) and (got12["n_both"] <= got["n_both"]).all()

    def bad(what, g=genotype, **change):
        s, a = sites.copy(), alleles.copy()
        for name, (idx, value) in change.items():
            which, field = name.split("__")
            (s if which == "sites" else a)[field][idx] = value
        with pytest.raises(ValueError, match=what):
            restate_sample_distances(s, a, g)

    bad("chain", sites__first_allele=(1, 2))
    bad("chain", sites__n_alleles=(2, 2))
    bad("n_alleles", sites__n_alleles=(0, 0))
    bad("allele site", alleles__site=(2, 0))
    bad("alt_length", alleles__alt_length=(1, 1024))
    bad("alt_length", alleles__alt_length=(3, -1))
    bad("ref_length", sites__ref_length=(1, -1))
    for value, at in ((-2, (0, 0)), (2, (0, 1)), (3, (1, 2))):
        g = genotype.copy()
        g[at] = value
        bad("genotype", g=g)


@pytest.mark.parametrize("n_sites,ns,seed", [(40, 7, 1), (25, 20, 2), (1, 3, 3)])
def test_properties_on_a_random_corpus(n_sites, ns, seed):
    rng = np.random.RandomState(seed)
    sites, alleles, g = fabricate(n_sites, ns, rng)
    if ns > 4:
        g[:, 4] = -1                                                          # a sample called nowhere
    d = restate_sample_distances(sites, alleles, g)
    for f in DIST.names:
        assert (d[f] == d[f].T).all(), f                                      # symmetric
    diag = np.diagonal(d["n_both"])
    assert (diag == (g >= 0).sum(0)).all() and (np.diagonal(d["n_differ"]) == 0).all() and (np.diagonal(d["length_diff"]) == 0).all()
    assert (d["n_differ"] <= d["n_both"]).all() and (d["n_both"] <= np.minimum(diag[:, None], diag[None, :])).all()
    assert (d["length_diff"][d["n_differ"] == 0] == 0).all() and (d["length_diff"] >= 0).all()
    if ns > 4:
        assert all((d[f][4] == 0).all() for f in DIST.names)
    # one pair by a plain loop
    a, b = 0, ns - 1
    want = [0, 0, 0]
    for i, s in enumerate(sites):
        ga, gb = int(g[i, a]), int(g[i, b])
        if ga >= 0 and gb >= 0:
            length = lambda x: int(s["ref_length"]) if x == 0 else int(alleles["alt_length"][int(s["first_allele"]) + x - 1])
            want[0] += 1; want[1] += ga != gb; want[2] += abs(length(ga) - length(gb))
    assert [int(v) for v in d[a, b]] == want


# ---- declarations and argument checks --------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_prototyped():
    L = tj.lib()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    own = strip(os.path.join(ROOT, "include", "tatajuba_distances.h"))
    exported = re.findall(r"[\w*]+(?=;)", open(os.path.join(ROOT, "tatajuba_amd", "csrc", "exports.map")).read().split("local:")[0])
    assert sorted(NEW_ENTRIES) == sorted(tj.DISTANCE_EXPORTS)
    assert sorted(set(re.findall(r"\b(tjamd_\w+)\s*\(", own))) == sorted(NEW_ENTRIES)       # the header declares these and nothing else
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "tatajuba_distances.h"]
    assert len(others) >= 9
    for s in NEW_ENTRIES:
        for path in others:
            assert not re.search(r"\b%s\s*\(" % s, strip(path)), (s, path)   # ... and no other header any of them
        assert any(fnmatch.fnmatchcase(s, pat) for pat in exported), s
        assert s not in (tj.EXPORTS + tj.VARIANT_EXPORTS + tj.FEATURE_EXPORTS + tj.LOCATE_EXPORTS + tj.EFFECT_EXPORTS + tj.SITE_EXPORTS
                         + tj.DEPTH_EXPORTS) and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert "tatajuba_distances.h" in open(os.path.join(ROOT, "include", "tatajuba_amd.h")).read()
    assert '#include "tatajuba_depths.h"' in own
    assert _fields(own, "tjamd_sample_distance") == list(DIST.names)
    assert DIST.itemsize == 16 and [DIST.fields[x][1] for x in DIST.names] == [0, 4, 8]
    assert L.tjamd_last_sample_distances_ms(None) == -1.0
    for name in ("sample_distances", "last_sample_distances_ms"):
        assert hasattr(tj.Counter, name)


def test_sample_distances_checks_its_arguments_without_a_gpu():
    L = tj.lib()
    fake = C.c_void_p(0x1000)                     # never dereferenced: each call below fails its argument checks first
    out = GuardedHost(64 * DIST.itemsize)

    def call(c=fake, sites=fake, n_sites=3, alleles=fake, n_alleles=4, gt=fake, ns=2, null_out=False):
        rc = L.tjamd_sample_distances(c, sites, n_sites, alleles, n_alleles, gt, ns, None if null_out else out.c)
        return rc, L.tjamd_last_error().decode()

    for kw, msg in [({"c": None}, "null counter"), ({"null_out": True}, "null d_out"),
                    ({"n_sites": -1}, "n_sites -1, n_alleles 4: a count below 0"), ({"n_alleles": -1}, "n_sites 3, n_alleles -1: a count below 0"),
                    ({"sites": None}, "null site, allele or genotype buffer"), ({"alleles": None}, "null site, allele or genotype buffer"),
                    ({"gt": None}, "null site, allele or genotype buffer"),
                    ({"ns": 0}, "n_samples 0 outside 1..4096"), ({"ns": -3}, "n_samples -3 outside 1..4096"), ({"ns": 4097}, "n_samples 4097 outside 1..4096"),
                    ({"n_alleles": 2}, "2 alleles for 3 sites"),
                    ({"n_alleles": 1 << 31}, "2147483648 alleles: 2^31 or more"),
                    ({"n_sites": 1 << 19, "n_alleles": 1 << 19, "ns": 4096}, "524288 sites x 4096 samples: 2^31 cells or more")]:
        got, err = call(**kw)
        assert got == -ERR_ARG and err.startswith("tjamd_sample_distances") and msg in err, (kw, got, err)
    if tj.device_count() == 0:                     # good arguments, but nothing to run on: named, before the handles are read
        for kw in ({}, {"n_sites": 0, "n_alleles": 0}, {"n_sites": 0, "n_alleles": 0, "sites": None, "alleles": None, "gt": None},
                   {"n_sites": (1 << 19) - 1, "n_alleles": (1 << 31) - 1, "ns": 4096}):
            got, err = call(**kw)
            assert got == -ERR_NO_DEVICE and err.startswith("tjamd_sample_distances") and "TJAMD_ERR_NO_DEVICE" in err, (kw, got, err)
    assert out.untouched()                         # host memory handed in as the output stays as it was
    out.check("d_out")
