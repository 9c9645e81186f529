"""Where tjamd_locate_gapped writes, as tests/test_buffer_bounds.py asks of the other device entries: d_loc and d_how sit in
guarded buffers (tests/guarded.py) of exactly n elements, at row counts on both sides of the wavefront and of the block; the
results equal the restatement and, beside them, no byte outside a payload changed and no const input changed.  Then the same
with d_how NULL, with nothing to do, and with arguments the entry refuses."""
import numpy as np
import pytest

import tatajuba_amd as tj
from tests.guarded import GuardedDevice, frozen
from tests.test_locate import _dev, _p
from tests.test_locate_gapped import long_range_case
from tests.test_locate_gapped_cabi import restate_locate_gapped

pytestmark = pytest.mark.gpu

ERR_ARG = 3
LOC = tj.LOCATION_DTYPE
K, TOTAL = 9, 34000                                      # seed ranges on both sides of the lane walk in every wavefront
ROWS = (1, 63, 64, 65, 257)
# what the entry writes: name -> bytes per row
OUTPUTS = {"d_loc": LOC.itemsize, "d_how": 4}


def _torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def lookup():
    g, entries, keys, first = long_range_case(K, TOTAL)
    assert len(keys) >= max(ROWS)
    c = tj.Counter(K)
    ref = tj.Reference(c, g)
    assert ref.add_seeds(c) == len(entries)
    yield c, ref, entries, keys, _dev(keys), first
    ref.close()
    c.close()


def guarded_call(c, ref, kd, first, n, max_edits, max_shift, with_how=True, counter=None):
    """the call with d_loc (holding first[:n]) and d_how in guarded buffers of exactly n elements -> (rc, loc buffer, how buffer)"""
    torch = _torch()
    loc, how = GuardedDevice(n * OUTPUTS["d_loc"]), GuardedDevice(n * OUTPUTS["d_how"]) if with_how else None
    if n:
        loc.payload.copy_(torch.from_numpy(np.frombuffer(first[:n].tobytes(), np.uint8).copy()).cuda())
    torch.cuda.synchronize()
    before = ref.download()
    with frozen(kd):
        rc = tj.lib().tjamd_locate_gapped((counter or c)._h, ref._h, _p(kd), n, max_edits, max_shift, loc.c, how.c if with_how else None)
        torch.cuda.synchronize()
    assert ref.download().tobytes() == before.tobytes()
    loc.check("d_loc")
    if with_how:
        how.check("d_how")
    return rc, loc, how


@pytest.mark.parametrize("n", ROWS)
def test_exact_fit_locate_gapped(lookup, n):
    c, ref, entries, keys, kd, first = lookup
    for max_edits, max_shift in ((3, 3), (2, 1)):
        want, want_how = restate_locate_gapped(entries, keys[:n], first[:n], max_edits, max_shift, K)
        rc, loc, how = guarded_call(c, ref, kd, first, n, max_edits, max_shift)
        assert rc == int((want_how == 1).sum()) and loc.view(LOC).tobytes() == want.tobytes() and (how.view(np.int32) == want_how).all(), (n, max_edits)
        rc, loc, _ = guarded_call(c, ref, kd, first, n, max_edits, max_shift, with_how=False)             # d_how may be NULL
        assert rc == int((want_how == 1).sum()) and loc.view(LOC).tobytes() == want.tobytes()


def test_nothing_to_do_touches_nothing(lookup):
    c, ref, entries, keys, kd, first = lookup
    rc, loc, how = guarded_call(c, ref, kd, first, 0, 3, 3)
    assert rc == 0 and c.last_locate_gapped_ms() == -1.0
    loc, how = GuardedDevice(64 * 32), GuardedDevice(64 * 4)                  # room that n = 0 must leave alone
    with frozen(kd):
        assert tj.lib().tjamd_locate_gapped(c._h, ref._h, _p(kd), 0, 3, 3, loc.c, how.c) == 0
    _torch().cuda.synchronize()
    assert loc.untouched() and how.untouched()
    loc.check("d_loc"); how.check("d_how")
    assert tj.lib().tjamd_locate_gapped(c._h, ref._h, None, 0, 3, 3, None, None) == 0


def test_a_refused_call_writes_nothing(lookup):
    c, ref, entries, keys, kd, first = lookup
    torch = _torch()
    other = tj.Counter(K + 1)
    bare = tj.Reference(c, b"ACGTACGTAAAACGTTGCAGTCAGT\n")                    # an index without its seed order
    for kw, words in (({"max_shift": 4}, "max_shift 4 outside 0..3"), ({"max_shift": -1}, "max_shift -1 outside 0..3"),
                      ({"max_edits": K + 1}, f"max_edits {K + 1} outside 0..{K}"), ({"max_edits": -1}, "max_edits -1 outside"),
                      ({"counter": other}, f"built with k = {K}, the counter has k = {K + 1}"), ({"ref": bare}, "no seed order"),
                      ({"n": -1}, "n -1 < 0")):
        loc, how = GuardedDevice(64 * 32), GuardedDevice(64 * 4)
        with frozen(kd):
            rc = tj.lib().tjamd_locate_gapped(kw.get("counter", c)._h, kw.get("ref", ref)._h, _p(kd), kw.get("n", 64), kw.get("max_edits", 3),
                                              kw.get("max_shift", 3), loc.c, how.c)
            torch.cuda.synchronize()
        err = tj.lib().tjamd_last_error().decode()
        assert rc == -ERR_ARG and err.startswith("tjamd_locate_gapped") and words in err, (kw, rc, err)
        assert loc.untouched() and how.untouched()
        loc.check("d_loc"); how.check("d_how")
    bare.close()
    other.close()
