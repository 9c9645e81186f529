"""The guarded buffers of tests/guarded.py see what they are there to see: one byte changed in front of the payload, one
byte behind it, each reported by its offset from the payload; an untouched buffer passes; frozen() sees a changed input."""
import numpy as np
import pytest

from tests.guarded import ALIGN, GUARD_BYTES, GuardedDevice, GuardedHost, frozen, guard_pattern


def test_guard_sizing_and_pattern():
    # a block of 256 threads storing the widest element (64 bytes), a row of 4096 counts, a list entry of 5 x 4096 doubles
    assert GUARD_BYTES >= max(64 << 10, 256 * 64, 4096 * 4, 5 * 4096 * 8)
    p = guard_pattern(GUARD_BYTES)
    for constant in (0x00, 0xFF, 0x5A, 0xC3):                                 # no run of 8 bytes of one value: a stray store of any
        assert not (np.lib.stride_tricks.sliding_window_view(p, 8) == constant).all(axis=1).any()   # constant changes a byte
    assert (np.diff(p.astype(np.int64)) != 0).all()


@pytest.mark.parametrize("nbytes", [0, 1, 24, 4096, 100003])
def test_guarded_host_reports_a_byte_before_and_a_byte_after(nbytes):
    g = GuardedHost(nbytes)
    assert g.ptr % ALIGN == 0 and g.damage() is None and g.untouched()
    g.check()
    g.payload[:] = 0                                                          # the payload is the caller's to write
    g.check()
    assert nbytes == 0 or not g.untouched()
    raw = g._raw
    at = g._off - 1
    raw[at] ^= 0xFF
    assert g.damage() == -1
    with pytest.raises(AssertionError, match="offset -1 from its start"):
        g.check("out")
    raw[at] ^= 0xFF
    g.check()
    at = g._off + nbytes
    raw[at] = (int(raw[at]) + 1) & 0xFF
    assert g.damage() == nbytes
    with pytest.raises(AssertionError, match=f"offset {nbytes} from its start"):
        g.check("out")
    raw[at] = (int(raw[at]) - 1) & 0xFF
    raw[g._off - GUARD_BYTES] ^= 1                                            # the far ends of both guards
    assert g.damage() == -GUARD_BYTES
    raw[g._off - GUARD_BYTES] ^= 1
    raw[g._off + nbytes + GUARD_BYTES - 1] ^= 1
    assert g.damage() == nbytes + GUARD_BYTES - 1


def test_guarded_host_views_its_payload():
    g = GuardedHost(40)
    np.frombuffer(g.payload, np.int32)[:] = np.arange(10)
    assert g.view(np.int32).tolist() == list(range(10)) and g.view(np.int32, 3).tolist() == [0, 1, 2]
    g.check()


def test_frozen_sees_a_changed_array():
    a, b = np.arange(10), np.zeros(4, np.uint8)
    with frozen(a, None, b):
        pass
    with pytest.raises(AssertionError, match="input 2 of the call was changed"):
        with frozen(a, None, b):
            b[3] = 1


@pytest.mark.gpu
@pytest.mark.parametrize("nbytes", [0, 24, 100003])
def test_guarded_device_reports_a_byte_before_and_a_byte_after(nbytes):
    torch = pytest.importorskip("torch")
    g = GuardedDevice(nbytes)
    assert g.ptr % ALIGN == 0 and g.damage() is None and g.untouched()
    assert g.payload.numel() == nbytes and g.payload.storage_offset() == g._off
    assert nbytes == 0 or g.payload.data_ptr() == g.ptr                       # (torch gives an empty view no address at all)
    g.payload[:] = 0                                                        # a slice assignment, as a kernel's stores would land
    g.check()
    raw = g._raw
    raw[g._off - 1: g._off] = 0
    assert g.damage() == -1
    with pytest.raises(AssertionError, match="offset -1 from its start"):
        g.check("d_out")
    raw[g._off - 1: g._off] = int(guard_pattern(GUARD_BYTES)[-1])
    g.check()
    raw[g._off + nbytes: g._off + nbytes + 1] = 0xEE
    assert g.damage() == nbytes
    with pytest.raises(AssertionError, match=f"offset {nbytes} from its start"):
        g.check("d_out")
    raw[g._off + nbytes: g._off + nbytes + 1] = int(guard_pattern(GUARD_BYTES)[0])
    g.check()
    raw[g._off + nbytes + 4096: g._off + nbytes + 4096 + 64] = 0              # a whole element of zeros well behind the payload
    assert g.damage() is not None and nbytes + 4096 <= g.damage() < nbytes + 4096 + 64
    t = torch.arange(10, device="cuda")
    with frozen(t):
        pass
    with pytest.raises(AssertionError, match="input 0 of the call was changed"):
        with frozen(t):
            t[3] = 7


@pytest.mark.gpu
def test_guarded_device_views_its_payload():
    torch = pytest.importorskip("torch")
    g = GuardedDevice(40)
    g.payload.view(torch.int32)[:] = torch.arange(10, dtype=torch.int32, device="cuda")
    assert g.view(np.int32).tolist() == list(range(10)) and g.view(np.int32, 3).tolist() == [0, 1, 2]
    g.check()
