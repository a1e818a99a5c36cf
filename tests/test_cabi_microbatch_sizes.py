"""The C ABI additions of the micro-batcher for bitmaps of different sizes, without a GPU: msdfhip_microbatch_hold and msdfhip_microbatch_mixed_stats exist,
keep host state only and leave the ABI version alone. What they do to running calls is in tests/test_gpu_microbatch_sizes.py."""
import ctypes as C

import msdfgen_amd as M
from msdfgen_amd import lib as L


def test_entry_points_are_exported():
    lib = L.load()
    for name in ("msdfhip_microbatch_hold", "msdfhip_microbatch_mixed_stats"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTED_SYMBOLS, name
    assert lib.msdfhip_abi_version() == 5
    assert C.sizeof(L.Config) == 48 and C.sizeof(L.Glyph) == 64            # no struct changed


def test_hold_on_an_empty_queue_needs_no_device():
    lib = L.load()
    assert lib.msdfhip_microbatch_hold(0) == 0                             # nothing held, nothing queued
    assert lib.msdfhip_microbatch_hold(50) == 0
    assert lib.msdfhip_microbatch_hold(50) == 0                            # set again while held
    assert lib.msdfhip_microbatch_hold(0) == 0
    assert lib.msdfhip_microbatch_hold(-1) == L.ERR_INVALID and b"msdfhip_microbatch_hold" in lib.msdfhip_last_error()
    with M.microbatch_hold(50) as hold:
        assert hold.queued() == 0
    assert lib.msdfhip_microbatch_hold(0) == 0


def test_mixed_stats_accept_null_and_reset():
    lib = L.load()
    assert lib.msdfhip_microbatch_mixed_stats(None, None, None, None, 1) == 0
    v = [C.c_longlong(-1) for _ in range(4)]
    assert lib.msdfhip_microbatch_mixed_stats(C.byref(v[0]), None, C.byref(v[2]), None, 0) == 0
    assert (v[0].value, v[1].value, v[2].value, v[3].value) == (0, -1, 0, -1)
    assert lib.msdfhip_microbatch_mixed_stats(*[C.byref(x) for x in v], 0) == 0
    assert [x.value for x in v] == [0, 0, 0, 0]
    st = M.microbatch_stats()
    assert {"calls", "batches", "largest", "stage_ms", "device_ms", "scatter_ms", "mixed_batches", "mixed_calls", "padded_texels", "box_texels"} <= set(st)
    assert (st["mixed_batches"], st["mixed_calls"], st["padded_texels"], st["box_texels"]) == (0, 0, 0, 0)
