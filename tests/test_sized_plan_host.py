"""Per-glyph box sizes without a GPU: the host-only header msdfgen_amd/csrc/msdf_sizedplan.hpp (validation, W, H, slot, packed offsets; compiled with the
host compiler from tests/sizedplan_host) on hand-computed cases, and the refusals of the two sized C entry points, which are returned before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from msdfgen_amd import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sizedplan_host", "sizedplan_host.cpp")
BOXES = [(1, 1), (7, 9), (8, 8), (9, 8), (8, 9), (24, 1), (1, 17), (23, 17), (16, 16), (17, 10), (24, 17)]     # the boxes of tests/test_gpu_sized.py


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sizedplan_host")), "sizedplan_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", SRC, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.sized_layout.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_longlong)]
    lib.sized_packed_offsets.argtypes = [C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int64)]
    return lib


def layout(host, sizes):
    out = (C.c_longlong*6)()
    a = None if sizes is None else np.ascontiguousarray(sizes, np.int32).reshape(-1)
    n = 0 if a is None else len(a)//2
    rc = host.sized_layout(n, None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32)), out)
    return rc, dict(zip(("W", "H", "slot", "box_texels", "bad_glyph", "grid_texels"), (int(v) for v in out)))


def test_layout_of_the_box_cycle(host):
    ok, none, bad, many = (host.sized_codes(k) for k in range(4))
    assert (ok, len({ok, none, bad, many})) == (0, 4)
    rc, l = layout(host, BOXES)
    texels = 1+63+64+72+72+24+17+391+256+170+408
    assert rc == ok and l == {"W": 24, "H": 17, "slot": 408, "box_texels": texels, "bad_glyph": -1, "grid_texels": 11*408}
    # W and H need not come from one glyph
    rc, l = layout(host, [(30, 2), (3, 40), (5, 5)])
    assert rc == ok and (l["W"], l["H"], l["slot"], l["box_texels"], l["grid_texels"]) == (30, 40, 1200, 60+120+25, 3600)
    rc, l = layout(host, [(16, 16)]*5)
    assert rc == ok and (l["W"], l["H"], l["slot"], l["box_texels"]) == (16, 16, 256, 5*256) and l["box_texels"] == l["grid_texels"]


def test_refused_sizes(host):
    ok, none, bad, many = (host.sized_codes(k) for k in range(4))
    out = (C.c_longlong*6)()
    assert host.sized_layout(3, None, out) == none
    assert host.sized_layout(0, None, out) == ok and list(out)[:4] == [0, 0, 0, 0]           # no glyphs: nothing to read
    for box in ((0, 5), (5, 0), (-1, 5), (5, -7), (0, 0)):
        rc, l = layout(host, [(4, 4), (8, 3), box, (2, 2)])
        assert rc == bad and l["bad_glyph"] == 2, box
    # the planners' bound on nGlyphs*W*H (the correction pass's 32-bit texel index): 65 536 slots of 256 x 256 are one too many, 65 535 slots fit
    assert layout(host, np.full((65536, 2), 256))[0] == many
    rc, l = layout(host, np.full((65535, 2), 256))
    assert rc == ok and l["grid_texels"] == 65535*65536
    # ... also where only ONE glyph is wide and another one tall
    assert layout(host, [(1 << 16, 1), (1, 1 << 16)])[0] == many
    assert layout(host, [(0x7fffffff, 0x7fffffff)])[0] == many                                # no overflow on the way to the refusal


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_packed_offsets(host, channels):
    sizes = np.ascontiguousarray(BOXES, np.int32)
    off = np.zeros(len(BOXES)+1, np.int64)
    host.sized_packed_offsets(len(BOXES), sizes.ctypes.data_as(C.POINTER(C.c_int32)), channels, off.ctypes.data_as(C.POINTER(C.c_int64)))
    want = [0, 1, 64, 128, 200, 272, 296, 313, 704, 960, 1130, 1538]
    assert off.tolist() == [channels*v for v in want]
    import msdfgen_amd as M
    assert M.GlyphBatch.packed_offsets(BOXES, channels).tolist() == off.tolist()              # the binding's default placement is the header's


def test_c_abi_refuses_bad_sizes_before_any_device_call():
    """msdfhip_tiles_to_bytes_sized takes its glyph count as an argument, so every refusal of the shared validation can be provoked through it with no batch
    and no device pointer that would be valid anywhere; msdfhip_batch_generate_sized reads the count from a batch, which only a device can create: its
    refusals with a batch are in tests/test_gpu_sized.py."""
    lib = L.load()
    cfg = L.default_config()
    fake = C.c_void_p(64)                                                                      # never dereferenced: the call must fail first
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def to_bytes(n, sizes, channels=3):
        a = None if sizes is None else np.ascontiguousarray(sizes, np.int32).reshape(-1)
        off = np.zeros(max(n, 1), np.int64)
        return lib.msdfhip_tiles_to_bytes_sized(fake, n, None if a is None else a.ctypes.data_as(i32), off.ctypes.data_as(i64), channels, fake, fake, None)
    assert to_bytes(2, None) == L.ERR_INVALID and b"sizes is NULL" in lib.msdfhip_last_error()
    for box in ((0, 4), (4, 0), (-3, 4), (4, -1)):
        assert to_bytes(3, [(4, 4), box, (4, 4)]) == L.ERR_INVALID, box
        assert b"glyph 1" in lib.msdfhip_last_error() and b"at least 1" in lib.msdfhip_last_error()
    assert to_bytes(65536, np.full((65536, 2), 256)) == L.ERR_INVALID and b"32-bit texel index" in lib.msdfhip_last_error()
    assert to_bytes(1, [(4, 4)], channels=2) == L.ERR_INVALID
    assert to_bytes(-1, [(4, 4)]) == L.ERR_INVALID
    assert to_bytes(0, None) == 0                                                              # no glyphs: a no-op, like msdfhip_tiles_to_bytes
    assert lib.msdfhip_batch_generate_sized(None, 3, None, fake, fake, None, None, C.byref(cfg), None) == L.ERR_INVALID
    assert lib.msdfhip_abi_version() == 5


def test_sanitized_build_of_the_host_program(tmp_path):
    """The header under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program (host code only). Skipped only where an EMPTY program
    cannot be built with those flags."""
    from test_ec_lazy_host import _sanitizers_link
    if not _sanitizers_link(tmp_path):
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    exe = os.path.join(str(tmp_path), "sizedplan_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSIZEDPLAN_MAIN", SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])
