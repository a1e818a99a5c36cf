"""The quality calls for boxes without a GPU: the host-only plan header msdfgen_amd/csrc/msdf_qualityplan.hpp (item prefix of the sized error estimate, its
inverse map, list capacities and chunks; the render's output texel prefix and its inverse map) on hand-computed cases, the MSDF_HD render texel function of
msdf_render.hpp against the oracle, acosRounded of msdf_device.hpp (the acos of the error estimate's cubic solver) against a high-precision reference, all
compiled with the host compiler from tests/sized_quality_host, and the refusals of the two sized C entry points, which
are returned before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import assert_bit_equal
from msdfgen_amd import lib as L
import sizedqualitycases as Q

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sized_quality_host", "sized_quality_host.cpp")
BOXES = [(1, 1), (7, 9), (8, 8), (9, 8), (8, 9), (24, 1), (1, 17), (23, 17), (16, 16), (17, 10), (24, 17)]     # the boxes of tests/test_gpu_sized.py
ITEMS = [0, 8, 7, 7, 8, 0, 0, 16, 15, 9, 16]                    # h-1 where w > 1 and h > 1: the sum of h-1 is 102, less the 16 of the 1 x 17 box
i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sized_quality_host")), "sized_quality_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", SRC, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.sq_max_count.restype = C.c_longlong
    lib.sq_item_prefix.argtypes = [C.c_int, i32, C.c_int, i64]
    lib.sq_item_of.argtypes = [i64, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_int)]
    lib.sq_caps.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    lib.sq_chunks.argtypes = [C.c_longlong]*3+[C.POINTER(C.c_longlong)]
    lib.sq_texel_prefix.argtypes = [C.c_int, i32, i64, C.POINTER(C.c_int)]
    lib.sq_texel_of.argtypes = [i64, C.c_int, i32, C.c_longlong, C.POINTER(C.c_int)]
    lib.sq_render.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_double, C.c_double, C.c_float]
    return lib


def item_prefix(host, sizes, spr):
    a = np.ascontiguousarray(sizes, np.int32).reshape(-1)
    out = np.full(len(a)//2+1, -1, np.int64)
    return host.sq_item_prefix(len(a)//2, a.ctypes.data_as(i32), spr, out.ctypes.data_as(i64)), out


def item_of(host, start, spr, item):
    out = (C.c_int*3)()
    host.sq_item_of(start.ctypes.data_as(i64), len(start)-1, spr, item, out)
    return tuple(out)


def chunks(host, items, lane_bytes, cap):
    out = (C.c_longlong*2)()
    host.sq_chunks(items, lane_bytes, cap, out)
    return tuple(out)


def texel_prefix(host, sizes):
    a = np.ascontiguousarray(sizes, np.int32).reshape(-1)
    out = np.full(len(a)//2+1, -1, np.int64)
    bad = C.c_int(-7)
    return host.sq_texel_prefix(len(a)//2, a.ctypes.data_as(i32), out.ctypes.data_as(i64), C.byref(bad)), out, bad.value


@pytest.mark.parametrize("spr", [1, 3])
def test_item_prefix_and_inverse_map_of_the_box_cycle(host, spr):
    ok = host.sq_codes(0)
    rc, start = item_prefix(host, BOXES, spr)
    assert rc == ok and sum(h-1 for _, h in BOXES) == 102 and sum(ITEMS) == 102-16 and ITEMS.count(0) == 3
    assert start.tolist() == np.concatenate([[0], np.cumsum(ITEMS)*spr]).tolist() == Q.item_prefix(BOXES, spr)
    # every item of the prefix: (glyph, row, subRow) in that order, the glyphs without items stepped over
    want = [(g, row, sub) for g, n in enumerate(ITEMS) for row in range(n) for sub in range(spr)]
    assert len(want) == start[-1]
    assert [item_of(host, start, spr, i) for i in range(len(want))] == want


def test_inverse_map_around_runs_of_empty_glyphs(host):
    """Glyphs without items first, last, several in a row and between single-item glyphs."""
    sizes = [(1, 9), (5, 1), (1, 1), (4, 2), (9, 1), (1, 1), (1, 30), (3, 4), (2, 2), (6, 1), (1, 6)]
    for spr in (1, 2):
        rc, start = item_prefix(host, sizes, spr)
        per = [0, 0, 0, 1, 0, 0, 0, 3, 1, 0, 0]
        assert rc == host.sq_codes(0) and start.tolist() == np.concatenate([[0], np.cumsum(per)*spr]).tolist()
        want = [(g, row, sub) for g, n in enumerate(per) for row in range(n) for sub in range(spr)]
        assert [item_of(host, start, spr, i) for i in range(int(start[-1]))] == want
    rc, start = item_prefix(host, [(1, 5), (7, 1)], 4)                  # nothing but empty glyphs
    assert rc == host.sq_codes(0) and start.tolist() == [0, 0, 0]
    rc, start = item_prefix(host, [(3, 3)], 5)                          # one glyph
    assert start.tolist() == [0, 10] and item_of(host, start, 5, 9) == (0, 1, 4)


def test_list_capacities_and_chunks(host):
    out = (C.c_longlong*3)()
    host.sq_caps(50, 24, out)
    assert tuple(out) == (150, 74, 224*12) and Q.lane_bytes(50, 24) == 224*12
    host.sq_caps(0, 1, out)                                             # a batch without edges keeps one edge's worth
    assert tuple(out) == (3, 5, 96)
    host.sq_caps(7, 0x7fffffff, out)                                    # no 32-bit overflow in 3*W+2
    assert out[1] == 3*0x7fffffff+2
    per = 224*12
    cases = [(258, per, 512 << 20, (320, 1)),                           # everything in one launch: the items rounded up to whole wavefronts
             (258, per, 129*per, (128, 3)),                             # 128 + 128 + 2
             (258, per, 200*per, (192, 2)),
             (258, per, 1, (64, 5)),                                    # a cap below one wavefront's lists: one wavefront all the same
             (258, per, 64*per-1, (64, 5)),
             (257, per, 128*per, (128, 3)),                             # a last chunk of 1 lane
             (65, per, 64*per, (64, 2)),
             (64, per, 64*per, (64, 1)),
             (1, per, 512 << 20, (64, 1)),
             (984, per, 1 << 20, (384, 3))]
    for items, lane, cap, want in cases:
        assert chunks(host, items, lane, cap) == want, (items, cap)
        assert Q.chunk_lanes(items, lane, cap) == want[0], (items, cap)
        lanes, count = want
        assert (count-1)*lanes < items <= count*lanes and lanes % 64 == 0
    # the uniform call's arithmetic before the knob: (512 << 20)//perLane rounded down to 64
    assert chunks(host, 10**9, 4000, 512 << 20)[0] == (512 << 20)//4000//64*64


def test_output_texel_prefix_with_empty_outputs(host):
    ok, many, bad = (host.sq_codes(k) for k in range(3))
    sizes = [(0, 5), (3, 2), (4, 0), (0, 0), (1, 1), (2, 3), (0, 7)]
    rc, start, _ = texel_prefix(host, sizes)
    assert rc == ok and start.tolist() == [0, 0, 6, 6, 6, 7, 13, 13]
    want = [(g, x, y) for g, (w, h) in enumerate(sizes) for y in range(h) for x in range(w)]
    out = (C.c_int*3)()
    a = np.ascontiguousarray(sizes, np.int32).reshape(-1)
    for t, w3 in enumerate(want):
        host.sq_texel_of(start.ctypes.data_as(i64), len(sizes), a.ctypes.data_as(i32), t, out)
        assert tuple(out) == w3, t
    rc, start, _ = texel_prefix(host, [(0, 3), (5, 0)])
    assert rc == ok and start.tolist() == [0, 0, 0]
    rc, _, g = texel_prefix(host, [(2, 2), (3, 3), (4, -1)])
    assert rc == bad and g == 2
    rc, _, g = texel_prefix(host, [(-5, 2)])
    assert rc == bad and g == 0


def test_overflow_refusals(host):
    ok, many, _ = (host.sq_codes(k) for k in range(3))
    top = 0x7fffffff
    cap = host.sq_max_count()
    assert cap == 1 << 48
    assert item_prefix(host, [(2, top)], top)[0] == many                # (2^31-2)*(2^31-1) scanlines of one glyph
    assert item_prefix(host, [(2, top)]*3, 1 << 16)[0] == many          # 2^47 - 2^17 scanlines each: the third glyph passes 2^48
    tall = (2, (1 << 16)+1)                                             # 2^16 rows of scanlines; 2^46 items at 2^30 scanlines per row
    rc, start = item_prefix(host, [tall]*4, 1 << 30)
    assert rc == ok and start[-1] == cap                                # exactly 2^48 is the last total that fits ...
    assert item_prefix(host, [tall]*4+[(2, 2)], 1 << 30)[0] == many     # ... one more glyph with items does not
    assert item_prefix(host, [tall]*4+[(1, 2), (2, 1)], 1 << 30)[0] == ok   # (glyphs without items behind it do)
    assert texel_prefix(host, [(top, top)])[0] == many
    assert texel_prefix(host, [(1 << 24, 1 << 24)])[0] == ok            # exactly 2^48 texels
    assert texel_prefix(host, [(1 << 24, 1 << 24), (1, 1)])[0] == many
    assert texel_prefix(host, [(1 << 24, 1 << 24), (0, 9)])[0] == ok


@pytest.mark.parametrize("n_out,n_sdf", Q.PAIRS)
def test_render_texel_function_vs_oracle(host, oracle, n_out, n_sdf):
    """renderMapping + renderSdfTexel (what both render kernels run per thread), per glyph over the 43 boxes, against oracle.render_sdf: bit for bit."""
    from test_gpu_sized import glyphs
    _, sizes, _ = glyphs()
    src = Q.fields(oracle, Q.MODE_OF_CHANNELS[n_sdf])
    fp = C.POINTER(C.c_float)
    compared = 0
    for g, (w, h) in enumerate(sizes.tolist()):
        f = np.ascontiguousarray(src[g])
        for ow, oh in Q.out_sizes(w, h):
            for lo, hi in Q.RANGES:
                for thr in Q.THRESHOLDS:
                    got = np.full((oh, ow, n_out), -1, np.float32)
                    assert host.sq_render(n_out, n_sdf, got.ctypes.data_as(fp), ow, oh, f.ctypes.data_as(fp), w, h, lo, hi, thr) == 0
                    assert_bit_equal(got, oracle.render_sdf(f, ow, oh, n_out, lo, hi, thr), "glyph %d %dx%d -> %dx%d range (%g, %g) threshold %g" % (g, w, h, ow, oh, lo, hi, thr))
                    compared += got.size
    assert compared > 0
    assert host.sq_render(2, 3, None, 1, 1, None, 1, 1, 0., 0., .5) == 1    # no such overload


def test_rounded_acos_is_the_correctly_rounded_value(host):
    """acosRounded, which the error estimate's scanlines take for the cubic solver's acos: the value of acos rounded to nearest, against a
    200-bit reference, on a spread of arguments, near 0, near +-1, at the switch of its two forms and at the end points."""
    import mpmath
    rng = np.random.default_rng(31)
    x = np.concatenate([rng.uniform(-1, 1, 6000), np.ldexp(rng.uniform(-1, 1, 1000), -rng.integers(1, 70, 1000)),
                        np.sign(rng.uniform(-1, 1, 1500))*(1-np.ldexp(rng.uniform(0, 1, 1500), -rng.integers(1, 50, 1500))),
                        [0., -0., .5, -.5, np.nextafter(.5, 1), np.nextafter(-.5, -1), 1., -1., np.nextafter(1, 0), np.nextafter(-1, 0), 5e-324, 1e-300]])
    y = np.zeros(len(x))
    dp = C.POINTER(C.c_double)
    host.sq_acos_rounded.argtypes = [dp, C.c_long, dp]
    host.sq_acos_rounded(np.ascontiguousarray(x).ctypes.data_as(dp), len(x), y.ctypes.data_as(dp))
    mpmath.mp.prec = 200
    worst = 0.
    for xv, yv in zip(x.tolist(), y.tolist()):
        t = mpmath.acos(mpmath.mpf(xv))
        if t == 0:
            assert yv == 0
            continue
        below, above = np.nextafter(yv, -np.inf), np.nextafter(yv, np.inf)
        err = abs(mpmath.mpf(yv)-t)
        assert err <= abs(mpmath.mpf(float(below))-t) and err <= abs(mpmath.mpf(float(above))-t), (xv, yv)
        worst = max(worst, float(err/mpmath.mpf(float(above-yv))))
    print("largest error %.4f ulp" % worst)
    out = np.zeros(2)
    host.sq_acos_rounded(np.array([2., np.nan]).ctypes.data_as(dp), 2, out.ctypes.data_as(dp))
    assert np.isnan(out).all()


def test_c_abi_refusals_before_any_device_call():
    """msdfhip_render_sdf_sized takes its glyph count as an argument: every refusal of the shared size validation, with the texts of
    msdfhip_tiles_to_bytes_sized, through fake pointers that are never dereferenced. The estimate's count comes from a batch, which only a device can
    create: without one it is refused."""
    lib = L.load()
    fake = C.c_void_p(64)

    def render(n, sdf_sizes, out_sizes=None, no=3, ns=3):
        a = None if sdf_sizes is None else np.ascontiguousarray(sdf_sizes, np.int32).reshape(-1)
        o = np.ascontiguousarray(out_sizes if out_sizes is not None else np.zeros((max(n, 1), 2)), np.int32).reshape(-1)
        off = np.zeros(max(n, 1), np.int64)
        return lib.msdfhip_render_sdf_sized(fake, n, None if a is None else a.ctypes.data_as(i32), off.ctypes.data_as(i64), ns, fake, o.ctypes.data_as(i32),
                                            off.ctypes.data_as(i64), no, -1., 1., .5, None)
    assert render(2, None) == L.ERR_INVALID and b"sizes is NULL" in lib.msdfhip_last_error()
    for box in ((0, 4), (4, 0), (-3, 4), (4, -1)):
        assert render(3, [(4, 4), box, (4, 4)]) == L.ERR_INVALID, box
        assert b"glyph 1" in lib.msdfhip_last_error() and b"at least 1" in lib.msdfhip_last_error()
    assert render(65536, np.full((65536, 2), 256)) == L.ERR_INVALID and b"32-bit texel index" in lib.msdfhip_last_error()
    for no, ns in ((2, 3), (3, 4), (4, 3), (4, 1), (1, 2), (0, 1), (3, 0)):
        assert render(1, [(4, 4)], no=no, ns=ns) == L.ERR_INVALID and b"no overload" in lib.msdfhip_last_error(), (no, ns)
    assert render(-1, [(4, 4)]) == L.ERR_INVALID
    assert render(0, None) == 0                                                                # no glyphs: a no-op, like msdfhip_render_sdf
    assert render(2, [(4, 4), (5, 5)], [(3, 3), (2, -1)]) == L.ERR_INVALID and b"glyph 1" in lib.msdfhip_last_error()
    assert render(2, [(4, 4), (5, 5)], [(0, 3), (2, 0)]) == 0                                  # no output texel anywhere: nothing to do, no pointer read
    off = np.zeros(1, np.int64)
    box = np.array([4, 4], np.int32)
    assert lib.msdfhip_batch_estimate_sdf_error_sized(None, 3, box.ctypes.data_as(i32), off.ctypes.data_as(i64), fake, fake, 1, 0, fake, None) == L.ERR_INVALID
    assert lib.msdfhip_abi_version() == 5
    for name in ("msdfhip_batch_estimate_sdf_error_sized", "msdfhip_render_sdf_sized"):
        assert name in L.EXPORTED_SYMBOLS, name


def test_sanitized_build_of_the_host_program(tmp_path):
    """The plan header and the render texel function under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program (host code only). Skipped
    only where an EMPTY program cannot be built with those flags."""
    from test_ec_lazy_host import _sanitizers_link
    if not _sanitizers_link(tmp_path):
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    exe = os.path.join(str(tmp_path), "sized_quality_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DSIZED_QUALITY_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])
