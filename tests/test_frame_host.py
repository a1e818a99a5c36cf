"""Framing on the device (msdf_frame.hpp: Shape::getBounds with lanes = edges, the CLI's -autoframe per glyph) without a GPU: the helpers compiled for the
host (tests/frame_host) against the compiled reference's Shape::getBounds and the reference CLI's recorded -printmetrics output
(tests/golden/frame.npz, tools/make_golden_frame.py), and the C ABI's answers to frames that cannot be used -- all before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from msdfgen_amd import lib as L
from msdfgen_amd.shape import FlatShape
import framecases as FC

W = 7


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return FC.build_host(tmp_path_factory.mktemp("frame_host"))


@pytest.fixture(scope="module")
def gold():
    return FC.golden()


def test_framed_entry_points_are_exported():
    lib = L.load()
    for name in ("msdfhip_batch_bounds", "msdfhip_batch_frame", "msdfhip_generate_stream_prepared_oriented_framed",
                 "msdfhip_generate_stream_csr_prepared_oriented_framed"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTED_SYMBOLS, name
    assert lib.msdfhip_abi_version() == 5
    assert C.sizeof(L.FrameConfig) == 40


def test_host_bounds_equal_the_recorded_reference_bounds(host, gold):
    """Every shape of the golden batch (Basic-Latin, the teardrop, tests/geomcases.py, empty, single point, 65 / 129 edges): all four doubles bit-equal."""
    z, batch, _ = gold
    assert batch.n_glyphs >= 150
    got = np.stack([FC.host_bounds(host, batch.shape(g)) for g in range(batch.n_glyphs)])
    assert_bit_equal(got, z["batch_bounds"], "bounds")
    names = list(batch.names)
    assert_bit_equal(got[names.index("hand/empty")], np.array([FC.LARGE, FC.LARGE, -FC.LARGE, -FC.LARGE]), "empty shape")
    assert_bit_equal(got[names.index("hand/point")], np.array([3., 4., 3., 4.]), "single point")
    for ring, n in (("hand/ring65", 65), ("hand/ring129", 129)):           # the extreme point is on the last edge: lane 0 of the second / third pass
        g = names.index(ring)
        s = batch.shape(g)
        assert s.n_edges == n
        last = FlatShape(np.array([0, 1], np.int32), s.points[n-1:], s.types[n-1:], s.colors[n-1:])
        assert FC.host_bounds(host, last)[2] == got[g][2]                     # (r: the last edge bulges to the right of every other point)


def test_host_bounds_equal_the_compiled_reference(ref, host, gold):
    """The same against Shape::getBounds called now (where the reference is built), incl. the recorded values themselves."""
    z, batch, _ = gold
    for g in range(batch.n_glyphs):
        s = batch.shape(g)
        h = ref.shape_from_flat(s)
        want = ref.bounds(h)
        ref.free(h)
        assert_bit_equal(FC.host_bounds(host, s), want, batch.names[g])
        assert_bit_equal(z["batch_bounds"][g], want, "recorded "+batch.names[g])


def test_signed_zeros_and_nan_follow_the_reference_order(ref, host):
    """pointBounds compares strictly: a NaN control point never enters, and of +0 / -0 the first in edge order stays -- across the 64-edge passes too."""
    pts = [(float(k % 7)+1, float(k % 5)+1) for k in range(70)]
    pts[3], pts[66], pts[68] = (0., 1.), (-0., -0.), (float("nan"), 0.)
    s = FlatShape.from_contours([[(W, pts[k], pts[(k+1) % 70]) for k in range(70)]])
    h = ref.shape_from_flat(s)
    want = ref.bounds(h)
    ref.free(h)
    got = FC.host_bounds(host, s)
    assert_bit_equal(got, want, "zeros / NaN")
    assert not np.signbit(got[0]) and np.signbit(got[1])


def test_frame_function_equals_the_cli_metrics(host, gold):
    """frameGlyph against the reference CLI's -autoframe -printmetrics (scale, translate: %.17g) over sizes x ranges x {no scale, -scale 20}; the mapping from
    the printed scale by range = pxRange/min(scale) (main.cpp:1183) and DistanceMapping(Range) (DistanceMapping.cpp:13). All bit-equal."""
    z = gold[0]
    rows = z["metrics"]
    assert len(rows) == 3*len(FC.frame_matrix())
    for k in range(3):
        for j, (w, h, ri, scale) in enumerate(FC.frame_matrix()):
            row = rows[k*len(FC.frame_matrix())+j]
            assert tuple(row[:5]) == (k, w, h, ri, float(scale is not None))
            mode, lower, upper = FC.RANGES[ri]
            assert_bit_equal(row[5:9], z["raw_bounds"][k], "printed bounds")
            xf = FC.host_frame(host, mode, lower, upper, scale, w, h, row[5:9])
            assert xf is not None
            assert_bit_equal(xf[:4], np.array([row[9], row[9], row[10], row[11]]), "scale / translate %s" % ((k, w, h, ri, scale),))
            lo, up = (np.float64(lower)/row[9], np.float64(upper)/row[9]) if mode == 1 else (np.float64(lower), np.float64(upper))
            assert_bit_equal(xf[4:], np.array([np.float64(1)/(up-lo), -lo]), "mapping %s" % ((k, w, h, ri, scale),))


def _unit_box_frame(w, h, mode, lower, upper, scale):
    """main.cpp:1153-1183 written out for l, b, r, t = 0, 0, 1, 1 (dims = 1, 1)."""
    fx, fy = np.float64(w), np.float64(h)
    if scale is None and mode == 1:
        fx, fy = fx+2*lower, fy+2*lower
    if scale is not None:
        sx = sy = np.float64(scale)
        tx, ty = .5*(fx/sx-1)-0, .5*(fy/sy-1)-0
    elif fy < fx:
        sx = sy = fy/1
        tx, ty = .5*(fx/fy*1-1)-0, -np.float64(0)
    else:
        sx = sy = fx/1
        tx, ty = -np.float64(0), .5*(fy/fx*1-1)-0
    if mode == 1 and scale is None:
        tx, ty = tx-lower/sx, ty-lower/sy
    lo, up = (lower/min(sx, sy), upper/min(sx, sy)) if mode == 1 else (lower, upper)
    return np.array([sx, sy, tx, ty, 1/(np.float64(up)-lo), -np.float64(lo)])


def test_empty_and_zero_width_glyphs_are_framed_as_the_unit_box(host, gold):
    """l >= r or b >= t (main.cpp:1162-1163): an empty glyph (bounds at +-1e240) and a vertical line. A unit range without a given scale grows the box first
    (main.cpp:1158): the line then has a width and is fitted as it is -- that one combination is checked against the grown box instead."""
    z, batch, _ = gold
    names = list(batch.names)
    for name in ("hand/empty", "hand/vline"):
        b = z["batch_bounds"][names.index(name)]
        assert b[0] >= b[2] or b[1] >= b[3]
        for (w, h, ri, scale) in FC.frame_matrix():
            mode, lower, upper = FC.RANGES[ri]
            got = FC.host_frame(host, mode, lower, upper, scale, w, h, b)
            if name == "hand/vline" and mode == 0 and scale is None:
                dx, dy = (b[2]-lower)-(b[0]+lower), (b[3]-lower)-(b[1]+lower)
                assert dx == .25 and got[0] == (h/dy if dx*h < dy*w else w/dx)
            else:
                assert_bit_equal(got, _unit_box_frame(w, h, mode, np.float64(lower), np.float64(upper), scale), "%s %s" % (name, (w, h, ri, scale)))


def test_unusable_frames_are_refused_before_the_device():
    """-pxrange 40 at 32x32 ("Cannot fit the specified pixel range"), equal range ends, a given scale of zero, a range mode outside 0..1: MSDFHIP_ERR_INVALID
    from every framed entry point, with nothing read and nothing written."""
    lib = L.load()
    cfg = L.default_config()
    gco, co = np.array([0, 1], np.int32), np.array([0, 3], np.int32)
    pts = np.zeros((3, 8), np.float64)
    pts[0, :4], pts[1, :4], pts[2, :4] = (0, 0, 1, 0), (1, 0, 0, 1), (0, 1, 0, 0)
    types = np.ones(3, np.uint8)
    glyphs = np.zeros(1, L.GLYPH_DTYPE)
    glyphs["row_stride"] = 32*3
    out = np.zeros((1, 32, 32, 3), np.float32)
    prep = L.PrepConfig(1, 1, 3.0, 0)
    called = []
    COUNT = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
    FILL = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8))

    class ShapeSource(C.Structure):
        _fields_ = [("user", C.c_void_p), ("count", COUNT), ("fill", FILL)]

    source = ShapeSource(None, COUNT(lambda user, g, nc, ne: called.append(g)), FILL(lambda user, g, base, ends, p, t, c: called.append(g)))

    def csr(f):
        return lib.msdfhip_generate_stream_csr_prepared_oriented_framed(-1, 3, 32, 32, 1, L.ptr(gco, L._ip), L.ptr(co, L._ip), L.ptr(pts, L._dp), L.ptr(types, L._bp),
                                                                        None, glyphs.ctypes.data, out.ctypes.data, out.size, None, 0, None, C.byref(cfg),
                                                                        C.byref(prep), None, None, C.byref(f))

    def src(f):
        return lib.msdfhip_generate_stream_prepared_oriented_framed(-1, 3, 32, 32, 1, C.byref(source), glyphs.ctypes.data, out.ctypes.data, out.size, None, 0, None,
                                                                    C.byref(cfg), C.byref(prep), None, None, C.byref(f))

    def batch(f):
        return lib.msdfhip_batch_frame(None, C.byref(f), 32, 32, None, None)

    bad = ((L.FrameConfig(1, 0, -20., 20., 1., 1.), b"pixel range"), (L.FrameConfig(1, 0, 2., 2., 1., 1.), b"range_lower == range_upper"),
           (L.FrameConfig(0, 0, .5, .5, 1., 1.), b"range_lower == range_upper"), (L.FrameConfig(1, 1, -2., 2., 0., 20.), b"scale"),
           (L.FrameConfig(0, 1, -2., 2., 20., 0.), b"scale"), (L.FrameConfig(2, 0, -2., 2., 1., 1.), b"range_mode"), (L.FrameConfig(-1, 0, -2., 2., 1., 1.), b"range_mode"))
    for call in (csr, src, batch):
        for f, word in bad:
            assert call(f) == L.ERR_INVALID, (call.__name__, word)
            assert word in lib.msdfhip_last_error(), (word, lib.msdfhip_last_error())
    assert not called and not out.any()
    assert lib.msdfhip_batch_bounds(None, None) == L.ERR_INVALID
