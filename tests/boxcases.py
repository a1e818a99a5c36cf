"""Shared by the box tests (test_box_host.py, test_gpu_boxes.py) and the recorder of their fixture (tools/make_golden_boxes.py): the parameter matrix of
Shape::getBounds(border, miterLimit, polarity), the recorded reference data of tests/golden/boxes.npz, the host build of the device's box helpers
(tests/box_host) and the binding of the compiled reference's own getBounds / boundMiters."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import load_npz
from msdfgen_amd import lib as L
from msdfgen_amd.shape import ShapeBatch

HERE = os.path.dirname(os.path.abspath(__file__))
W = 7
BORDERS = (0., .125, 2.)
LIMITS = (0., 1., 2., 4., 1e9)
POLARITIES = (-1, 0, 1)
MATRIX = tuple((b, m, p) for b in BORDERS for m in LIMITS for p in POLARITIES)       # the order of the fixture's rows per shape
SEED = 0                                                                              # edgeColoringSimple(3.0, SEED) of the raw outlines


def combo(border, limit, polarity):
    return MATRIX.index((border, limit, polarity))


def _batch(z, prefix, colors=True):
    n = len(z[prefix+"_names"])
    cols = z[prefix+"_colors"].astype(np.int32) if colors else np.full(len(z[prefix+"_types"]), W, np.int32)
    return ShapeBatch(z[prefix+"_gco"].astype(np.int32), z[prefix+"_co"].astype(np.int32), z[prefix+"_points"], z[prefix+"_types"].astype(np.int32), cols,
                      np.zeros(n, np.uint8), [str(s) for s in z[prefix+"_names"]])


def golden():
    """(z, arrays, raw, prepared): the fixture; one batch of its array shapes (frame.npz's batch set + the hand-built ones), its raw outlines, and what the
    reference's orientContours, normalize and edgeColoringSimple(3.0, SEED) made of them."""
    z = load_npz("boxes.npz")
    return z, _batch(z, "batch"), _batch(z, "raw", colors=False), _batch(z, "prep")


def build_host(tmp):
    so = os.path.join(str(tmp), "libbox_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "box_host", "box_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.miters_host.argtypes = [C.c_int, L._ip, L._dp, L._bp, L._bp, L._dp, C.c_double, C.c_double, C.c_int, L._dp]
    lib.miters_host.restype = None
    lib.plan_box_host.argtypes = [C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, L._dp]
    lib.box_host.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, L._dp, L._dp, L._ip, L._dp]
    lib.box_host.restype = None
    return lib


class HostShape:
    """The arrays of one glyph as tests/box_host takes them, marshalled once for the whole matrix."""

    def __init__(self, shape):
        ne = shape.n_edges
        self.nc = shape.n_contours
        self.co = np.ascontiguousarray(shape.contour_offsets, np.int32)
        self.pts = np.zeros((max(ne, 1), 8))
        self.pts[:ne] = np.asarray(shape.points, np.float64).reshape(-1, 8)
        self.types = np.ones(max(ne, 1), np.uint8)
        self.types[:ne] = shape.types
        self.cols = np.full(max(ne, 1), W, np.uint8)
        self.cols[:ne] = shape.colors

    def miters(self, lib, border, limit, polarity, plain=None):
        """mitersGlyphWave on top of boundsGlyphWave (plain: on top of those four doubles instead): l, b, r, t."""
        out = np.zeros(4)
        p = None if plain is None else L.ptr(np.ascontiguousarray(plain, np.float64), L._dp)
        lib.miters_host(self.nc, L.ptr(self.co, L._ip), L.ptr(self.pts, L._dp), L.ptr(self.types, L._bp), L.ptr(self.cols, L._bp), p, border, limit, polarity,
                        L.ptr(out, L._dp))
        return out

    def matrix(self, lib, plain=None):
        return np.stack([self.miters(lib, b, m, p, plain) for (b, m, p) in MATRIX])


def host_plan(lib, scale, mode, lower, upper, align=(0, 0)):
    """planBox: (status, (s, lo, hi, border))."""
    out = np.zeros(4)
    status = lib.plan_box_host(scale, mode, lower, upper, int(align[0]), int(align[1]), L.ptr(out, L._dp))
    return status, out


def host_box(lib, s, lo, hi, align, plain, ext):
    """boxGlyph: (wh (2,) int32, xf (6,))."""
    wh, xf = np.zeros(2, np.int32), np.zeros(6)
    lib.box_host(s, lo, hi, int(align[0]), int(align[1]), L.ptr(np.ascontiguousarray(plain, np.float64), L._dp), L.ptr(np.ascontiguousarray(ext, np.float64), L._dp),
                 L.ptr(wh, L._ip), L.ptr(xf, L._dp))
    return wh, xf


class _Bounds(C.Structure):
    _fields_ = [("l", C.c_double), ("b", C.c_double), ("r", C.c_double), ("t", C.c_double)]


class RefBounds:
    """Shape::getBounds(double, double, int) and Shape::boundMiters of the compiled reference, by mangled name. `ref`: oracle.pyoracle.Ref (its shape
    handles are msdfgen::Shape *). Shape::Bounds is four doubles, returned by value under the C ABI of trivially copyable structs."""

    def __init__(self, ref):
        self.ref = ref
        self.get = ref.lib["_ZNK7msdfgen5Shape9getBoundsEddi"]
        self.get.restype = _Bounds
        self.get.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int]
        self.miters = ref.lib["_ZNK7msdfgen5Shape11boundMitersERdS1_S1_S1_ddi"]
        self.miters.restype = None
        self.miters.argtypes = [C.c_void_p]+[C.POINTER(C.c_double)]*4+[C.c_double, C.c_double, C.c_int]

    def bounds(self, h, border=0., limit=0., polarity=0):
        b = self.get(h, border, limit, polarity)
        return np.array([b.l, b.b, b.r, b.t])

    def matrix(self, shape):
        """getBounds over MATRIX: (45, 4)."""
        h, own = self.ref._handle(shape)
        out = np.stack([self.bounds(h, b, m, p) for (b, m, p) in MATRIX])
        if own:
            self.ref.free(h)
        return out

    def composed(self, plain, h, border, limit, polarity):
        """Shape::getBounds' own lines (core/Shape.cpp:108-113) with the plain bounds given and boundMiters taken on the shape `h`: what a caller does who
        keeps getBounds() from load time and bounds the miters of the shape it is about to render."""
        v = [C.c_double(float(x)) for x in plain]
        if border > 0:
            v[0].value -= border
            v[1].value -= border
            v[2].value += border
            v[3].value += border
            if limit > 0:
                self.miters(h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), border, limit, polarity)
        return np.array([x.value for x in v])


def ref_raw(ref, shape):
    """What the device makes of a raw outline under orient_contours + normalize + edgeColoringSimple, by the reference in the reference CLI's order
    (main.cpp:1105-1132, 1255): (handle of the prepared shape, getBounds() after normalize -- before the colouring)."""
    h = ref.shape_from_flat(shape)
    ref.lib.ref_shape_orient_contours(h)
    ref.lib.ref_shape_normalize(h)
    plain = ref.bounds(h)
    ref.lib.ref_shape_color_simple(h, 3.0, SEED)
    return h, plain


def no_box(plain):
    plain = np.asarray(plain)
    return ~((plain[..., 0] < plain[..., 2]) & (plain[..., 1] < plain[..., 3]))
