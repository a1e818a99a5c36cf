"""Shared by the tests of the legacy generators and the legacy correction (test_legacy_host.py, test_gpu_legacy.py) and by tools/make_golden_legacy.py:
the recorded reference data of tests/golden/legacy.npz, the host build of msdf_legacy.hpp (tests/legacy_host), and a ctypes binding of the compiled
reference's own legacy functions (oracle/_ref/libmsdfgen_ref.so, by mangled name: its C driver does not cover them)."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

from conftest import load_npz
from msdfgen_amd import lib as L
from msdfgen_amd.shape import ShapeBatch, distance_mapping

HERE = os.path.dirname(os.path.abspath(__file__))
CHANNELS = {1: 1, 2: 1, 3: 3, 4: 4}
SIZES = ((1, 1), (7, 5), (8, 8), (9, 17), (40, 32))            # one texel, a partial tile, exactly one tile, partial tiles on both axes, several tiles
EC_SIZES = ((1, 9), (9, 1), (2, 2), (9, 17))                    # (width, height) of the legacy correction's random fields
EC_THRESHOLDS = ((.3, .3), (.1, .5))

# One recorded call of a legacy generator: shape index into the batch, mode 1..4, bitmap size, xf = (sx, sy, tx, ty, range lower, range upper),
# ErrorCorrectionConfig::Mode, the bitmap's orientation, whether the CLI's scanline pass ran (fill rule, zero level), the expected bitmap in memory-row
# order and the expected stencil (None where none was asked for).
Record = namedtuple("Record", "name shape mode w h xf ec y_down sign fill zero out stencil")
EcRecord = namedtuple("EcRecord", "n w h tx ty field out")


def golden():
    """(batch of the fixture's shapes, [Record], [EcRecord])."""
    z = load_npz("legacy.npz")
    batch = ShapeBatch(z["shapes_gco"].astype(np.int32), z["shapes_co"].astype(np.int32), z["shapes_points"], z["shapes_types"].astype(np.int32),
                       z["shapes_colors"].astype(np.int32), z["shapes_inverse_y"].astype(np.uint8), [str(s) for s in z["shapes_names"]])
    recs = []
    for k in range(len(z["rec_name"])):
        mode, w, h = int(z["rec_mode"][k]), int(z["rec_w"][k]), int(z["rec_h"][k])
        n = CHANNELS[mode]
        o, so = int(z["rec_off"][k]), int(z["rec_stencil_off"][k])
        recs.append(Record(str(z["rec_name"][k]), int(z["rec_shape"][k]), mode, w, h, z["rec_xf"][k].copy(), int(z["rec_ec"][k]), bool(z["rec_ydown"][k]),
                           bool(z["rec_sign"][k]), int(z["rec_fill"][k]), float(z["rec_zero"][k]), z["rec_out"][o:o+w*h*n].reshape(h, w, n),
                           z["rec_stencils"][so:so+w*h].reshape(h, w) if so >= 0 else None))
    ecs = []
    for k in range(len(z["ec_n"])):
        n, w, h, o = int(z["ec_n"][k]), int(z["ec_w"][k]), int(z["ec_h"][k]), int(z["ec_off"][k])
        ecs.append(EcRecord(n, w, h, float(z["ec_tx"][k]), float(z["ec_ty"][k]), z["ec_in"][o:o+w*h*n].reshape(h, w, n), z["ec_out"][o:o+w*h*n].reshape(h, w, n)))
    return batch, recs, ecs


def xf6(xf):
    """(sx, sy, tx, ty, range lower, range upper) -> the C ABI's (sx, sy, tx, ty, mapScale, mapTranslate)."""
    ms, mt = distance_mapping(xf[4], xf[5])
    return np.array([xf[0], xf[1], xf[2], xf[3], ms, mt], np.float64)


def shape_arrays(shape):
    co = np.ascontiguousarray(shape.contour_offsets, np.int32)
    ne = shape.n_edges
    pts = np.zeros((max(ne, 1), 8))
    pts[:ne] = shape.points
    types = np.ones(max(ne, 1), np.uint8)
    types[:ne] = shape.types
    colors = np.zeros(max(ne, 1), np.uint8)
    colors[:ne] = shape.colors
    return co, pts, types, colors


# ------------------------------------------------------------------------------------------------------ host build

def build_host(tmp):
    so = os.path.join(str(tmp), "liblegacy_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "legacy_host", "legacy_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.legacy_generate_host.argtypes = [C.c_int, L._fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, L._ip, L._dp, L._bp, L._bp, L._dp]
    lib.legacy_correction_host.argtypes = [C.c_int, L._fp, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.legacy_plan_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
    lib.legacy_plan_host.restype = None
    return lib


def host_plan(lib, n_glyphs, w, h, channels):
    """(distance blocks, refused, correction texels, scratch floats, correction blocks) of msdf_launchplan.hpp's legacy plans."""
    out = (C.c_ulonglong*5)()
    lib.legacy_plan_host(n_glyphs, w, h, channels, out)
    return tuple(int(v) for v in out)


def host_generate(lib, shape, mode, w, h, xf, y_down=False):
    """The raw legacy field (no correction) of the host build: (h, w, N) in memory-row order."""
    n = CHANNELS[mode]
    out = np.zeros((h, w, n), np.float32)
    co, pts, types, colors = shape_arrays(shape)
    x6 = xf6(xf)
    flip = int(bool(shape.inverse_y) != bool(y_down))
    assert lib.legacy_generate_host(mode, L.ptr(out, L._fp), w, h, w*n, flip, shape.n_contours, L.ptr(co, L._ip), L.ptr(pts, L._dp), L.ptr(types, L._bp),
                                    L.ptr(colors, L._bp), L.ptr(x6, L._dp)) == 0
    return out


def host_correction(lib, field, tx, ty):
    out = np.array(field, np.float32, order="C")
    h, w, n = out.shape
    assert lib.legacy_correction_host(n, L.ptr(out, L._fp), w, h, tx, ty) == 0
    return out


# ------------------------------------------------------------------------------- the compiled reference's legacy functions

class _BitmapSection(C.Structure):                                  # BitmapSection<float, N>, core/BitmapRef.hpp:74-81
    _fields_ = [("pixels", L._fp), ("width", C.c_int), ("height", C.c_int), ("rowStride", C.c_int), ("yOrientation", C.c_int)]


class _Range(C.Structure):                                          # core/Range.hpp:12-14
    _fields_ = [("lower", C.c_double), ("upper", C.c_double)]


class _Vector2(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double)]


class _EcConfig(C.Structure):                                       # ErrorCorrectionConfig, core/generator-config.h:13-47
    _fields_ = [("mode", C.c_int), ("distanceCheckMode", C.c_int), ("minDeviationRatio", C.c_double), ("minImproveRatio", C.c_double), ("buffer", L._bp)]


_SECTION = "NS_13BitmapSectionIfLi%dEEE"
_TAIL = "RKNS_5ShapeENS_5RangeERKNS_7Vector2ES8_"
_GENERATORS = {1: ("_ZN7msdfgen18generateSDF_legacyE"+_SECTION % 1+_TAIL, False), 2: ("_ZN7msdfgen19generatePSDF_legacyE"+_SECTION % 1+_TAIL, False),
               3: ("_ZN7msdfgen19generateMSDF_legacyE"+_SECTION % 3+_TAIL+"NS_21ErrorCorrectionConfigE", True),
               4: ("_ZN7msdfgen20generateMTSDF_legacyE"+_SECTION % 4+_TAIL+"NS_21ErrorCorrectionConfigE", True)}
_CORRECTION = "_ZN7msdfgen26msdfErrorCorrection_legacyERKNS_13BitmapSectionIfLi%dEEERKNS_7Vector2E"
DEFAULT_RATIO = 1.11111111111111111


class RefLegacy:
    """generate*_legacy and msdfErrorCorrection_legacy of the compiled reference. `ref`: oracle.pyoracle.Ref (its shape handles are msdfgen::Shape *).
    The by-value arguments (BitmapSection, Range, ErrorCorrectionConfig) follow the C++ ABI of trivially copyable structs, which is C's;
    tools/make_golden_legacy.py proves the binding against the reference CLI's own output before it records anything."""

    def __init__(self, ref):
        self.ref = ref
        self.gen = {}
        for mode, (name, with_ec) in _GENERATORS.items():
            fn = ref.lib[name]
            fn.restype = None
            fn.argtypes = [_BitmapSection, C.c_void_p, _Range, C.POINTER(_Vector2), C.POINTER(_Vector2)]+([_EcConfig] if with_ec else [])
            self.gen[mode] = fn
        self.ec = {}
        for n in (3, 4):
            fn = ref.lib[_CORRECTION % n]
            fn.restype = None
            fn.argtypes = [C.POINTER(_BitmapSection), C.POINTER(_Vector2)]
            self.ec[n] = fn

    def generate(self, shape, mode, w, h, xf, ec_mode=2, y_down=False, stencil=None, min_dev=DEFAULT_RATIO, min_imp=DEFAULT_RATIO):
        """shape: a FlatShape or a handle of `ref`. Returns the bitmap (h, w, N) in memory-row order; stencil: uint8 (h, w) or None."""
        hd, own = self.ref._handle(shape)
        n = CHANNELS[mode]
        out = np.zeros((h, w, n), np.float32)
        section = _BitmapSection(L.ptr(out, L._fp), w, h, w*n, int(bool(y_down)))
        scale, translate = _Vector2(float(xf[0]), float(xf[1])), _Vector2(float(xf[2]), float(xf[3]))
        args = [section, hd, _Range(float(xf[4]), float(xf[5])), C.byref(scale), C.byref(translate)]
        if mode >= 3:
            args.append(_EcConfig(int(ec_mode), 1, min_dev, min_imp, L.ptr(stencil, L._bp) if stencil is not None else None))
        self.gen[mode](*args)
        if own:
            self.ref.free(hd)
        return out

    def correction(self, field, tx, ty):
        out = np.array(field, np.float32, order="C")
        h, w, n = out.shape
        section, threshold = _BitmapSection(L.ptr(out, L._fp), w, h, w*n, 0), _Vector2(float(tx), float(ty))
        self.ec[n](C.byref(section), C.byref(threshold))
        return out
