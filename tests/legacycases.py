"""Shared by the tests of the legacy generators and the legacy correction (test_legacy_host.py, test_gpu_legacy.py, test_legacy_cases_host.py,
test_gpu_legacy_cases.py) and by tools/make_golden_legacy.py / make_golden_legacy_crafted.py: the recorded reference data of tests/golden/legacy.npz and
legacy_crafted.npz, the host build of msdf_legacy.hpp (tests/legacy_host), what the reference makes of a legacy call from pieces that run anywhere
(reference_call), and a ctypes binding of the compiled reference's own legacy functions (oracle/_ref/libmsdfgen_ref.so, by mangled name: its C driver
does not cover them)."""
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


def range_of(map_scale, map_translate):
    """(range lower, range upper) that distance_mapping() turns into exactly (map_scale, map_translate): the inverse of xf6 for transformations that come
    from the device (GlyphBatch.frame). translate = -lower is exact; the width is searched among the neighbours of 1/scale."""
    lower = -np.float64(map_translate)
    span = np.float64(1)/np.float64(map_scale)
    cands = [span]
    for _ in range(8):
        cands = [np.nextafter(cands[0], -np.inf)]+cands+[np.nextafter(cands[-1], np.inf)]
    for s in sorted(cands, key=lambda s: abs(s-span)):
        upper = lower+s
        if distance_mapping(lower, upper) == (float(map_scale), float(map_translate)):
            return float(lower), float(upper)
    raise AssertionError("no range maps to (%r, %r)" % (map_scale, map_translate))


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


# ------------------------------------------------------------------------------------ what the reference makes of a legacy call

DEFAULT_RATIO = 1.11111111111111111
SignPass = namedtuple("SignPass", "fill_rule zero")                 # the CLI's scanline pass: FillRule 0..3, the SDF's zero level


def differing(a, b):
    """Number of float32 values that differ in their bits, a NaN counting as equal to a NaN only."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


def reference_call(host, oracle, shape, mode, w, h, xf, ec_mode=2, y_down=False, sign=None, min_dev=DEFAULT_RATIO, min_imp=DEFAULT_RATIO, stencil=True):
    """(bitmap (h, w, N) in memory-row order, stencil uint8 (h, w) as the reference writes it or None) of one legacy call, from pieces that need neither
    a GPU nor the compiled reference: the host build of msdf_legacy.hpp for the raw field, the plain-C oracle for the rest. Two flows:
      sign is None   generate*_legacy proper. generateMSDF_legacy / generateMTSDF_legacy re-orient their by-value bitmap to the shape (msdfgen.cpp:223, 278)
                     and correct THAT section (:273, :332): the correction walks the shape's rows. So the rows are reversed where the bitmap's orientation
                     is not the shape's, the correction runs on a bitmap of the shape's orientation, and the rows are reversed back. The stencil section
                     is made upward and re-oriented to the shape's (msdf-error-correction.cpp:19, MSDFErrorCorrection.cpp:122, 192, 385): exactly what the
                     oracle writes for a bitmap of that orientation.
      sign           the reference CLI's -legacy flow (main.cpp:1260-1294): field -> distanceSignCorrection -> msdfErrorCorrection, both on the bitmap as
                     it lies.
    Either correction runs without overlap support and without the distance check (msdfgen.cpp:272, 331)."""
    field = host_generate(host, shape, mode, w, h, xf, y_down)
    correct = mode >= 3 and ec_mode != 0
    st = np.zeros((h, w), np.uint8) if stencil and correct else None
    kw = dict(overlap=False, ec_mode=ec_mode, ec_dist=0, min_dev=min_dev, min_imp=min_imp, stencil=st)
    if sign is not None:
        field = oracle.sign_correction(shape, field, xf, zero=sign.zero, fill_rule=sign.fill_rule, y_down=y_down)
        if correct:
            field = oracle.error_correction(shape, field, xf, y_down=y_down, **kw)
    elif correct:
        rev = bool(shape.inverse_y) != bool(y_down)
        field = oracle.error_correction(shape, np.ascontiguousarray(field[::-1]) if rev else field, xf, y_down=bool(shape.inverse_y), **kw)
        field = np.ascontiguousarray(field[::-1]) if rev else field
    return field, st


def fuzz_cases(n=60, seed=77):
    """Seeded random outlines of fuzzlib's kinds 5, 6, 0, 3, 1, 2 in turn, at sizes drawn from 1..40 on each axis; every third is inverse-Y, the bitmap's
    orientation alternates."""
    import fuzzlib
    from msdfgen_amd.shape import autoframe
    from xformcases import Case
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = fuzzlib._shape(rng, (5, 6, 0, 3, 1, 2)[i % 6], int(rng.integers(0, 2**31)))
        s.inverse_y = bool(i % 3 == 0)
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        out.append(Case("fuzz/%d" % i, s, w, h, autoframe(s.bounds(), w, h, min(2., .5*min(w, h))), bool(i & 1)))
    return out


# ---------------------------------------------------------------- crafted fields for the legacy correction (legacyClashTexel, k_ec_legacy)

CRAFTED_SIZES = ((1, 1), (2, 2), (9, 17), (17, 9))                  # (width, height)
CRAFTED_TX, CRAFTED_TY = .25, .375                                  # exact in float32, and so is their sum: a difference can EQUAL a threshold


def _around(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(1))]


def crafted_fields():
    """[EcRecord with out=None]: per channel count and size of CRAFTED_SIZES one field of special values. Every channel is drawn from a palette of
    0, -0, the three thresholds (horizontal, vertical, diagonal) and their float32 neighbours on either side -- next to a 0 they ARE the neighbour
    difference --, .5, infinities, NaN and +-FLT_MAX (what the float of a mapped -DBL_MAX is where it does not overflow; where it does, -inf). A fifth
    of the texels is equalized (three equal channels: detectClash's `b0 == b1 && b0 == b2` exit), some are NaN in all channels. On top, planted
    pairs whose second largest channel difference is exactly a threshold, one ulp less and one ulp more, in each of the three directions."""
    rng = np.random.default_rng(2024)
    f32 = np.float32
    big = np.finfo(np.float32).max
    palette = np.array([0., 0., 0., -0., .5, .125, 1.]+_around(CRAFTED_TX)+_around(CRAFTED_TY)+_around(CRAFTED_TX+CRAFTED_TY)
                       + [np.inf, -np.inf, np.nan, big, -big], np.float32)
    out = []
    for n in (3, 4):
        for (w, h) in CRAFTED_SIZES:
            field = palette[rng.integers(0, len(palette), (h, w, n))]
            same = rng.uniform(0, 1, (h, w)) < .2
            field[same, 0:3] = field[same, 0:1]
            field[rng.uniform(0, 1, (h, w)) < .04] = np.nan
            if (w, h) == (1, 1):
                field[0, 0, :3] = np.nan, -np.inf, -0.
            elif (w, h) == (2, 2):
                field[0, 0, :3], field[0, 1, :3] = (0., 0., 1.), (CRAFTED_TX, CRAFTED_TX, 0.)
                field[1, 0, :3], field[1, 1, :3] = (CRAFTED_TY, CRAFTED_TY, 0.), (np.nan, np.inf, -0.)
            else:
                for k in range(3):                                  # below, at, above
                    tx, ty, td = _around(CRAFTED_TX)[k], _around(CRAFTED_TY)[k], _around(CRAFTED_TX+CRAFTED_TY)[k]
                    field[2*k, 1, :3], field[2*k, 2, :3] = (0., 0., 1.), (tx, tx, 0.)                     # horizontal pair
                    field[6, 1+3*k, :3], field[7, 1+3*k, :3] = (-0., 0., 1.), (ty, ty, 0.)                 # vertical pair
                    field[2*k, 5, :3], field[2*k+1, 6, :3] = (0., -0., 1.), (td, td, 0.)                   # diagonal pair
                field[8, 3, :3], field[8, 4, :3] = (.5, .5, .5), (0., 1., .125)                            # equalized next to unequal
                field[8, 6, :3], field[8, 7, :3] = (np.nan, 0., 1.), (-np.inf, np.inf, -big)
            out.append(EcRecord(n, w, h, CRAFTED_TX, CRAFTED_TY, np.ascontiguousarray(field, f32), None))
    return out


def crafted_golden():
    """[EcRecord]: crafted_fields() as recorded in tests/golden/legacy_crafted.npz with the reference's outputs (tools/make_golden_legacy_crafted.py)."""
    z = load_npz("legacy_crafted.npz")
    out = []
    for k in range(len(z["ec_n"])):
        n, w, h, o = int(z["ec_n"][k]), int(z["ec_w"][k]), int(z["ec_h"][k]), int(z["ec_off"][k])
        out.append(EcRecord(n, w, h, float(z["ec_tx"][k]), float(z["ec_ty"][k]), z["ec_in"][o:o+w*h*n].reshape(h, w, n), z["ec_out"][o:o+w*h*n].reshape(h, w, n)))
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
