"""Orientation around the device's shape preparation (Shape::orientContours before normalize, the CLI's -reversewinding / -guesswinding after it) at
the C-ABI surface, without a GPU: the three _oriented entry points are exported, the ABI stays at 5, and a bad MsdfHipOrientConfig answers
MSDFHIP_ERR_INVALID, naming the field, before the shape source is read or anything is written. Then the device helpers themselves (orientGlyphWave,
windingGlyphWave in msdf_shapeprep.hpp), compiled for the host from tests/orient_host, against the compiled reference where it exists."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import load_npz
from msdfgen_amd import lib as L
from msdfgen_amd import synth
from msdfgen_amd.shape import ShapeBatch
import orientcases as OC

ORIENTED = ("msdfhip_batch_create_prepared_oriented", "msdfhip_generate_stream_prepared_oriented", "msdfhip_generate_stream_csr_prepared_oriented")
COUNT = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
FILL = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8))
HERE = os.path.dirname(os.path.abspath(__file__))


class ShapeSource(C.Structure):
    """MsdfHipShapeSource."""
    _fields_ = [("user", C.c_void_p), ("count", COUNT), ("fill", FILL)]


def test_oriented_entry_points_are_exported():
    lib = L.load()
    for name in ORIENTED:
        assert hasattr(lib, name), name
        assert name in L.EXPORTED_SYMBOLS, name
    assert lib.msdfhip_abi_version() == 5
    assert C.sizeof(L.OrientConfig) == 8 and C.sizeof(L.PrepConfig) == 24


def test_bad_orient_config_is_refused_before_the_source_or_the_device():
    lib = L.load()
    cfg = L.default_config()
    gco, co = np.array([0, 1], np.int32), np.array([0, 3], np.int32)
    pts = np.zeros((3, 8), np.float64)
    pts[0, :4], pts[1, :4], pts[2, :4] = (0, 0, 1, 0), (1, 0, 0, 1), (0, 1, 0, 0)
    types = np.ones(3, np.uint8)
    glyphs = np.zeros(1, L.GLYPH_DTYPE)
    glyphs["xf"][0] = (8, 8, 0, 0, 1, 0)
    glyphs["row_stride"] = 8*3
    out = np.zeros((1, 8, 8, 3), np.float32)
    atlas = np.zeros((1, 8, 8, 3), np.uint8)
    called = []
    source = ShapeSource(None, COUNT(lambda user, g, nc, ne: called.append(g)), FILL(lambda user, g, base, ends, p, t, c: called.append(g)))
    prep = L.PrepConfig(1, 1, 3.0, 0)
    seeds = np.zeros(1, np.uint64)

    def batch(o):
        h = C.c_void_p()
        rc = lib.msdfhip_batch_create_prepared_oriented(C.byref(h), 1, L.ptr(gco, L._ip), L.ptr(co, L._ip), L.ptr(pts, L._dp), L.ptr(types, L._bp), None,
                                                        seeds.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(prep), C.byref(o))
        assert not h.value, "a batch was created"
        return rc

    def src(o, to_atlas=False):
        return lib.msdfhip_generate_stream_prepared_oriented(-1, 3, 8, 8, 1, C.byref(source), glyphs.ctypes.data, None if to_atlas else out.ctypes.data,
                                                             0 if to_atlas else out.size, atlas.ctypes.data if to_atlas else None, atlas.size if to_atlas else 0,
                                                             None, C.byref(cfg), C.byref(prep), None, C.byref(o))

    def csr(o, to_atlas=False):
        return lib.msdfhip_generate_stream_csr_prepared_oriented(-1, 3, 8, 8, 1, L.ptr(gco, L._ip), L.ptr(co, L._ip), L.ptr(pts, L._dp), L.ptr(types, L._bp),
                                                                 None, glyphs.ctypes.data, None if to_atlas else out.ctypes.data, 0 if to_atlas else out.size,
                                                                 atlas.ctypes.data if to_atlas else None, atlas.size if to_atlas else 0, None, C.byref(cfg),
                                                                 C.byref(prep), None, C.byref(o))

    for call in (batch, src, csr, lambda o: src(o, True), lambda o: csr(o, True)):
        for bad, field in (((-1, 0), b"orient_contours"), ((2, 0), b"orient_contours"), ((0, -1), b"winding"), ((0, 3), b"winding"), ((1, 7), b"winding")):
            assert call(L.OrientConfig(*bad)) == L.ERR_INVALID, bad
            assert field in lib.msdfhip_last_error(), (bad, lib.msdfhip_last_error())
    assert not called, "the shape source was read before the orientation config was checked"
    assert not out.any() and not atlas.any()


# ---- the device helpers on the host -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("orient_host")/"liborient_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "orient_host", "orient_host.cpp")],
                   check=True)
    lib = C.CDLL(so)
    lib.orient_host.argtypes = [C.c_int, L._ip, L._dp, L._bp, L._bp, C.c_int]
    lib.winding_host.argtypes = [C.c_int, L._ip, L._dp, L._bp, L._bp, C.c_int]
    return lib


def _host_run(fn, shape, arg, colors=True):
    co = np.ascontiguousarray(shape.contour_offsets, np.int32)
    pts = np.ascontiguousarray(shape.points, np.float64).reshape(-1, 8).copy()
    if not len(pts):
        pts = np.zeros((1, 8))
    types = np.ascontiguousarray(shape.types, np.uint8).copy()
    types = types if len(types) else np.ones(1, np.uint8)
    cols = np.ascontiguousarray(shape.colors, np.uint8).copy() if colors else None
    r = fn(shape.n_contours, L.ptr(co, L._ip), L.ptr(pts, L._dp), L.ptr(types, L._bp), L.ptr(cols, L._bp) if colors else None, arg)
    ne = shape.n_edges
    return r, OC.FlatShape(co, pts[:ne], types[:ne].astype(np.int32), cols[:ne].astype(np.int32) if colors else np.full(ne, OC.WHITE, np.int32), shape.inverse_y)


def _shape_sets():
    z = load_npz("prep.npz")
    raw = ShapeBatch(z["raw_gco"].astype(np.int32), z["raw_co"].astype(np.int32), z["raw_points"], z["raw_types"].astype(np.int32),
                     z["raw_colors"].astype(np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    cjk = ShapeBatch.from_shapes([synth.cjk_like_shape(500+k) for k in range(40)])
    hand = OC.hand_built_batch()
    out = []
    for name, b in (("prep", raw), ("cjk", cjk), ("hand", hand)):
        out += [(name, b), (name+"-perturbed", OC.perturbed(b))]
    return out


def test_host_orient_contours_equals_the_reference(ref, host):
    """orientGlyphWave (hits by atomic slot, rank by counting, votes by atomic adds; LDS or global votes, LDS and global hits) == Shape::orientContours,
    bit for bit, with and without colours."""
    for name, batch in _shape_sets():
        for g in range(batch.n_glyphs):
            s = batch.shape(g)
            h = ref.shape_from_flat(s)
            ref.lib.ref_shape_orient_contours(h)
            fa = ref.flatten(h)
            ref.free(h)
            want = OC.FlatShape(fa.contour_offsets, fa.points, fa.types, fa.colors)
            for colors, global_votes in ((True, 0), (False, 1)):             # (no colour array: WHITE, nothing moves)
                _, got = _host_run(host.orient_host, s, global_votes, colors)
                w = want if colors else OC.FlatShape(want.contour_offsets, want.points, want.types, np.full(want.n_edges, OC.WHITE, np.int32))
                OC.same_batch(ShapeBatch.from_shapes([got]), ShapeBatch.from_shapes([w]), "%s glyph %d colours %s" % (name, g, colors))


def test_host_winding_guess_equals_the_reference(ref, host):
    """windingGlyphWave on normalized glyphs: the decision of -guesswinding (and the reversal) equals the reference's, for orient on and off."""
    flips = 0
    for name, batch in _shape_sets():
        for orient in (False, True):
            for g in range(batch.n_glyphs):
                s = batch.shape(g)
                base = OC.ref_prepare(ref, s, orient, 0, True, 0)
                want = OC.ref_prepare(ref, s, orient, 2, True, 0)
                rev, got = _host_run(host.winding_host, base, 2)
                OC.same_batch(ShapeBatch.from_shapes([got]), ShapeBatch.from_shapes([want]), "%s glyph %d orient %s" % (name, g, orient))
                flips += rev
                _, got = _host_run(host.winding_host, base, 1)
                OC.same_batch(ShapeBatch.from_shapes([got]), ShapeBatch.from_shapes([OC.ref_prepare(ref, s, orient, 1, True, 0)]), "reverse")
    assert flips > 0
