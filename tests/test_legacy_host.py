"""The legacy generators and the legacy error correction (msdf_legacy.hpp) without a GPU: the texel function and the clash passes compiled for the host
(tests/legacy_host) against the recorded reference (tests/golden/legacy.npz, tools/make_golden_legacy.py) and, where it is built, the compiled
reference called now; the correction that follows the legacy field in modes 3 and 4 is the product's own pass as tests/hostemu runs it. Plus the C
ABI's surface: the four entry points, the ABI version, and the refusals, which come before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from msdfgen_amd import lib as L
import legacycases as LC

NAMES = ("msdfhip_generate_legacy", "msdfhip_batch_generate_legacy", "msdfhip_error_correction_legacy", "msdfhip_batch_error_correction_legacy")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return LC.build_host(tmp_path_factory.mktemp("legacy_host"))


@pytest.fixture(scope="module")
def gold():
    return LC.golden()


@pytest.fixture(scope="module")
def emu():
    from emu import Emu
    return Emu()


def test_legacy_entry_points_are_exported():
    lib = L.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in L.EXPORTED_SYMBOLS, name
    assert lib.msdfhip_abi_version() == 5
    assert C.sizeof(L.Config) == 48 and C.sizeof(L.Glyph) == 64           # no struct changed


def test_fixture_covers_what_it_should(gold):
    batch, recs, ecs = gold
    assert {(r.w, r.h) for r in recs} >= set(LC.SIZES)
    assert {r.mode for r in recs} == {1, 2, 3, 4} and {r.ec for r in recs if r.mode >= 3} == {0, 1, 2, 3}
    assert sum(r.sign for r in recs) == 2 and sum(r.stencil is not None for r in recs) == 4
    assert {(bool(batch.inverse_y[r.shape]), r.y_down) for r in recs if r.stencil is not None} == {(False, False), (False, True), (True, False), (True, True)}
    assert max(r.w for r in recs) <= 40 and max(r.h for r in recs) <= 32
    assert {(e.n, e.w, e.h, e.tx, e.ty) for e in ecs} == {(n, w, h, tx, ty) for n in (3, 4) for (w, h) in LC.EC_SIZES for (tx, ty) in LC.EC_THRESHOLDS}
    for name in ("empty", "yellow", "ring65", "ring129", "blobs", "cubic_teardrop", "shape_a_ydown"):
        assert name in batch.names


def corrected(emu, shape, r, field, stencil=None):
    """msdfErrorCorrection without the distance check and without overlap support on the legacy field, as generateMSDF_legacy runs it: along the
    shape's rows (msdfgen.cpp:223)."""
    if r.mode < 3 or r.ec == 0:
        return field
    return emu.generate(shape, r.mode, r.w, r.h, r.xf, overlap=False, ec_mode=r.ec, ec_dist=0, y_down=r.y_down, correct_only=field, stencil=stencil, shape_rows=True)


def test_host_texels_equal_the_recorded_reference(host, gold, emu):
    """Every generator record without the sign pass: the raw legacy field where the correction is off, else the field corrected by the product's pass."""
    batch, recs, _ = gold
    checked = 0
    for r in (r for r in recs if not r.sign):
        shape = batch.shape(r.shape)
        field = LC.host_generate(host, shape, r.mode, r.w, r.h, r.xf, r.y_down)
        stencil = np.zeros((r.h, r.w), np.uint8) if r.stencil is not None else None
        assert_bit_equal(corrected(emu, shape, r, field, stencil), r.out, r.name)
        if stencil is not None:                                                # hostemu writes the bitmap's memory rows; the reference's stencil rows go upward
            assert_bit_equal(stencil[::-1] if r.y_down else stencil, r.stencil, "stencil of "+r.name)
        checked += 1
    assert checked == len(recs)-2


def test_ties_keep_the_first_edge_in_shape_order(host, gold):
    """A square and the same square walked the other way round: every texel is equidistant from an edge of each, with the same alignment and opposite
    signs, and the strict `<` keeps the first in shape order -- so swapping the two contours must flip the field's sign about the range's centre: the
    order of the walk is really what decides. (The recorded reference fields of this and the other tied outlines are compared above.)"""
    from msdfgen_amd.shape import FlatShape
    batch, recs, _ = gold
    r = next(r for r in recs if r.name == "coincident/reversed")
    shape = batch.shape(r.shape)
    n = shape.n_edges//2
    order = np.r_[n:2*n, 0:n]
    swapped = FlatShape(shape.contour_offsets, shape.points[order], shape.types[order], shape.colors[order], shape.inverse_y)
    a = LC.host_generate(host, shape, 1, r.w, r.h, r.xf, r.y_down)
    b = LC.host_generate(host, swapped, 1, r.w, r.h, r.xf, r.y_down)
    off = a != .5                                                              # (texels on the outline: distance 0 either way)
    assert off.sum() > a.size//2
    assert (np.sign(a-.5)[off] == -np.sign(b-.5)[off]).all()
    assert np.abs((a-.5)+(b-.5)).max() <= 2.**-23                             # (the same |distance|, rounded to float on either side of .5)


def test_host_texels_equal_the_compiled_reference(ref, host, gold):
    """The same against generate*_legacy called now with the correction disabled, and the recorded raw fields themselves."""
    batch, recs, _ = gold
    rl = LC.RefLegacy(ref)
    for r in (r for r in recs if not r.sign):
        shape = batch.shape(r.shape)
        want = rl.generate(shape, r.mode, r.w, r.h, r.xf, ec_mode=0, y_down=r.y_down)
        assert_bit_equal(LC.host_generate(host, shape, r.mode, r.w, r.h, r.xf, r.y_down), want, r.name)
        if r.mode < 3 or r.ec == 0:
            assert_bit_equal(r.out, want, "recorded "+r.name)
        else:
            assert_bit_equal(r.out, rl.generate(shape, r.mode, r.w, r.h, r.xf, ec_mode=r.ec, y_down=r.y_down), "recorded "+r.name)


def test_host_clash_passes_equal_the_recorded_reference(host, gold):
    _, _, ecs = gold
    for e in ecs:
        got = LC.host_correction(host, e.field, e.tx, e.ty)
        assert_bit_equal(got, e.out, "legacy correction %dx%dx%d (%g, %g)" % (e.w, e.h, e.n, e.tx, e.ty))
        if e.n == 4:
            assert_bit_equal(got[..., 3], e.field[..., 3], "alpha")
        if min(e.w, e.h) >= 2:
            assert (e.out.view(np.uint32) != e.field.view(np.uint32)).any()


def test_host_clash_passes_equal_the_compiled_reference(ref, host, gold):
    _, _, ecs = gold
    rl = LC.RefLegacy(ref)
    rng = np.random.default_rng(7)
    fields = [(e.field, e.tx, e.ty) for e in ecs]+[(rng.uniform(0, 1, (h, w, n)).astype(np.float32), .2, .4) for n in (3, 4) for (w, h) in ((3, 2), (16, 9))]
    for field, tx, ty in fields:
        assert_bit_equal(LC.host_correction(host, field, tx, ty), rl.correction(field, tx, ty), "legacy correction %s" % (field.shape,))


def test_legacy_launch_plans(host):
    """msdf_launchplan.hpp: a wavefront per tile of every glyph; two passes over all texels through a scratch of the tiles' size."""
    assert LC.host_plan(host, 9, 40, 32, 3) == (9*5*4, 0, 9*40*32, 9*40*32*3, (9*40*32+255)//256)
    assert LC.host_plan(host, 1, 1, 1, 4) == (1, 0, 1, 4, 1)
    assert LC.host_plan(host, 0, 8, 8, 3)[:2] == (0, 0) and LC.host_plan(host, 0, 8, 8, 3)[4] == 0
    assert LC.host_plan(host, 5, 0, 8, 3)[4] == 0
    assert LC.host_plan(host, 1 << 20, 512, 512, 3)[1] == 1                   # 2^32 tiles: beyond the grid
    assert LC.host_plan(host, 8192, 64, 64, 3)[4] == 65536                    # grid-stride beyond 65 536 workgroups


def test_bad_arguments_are_refused_before_any_device_work(gold):
    """mode outside 1..4, channels other than 3 / 4, a NULL the call needs: MSDFHIP_ERR_INVALID, outputs untouched. Zero-size bitmaps: a no-op."""
    lib = L.load()
    batch, _, _ = gold
    shape = batch.shape(0)
    co, pts, types, colors = LC.shape_arrays(shape)
    sargs = (L.ptr(co, L._ip), shape.n_contours, L.ptr(pts, L._dp), L.ptr(types, L._bp), L.ptr(colors, L._bp))
    xf = np.array([1., 1., 0., 0., .25, 2.])
    cfg = L.Config()
    lib.msdfhip_default_config(C.byref(cfg))
    px = np.full((4, 4, 3), 7., np.float32)
    stencil = np.full((4, 4), 9, np.uint8)
    for mode in (0, 5, -1):
        assert lib.msdfhip_generate_legacy(mode, L.ptr(px, L._fp), 4, 4, 12, 0, *sargs, L.ptr(xf, L._dp), C.byref(cfg), L.ptr(stencil, L._bp)) == L.ERR_INVALID
        assert b"mode" in lib.msdfhip_last_error()
        assert lib.msdfhip_batch_generate_legacy(None, mode, 4, 4, None, None, None, None, C.byref(cfg), None) == L.ERR_INVALID
    assert lib.msdfhip_generate_legacy(3, L.ptr(px, L._fp), 4, 4, 12, 0, *sargs, L.ptr(xf, L._dp), None, None) == L.ERR_INVALID           # no config
    assert lib.msdfhip_generate_legacy(3, None, 4, 4, 12, 0, *sargs, L.ptr(xf, L._dp), C.byref(cfg), None) == L.ERR_INVALID               # no bitmap
    assert lib.msdfhip_generate_legacy(3, L.ptr(px, L._fp), 4, 4, 12, 0, None, *sargs[1:], L.ptr(xf, L._dp), C.byref(cfg), None) == L.ERR_INVALID   # no offsets
    assert lib.msdfhip_generate_legacy(3, L.ptr(px, L._fp), 4, 4, 12, 0, *sargs, None, C.byref(cfg), None) == L.ERR_INVALID               # no transformation
    assert lib.msdfhip_generate_legacy(3, L.ptr(px, L._fp), -1, 4, 12, 0, *sargs, L.ptr(xf, L._dp), C.byref(cfg), None) == L.ERR_INVALID
    bad = L.Config()
    lib.msdfhip_default_config(C.byref(bad))
    bad.ec_mode = 4
    assert lib.msdfhip_generate_legacy(3, L.ptr(px, L._fp), 4, 4, 12, 0, *sargs, L.ptr(xf, L._dp), C.byref(bad), None) == L.ERR_INVALID
    assert lib.msdfhip_batch_generate_legacy(None, 3, 4, 4, None, None, None, None, C.byref(cfg), None) == L.ERR_INVALID                  # no batch
    for channels in (0, 1, 2, 5):
        assert lib.msdfhip_error_correction_legacy(channels, L.ptr(px, L._fp), 4, 4, 12, .3, .3) == L.ERR_INVALID
        assert lib.msdfhip_batch_error_correction_legacy(None, 1, 4, 4, channels, None, .3, .3, None) == L.ERR_INVALID
    assert b"channels" in lib.msdfhip_last_error()
    assert lib.msdfhip_error_correction_legacy(3, None, 4, 4, 12, .3, .3) == L.ERR_INVALID
    assert lib.msdfhip_batch_error_correction_legacy(None, 1, 4, 4, 3, None, .3, .3, None) == L.ERR_INVALID
    assert lib.msdfhip_batch_error_correction_legacy(None, -1, 4, 4, 3, None, .3, .3, None) == L.ERR_INVALID
    # zero-size bitmaps
    assert lib.msdfhip_generate_legacy(3, L.ptr(px, L._fp), 0, 4, 0, 0, *sargs, L.ptr(xf, L._dp), C.byref(cfg), L.ptr(stencil, L._bp)) == 0
    assert lib.msdfhip_generate_legacy(1, None, 4, 0, 4, 0, *sargs, L.ptr(xf, L._dp), C.byref(cfg), None) == 0
    assert lib.msdfhip_error_correction_legacy(3, L.ptr(px, L._fp), 4, 0, 12, .3, .3) == 0
    assert lib.msdfhip_error_correction_legacy(4, None, 0, 0, 0, .3, .3) == 0
    assert lib.msdfhip_batch_error_correction_legacy(None, 0, 4, 4, 3, None, .3, .3, None) == 0
    assert lib.msdfhip_batch_error_correction_legacy(None, 3, 0, 4, 4, None, .3, .3, None) == 0
    assert (px == 7.).all() and (stencil == 9).all()
