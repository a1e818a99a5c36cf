"""Box sizes on the device (msdf_frame.hpp: Shape::getBounds with border and miters -- mitersGlyphWave -- and the box rule -- boxGlyph, planBox) without a
GPU: the helpers compiled for the host (tests/box_host) against the reference's recorded bounds (tests/golden/boxes.npz, tools/make_golden_boxes.py),
against the compiled reference's own getBounds(border, miterLimit, polarity) called now, and against the box rule written out in numpy; and the C ABI's
answers to configurations that cannot be used -- all before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from msdfgen_amd import lib as L
from msdfgen_amd.shape import FlatShape
import boxcases as BC

W = 7


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return BC.build_host(tmp_path_factory.mktemp("box_host"))


@pytest.fixture(scope="module")
def gold():
    return BC.golden()


@pytest.fixture(scope="module")
def refb(ref):
    return BC.RefBounds(ref)


def test_box_entry_points_are_exported():
    lib = L.load()
    for name in ("msdfhip_batch_bounds_miters", "msdfhip_batch_boxes"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTED_SYMBOLS, name
    assert lib.msdfhip_abi_version() == 5
    assert C.sizeof(L.BoxConfig) == 56


def test_fixture_is_what_its_recorder_promises(gold):
    z, arrays, raw, prep = gold
    n = int(z["n_set"])
    assert n == 159 and arrays.n_glyphs == n+5 and raw.n_glyphs == prep.n_glyphs == 4
    assert tuple(map(tuple, z["matrix"])) == BC.MATRIX and z["bounds"].shape == (arrays.n_glyphs, 45, 4) and z["raw_bounds"].shape == (4, 45, 4)
    assert not np.isnan(z["bounds"]).any() and not np.isnan(z["raw_bounds"]).any()
    names = list(arrays.names)
    assert [arrays.shape(names.index(k)).n_edges for k in ("hand/ring63", "hand/ring64", "hand/cubic_loop", "hand/ring60_star8", "hand/ring1000")] == [63, 64, 1, 68, 1000]
    two = arrays.shape(names.index("hand/ring60_star8"))
    assert list(two.contour_offsets) == [0, 60, 68]
    b = z["bounds"][:n]
    border_only = b[:, BC.combo(.125, 0., 0)]
    moved = lambda limit, p: int((b[:, BC.combo(.125, limit, p)].view(np.uint64) != border_only.view(np.uint64)).any(1).sum())
    assert moved(4., 0) >= 60 and moved(4., 1) >= 30 and moved(4., -1) >= 30
    assert (b[:, BC.combo(.125, 4., 1)].view(np.uint64) != b[:, BC.combo(.125, 4., -1)].view(np.uint64)).any()
    assert moved(1., 0) == 0                                              # a miter of length 1 lies on the border circle: inside border-only bounds
    assert int(BC.no_box(b[:, BC.combo(0., 0., 0)]).sum()) == 4


def test_host_miters_equal_the_recorded_reference_bounds(host, gold):
    """Every array shape of the fixture over the whole matrix, all four doubles bit-equal: incl. the joins whose previous edge lies in a later pass (ring64:
    lane 0 pairs with lane 63; ring1000: with the 16th pass), is the edge itself (cubic_loop), or sits at lane 59 next to another contour's edges."""
    z, arrays, _, _ = gold
    for g in range(arrays.n_glyphs):
        assert_bit_equal(BC.HostShape(arrays.shape(g)).matrix(host), z["bounds"][g], arrays.names[g])


def test_host_composition_on_raw_outlines_equals_the_recorded_one(host, gold):
    """Plain bounds fixed after normalize, miters over the oriented, coloured edges (what k_box reads of a batch prepared from raw outlines)."""
    z, _, _, prep = gold
    for g in range(prep.n_glyphs):
        assert_bit_equal(BC.HostShape(prep.shape(g)).matrix(host, plain=z["raw_plain"][g]), z["raw_bounds"][g], prep.names[g])


def test_recorded_bounds_equal_the_compiled_reference(refb, gold):
    z, arrays, raw, _ = gold
    for g in range(arrays.n_glyphs):
        assert_bit_equal(z["bounds"][g], refb.matrix(arrays.shape(g)), "recorded "+arrays.names[g])
    for g in range(raw.n_glyphs):
        h, plain = BC.ref_raw(refb.ref, raw.shape(g))
        want = np.stack([refb.composed(plain, h, b, m, p) for (b, m, p) in BC.MATRIX])
        refb.ref.free(h)
        assert_bit_equal(z["raw_plain"][g], plain, "recorded plain "+raw.names[g])
        assert_bit_equal(z["raw_bounds"][g], want, "recorded composition "+raw.names[g])


def _live(host, refb, shapes):
    n = 0
    for name, s in shapes:
        want = refb.matrix(s)
        assert_bit_equal(BC.HostShape(s).matrix(host), want, name)
        n += int((want[BC.combo(.125, 4., 0)].view(np.uint64) != want[BC.combo(.125, 0., 0)].view(np.uint64)).any())
    return n


def test_host_miters_equal_the_compiled_reference_on_the_geometry_cases(host, refb):
    """tests/geomcases.py as they are (not normalized): lattice ties, coincident and degenerate edges (zero-length directions: normalize(true) gives the zero
    vector, q = .5, the miter point is point(0) itself), slivers."""
    import geomcases as GC
    cs = GC.cases()
    assert len(cs) >= 40
    assert _live(host, refb, [(c.name, c.shape) for c in cs]) >= 10


def test_host_miters_equal_the_compiled_reference_on_the_orientation_cases(host, refb):
    """tests/orientcases.py: empty contours between others and alone, no contours, single-edge contours, a 2 100-edge contour, 600 and 900 contours. (Most are
    made of rectangles, whose miters end exactly on the corner of the border-only bounds: few of them move.)"""
    import orientcases as OC
    assert _live(host, refb, OC.hand_built()) >= 1


def test_host_miters_equal_the_compiled_reference_on_random_outlines(host, refb):
    """300 seeded outlines of tests/fuzzlib.py's kinds, raw."""
    import fuzzlib
    rng = np.random.default_rng(0xb0c5)
    shapes = [("fuzz/%d/kind%d" % (k, k % 7), fuzzlib._shape(rng, k % 7, 7000+k)) for k in range(300)]
    assert _live(host, refb, shapes) >= 100


def test_gates_and_nan_follow_the_reference(host, refb):
    """border <= 0 or NaN changes nothing whatever the limit; a NaN control point never enters through a miter; a negative border is no border."""
    pts = [(float(k % 7)+1, float(k % 5)+1) for k in range(70)]
    pts[3], pts[66] = (0., 1.), (float("nan"), 2.)
    s = FlatShape.from_contours([[(W, pts[k], pts[(k+1) % 70]) for k in range(70)]])
    hs = BC.HostShape(s)
    h = refb.ref.shape_from_flat(s)
    for (border, limit, pol) in ((0., 4., 0), (-1., 4., 0), (float("nan"), 4., 1), (.5, -1., 0), (.5, float("nan"), 0), (.5, 4., 0), (.5, 4., -1), (.5, 1e300, 1), (1e300, 4., 0)):
        want = refb.bounds(h, border, limit, pol)
        got = hs.miters(host, border, limit, pol)
        assert not np.isnan(got).any()
        assert_bit_equal(got, want, "gates %s" % ((border, limit, pol),))
    refb.ref.free(h)


# ---- the box rule ---------------------------------------------------------------------------------------------------------------------------------------

def box_rule(s, lo, hi, align, plain, ext):
    """The rule of msdfhip_batch_boxes (msdfgen_hip.h), operation for operation in float64."""
    s, lo, hi = np.float64(s), np.float64(lo), np.float64(hi)
    plain, ext = np.asarray(plain, np.float64), np.asarray(ext, np.float64)
    side, tr = [np.float64(0), np.float64(0)], [np.float64(0), np.float64(0)]
    with np.errstate(all="ignore"):
        if plain[0] < plain[2] and plain[1] < plain[3]:
            for axis in (0, 1):
                l, r = ext[axis], ext[axis+2]
                if align[axis]:
                    sl, sr = np.floor(s*l-.5), np.ceil(s*r+.5)
                    side[axis] = sr-sl
                    tr[axis] = -sl/s
                else:
                    d = s*(r-l)
                    side[axis] = np.ceil(d)+1
                    tr[axis] = -l+(.5*(side[axis]-d))/s
        wh = np.array([int(v) if 0 <= v <= 2.**30 else -1 for v in side], np.int32)
        return wh, np.array([s, s, tr[0], tr[1], 1/(hi-lo), -lo])


BOX_BOUNDS = ((0., 0., 8., 10.), (-0., -0., 8., 10.), (-3.25, -7.5, -1.125, -.0625), (-5.3, -2.1, 0., -0.), (1e15, 1e15, 1e15+8, 1e15+4), (-1e15, -1e15, 1e15, 1e15),
              (.1, .2, .30000000000000004, .7), (-.5, -.5, .5, .5), (0., 0., 1./3, 1e-3), (-1e-9, 2., 1e-9, 2.+1e-9))
BOX_RANGES = ((1, -2., 2.), (1, -1., 3.), (1, 0., 4.), (0, -.125, .125), (0, -.0625, .25))
BOX_SCALES = (1., 32., 1./3, 1e-3)


def test_box_function_equals_the_rule_written_out(host):
    """Aligned and not, per axis; pixel and unit ranges; the four scales; bounds at +-0, at negative coordinates, at 1e15 (where s*l - .5 rounds to s*l), a
    box beyond 2^30 (-1). The extended bounds are the plain ones grown by the border, and once more by an uneven push as the miters make it."""
    n = boxes = 0
    for s in BOX_SCALES:
        for (mode, lower, upper) in BOX_RANGES:
            status, (ps, lo, hi, border) = BC.host_plan(host, s, mode, lower, upper)
            assert status == 0 and ps == s
            assert_bit_equal(np.array([lo, hi, border]), np.array([np.float64(lower)/s, np.float64(upper)/s, -(np.float64(lower)/s)] if mode else [lower, upper, -lower]), "planBox")
            for plain in BOX_BOUNDS:
                p = np.array(plain)
                for push in ((0., 0., 0., 0.), (.375, 0., 1.0625, 2.5)):
                    ext = np.array([p[0]-border-push[0], p[1]-border-push[1], p[2]+border+push[2], p[3]+border+push[3]])
                    for align in ((0, 0), (1, 1), (1, 0), (0, 1)):
                        wh, xf = BC.host_box(host, s, lo, hi, align, p, ext)
                        want_wh, want_xf = box_rule(s, lo, hi, align, p, ext)
                        assert (wh == want_wh).all(), (s, mode, lower, plain, push, align, wh, want_wh)
                        assert_bit_equal(xf, want_xf, "xf %s" % ((s, mode, lower, plain, push, align),))
                        n += 1
                        boxes += int((wh > 0).all())
                        if (wh > 0).all():                                  # the box contains the extended bounds
                            for axis in (0, 1):
                                assert 0 <= s*(ext[axis]+xf[2+axis]) and s*(ext[axis+2]+xf[2+axis]) <= wh[axis], (s, plain, push, align, axis)
    assert n == 4*5*10*2*4 and boxes > n//2


def test_a_glyph_without_plain_bounds_has_no_box(host):
    for plain in ((1e240, 1e240, -1e240, -1e240), (3., 4., 3., 4.), (2., 1., 2., 9.), (1., 5., 7., 5.)):
        p = np.array(plain)
        ext = np.array([p[0]-2, p[1]-2, p[2]+2, p[3]+2])
        for align in ((0, 0), (1, 1)):
            wh, xf = BC.host_box(host, 32., -.0625, .0625, align, p, ext)
            assert (wh == 0).all()
            assert_bit_equal(xf, np.array([32., 32., 0., 0., 1/np.float64(.125), .0625]), "no box")


def test_overflowing_and_nan_boxes_carry_the_marker(host):
    p = np.array([0., 0., 2.**26, 1.])
    wh, _ = BC.host_box(host, 32., -.0625, .0625, (0, 0), p, p)
    assert wh[0] == -1 and wh[1] == 33
    wh, _ = BC.host_box(host, 32., -.0625, .0625, (1, 1), p, p)
    assert wh[0] == -1 and wh[1] == 34                                      # floor(-.5) = -1 to ceil(32.5) = 33
    p = np.array([0., 0., 2.**25-1./32, 1.])                                # exactly 2^30 texels wide once the edge texel is added: still a box
    wh, _ = BC.host_box(host, 32., -.0625, .0625, (0, 0), p, p)
    assert wh[0] == 2**30
    e = np.array([0., -np.inf, 1., 1.])
    wh, _ = BC.host_box(host, 1., -1., 1., (0, 0), np.array([0., 0., 1., 1.]), e)
    assert wh[0] == 2 and wh[1] == -1
    e = np.array([np.nan, 0., 1., 1.])
    for align in ((0, 0), (1, 1)):
        wh, _ = BC.host_box(host, 1., -1., 1., align, np.array([0., 0., 1., 1.]), e)
        assert wh[0] == -1 and wh[1] > 0


def test_plan_refuses_each_bad_field(host):
    good = (32., 1, -2., 2., (0, 1))
    assert BC.host_plan(host, *good)[0] == 0
    inf, nan = float("inf"), float("nan")
    for scale in (0., -1., inf, nan):
        assert BC.host_plan(host, scale, 1, -2., 2.)[0] == 1, scale
    for mode in (-1, 2):
        assert BC.host_plan(host, 32., mode, -2., 2.)[0] == 2, mode
    for (lower, upper) in ((2., 2.), (1., -1.), (.5, 2.), (-inf, 2.), (-2., inf), (nan, 2.), (-2., nan)):
        for mode in (0, 1):
            assert BC.host_plan(host, 32., mode, lower, upper)[0] == 3, (lower, upper)
    assert BC.host_plan(host, 1e-300, 1, -1e10, 1e10)[0] == 3              # the pixel range in shape units overflows
    for align in ((2, 0), (0, -1)):
        assert BC.host_plan(host, 32., 1, -2., 2., align)[0] == 4, align
    status, (s, lo, hi, border) = BC.host_plan(host, 3., 1, 0., 4.)         # lower == 0: no border, so no miters either
    assert status == 0 and border == 0 and hi == np.float64(4.)/3


def test_unusable_box_configs_are_refused_before_the_device():
    """Every bad field from msdfhip_batch_boxes, with nothing read (the batch is NULL) and nothing written."""
    lib = L.load()
    sizes, xf = np.zeros((1, 2), np.int32), np.zeros((1, 6))

    def call(cfg):
        return lib.msdfhip_batch_boxes(None, C.byref(cfg) if cfg is not None else None, L.ptr(sizes, L._ip), L.ptr(xf, L._dp), None)

    bad = ((L.BoxConfig(0., 1, -2., 2., 4., 1, 0, 0), b"scale"), (L.BoxConfig(float("inf"), 1, -2., 2., 4., 1, 0, 0), b"scale"),
           (L.BoxConfig(32., 2, -2., 2., 4., 1, 0, 0), b"range_mode"), (L.BoxConfig(32., 1, 2., 2., 4., 1, 0, 0), b"range_lower < range_upper"),
           (L.BoxConfig(32., 0, .5, 2., 4., 1, 0, 0), b"range_lower <= 0"), (L.BoxConfig(32., 1, -2., float("nan"), 4., 1, 0, 0), b"finite"),
           (L.BoxConfig(32., 1, -2., 2., 4., 1, 2, 0), b"align"), (None, b"NULL config"))
    for cfg, word in bad:
        assert call(cfg) == L.ERR_INVALID, word
        assert word in lib.msdfhip_last_error(), (word, lib.msdfhip_last_error())
    good = L.BoxConfig(32., 1, -2., 2., float("nan"), -7, 1, 1)             # no miter limit and no polarity is invalid; the NULL batch is
    assert call(good) == L.ERR_INVALID and b"NULL argument" in lib.msdfhip_last_error()
    assert lib.msdfhip_batch_bounds_miters(None, .125, 4., 0, None) == L.ERR_INVALID
    assert not sizes.any() and not xf.any()
