"""The framing families of tests/xformcases.py on the CPU: their premises, the plain-C oracle against the compiled reference (where oracle/_ref
exists), and the device headers compiled for the host (tests/emu.py: the kernels' tile cull and error correction) against the oracle. This is
what makes the oracle a valid reference for tests/test_gpu_transforms.py on these inputs."""
import ctypes as C

import numpy as np
import pytest

import xformcases as X
from conftest import assert_bit_equal
from msdfgen_amd.shape import autoframe

EC_PAIRS = [(m, d) for m in range(4) for d in range(3)]


@pytest.fixture(scope="module")
def emu():
    from emu import Emu
    return Emu()


@pytest.mark.parametrize("family", X.FAMILIES)
def test_family_premises(oracle, family):
    cs = X.cases((family,), seeds=(0, 1))
    assert len(cs) >= 4
    for c in cs:
        X.check_premise(c, oracle)
    if family == "tiny_bitmaps":
        assert {(c.w, c.h) for c in cs} == set(X.TINY_SIZES)
        return
    if family in X.MIRRORS:
        assert {(bool(c.shape.inverse_y), c.y_down) for c in cs} == {(a, b) for a in (False, True) for b in (False, True)}
    for c in cs:                                                  # the autoframe case is not a member of any family
        auto = c._replace(xf=autoframe(c.shape.bounds(), c.w, c.h, 2.))
        with pytest.raises(AssertionError):
            X.check_premise(auto, oracle)


def test_fixed_size_cases_keep_their_premises(oracle):
    """The batched GPU test puts every family but tiny_bitmaps into one bitmap size."""
    for c in X.cases(tuple(f for f in X.FAMILIES if f != "tiny_bitmaps"), seeds=(0, 1), w=41, h=27):
        assert (c.w, c.h) == (41, 27)
        X.check_premise(c, oracle)


@pytest.mark.parametrize("family", X.FAMILIES)
def test_oracle_matches_reference_under_framing(oracle, ref, family):
    """All four modes, both combiners; msdf / mtsdf with every error-correction mode x distance check, stencils compared."""
    for c in X.cases((family,), seeds=(0,)):
        for ov in (True, False):
            for mode in (1, 2):
                a = ref.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, y_down=c.y_down)
                b = oracle.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, y_down=c.y_down)
                assert_bit_equal(b, a, "%s mode %d overlap %d" % (c.name, mode, ov))
            for mode in (3, 4):
                for ec, dc in EC_PAIRS:
                    sa, sb = np.zeros((c.h, c.w), np.uint8), np.zeros((c.h, c.w), np.uint8)
                    a = ref.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, ec_mode=ec, ec_dist=dc, y_down=c.y_down, stencil=sa)
                    b = oracle.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, ec_mode=ec, ec_dist=dc, y_down=c.y_down, stencil=sb)
                    what = "%s mode %d overlap %d ec %d/%d" % (c.name, mode, ov, ec, dc)
                    assert_bit_equal(b, a, what)
                    assert (sa == sb).all(), what+": stencil"


@pytest.mark.parametrize("family", X.FAMILIES)
def test_host_build_of_the_kernels_matches_oracle_under_framing(oracle, emu, family):
    """The kernels' tile cull (msdf_cull.hpp) and correction (msdf_ec.hpp) compiled for the host, against the oracle. In zoom_in and aniso the cull
    must really drop edges: tiles deep inside / outside the glyph, and tiles eight times taller than wide in shape space."""
    kept, total = C.c_long(), C.c_long()
    emu.lib.emu_cull_stats(C.byref(kept), C.byref(total), 1)
    for i, c in enumerate(X.cases((family,), seeds=(0,))):
        for ov in (True, False):
            for mode in (1, 2):
                a = oracle.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, y_down=c.y_down)
                b = emu.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, y_down=c.y_down)
                assert_bit_equal(b, a, "%s mode %d overlap %d" % (c.name, mode, ov))
            for mode in (3, 4):
                for k in range(3):
                    ec, dc = EC_PAIRS[(4*i+3*k+mode+ov) % len(EC_PAIRS)]
                    sa, sb = np.zeros((c.h, c.w), np.uint8), np.zeros((c.h, c.w), np.uint8)
                    a = oracle.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, ec_mode=ec, ec_dist=dc, y_down=c.y_down, stencil=sa)
                    b = emu.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, ec_mode=ec, ec_dist=dc, y_down=c.y_down, stencil=sb)
                    what = "%s mode %d overlap %d ec %d/%d" % (c.name, mode, ov, ec, dc)
                    assert_bit_equal(b, a, what)
                    assert ((sa[::-1] if c.y_down else sa) == sb).all(), what+": stencil"     # the host build keeps the bitmap's memory rows
    emu.lib.emu_cull_stats(C.byref(kept), C.byref(total), 1)
    assert 0 < kept.value <= total.value
    if family in ("zoom_in", "aniso"):
        assert kept.value < .8*total.value, (family, kept.value, total.value)


def test_oracle_standalone_passes_match_reference_under_framing(oracle, ref):
    """What tests/test_gpu_transforms.py runs besides generate: the standalone correction, the sign pass and rasterize with every fill rule,
    estimateSDFError, and renderSDF from 1-texel-wide fields into 1x1 outputs and with an inverted range."""
    fams = X.MIRRORS+("aniso", "zoom_in", "zoom_out", "nondivsafe", "far_coords", "neg_range")
    cs = X.cases(fams, seeds=(0,))+X.cases(("tiny_bitmaps",), seeds=(0,))
    for i, c in enumerate(cs):
        for mode in (3, 4):
            pre = oracle.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
            ov = bool(i & 1)
            for ec, dc in ((2, 1), (1, 2), (3, 0)):
                sa, sb = np.zeros((c.h, c.w), np.uint8), np.zeros((c.h, c.w), np.uint8)
                a = ref.error_correction(c.shape, pre, c.xf, overlap=ov, ec_mode=ec, ec_dist=dc, y_down=c.y_down, stencil=sa)
                b = oracle.error_correction(c.shape, pre, c.xf, overlap=ov, ec_mode=ec, ec_dist=dc, y_down=c.y_down, stencil=sb)
                assert_bit_equal(b, a, "%s error_correction mode %d ec %d/%d" % (c.name, mode, ec, dc))
                assert (sa == sb).all()
        for mode in (1, 3):
            field = oracle.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
            for rule in range(4):
                assert_bit_equal(oracle.sign_correction(c.shape, field, c.xf, .5, rule, y_down=c.y_down),
                                 ref.sign_correction(c.shape, field, c.xf, .5, rule, y_down=c.y_down), "%s sign correction rule %d" % (c.name, rule))
            for spr, rule in ((1, 0), (3, 1)):
                if c.xf[0] < 0 and c.w > 1 and c.h > 1:
                    continue                                      # the reference never returns there: see the next test
                a, b = ref.estimate_sdf_error(c.shape, field, c.xf, spr, rule), oracle.estimate_sdf_error(c.shape, field, c.xf, spr, rule)
                assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64), (c.name, spr, rule, a, b)
        for rule in range(4):
            assert_bit_equal(oracle.rasterize(c.shape, c.w, c.h, c.xf, rule, y_down=c.y_down), ref.rasterize(c.shape, c.w, c.h, c.xf, rule, y_down=c.y_down),
                             "%s rasterize rule %d" % (c.name, rule))
        if c.name.startswith("tiny_bitmaps"):
            for mode, n_out in ((1, 3), (3, 1), (4, 4)):
                src = oracle.generate(c.shape, mode, c.w, c.h, c.xf)
                for ow, oh in ((1, 1), (1, 7), (13, 11)):
                    for lo, hi, thr in ((0, 0, .5), (-2, 2, .5), (2, -2, .5), (1.5, -.5, .4)):
                        assert_bit_equal(oracle.render_sdf(src, ow, oh, n_out, lo, hi, thr), ref.render_sdf(src, ow, oh, n_out, lo, hi, thr),
                                         "%s renderSDF %d<-%d %dx%d (%g, %g)" % (c.name, n_out, mode, ow, oh, lo, hi))


def test_error_estimate_of_mirrored_projections(oracle, emu):
    """estimateSDFError with a negative x scale: the reference's Scanline::overlap loops forever on the reversed interval, and so did the kernel's
    sdfErrorOfLine. Both ends are now taken in ascending order: the call returns, and the host build of the kernel's helper equals the oracle."""
    cs = X.cases(("mirror_x", "mirror_xy", "mirror_y"), seeds=(0, 1))
    for c in cs:
        for mode in (1, 3, 4):
            field = oracle.generate(c.shape, mode, c.w, c.h, c.xf)
            for spr, rule in ((1, 0), (3, 1), (2, 2)):
                a, b = oracle.estimate_sdf_error(c.shape, field, c.xf, spr, rule), emu.estimate_sdf_error(c.shape, field, c.xf, spr, rule)
                assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64), (c.name, mode, spr, rule, a, b)
                assert 0 <= a <= 1, (c.name, a)
