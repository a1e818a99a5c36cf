"""The lazy protection order of k_ec_fast (msdf_kernels.hpp: ecFastBody; msdf_ec_fast.hpp: ecLazyProtect) on the device, against the oracle bit for bit.

The 40 fixture glyphs of tests/eclazycases.py through GlyphBatch.generate at 8x8 (a single tile, all of its halo outside the bitmap), 9x9 (partial tiles),
16x16 and 23x17, as msdf and mtsdf, under all nine Mode x DistanceCheckMode combinations (one of them takes the lazy order, eight must keep the eager one),
upward and downward rows (both flips), with and without a stencil buffer; and single-shape calls (k_single_call runs the same body).

Every device call is made by ONE child process (tests/eclazy_gpu_child.py) under a time limit of its own, CHILD_TIMEOUT seconds; this process never opens
the GPU and only compares what the child wrote. Expected tiles and stencils: the oracle's whole pipeline (Oracle.generate), and the oracle's error correction
alone applied to the device's own pre-correction field (Oracle.error_correction) -- both must be met bit for bit. The host program of
tests/test_ec_lazy_host.py counts, on those pre-correction fields, the kinds of texel the lazy order distinguishes, so that the comparison is known not to
be vacuous.

Wall time on one MI355X with 16 CPUs: the child 2.5 s (torch import and device start included; 304 small generate calls of 40 glyphs and 56 single calls),
each of the eight comparisons 0.05-0.14 s, the whole file 4.8 s (the bitmaps are at most 23x17: the oracle's ALWAYS_CHECK pass over 40 of them takes milliseconds)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bit_equal
import eclazycases as E
import eclazy_gpu_child as child

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 240          # seconds; the child needs two and a half


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """What the child computed on the GPU. A child that faults, hangs into its limit or returns non-zero fails every test here."""
    out = os.path.join(str(tmp_path_factory.mktemp("ec_lazy_gpu")), "device.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable]+flags+[child.__file__, out], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def glyphs():
    return child.fixture()


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("w,h", E.GPU_SIZES)
def test_batched_sweep_equals_the_oracle(device, glyphs, oracle, w, h, n):
    sub, bounds = glyphs
    xfs = child.frames(bounds, w, h)
    for yi, y_down in enumerate((False, True)):
        pre = device["pre_%d_%d_%d_%d" % (w, h, n, yi)]
        for g in range(sub.n_glyphs):
            assert_bit_equal(pre[g], oracle.generate(sub.shape(g), n, w, h, xfs[g], ec_mode=0, y_down=y_down), "pre-correction field, glyph %d" % g)
        for (mode, dist) in child.CONFIGS:
            what = "%dx%d N=%d mode %d check %d y_down %d" % (w, h, n, mode, dist, y_down)
            key = "%d_%d_%d_%d_%d_%d" % (w, h, n, yi, mode, dist)
            want = np.zeros((sub.n_glyphs, h, w, n), np.float32)
            want_st = np.zeros((sub.n_glyphs, h, w), np.uint8)
            for g in range(sub.n_glyphs):
                want[g] = oracle.error_correction(sub.shape(g), pre[g], xfs[g], ec_mode=mode, ec_dist=dist, y_down=y_down, stencil=want_st[g])
            g0 = 7 % sub.n_glyphs                                            # the whole pipeline of the oracle gives the same (one glyph per configuration)
            assert_bit_equal(want[g0], oracle.generate(sub.shape(g0), n, w, h, xfs[g0], ec_mode=mode, ec_dist=dist, y_down=y_down), what+": oracle pipeline")
            assert_bit_equal(device["tiles_"+key+"_1"], want, what+": tiles (stencil buffer given)")
            assert_bit_equal(device["tiles_"+key+"_0"], want, what+": tiles (no stencil buffer)")
            assert (device["stencil_"+key] == want_st).all(), what+": stencil"


def test_single_shape_calls_equal_the_oracle(device, glyphs, oracle):
    """k_single_call: one launch per shape, the sweep's body per tile; the lazy configuration and an eager one, stencil through ErrorCorrectionConfig.buffer."""
    sub, bounds = glyphs
    w, h = child.SINGLE_SIZE
    xfs = child.frames(bounds, w, h)
    for (mode, dist) in child.SINGLE_CONFIGS:
        for g in child.single_glyphs(sub.n_glyphs):
            for yi, y_down in enumerate((False, True)):
                key = "%d_%d_%d_%d" % (mode, dist, g, yi)
                want_st = np.zeros((h, w), np.uint8)
                want = oracle.generate(sub.shape(g), 3, w, h, xfs[g], ec_mode=mode, ec_dist=dist, y_down=y_down, stencil=want_st)
                assert_bit_equal(device["single_"+key], want, "single call "+key)
                assert (device["singlest_"+key] == want_st).all(), "single call stencil "+key


def test_the_fixture_holds_every_kind_of_texel(device, glyphs, tmp_path):
    """From the CPU counts of the host program over the DEVICE's pre-correction fields at the four sizes: conditional texels protected by an edge pair, by a
    corner, left unprotected, and unconditional ERRORs with a conditional bit all occur (8x8 alone has no edge-protected one: 10 / 90 / 1 540 / 24 over the
    four sizes when first counted); the program's own comparison of the lazy walk with the per-texel pipeline holds on these fields too."""
    sub, bounds = glyphs
    cases = []
    for (w, h) in E.GPU_SIZES:
        xfs = child.frames(bounds, w, h)
        for yi in (0, 1):
            pre = device["pre_%d_%d_3_%d" % (w, h, yi)]
            for g in range(sub.n_glyphs):
                s = sub.shape(g)
                cases.append({"w": w, "h": h, "flip": int(bool(s.inverse_y) != bool(yi)), "group": E.GROUP_GLYPHS, "shape": s, "xf": xfs[g], "field": pre[g]})
    status, r = E.run_host(E.build_host(tmp_path), cases, tmp_path)
    assert status == 0, {k: v for k, v in r.items() if k != "groups"}
    for kind in E.KINDS:
        assert r["groups"][E.GROUP_GLYPHS][kind] >= 1, (kind, r["groups"][E.GROUP_GLYPHS])
    assert r["groups"][E.GROUP_GLYPHS]["tiles_with_lazy_round"] >= 1
