"""The diagonal artifact test of k_ec_fast and k_single_call with in-range roots and extrema first (msdf_ec_fast.hpp: diagonalPairFast) on the device.

Twelve Basic-Latin fixture glyphs through GlyphBatch.generate with a stencil buffer at 1x1, 3x5, 8x8, 9x9, 10x17 and 23x17, upward and downward rows, msdf
and mtsdf, under the library default (the lazy order), EDGE_PRIORITY + DO_NOT_CHECK and EDGE_PRIORITY + ALWAYS_CHECK (the eager order): tiles and stencil
bytes equal the oracle's bit for bit. One single-shape call per size and order (k_single_call runs the same body). And the crafted 2x2 cells of
tests/ecrootscases.py (both roots in range, one of either index, a zero discriminant, the linear branches, extrema at exactly 0 and 1, NaN and infinite
extremum parameters, non-finite texels), the crafted fields of tests/ecwordscases.py and seeded plane-wave fields through the shapeless entries
msdf_fast_distance_error_correction / msdf_fast_edge_error_correction, against the host walk ecTexelFast of the same headers, bit for bit; among the 8x8
fields is one whose queue holds a round of more than 64 (item, root, test) units by the count of tests/ec_roots_host.

Every device call is made by ONE child process (tests/ecroots_gpu_child.py) under a time limit of its own; this process never opens the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bit_equal
import ecrootscases as R
import ecwordscases as W
import ecroots_gpu_child as child

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 240          # seconds; the child needs a few


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """What the child computed on the GPU. A child that faults, hangs into its limit or returns non-zero fails every test here."""
    out = os.path.join(str(tmp_path_factory.mktemp("ec_roots_gpu")), "device.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable]+flags+[child.__file__, out], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def glyphs():
    return child.fixture()


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("w,h", child.SIZES)
def test_batched_sweep_equals_the_oracle(device, glyphs, oracle, w, h, n):
    sub, bounds = glyphs
    assert sub.n_glyphs == 12
    xfs = child.frames(bounds, w, h)
    for yi, y_down in enumerate((False, True)):
        for (mode, dist) in child.CONFIGS:
            what = "%dx%d N=%d mode %d check %d y_down %d" % (w, h, n, mode, dist, y_down)
            key = "%d_%d_%d_%d_%d_%d" % (w, h, n, yi, mode, dist)
            want = np.zeros((sub.n_glyphs, h, w, n), np.float32)
            want_st = np.zeros((sub.n_glyphs, h, w), np.uint8)
            for g in range(sub.n_glyphs):
                want[g] = oracle.generate(sub.shape(g), n, w, h, xfs[g], ec_mode=mode, ec_dist=dist, y_down=y_down, stencil=want_st[g])
            assert_bit_equal(device["tiles_"+key], want, what+": tiles")
            assert (device["stencil_"+key] == want_st).all(), what+": stencil"


def test_single_shape_calls_equal_the_oracle(device, glyphs, oracle):
    sub, bounds = glyphs
    for i, (w, h) in enumerate(child.SIZES):
        xfs = child.frames(bounds, w, h)
        g = child.single_glyph(i)
        for (mode, dist) in child.SINGLE_CONFIGS:
            key = "%d_%d_%d_%d" % (w, h, mode, dist)
            want_st = np.zeros((h, w), np.uint8)
            want = oracle.generate(sub.shape(g), 3, w, h, xfs[g], ec_mode=mode, ec_dist=dist, y_down=bool(i % 2), stencil=want_st)
            assert_bit_equal(device["single_"+key], want, "single call "+key)
            assert (device["singlest_"+key] == want_st).all(), "single call stencil "+key


def test_shapeless_entries_equal_the_host_walk(device, tmp_path):
    """The device's sweep and the host walk of the same headers correct the same texels of every field, and both correct some."""
    fields = child.shapeless_fields()
    cases = [dict(c, protect_all=p, ratio=W.RATIOS[i % len(W.RATIOS)]) for i, c in enumerate(fields) for p in (0, 1)]
    want = W.run_correct(W.build_host(tmp_path), cases, tmp_path)
    changed = 0
    for k, c in enumerate(cases):
        i, p = divmod(k, 2)
        got = device["shapeless_%d_%d" % (i, p)]
        assert got.shape == want[k].shape
        assert (got.view(np.uint32) == want[k].view(np.uint32)).all(), ("field %d (%dx%d), protect_all %d" % (i, c["w"], c["h"], p),
                                                                       int((got.view(np.uint32) != want[k].view(np.uint32)).sum()))
        changed += int((got.view(np.uint32) != c["field"].view(np.uint32)).any())
    assert changed >= len(cases)//4


def test_an_8x8_field_has_a_round_of_more_than_64_units(tmp_path):
    """No device call: the host program's count for the fields the child sends through the shapeless entries (a dense form of stage 2 would need a
    second chunk of unit lanes there)."""
    fields = child.shapeless_fields()
    _, r = R.run_host(R.build_host(tmp_path), [dict(c, group=R.GROUP_CRAFTED) for c in fields], tmp_path)
    units = r["case_max_units_per_round"]
    assert len(units) == len(fields)
    assert any(u > 64 for c, u in zip(fields, units) if (c["w"], c["h"]) == (8, 8)), units
