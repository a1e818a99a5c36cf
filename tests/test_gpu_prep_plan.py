"""The preparation's buffers as msdf_prepplan.hpp lays them out, on the device, with EVERY optional region present in one chunk and with none.

The hand-built raw batch of tests/orientcases.py (a 2 100-edge contour: the colouring's global tables; 600 rectangles in a row: hits and votes past
k_prep_orient's LDS tiers; 900 contours; empty and single-edge glyphs) goes through generate_stream at 32x32 msdf with pipeline chunks 0 (one chunk), 3 and 1,
under ink-trap colouring + per-glyph seeds + orient_contours + WINDING_GUESS + framing on the device ("full"), and under the leanest preparation -- normalize
off, colouring 0, no orientation, the caller's transformations ("lean"). Each must equal GlyphBatch.from_raw(...) + generate(frame=...) -- whose buffers are
single allocations -- as bit patterns. The streamed call hands out no bounds: its bounds region feeds the chunk's transformations, so the framed tiles are the
comparison; the resident batch's bounds are held against the vertex boxes of the glyphs made of line segments (normalize moves no point of those).

Every device call is made by ONE child process (tests/prepplan_gpu_child.py) under a time limit of its own; this process never opens the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bit_equal, bits
import prepplan_gpu_child as child

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 240          # seconds; the child needs a few


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """What the child computed on the GPU. A child that faults, hangs into its limit or returns non-zero fails every test here."""
    out = os.path.join(str(tmp_path_factory.mktemp("prep_plan_gpu")), "device.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable]+flags+[child.__file__, out], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", ["full", "lean"])
def test_streamed_chunks_equal_the_resident_preparation(device, name):
    want = device["want_"+name]
    assert want.shape == (child.raw_batch().n_glyphs, child.SIZE, child.SIZE, 3)
    assert len(np.unique(bits(want))) > 100                                   # (not blank tiles)
    for chunk in child.CHUNKS:
        assert_bit_equal(device["stream_%s_%d" % (name, chunk)], want, "%s, pipeline chunk %d" % (name, chunk))


@pytest.mark.parametrize("name", ["full", "lean"])
def test_bounds_of_the_resident_batch(device, name):
    raw = child.raw_batch()
    got = device["bounds_"+name]
    checked = 0
    for g, s in enumerate(raw.shapes()):
        if s.n_edges == 0:
            assert got[g].tolist() == [1e240, 1e240, -1e240, -1e240], g
        elif (np.asarray(s.types) == 1).all():                               # line segments: orientation and normalize move no point
            pts = np.asarray(s.points, np.float64).reshape(-1, 8)[:, :4].reshape(-1, 2)
            assert_bit_equal(got[g], np.array([pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()]), "bounds of glyph %d" % g)
            checked += 1
    assert checked >= 5
