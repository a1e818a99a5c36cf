"""Framing on the device (k_frame: Shape::getBounds with lanes = edges, then the CLI's -autoframe per glyph) on the GPU: GlyphBatch.bounds() / frame()
against the reference's recorded bounds and the host build of the same framing function, the streamed generator with frame= against the same call with host
transformations from the reference's bounds (float tiles, 8-bit atlas, four chunks and one), the reference CLI's own -autoframe tiles, and the resident
path msdfhip_batch_frame -> msdfhip_batch_generate."""
import numpy as np
import pytest

import msdfgen_amd as M
from msdfgen_amd import lib as L
from msdfgen_amd.shape import ShapeBatch, autoframe
from conftest import assert_bit_equal, load_npz
import framecases as FC

pytestmark = pytest.mark.gpu
N_STREAM, CHUNK = 200, 64


@pytest.fixture(scope="module")
def gold():
    return FC.golden()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return FC.build_host(tmp_path_factory.mktemp("frame_host"))


@pytest.fixture(scope="module")
def outlines(gold):
    """The first 200 raw outlines of prep.npz, colours wiped, and the reference's bounds of each after its normalize."""
    z = load_npz("prep.npz")
    raw = ShapeBatch(z["raw_gco"].astype(np.int32), z["raw_co"].astype(np.int32), z["raw_points"], z["raw_types"].astype(np.int32),
                     np.full(len(z["raw_types"]), 7, np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    return raw.select(list(range(N_STREAM))), gold[0]["prep_bounds"][:N_STREAM]


class _Streamed:
    """generate_stream(frame=FrameConfig(px_range=4)) at 32x32 msdf with a pipeline chunk of 64 (four chunks, the last of 8), per preparation, computed once."""

    def __init__(self, raw):
        self.raw, self.cache = raw, {}

    def tiles(self, winding):
        if winding not in self.cache:
            L.check(L.load().msdfhip_set_pipeline_chunk(CHUNK))
            try:
                self.cache[winding] = M.generate_stream(self.raw, M.MODE_MSDF, 32, 32, prepare=M.PrepareConfig(winding=winding), frame=M.FrameConfig(px_range=4))
            finally:
                L.check(L.load().msdfhip_set_pipeline_chunk(0))
        return self.cache[winding]


@pytest.fixture(scope="module")
def streamed(outlines):
    return _Streamed(outlines[0])


def test_batch_bounds_equal_the_reference(gold):
    """One batch of every golden shape, incl. 65 and 129 edges (second and third lane pass, loop remainder) and an empty glyph between two others."""
    z, batch, _ = gold
    names = list(batch.names)
    assert names.index("hand/empty") == names.index("hand/ring65")+1 == names.index("hand/ring129")-1
    gb = M.GlyphBatch(batch)
    assert_bit_equal(gb.bounds(), z["batch_bounds"], "GlyphBatch.bounds()")
    gb.close()


def test_bounds_of_raw_outlines_are_those_of_the_normalized_shape(gold):
    """from_raw: the bounds are taken after normalize and before the colouring, whatever the colouring does to the arrays the batch keeps; incl. a contour of
    one edge (three once normalized)."""
    z, _, raw = gold
    assert "single" in raw.names and raw.shape(raw.names.index("single")).n_edges == 1
    for coloring in (0, 1, 2):
        gb = M.GlyphBatch.from_raw(raw, normalize=True, coloring=coloring)
        assert_bit_equal(gb.bounds(), z["raw_bounds"], "from_raw bounds, coloring %d" % coloring)
        gb.close()


def test_batch_frame_equals_the_host_function_on_reference_bounds(gold, host):
    z, batch, _ = gold
    gb = M.GlyphBatch(batch)
    for (w, h, ri, scale) in FC.frame_matrix():
        mode, lower, upper = FC.RANGES[ri]
        fc = M.FrameConfig(px_range=(lower, upper), scale=scale) if mode == 1 else M.FrameConfig(unit_range=(lower, upper), scale=scale)
        got = gb.frame(w, h, fc)
        want = np.stack([FC.host_frame(host, mode, lower, upper, scale, w, h, b) for b in z["batch_bounds"]])
        assert_bit_equal(got, want, "frame %s" % ((w, h, ri, scale),))
    gb.close()


def test_frame_leaves_placement_alone(gold):
    _, batch, _ = gold
    gb = M.GlyphBatch(batch)
    d = gb.descriptors(None, 32, 32, 3, out_offsets=np.arange(batch.n_glyphs)[::-1]*7, row_stride=123)
    before = d.cpu().numpy().reshape(-1).view(L.GLYPH_DTYPE).copy()
    gb.frame(32, 32, M.FrameConfig(px_range=4), descriptors=d)
    after = d.cpu().numpy().reshape(-1).view(L.GLYPH_DTYPE)
    for k in ("out_offset", "row_stride", "flip"):
        assert (before[k] == after[k]).all(), k
    assert (after["xf"][:, 0] > 0).all()
    gb.close()


def test_streamed_frame_equals_host_transformations_from_reference_bounds(outlines, streamed):
    raw, bounds = outlines
    xfs = np.stack([autoframe(b, 32, 32, 4) for b in bounds])
    prep = M.PrepareConfig()
    got = streamed.tiles(M.WINDING_KEEP)
    L.check(L.load().msdfhip_set_pipeline_chunk(CHUNK))
    try:
        want = M.generate_stream(raw, M.MODE_MSDF, 32, 32, xfs, prepare=prep)
        offs = np.arange(N_STREAM, dtype=np.int64)*32*32*3
        atlas = M.generate_stream(raw, M.MODE_MSDF, 32, 32, prepare=prep, frame=M.FrameConfig(px_range=4), atlas=np.zeros((N_STREAM, 32, 32, 3), np.uint8),
                                  out_offsets=offs, row_stride=32*3)
        atlas_want = M.generate_stream(raw, M.MODE_MSDF, 32, 32, xfs, prepare=prep, atlas=np.zeros((N_STREAM, 32, 32, 3), np.uint8), out_offsets=offs,
                                       row_stride=32*3)
        L.check(L.load().msdfhip_set_pipeline_chunk(N_STREAM))
        one = M.generate_stream(raw, M.MODE_MSDF, 32, 32, prepare=prep, frame=M.FrameConfig(px_range=4))
    finally:
        L.check(L.load().msdfhip_set_pipeline_chunk(0))
    assert want.any()
    assert_bit_equal(got, want, "framed float tiles vs host xfs")
    assert_bit_equal(atlas, atlas_want, "framed atlas vs host xfs")
    assert_bit_equal(got, one, "four chunks vs one")


def test_framed_tiles_equal_the_reference_cli_autoframe(gold):
    """The 'A' of BASELINE config 1, DejaVu 'S' and the cubic teardrop: msdfgen msdf -autoframe -pxrange 4 at 32x32, zero differing floats."""
    z, _, raw = gold
    three = raw.select([0, 1, 2])
    got = M.generate_stream(three, M.MODE_MSDF, 32, 32, prepare=M.PrepareConfig(), frame=M.FrameConfig(px_range=4))
    assert_bit_equal(got, z["tiles32"], "framed tiles vs the CLI's")


def test_resident_frame_then_generate_equals_the_streamed_tiles(outlines, streamed):
    raw, _ = outlines
    gb = M.GlyphBatch.from_raw(raw, winding=M.WINDING_GUESS)
    got = gb.generate(M.MODE_MSDF, 32, 32, frame=M.FrameConfig(px_range=4)).cpu().numpy()
    gb.close()
    assert_bit_equal(got, streamed.tiles(M.WINDING_GUESS), "msdfhip_batch_frame + msdfhip_batch_generate vs the streamed call")
