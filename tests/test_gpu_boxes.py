"""Box sizes on the device (k_box: Shape::getBounds with border and miters, lanes = joins, then the box rule per glyph) on the GPU:
GlyphBatch.bounds(border, miter_limit, polarity) against the reference's recorded bounds (tests/golden/boxes.npz) over the whole parameter matrix, the
composition a batch prepared from raw outlines makes (plain bounds fixed after normalize, miters over the oriented, coloured edges), GlyphBatch.boxes()
against the host build of the same box function, the boxes rendered by generate_sized against the oracle, and the batch's buffers across calls."""
import numpy as np
import pytest

import msdfgen_amd as M
from msdfgen_amd import lib as L
from msdfgen_amd.shape import ShapeBatch
from conftest import assert_bit_equal
import boxcases as BC
import framecases as FC
import orientcases as OC
from test_gpu_sized import Tally

pytestmark = pytest.mark.gpu
SCALE, PX_RANGE = 32., 4.


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)
    info = M.device_info()
    assert info["arch"].startswith("gfx950"), info
    return info


@pytest.fixture(scope="module")
def gold():
    return BC.golden()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return BC.build_host(tmp_path_factory.mktemp("box_host"))


@pytest.fixture(scope="module")
def batch(gold):
    gb = M.GlyphBatch(gold[1])
    yield gb
    gb.close()


def test_bounds_matrix_equals_the_reference(gold, batch):
    """One batch of every array shape of the fixture (joins whose previous edge lies in a later pass, a one-edge contour, a contour boundary inside a pass,
    1 000 edges, empty glyphs between others): getBounds(border, miterLimit, polarity) over 3 x 5 x 3 parameters, all four doubles bit-equal."""
    z, arrays, _, _ = gold
    for k, (border, limit, polarity) in enumerate(BC.MATRIX):
        assert_bit_equal(batch.bounds(border, limit, polarity), z["bounds"][:, k], "bounds%s" % ((border, limit, polarity),))
    n = int(z["n_set"])
    plain = batch.bounds()
    assert_bit_equal(plain[:n], FC.golden()[0]["batch_bounds"], "bounds() with the defaults vs frame.npz")
    assert_bit_equal(plain, z["bounds"][:, BC.combo(0., 0., 0)], "bounds() with the defaults")


def test_raw_batch_composes_fixed_bounds_with_the_miters_of_its_edges(gold):
    """from_raw with orient_contours: the plain bounds are those fixed after normalize, the miters those of the oriented, coloured edges the batch holds."""
    z, _, raw, prep = gold
    gb = M.GlyphBatch.from_raw(raw, orient_contours=True, seed=BC.SEED)
    OC.same_batch(gb.shapes, prep, "the batch's edges vs the reference's prepared outlines")
    assert_bit_equal(gb.bounds(), z["raw_plain"], "plain bounds")
    for k, (border, limit, polarity) in enumerate(BC.MATRIX):
        assert_bit_equal(gb.bounds(border, limit, polarity), z["raw_bounds"][:, k], "raw bounds%s" % ((border, limit, polarity),))
    sizes, xf, ext = gb.boxes(M.BoxConfig(1., range=(-.125, .125), miter_limit=4., polarity=0))
    assert_bit_equal(ext, z["raw_bounds"][:, BC.combo(.125, 4., 0)], "boxes() on the raw batch")
    assert (sizes > 0).all()
    gb.close()


def test_boxes_equal_the_host_function_on_the_same_bounds(gold, batch, host):
    """The 159 shapes of frame.npz's set (and the hand-built ones) at scale 32, a pixel range of 4, miter limits 0 and 4, both alignments: the extended bounds
    equal the host build's walk, sizes and transformations the host build's boxGlyph on them, bit for bit; the 4 shapes without a box come out 0 x 0."""
    z, arrays, _, _ = gold
    n = int(z["n_set"])
    plain = z["bounds"][:, BC.combo(0., 0., 0)]
    status, (s, lo, hi, border) = BC.host_plan(host, SCALE, 1, -.5*PX_RANGE, .5*PX_RANGE)
    assert status == 0 and border == .0625
    shapes = [BC.HostShape(arrays.shape(g)) for g in range(arrays.n_glyphs)]
    grown = {}
    for limit in (0., 4.):
        want_ext = np.stack([hs.miters(host, border, limit, 1) for hs in shapes])
        grown[limit] = want_ext
        for align in ((False, False), (True, True), (True, False)):
            sizes, xf, ext = batch.boxes(M.BoxConfig(SCALE, px_range=PX_RANGE, miter_limit=limit, polarity=1, align=align))
            assert sizes.dtype == np.int32 and sizes.shape == (arrays.n_glyphs, 2) and xf.shape == (arrays.n_glyphs, 6)
            assert_bit_equal(ext, want_ext, "extended bounds, limit %g" % limit)
            want = [BC.host_box(host, s, lo, hi, align, plain[g], ext[g]) for g in range(arrays.n_glyphs)]
            assert (sizes == np.stack([w for w, _ in want])).all(), (limit, align)
            assert_bit_equal(xf, np.stack([x for _, x in want]), "xf, limit %g, align %s" % (limit, align))
            none = BC.no_box(plain)
            assert int(none[:n].sum()) == 4 and (sizes[none] == 0).all() and (sizes[~none] >= 2).all()
    larger = (grown[4.].view(np.uint64) != grown[0.].view(np.uint64)).any(1)
    assert int(larger[:n].sum()) >= 30                                      # the miter limit moves the boxes it is there for
    unit = batch.boxes(M.BoxConfig(SCALE, range=(-.0625, .0625), miter_limit=4.))      # the same range in shape units: the same boxes
    px = batch.boxes(M.BoxConfig(SCALE, px_range=PX_RANGE, miter_limit=4.))
    assert (unit[0] == px[0]).all()
    assert_bit_equal(unit[1], px[1], "unit range vs pixel range")


def _end_to_end(oracle, shapes: ShapeBatch, scale, align):
    """boxes() -> generate_sized in one call -> every glyph against the oracle at its own size; every box holds its extended bounds."""
    gb = M.GlyphBatch(shapes)
    sizes, xf, ext = gb.boxes(M.BoxConfig(scale, px_range=PX_RANGE, miter_limit=4., polarity=1, align=align))
    plain = gb.bounds()
    boxed = ~BC.no_box(plain)
    s = np.float64(scale)
    for axis in (0, 1):                                                     # in double, from the returned xf
        assert (0 <= s*(ext[boxed, axis]+xf[boxed, 2+axis])).all() and (s*(ext[boxed, axis+2]+xf[boxed, 2+axis]) <= sizes[boxed, axis]).all(), axis
    assert (ext[boxed, 0] <= plain[boxed, 0]).all() and (ext[boxed, 3] >= plain[boxed, 3]).all()
    render = np.maximum(sizes, 1)
    import torch
    out = torch.zeros(int(M.GlyphBatch.packed_offsets(render, 3)[-1]), dtype=torch.float32, device="cuda")
    out, off = gb.generate_sized(M.MODE_MSDF, render, out=out, descriptors=gb.descriptors_sized(None, render, 3, raw_xf=xf))
    flat = out.cpu().numpy()
    gb.close()
    lo, hi = np.float64(-.5*PX_RANGE)/s, np.float64(.5*PX_RANGE)/s
    assert_bit_equal(xf[:, 4:], np.tile([1/(hi-lo), -lo], (len(xf), 1)), "distance mapping")
    got = [flat[off[g]:off[g+1]].reshape(int(render[g, 1]), int(render[g, 0]), 3) for g in range(shapes.n_glyphs)]
    want = [oracle.generate(shapes.shape(g), 3, int(render[g, 0]), int(render[g, 1]), np.array([s, s, xf[g, 2], xf[g, 3], lo, hi])) for g in range(shapes.n_glyphs)]
    t = Tally()
    t.add(("boxes", scale, align), got, None, want, None)
    t.check()
    return sizes, boxed


def test_boxes_rendered_by_generate_sized_equal_the_oracle(oracle, gold):
    """End to end at miter limit 4 over the 159 shapes of frame.npz's set, every glyph against the oracle at its own size under the bounds of
    tests/test_gpu_routes.py: check_parity. The glyph-sized shapes (extent up to 2 units: the font glyphs and the normalized outlines) at scale 32,
    centred; the lattice-sized ones (tests/geomcases.py and the rings: up to 27 units, 869 x 869 texels and half a minute of oracle time at scale 32) at
    scale 2, pixel-aligned on both axes -- two calls, every shape in one of them, the shapes without a box rendered as 1 x 1."""
    z, arrays, _, _ = gold
    n = int(z["n_set"])
    plain = z["bounds"][:n, BC.combo(0., 0., 0)]
    none = BC.no_box(plain)
    extent = np.where(none, 0., np.maximum(plain[:, 2]-plain[:, 0], plain[:, 3]-plain[:, 1]))
    small = [g for g in range(n) if extent[g] <= 2.]
    large = [g for g in range(n) if extent[g] > 2.]
    assert len(small) >= 90 and len(large) >= 40 and none[small].any()
    sizes, boxed = _end_to_end(oracle, arrays.select(small), SCALE, (False, False))
    assert sizes[boxed].max() <= 96 and (sizes[~boxed] == 0).all()             # (both calls stay small: 2 units or 27 units, plus range and miters)
    sizes, boxed = _end_to_end(oracle, arrays.select(large), 2., (True, True))
    assert sizes[boxed].max() <= 96


def test_buffers_across_batches_and_calls(gold, batch):
    """A batch of one glyph, a batch of none, then the big batch asked twice with different parameters: every answer is the recorded one."""
    z, arrays, _, _ = gold
    g = list(arrays.names).index("hand/ring60_star8")
    one = M.GlyphBatch(arrays.select([g]))
    k = BC.combo(.125, 4., 0)
    assert_bit_equal(one.bounds(.125, 4., 0), z["bounds"][g:g+1, k], "one glyph")
    sizes, xf, ext = one.boxes(M.BoxConfig(1., range=(-.125, .125), miter_limit=4., polarity=0))
    assert_bit_equal(ext, z["bounds"][g:g+1, k], "one glyph, boxes()")
    assert sizes.shape == (1, 2) and (sizes > 0).all()
    one.close()
    empty = M.GlyphBatch(ShapeBatch.from_shapes([]))
    assert empty.bounds(.125, 4., 0).shape == (0, 4)
    sizes, xf, ext = empty.boxes(M.BoxConfig(SCALE, px_range=PX_RANGE, miter_limit=4.))
    assert sizes.shape == (0, 2) and xf.shape == (0, 6) and ext.shape == (0, 4)
    empty.close()
    for (border, limit, polarity) in ((2., 1e9, -1), (.125, 2., 1), (2., 1e9, -1)):
        assert_bit_equal(batch.bounds(border, limit, polarity), z["bounds"][:, BC.combo(border, limit, polarity)], "again%s" % ((border, limit, polarity),))
    with pytest.raises(M.MsdfHipError) as e:                                # the miter of a corner that turns back lies up to 2e9 units out at limit 1e9: no such box
        batch.boxes(M.BoxConfig(1., range=(-2., 2.), miter_limit=1e9, polarity=-1))
    assert e.value.code == L.ERR_INVALID and "beyond" in str(e.value)
    a = batch.boxes(M.BoxConfig(1., range=(-2., 2.), miter_limit=4., polarity=-1))[2]
    b = batch.boxes(M.BoxConfig(1., range=(-.125, .125), miter_limit=2., polarity=1))[2]
    assert_bit_equal(a, z["bounds"][:, BC.combo(2., 4., -1)], "boxes() bounds, first")
    assert_bit_equal(b, z["bounds"][:, BC.combo(.125, 2., 1)], "boxes() bounds, second")
    assert_bit_equal(batch.bounds(), z["bounds"][:, BC.combo(0., 0., 0)], "plain bounds after all of it")
