"""Orientation around the device's shape preparation on a real MI355X: k_prep_orient (Shape::orientContours on the raw edges, before normalize) and
k_prep_winding (the CLI's -reversewinding / -guesswinding on the normalized edges, before the colouring). The prepared batches must equal the
compiled reference's own sequence bit for bit (orientcases.ref_prepare, live from oracle/_ref); the streamed generator must equal the resident path."""
import ctypes as C

import numpy as np
import pytest

import msdfgen_amd as M
from conftest import load_npz, bits
from msdfgen_amd import lib as L
from msdfgen_amd import synth
from msdfgen_amd.shape import ShapeBatch, autoframe
import orientcases as OC

pytestmark = pytest.mark.gpu

COUNT = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
FILL = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8))


class ShapeSource(C.Structure):
    """MsdfHipShapeSource."""
    _fields_ = [("user", C.c_void_p), ("count", COUNT), ("fill", FILL)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)
    yield
    L.load().msdfhip_set_pipeline_chunk(0)


@pytest.fixture(scope="module")
def dejavu():
    z = load_npz("dejavu8192.npz")
    full = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                      z["colors"].astype(np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    return OC.wiped(full), z["xf48"]


def _prep_raw():
    z = load_npz("prep.npz")
    raw = ShapeBatch(z["raw_gco"].astype(np.int32), z["raw_co"].astype(np.int32), z["raw_points"], z["raw_types"].astype(np.int32),
                     z["raw_colors"].astype(np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    return raw, np.ascontiguousarray(z["seeds"], np.uint64)


def _inputs(dejavu):
    raw, seeds = _prep_raw()
    cjk = ShapeBatch.from_shapes([synth.cjk_like_shape(700+k) for k in range(256)])
    hand = OC.hand_built_batch()
    sets = []
    for name, b, sd in (("prep", raw, seeds), ("dejavu", dejavu[0], None), ("cjk", cjk, None), ("hand", hand, None)):
        sets += [(name, b, sd), (name+"-perturbed", OC.perturbed(b), sd)]
    return sets


def test_prepared_batches_equal_the_reference_sequence(ref, dejavu):
    """orient_contours {0, 1} x winding {keep, reverse, guess} x coloring {0, 1, 2} over the fixture's raw set, the 8 192 wiped DejaVu glyphs, the
    CJK-like generator and the hand-built cases (horizontal first edges, an all-horizontal contour, a tie at a shared vertex, holes three deep,
    overlaps, empty contours / glyphs, single-edge contours, a 2 100-edge contour, 1 200 hits and 900 contours in one glyph), each as is, with every
    contour of every 3rd glyph reversed and with one seeded contour reversed in every 5th: offsets, types, colours and points bit for bit."""
    for name, batch, seeds in _inputs(dejavu):
        for orient in (False, True):
            for winding in (M.WINDING_KEEP, M.WINDING_REVERSE, M.WINDING_GUESS):
                for coloring in (0, 1, 2):
                    want = OC.ref_prepare_batch(ref, batch, orient, winding, True, coloring, 3.0, seeds)
                    gb = M.GlyphBatch.from_raw(batch, True, coloring, 3.0, seeds=seeds, orient_contours=orient, winding=winding)
                    try:
                        OC.same_batch(gb.shapes, want, "%s orient %d winding %d coloring %d" % (name, orient, winding, coloring))
                    finally:
                        gb.close()


def test_orientation_is_needed_and_defaults_keep(ref):
    """The perturbed raw set really changes under orientation (the test above is not vacuous), and the defaults give the v5 entry point's bytes."""
    raw, seeds = _prep_raw()
    pert = OC.perturbed(raw)
    plain = M.GlyphBatch.from_raw(pert, True, 1, 3.0, seeds=seeds)
    oriented = M.GlyphBatch.from_raw(pert, True, 1, 3.0, seeds=seeds, orient_contours=True, winding=M.WINDING_GUESS)
    try:
        OC.same_batch(plain.shapes, OC.ref_prepare_batch(ref, pert, False, 0, True, 1, 3.0, seeds), "defaults")
        assert (plain.shapes.points.view(np.uint64) != oriented.shapes.points.view(np.uint64)).any()
    finally:
        plain.close(), oriented.close()


def test_oriented_tiles_equal_the_oracle_on_reference_prepared_shapes(ref, oracle):
    """A sample of 32x32 MSDF tiles rendered from device-prepared (oriented, winding guessed) shapes == the oracle's rendering of the reference-prepared
    shapes."""
    raw, seeds = _prep_raw()
    pert = OC.perturbed(raw)
    want = OC.ref_prepare_batch(ref, pert, True, 2, True, 1, 3.0, seeds)
    gb = M.GlyphBatch.from_raw(pert, True, 1, 3.0, seeds=seeds, orient_contours=True, winding=M.WINDING_GUESS)
    try:
        extent = [want.shape(g).bounds() for g in range(want.n_glyphs)]
        # (synthetic-2 / -10: a quadratic running straight back over itself, whose distance sign is rounding noise -- see test_gpu_parity.py)
        pick = [g for g in range(0, raw.n_glyphs, 11) if extent[g][2]-extent[g][0] > 1e-3 and extent[g][3]-extent[g][1] > 1e-3
                and raw.names[g] not in ("synthetic-2", "synthetic-10")]
        xfs = np.stack([autoframe(b if b[2]-b[0] > 1e-3 and b[3]-b[1] > 1e-3 else (0, 0, 1, 1), 32, 32, 4) for b in extent])
        tiles = gb.generate(M.MODE_MSDF, 32, 32, xfs).cpu().numpy()
        for g in pick:
            o = oracle.generate(want.shape(g), 3, 32, 32, xfs[g])
            assert np.abs(tiles[g].astype(np.float64)-o).max() <= 1e-5, raw.names[g]
    finally:
        gb.close()


def _resident_bytes(raw, prep, xfs, w):
    gb = M.GlyphBatch.from_raw(raw, prep.normalize, prep.coloring, prep.angle_threshold, seed=prep.seed, orient_contours=prep.orient_contours,
                               winding=prep.winding)
    try:
        f = gb.generate(M.MODE_MSDF, w, w, xfs).cpu().numpy()
    finally:
        gb.close()
    return (255-(np.float32(255.5)-np.float32(255)*np.clip(f, np.float32(0), np.float32(1))).astype(np.int32)).astype(np.uint8)


def test_stream_oriented_equals_the_resident_path(dejavu):
    """generate_stream over the perturbed 8 192 DejaVu glyphs into a 48x48 8-bit atlas with orient_contours and winding guess, over two chunk sizes and the
    shape-source form: every byte equals from_raw(...) + generate."""
    raw, xf48 = dejavu
    pert = OC.perturbed(raw)
    prep = M.PrepareConfig(True, 1, 3.0, 0, orient_contours=True, winding=M.WINDING_GUESS)
    want = _resident_bytes(pert, prep, xf48, 48)
    offs = np.arange(pert.n_glyphs, dtype=np.int64)*48*48*3
    lib = L.load()
    try:
        for chunk in (0, 700):
            lib.msdfhip_set_pipeline_chunk(chunk)
            atlas = np.zeros((pert.n_glyphs, 48, 48, 3), np.uint8)
            M.generate_stream(pert, M.MODE_MSDF, 48, 48, xf48, atlas=atlas, out_offsets=offs, row_stride=48*3, prepare=prep)
            assert (atlas == want).all(), "chunk %d: %d bytes differ" % (chunk, int((atlas != want).sum()))
    finally:
        lib.msdfhip_set_pipeline_chunk(0)
    from msdfgen_amd import api as A
    sub = pert.select(list(range(0, pert.n_glyphs, 7)))
    sxf = xf48[::7]
    gco, co = sub.glyph_contour_offsets.astype(np.int64), sub.contour_offsets.astype(np.int64)
    pts = np.ascontiguousarray(sub.points, np.float64).reshape(-1, 8)

    def count(user, g, nc, ne):
        nc[0] = int(gco[g+1]-gco[g])
        ne[0] = int(co[gco[g+1]]-co[gco[g]])

    def fill(user, g, base, ends, p, t, c):
        c0, c1 = int(gco[g]), int(gco[g+1])
        e0, e1 = int(co[c0]), int(co[c1])
        for k in range(c1-c0):
            ends[k] = base+int(co[c0+k+1])-e0
        np.ctypeslib.as_array(p, ((e1-e0)*8,))[:] = pts[e0:e1].reshape(-1)
        np.ctypeslib.as_array(t, (e1-e0,))[:] = sub.types[e0:e1]
        np.ctypeslib.as_array(c, (e1-e0,))[:] = sub.colors[e0:e1]

    cb_count, cb_fill = COUNT(count), FILL(fill)
    source = ShapeSource(None, cb_count, cb_fill)
    n = sub.n_glyphs
    d = A._descriptors_host(sub, sxf, np.arange(n, dtype=np.int64)*48*48*3, 48*3)
    cfg = A._c_config(M.MSDFGeneratorConfig(), M.Y_UPWARD)
    atlas = np.zeros((n, 48, 48, 3), np.uint8)
    pc, po = prep.c_struct(), prep.c_orient()
    L.check(lib.msdfhip_generate_stream_prepared_oriented(-1, M.MODE_MSDF, 48, 48, n, C.byref(source), d.ctypes.data, None, 0, atlas.ctypes.data, atlas.size,
                                                          None, C.byref(cfg), C.byref(pc), None, C.byref(po)))
    assert (atlas == want[::7]).all()


def test_stream_hand_built_cases_equal_the_resident_path():
    """The hand-built cases (hits and votes past the LDS tier, a 2 100-edge contour, empty glyphs) through the streamed generator, float tiles."""
    hand = OC.perturbed(OC.hand_built_batch())
    xfs = np.stack([autoframe(s.bounds() if s.n_edges else (0, 0, 1, 1), 32, 32, 4) for s in hand.shapes()])
    for winding in (M.WINDING_REVERSE, M.WINDING_GUESS):
        prep = M.PrepareConfig(True, 1, 3.0, 0, orient_contours=True, winding=winding)
        gb = M.GlyphBatch.from_raw(hand, True, 1, 3.0, orient_contours=True, winding=winding)
        try:
            want = gb.generate(M.MODE_MSDF, 32, 32, xfs).cpu().numpy()
        finally:
            gb.close()
        got = M.generate_stream(hand, M.MODE_MSDF, 32, 32, xfs, prepare=prep)
        assert (bits(got) == bits(want)).all(), "winding %d" % winding
