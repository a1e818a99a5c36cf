"""Who owns what, on a real MI355X: every way of making a batch, made, used and destroyed several times over with the pools trimmed in between; the
caller's device arrays after a batch that borrowed them has gone; the pooled arenas and pipelines before and after msdfhip_trim. A handful of glyphs
at 16x16, MTSDF with error correction and the distance check always on (candidate, parameter, class-list and scratch buffers all in use); every
tile against the oracle, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import msdfgen_amd as M
from conftest import load_npz, assert_bit_equal
from msdfgen_amd import lib as L
from msdfgen_amd.shape import FlatShape, ShapeBatch, autoframe

pytestmark = pytest.mark.gpu

W = H = 16
MODE = M.MODE_MTSDF
CONFIG = M.MSDFGeneratorConfig(True, M.ErrorCorrectionConfig(M.EC_EDGE_PRIORITY, M.ALWAYS_CHECK_DISTANCE))
ORACLE = dict(overlap=True, ec_mode=2, ec_dist=2)                                 # the same configuration in the oracle's terms


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)


@pytest.fixture(scope="module")
def glyphs(oracle):
    """The first six glyphs of the pipeline tests' fixture (and the first one with two contours, should those have none): the batch, its frames, the
    oracle's tiles of the glyphs as they are and of the glyphs as oracle.shape_prepare (normalize, edgeColoringSimple) leaves them."""
    z = load_npz("dejavu8192.npz")
    full = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                      z["colors"].astype(np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    idx = list(range(6))
    contours = np.diff(full.glyph_contour_offsets)
    if contours[idx].max() < 2:
        idx.append(int(np.argmax(contours >= 2)))
    sub = full.select(idx)
    assert np.diff(sub.glyph_contour_offsets).max() >= 2
    xfs = np.stack([autoframe(sub.shape(g).bounds(), W, H, 2) for g in range(sub.n_glyphs)])
    want = np.stack([oracle.generate(sub.shape(g), MODE, W, H, xfs[g], **ORACLE) for g in range(sub.n_glyphs)])
    prepared = [oracle.shape_prepare(sub.shape(g), True, 1, 3.0, 0) for g in range(sub.n_glyphs)]
    want_prepared = np.stack([oracle.generate(FlatShape(p.contour_offsets, p.points, p.types, p.colors), MODE, W, H, xfs[g], **ORACLE)
                              for g, p in enumerate(prepared)])
    return sub, xfs, want, want_prepared


def _batch_bounds(handle, n):
    out = np.zeros((n, 4), np.float64)
    L.check(L.load().msdfhip_batch_bounds(handle, L.ptr(out, L._dp)))
    return out


def _host_round(sub, xfs):
    hb = M.HostBatch(sub)
    try:
        return hb.generate_host(MODE, W, H, xfs, config=CONFIG), _batch_bounds(hb._handle, sub.n_glyphs)
    finally:
        hb.close()


def _device_round(sub, xfs):
    gb = M.GlyphBatch(sub)
    try:
        return gb.generate(MODE, W, H, xfs, config=CONFIG).cpu().numpy(), gb.bounds()
    finally:
        gb.close()


def _prepared_round(sub, xfs):
    gb = M.GlyphBatch.from_raw(sub, True, 1, 3.0, seed=0)
    try:
        return gb.generate(MODE, W, H, xfs, config=CONFIG).cpu().numpy(), gb.bounds()
    finally:
        gb.close()


@pytest.mark.parametrize("route", ("host_arrays", "device_arrays", "prepared"))
def test_create_generate_bounds_close_three_times_with_trims_between(glyphs, route):
    sub, xfs, want, want_prepared = glyphs
    one_round = {"host_arrays": _host_round, "device_arrays": _device_round, "prepared": _prepared_round}[route]
    first_bounds = None
    for k in range(3):
        tiles, bounds = one_round(sub, xfs)
        assert_bit_equal(tiles, want_prepared if route == "prepared" else want, "%s, round %d" % (route, k))
        assert np.isfinite(bounds).all() and (bounds[:, 0] < bounds[:, 2]).all() and (bounds[:, 1] < bounds[:, 3]).all()
        first_bounds = bounds if first_bounds is None else first_bounds
        assert_bit_equal(bounds, first_bounds, "%s, bounds of round %d" % (route, k))
        assert L.load().msdfhip_trim() == 0


def _batch_on(tensors, like):
    """A GlyphBatch over device arrays that are already there (GlyphBatch uploads its own)."""
    gb = object.__new__(M.GlyphBatch)
    gb.__dict__.update({k: v for k, v in like.__dict__.items() if k not in ("_handle", "_scratch", "_glyph_cache")})
    gb._gco, gb._co, gb._pts, gb._types, gb._colors = tensors
    gb._handle, gb._scratch, gb._glyph_cache = C.c_void_p(), None, {}
    s = gb.shapes
    L.check(L.load().msdfhip_batch_create_device(C.byref(gb._handle), gb.n_glyphs, s.n_contours, s.n_edges, gb.max_contours, gb.max_edges, gb._gco.data_ptr(),
                                                 gb._co.data_ptr(), gb._pts.data_ptr(), gb._types.data_ptr(), gb._colors.data_ptr(),
                                                 gb.torch.cuda.current_stream(gb.device).cuda_stream))
    return gb


def test_the_callers_device_arrays_survive_the_batch_that_borrowed_them(glyphs):
    sub, xfs, want, _ = glyphs
    gb = M.GlyphBatch(sub)
    tensors = (gb._gco, gb._co, gb._pts, gb._types, gb._colors)
    uploaded = [t.cpu().numpy().copy() for t in tensors]
    first = gb.generate(MODE, W, H, xfs, config=CONFIG).cpu().numpy()
    gb.close()
    assert L.load().msdfhip_trim() == 0
    for t, u in zip(tensors, uploaded):
        assert (t.cpu().numpy() == u).all()
    assert (uploaded[0] == sub.glyph_contour_offsets).all() and (uploaded[2][:sub.n_edges] == np.asarray(sub.points).reshape(-1, 8)).all()
    again = _batch_on(tensors, gb)
    try:
        second = again.generate(MODE, W, H, xfs, config=CONFIG).cpu().numpy()
    finally:
        again.close()
    assert_bit_equal(first, want, "first batch")
    assert_bit_equal(second, first, "second batch over the same arrays")
    for t, u in zip(tensors, uploaded):
        assert (t.cpu().numpy() == u).all()


def _pooled_calls(sub, xfs):
    """One call through each pool: a single-shape call (arena), a host-output call and a streamed call (pipeline; chunks of two glyphs, so that the
    glyphs pass through at least three chunks and the slots are reused)."""
    lib = L.load()
    g = int(np.argmax(np.diff(sub.glyph_contour_offsets) >= 2))
    one = np.zeros((H, W, 4), np.float32)
    M.generate_mtsdf(one, sub.shape(g), M.SDFTransformation.from_xf(xfs[g]), CONFIG)
    L.check(lib.msdfhip_set_pipeline_chunk(2))
    try:
        hb = M.HostBatch(sub)
        try:
            host = hb.generate_host(MODE, W, H, xfs, config=CONFIG)
        finally:
            hb.close()
        streamed = M.generate_stream(sub, MODE, W, H, xfs, config=CONFIG)
    finally:
        lib.msdfhip_set_pipeline_chunk(0)
    return g, one, host, streamed


def test_pooled_arenas_and_pipelines_before_and_after_trim(glyphs):
    sub, xfs, want, _ = glyphs
    g, one, host, streamed = _pooled_calls(sub, xfs)
    assert L.load().msdfhip_trim() == 0
    g2, one2, host2, streamed2 = _pooled_calls(sub, xfs)
    assert g2 == g
    for what, before, after, expected in (("single-shape call", one, one2, want[g]), ("host-output call", host, host2, want), ("streamed call", streamed, streamed2, want)):
        assert_bit_equal(before, expected, what+" before trim")
        assert_bit_equal(after, before, what+" after trim")
