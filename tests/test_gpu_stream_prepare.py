"""The streamed generator over RAW outlines (msdfhip_generate_stream_prepared / _csr_prepared, generate_stream(prepare=...)) on a real MI355X: every
chunk is uploaded, prepared on the device, digested, rendered and copied back on its own stream. The contract is bytes: the same as the resident
path msdfhip_batch_create_prepared + generate (GlyphBatch.from_raw), which test_gpu_parity.py pins to the reference's normalize + colouring, and --
for the 8 192 DejaVu glyphs with their colours wiped -- the reference's own per-tile hashes of the fixture."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import msdfgen_amd as M
from conftest import load_npz, bits
from msdfgen_amd import api as A
from msdfgen_amd import lib as L
from msdfgen_amd.shape import FlatShape, ShapeBatch, autoframe

pytestmark = pytest.mark.gpu

WHITE = 7
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


def byte_tiles(f):
    """pixelFloatToByte (core/pixel-conversion.hpp:8-10) as the device computes it."""
    return (255-(np.float32(255.5)-np.float32(255)*np.clip(f, np.float32(0), np.float32(1))).astype(np.int32)).astype(np.uint8)


def sha_rows(tiles):
    return np.stack([np.frombuffer(hashlib.sha256(np.ascontiguousarray(t).tobytes()).digest(), np.uint8) for t in tiles])


def wiped(batch: ShapeBatch) -> ShapeBatch:
    return ShapeBatch(batch.glyph_contour_offsets, batch.contour_offsets, batch.points, batch.types, np.full(batch.n_edges, WHITE, np.int32),
                      batch.inverse_y, batch.names)


@pytest.fixture(scope="module")
def dejavu():
    z = load_npz("dejavu8192.npz")
    full = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                      z["colors"].astype(np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    return wiped(full), z["xf48"], z["sha48"]


@pytest.fixture(scope="module")
def prep_raw():
    z = load_npz("prep.npz")
    raw = ShapeBatch(z["raw_gco"].astype(np.int32), z["raw_co"].astype(np.int32), z["raw_points"], z["raw_types"].astype(np.int32),
                     z["raw_colors"].astype(np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    prepared = M.GlyphBatch.from_raw(raw, True, 1, 3.0, seeds=z["seeds"])
    extent = [prepared.shapes.shape(g).bounds() for g in range(raw.n_glyphs)]
    prepared.close()
    xfs = np.stack([autoframe(b if b[2]-b[0] > 1e-3 and b[3]-b[1] > 1e-3 else (0, 0, 1, 1), 32, 32, 4) for b in extent])
    return raw, xfs, np.ascontiguousarray(z["seeds"], np.uint64)


def resident(raw, prep, seeds, mode, w, h, xfs, config=None, scanline_pass=False, stencil=False):
    """GlyphBatch.from_raw + generate: the resident path the streamed one must equal."""
    import torch
    gb = M.GlyphBatch.from_raw(raw, prep.normalize, prep.coloring, prep.angle_threshold, seeds=seeds, seed=prep.seed)
    try:
        st = torch.zeros((raw.n_glyphs, h, w), dtype=torch.uint8, device=gb.device) if stencil else None
        out = gb.generate(mode, w, h, xfs, config=config, stencil=st, scanline_pass=scanline_pass).cpu().numpy()
        return out, (st.cpu().numpy() if stencil else None)
    finally:
        gb.close()


def stream_c(raw, prep, seeds, mode, w, h, xfs, config=None, scanline_pass=False, stencil=None):
    """msdfhip_generate_stream_csr_prepared straight through ctypes (the config of the resident path, incl. its scanline pass)."""
    n = M.CHANNELS[mode]
    d = A._descriptors_host(raw, xfs, np.arange(raw.n_glyphs, dtype=np.int64)*w*h*n, w*n)
    cfg = A._c_config(config if config is not None else (M.MSDFGeneratorConfig() if mode >= 3 else M.GeneratorConfig()), M.Y_UPWARD)
    A._with_scanline_pass(cfg, scanline_pass, M.FILL_NONZERO, .5)
    out = np.zeros((raw.n_glyphs, h, w, n), np.float32)
    gco, co = np.ascontiguousarray(raw.glyph_contour_offsets, np.int32), np.ascontiguousarray(raw.contour_offsets, np.int32)
    pts, types = np.ascontiguousarray(raw.points, np.float64).reshape(-1, 8), np.ascontiguousarray(raw.types, np.uint8)
    colors = np.ascontiguousarray(raw.colors, np.uint8)
    pc = prep.c_struct()
    L.check(L.load().msdfhip_generate_stream_csr_prepared(-1, mode, w, h, raw.n_glyphs, L.ptr(gco, L._ip), L.ptr(co, L._ip), L.ptr(pts, L._dp),
                                                          L.ptr(types, L._bp), L.ptr(colors, L._bp), d.ctypes.data, out.ctypes.data, out.size, None, 0,
                                                          stencil.ctypes.data if stencil is not None else None, C.byref(cfg), C.byref(pc),
                                                          seeds.ctypes.data_as(C.POINTER(C.c_uint64)) if seeds is not None else None))
    return out


def test_full_size_raw_dejavu_streams_into_the_reference_tiles(dejavu):
    """8 192 DejaVu glyphs with every colour wiped to WHITE, prepared inside the pipeline (normalize + edgeColoringSimple, 3.0, seed 0): every 48x48 MSDF
    tile hashes to the compiled reference's (the fixture's sha48), the 8-bit atlas is pixelFloatToByte of those tiles; the same without normalize."""
    raw, xf48, sha48 = dejavu
    for normalize in (True, False):
        prep = M.PrepareConfig(normalize, 1, 3.0, 0)
        tiles = M.generate_stream(raw, M.MODE_MSDF, 48, 48, xf48, prepare=prep)
        bad = np.nonzero(~(sha_rows(tiles) == sha48).all(axis=1))[0]
        assert len(bad) == 0, "normalize=%d: %d tiles differ from the reference, first %s" % (normalize, len(bad), [raw.names[g] for g in bad[:5]])
        atlas = np.zeros((raw.n_glyphs, 48, 48, 3), np.uint8)
        M.generate_stream(raw, M.MODE_MSDF, 48, 48, xf48, atlas=atlas, out_offsets=np.arange(raw.n_glyphs, dtype=np.int64)*48*48*3, row_stride=48*3,
                          prepare=prep)
        assert (atlas == byte_tiles(tiles)).all(), "normalize=%d: 8-bit atlas" % normalize


def test_ink_trap_seeds_and_every_strategy_equal_the_resident_path(prep_raw):
    """prep.npz's raw outlines (fonts + single-edge contours, two-edge teardrops, cusps) in every (normalize, coloring) combination with the fixture's
    per-glyph seeds: float tiles and the correction stencil equal GlyphBatch.from_raw + generate, with and without the scanline sign pass."""
    raw, xfs, seeds = prep_raw
    for normalize in (True, False):
        for coloring in (0, 1, 2):
            prep = M.PrepareConfig(normalize, coloring, 3.0, 0)
            for scan in (False, True):
                config = M.MSDFGeneratorConfig(not scan, M.ErrorCorrectionConfig(M.EC_EDGE_PRIORITY, M.DO_NOT_CHECK_DISTANCE if scan else M.CHECK_DISTANCE_AT_EDGE))
                want, want_st = resident(raw, prep, seeds, M.MODE_MSDF, 32, 32, xfs, config=config, scanline_pass=scan, stencil=True)
                st = np.zeros((raw.n_glyphs, 32, 32), np.uint8)
                got = stream_c(raw, prep, seeds, M.MODE_MSDF, 32, 32, xfs, config=config, scanline_pass=scan, stencil=st)
                what = "normalize=%d coloring=%d scanline=%d" % (normalize, coloring, scan)
                assert (bits(got) == bits(want)).all(), what
                assert (st == want_st).all(), what+": stencil"
    # the Python form, with one seed for all glyphs (seeds=None)
    prep = M.PrepareConfig(True, 2, 3.0, 11)
    want, _ = resident(raw, prep, None, M.MODE_MTSDF, 32, 32, xfs)
    assert (bits(M.generate_stream(raw, M.MODE_MTSDF, 32, 32, xfs, prepare=prep)) == bits(want)).all()


def test_chunk_size_does_not_change_the_bytes(prep_raw):
    raw, xfs, seeds = prep_raw
    prep = M.PrepareConfig(True, 1, 3.0, 0)
    want, _ = resident(raw, prep, seeds, M.MODE_MSDF, 32, 32, xfs)
    lib = L.load()
    try:
        for chunk in (1, 7, 64, 0):
            lib.msdfhip_set_pipeline_chunk(chunk)
            got = M.generate_stream(raw, M.MODE_MSDF, 32, 32, xfs, prepare=prep, seeds=seeds)
            assert (bits(got) == bits(want)).all(), "chunk %d" % chunk
            a8 = np.zeros((raw.n_glyphs, 32, 32, 3), np.uint8)
            M.generate_stream(raw, M.MODE_MSDF, 32, 32, xfs, atlas=a8, out_offsets=np.arange(raw.n_glyphs, dtype=np.int64)*32*32*3, row_stride=32*3,
                              prepare=prep, seeds=seeds)
            assert (a8 == byte_tiles(want)).all(), "chunk %d, 8-bit" % chunk
    finally:
        lib.msdfhip_set_pipeline_chunk(0)


def star(n, r0, r1, cx=0., cy=0.):
    """A closed polygon of n straight edges whose vertices alternate between radii r0 and r1: a corner at every vertex."""
    a = np.arange(n)*2*np.pi/n
    r = np.where(np.arange(n) % 2 == 0, r0, r1)
    p = np.stack([cx+r*np.cos(a), cy+r*np.sin(a)], 1)
    return [(WHITE, tuple(p[i]), tuple(p[(i+1) % n])) for i in range(n)]


def test_contours_beyond_the_colouring_lds_tier_next_to_ordinary_glyphs(prep_raw):
    """A chunk that holds contours of more than PREP_WAVE_MAX_EDGES (2 048) edges (the colouring's tables in global memory) next to ordinary glyphs."""
    raw, xfs, _ = prep_raw
    shapes = [raw.shape(g) for g in range(40)]
    frames = list(xfs[:40])
    longs = [FlatShape.from_contours([star(2600, 1., .93)]), FlatShape.from_contours([star(2200, 1., .9), star(12, .4, .3)]),
             FlatShape.from_contours([star(2050, 1., .95, 3., 0.)])]
    for k, s in enumerate(longs):
        shapes.insert(5+9*k, s), frames.insert(5+9*k, autoframe(s.bounds(), 32, 32, 4))
    mix, mxf = ShapeBatch.from_shapes(shapes), np.stack(frames)
    seeds = np.arange(mix.n_glyphs, dtype=np.uint64)*977
    lib = L.load()
    try:
        for chunk in (0, 16):
            lib.msdfhip_set_pipeline_chunk(chunk)
            for coloring in (1, 2):
                prep = M.PrepareConfig(True, coloring, 3.0, 0)
                want, _ = resident(mix, prep, seeds, M.MODE_MSDF, 32, 32, mxf)
                got = M.generate_stream(mix, M.MODE_MSDF, 32, 32, mxf, prepare=prep, seeds=seeds)
                assert (bits(got) == bits(want)).all(), "chunk %d coloring %d" % (chunk, coloring)
    finally:
        lib.msdfhip_set_pipeline_chunk(0)


def test_source_callbacks_equal_the_csr_form(prep_raw):
    """The shape-source form (count / fill callbacks, called from the library's host threads) over the same raw arrays equals the CSR form; the colours
    `fill` writes count only with coloring 0."""
    raw, xfs, seeds = prep_raw
    raw = raw.select(list(range(300)))
    xfs, seeds = xfs[:300], np.ascontiguousarray(seeds[:300])
    gco, co = raw.glyph_contour_offsets.astype(np.int64), raw.contour_offsets.astype(np.int64)
    pts = np.ascontiguousarray(raw.points, np.float64).reshape(-1, 8)

    def count(user, g, nc, ne):
        nc[0] = int(gco[g+1]-gco[g])
        ne[0] = int(co[gco[g+1]]-co[gco[g]])

    def fill(user, g, base, ends, p, t, c):
        c0, c1 = int(gco[g]), int(gco[g+1])
        e0, e1 = int(co[c0]), int(co[c1])
        for k in range(c1-c0):
            ends[k] = base+int(co[c0+k+1])-e0
        np.ctypeslib.as_array(p, ((e1-e0)*8,))[:] = pts[e0:e1].reshape(-1)
        np.ctypeslib.as_array(t, (e1-e0,))[:] = raw.types[e0:e1]
        np.ctypeslib.as_array(c, (e1-e0,))[:] = raw.colors[e0:e1]

    cb_count, cb_fill = COUNT(count), FILL(fill)
    source = ShapeSource(None, cb_count, cb_fill)
    n = raw.n_glyphs
    d = A._descriptors_host(raw, xfs, np.arange(n, dtype=np.int64)*32*32*3, 32*3)
    cfg = A._c_config(M.MSDFGeneratorConfig(), M.Y_UPWARD)
    lib = L.load()
    for coloring in (0, 1, 2):
        prep = M.PrepareConfig(True, coloring, 3.0, 0)
        pc = prep.c_struct()
        got = np.zeros((n, 32, 32, 3), np.float32)
        L.check(lib.msdfhip_generate_stream_prepared(-1, M.MODE_MSDF, 32, 32, n, C.byref(source), d.ctypes.data, got.ctypes.data, got.size, None, 0, None,
                                                     C.byref(cfg), C.byref(pc), seeds.ctypes.data_as(C.POINTER(C.c_uint64))))
        want = M.generate_stream(raw, M.MODE_MSDF, 32, 32, xfs, prepare=prep, seeds=seeds)
        assert (bits(got) == bits(want)).all(), "coloring %d" % coloring


def test_candidate_overflow_rerun_prepares_again():
    """test_gpu_pipeline.py's overflow mix (overlapping strokes without overlap support under ALWAYS_CHECK_DISTANCE, among ordinary glyphs), as raw
    outlines: the call runs a second time with the overflow pass, preparing every chunk again, and equals the resident path."""
    from msdfgen_amd import synth
    z = load_npz("dejavu8192.npz")
    full = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                      z["colors"].astype(np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    idx = list(range(0, 3000, 15))
    shapes, fr = [full.shape(g) for g in idx], [z["xf48"][g] for g in idx]
    for k, at in enumerate((17, 90, 91, 160)):
        s = synth.cjk_like_shape(8801+k)
        shapes.insert(at, s), fr.insert(at, autoframe(s.bounds(), 48, 48, 4))
    mix, mxf = wiped(ShapeBatch.from_shapes(shapes)), np.stack(fr)
    c = M.MSDFGeneratorConfig(False, M.ErrorCorrectionConfig(M.EC_EDGE_PRIORITY, M.ALWAYS_CHECK_DISTANCE))
    prep = M.PrepareConfig(True, 1, 3.0, 0)
    want, _ = resident(mix, prep, None, M.MODE_MSDF, 48, 48, mxf, config=c)
    lib = L.load()
    try:
        lib.msdfhip_set_pipeline_chunk(64)
        lib.msdfhip_pipeline_overflow_reruns(1)
        got = M.generate_stream(mix, M.MODE_MSDF, 48, 48, mxf, config=c, prepare=prep)
        assert lib.msdfhip_pipeline_overflow_reruns(1) == 1, "the stroke glyphs were meant to overflow their candidate segments"
        assert (bits(got) == bits(want)).all()
        a8 = np.zeros((mix.n_glyphs, 48, 48, 3), np.uint8)
        M.generate_stream(mix, M.MODE_MSDF, 48, 48, mxf, atlas=a8, out_offsets=np.arange(mix.n_glyphs, dtype=np.int64)*48*48*3, row_stride=48*3, config=c,
                          prepare=prep)
        assert lib.msdfhip_pipeline_overflow_reruns(1) == 1
        assert (a8 == byte_tiles(want)).all()
    finally:
        lib.msdfhip_set_pipeline_chunk(0)


def test_device_memory_stays_flat_over_repeated_calls(dejavu):
    """The preparation's buffers come from the pooled pipeline slots: grown once, reused by every later call, returned by msdfhip_trim."""
    import torch
    raw, xf48, _ = dejavu
    prep = M.PrepareConfig(True, 1, 3.0, 0)
    offs = np.arange(raw.n_glyphs, dtype=np.int64)*48*48*3
    atlas = np.zeros((raw.n_glyphs, 48, 48, 3), np.uint8)
    M.generate_stream(raw, M.MODE_MSDF, 48, 48, xf48, atlas=atlas, out_offsets=offs, row_stride=48*3, prepare=prep)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        M.generate_stream(raw, M.MODE_MSDF, 48, 48, xf48, atlas=atlas, out_offsets=offs, row_stride=48*3, prepare=prep)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free1 >= free0-(8 << 20), "device memory grew by %.1f MB over 20 calls" % ((free0-free1)/2**20)
    L.check(L.load().msdfhip_trim())
    free2, _ = torch.cuda.mem_get_info()
    assert free2 >= free1
