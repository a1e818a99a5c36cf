"""msdfhip_batch_gather on the GPU (GlyphBatch.select / .gather / .concat): a new batch out of glyphs of resident ones. The source is the 43 glyphs of
tests/test_gpu_sized.py plus one glyph without contours: 44 glyphs, 202 contours, 1 249 edges. Every comparison is bitwise: the result's arrays against the
host mirror's ShapeBatch.select, its tiles against the source's tiles for the same glyphs and against the oracle's, its bounds against the reference's
recorded ones (tests/golden/boxes.npz); then ownership (the source closed before the result renders) and stream order (the source's arrays overwritten on
the stream in front of the gather)."""
import ctypes as C
import functools

import numpy as np
import pytest

import msdfgen_amd as M
from msdfgen_amd import lib as L
from msdfgen_amd.shape import FlatShape, ShapeBatch
from conftest import assert_bit_equal
import boxcases as BC
import streamcases as SC
import test_gpu_sized as TS

pytestmark = pytest.mark.gpu
W, H = SC.W, SC.H
EMPTY_XF = (1., 1., 0., 0., -1., 1.)
EMPTY_BOX = (8, 8)
ODD = [43, 5, 5, 0, 42, 43, 5]
EC = (M.EC_EDGE_PRIORITY, M.CHECK_DISTANCE_AT_EDGE)
CASES = [(mode, overlap) for mode in (1, 2, 3, 4) for overlap in (True, False)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)
    info = M.device_info()
    assert info["arch"].startswith("gfx950"), info
    return info


def empty_shape():
    return FlatShape(np.zeros(1, np.int32), np.zeros((0, 8), np.float64), np.zeros(0, np.int32), np.zeros(0, np.int32), False)


@functools.lru_cache(maxsize=None)
def inputs():
    """(host batch of the 44, xfs (44, 6) for the W x H tile, sizes (44, 2), sized xfs (44, 6))."""
    a = SC.variants()["A"]
    shapes = ShapeBatch.from_shapes(list(a["shapes"])+[empty_shape()])
    return (shapes, np.vstack([a["xfs"], [EMPTY_XF]]), np.vstack([a["sizes"], [EMPTY_BOX]]).astype(np.int32), np.vstack([a["sized_xfs"], [EMPTY_XF]]))


def selections():
    rng = np.random.default_rng(4400)
    return {"identity": list(range(44)), "reversed": list(range(43, -1, -1)), "odd": list(ODD), "none": [], "one": [7],
            "draws": [int(v) for v in rng.integers(0, 44, 200)]}


@pytest.fixture(scope="module")
def source():
    gb = M.GlyphBatch(inputs()[0])
    yield gb
    gb.close()


def info_of(gb):
    v = [C.c_int() for _ in range(5)]
    L.check(L.load().msdfhip_batch_info(gb._handle, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def download(gb):
    ng, nc, ne, _, _ = info_of(gb)
    co, pts = np.full(nc+1, -1, np.int32), np.full((max(ne, 1), 8), np.nan)
    types, colors = np.full(max(ne, 1), 255, np.uint8), np.full(max(ne, 1), 255, np.uint8)
    L.check(L.load().msdfhip_batch_download(gb._handle, L.ptr(co, L._ip), L.ptr(pts, L._dp), L.ptr(types, L._bp), L.ptr(colors, L._bp)))
    return co, pts[:ne], types[:ne], colors[:ne]


def check_structure(gb, want: ShapeBatch, what):
    """The result's counts, maxima and arrays are those of the host batch `want`, byte for byte."""
    gco, co = want.glyph_contour_offsets, want.contour_offsets
    max_c = int(np.diff(gco).max()) if want.n_glyphs else 0
    max_e = int((co[gco[1:]]-co[gco[:-1]]).max()) if want.n_glyphs else 0
    assert info_of(gb) == (want.n_glyphs, want.n_contours, want.n_edges, max_c, max_e), what
    assert (gb.n_glyphs, gb.max_contours, gb.max_edges) == (want.n_glyphs, max_c, max_e), what
    got_co, pts, types, colors = download(gb)
    assert got_co.tolist() == np.asarray(co).tolist(), what
    assert SC.verdict(what+": points", pts, np.ascontiguousarray(want.points, np.float64).reshape(-1, 8)) is None
    assert types.tolist() == np.asarray(want.types).tolist() and colors.tolist() == np.asarray(want.colors).tolist(), what
    s = gb.shapes
    assert s.glyph_contour_offsets.tolist() == gco.tolist() and s.contour_offsets.tolist() == np.asarray(co).tolist() and s.inverse_y.tolist() == want.inverse_y.tolist(), what


def contours_of(shapes: ShapeBatch, idx):
    gco = shapes.glyph_contour_offsets
    return np.concatenate([np.arange(gco[i], gco[i+1]) for i in idx]+[np.zeros(0, np.int64)]).astype(np.int64)


def render(gb, mode, overlap, xfs):
    """(tiles (G, H, W, N), stencil (G, H, W) or None) of one generate call."""
    import torch
    if gb.n_glyphs == 0:                                           # (an empty batch has no descriptors to point at: nothing to call)
        return np.zeros((0, H, W, M.CHANNELS[mode]), np.float32), np.zeros((0, H, W), np.uint8) if mode >= 3 else None
    st = torch.full((max(gb.n_glyphs, 1)*H*W,), 77, dtype=torch.uint8, device="cuda") if mode >= 3 else None
    out = gb.generate(mode, W, H, xfs, config=TS.config(mode, overlap, EC), stencil=st)
    return out.cpu().numpy(), None if st is None else st.cpu().numpy()[:gb.n_glyphs*H*W].reshape(gb.n_glyphs, H, W)


_CACHE = {}


def source_tiles(source, mode, overlap):
    """The source's own tiles (and stencil) of all 44 glyphs: rendered once per configuration, shared, never written to."""
    key = ("tiles", mode, overlap)
    if key not in _CACHE:
        _CACHE[key] = render(source, mode, overlap, inputs()[1])
        for a in _CACHE[key]:
            if a is not None:
                a.setflags(write=False)
    return _CACHE[key]


def oracle_tiles(oracle, mode, overlap, shapes=None, xfs=None, key="A"):
    """The oracle's W x H tiles (and stencils) of the 44 glyphs (or of `shapes`, cached under `key`)."""
    k = ("oracle", key, mode, overlap)
    if k not in _CACHE:
        if shapes is None:
            shapes, xfs = inputs()[0].shapes(), inputs()[1]
        f, s = [], []
        for shape, xf in zip(shapes, xfs):
            sb = np.zeros((H, W), np.uint8)
            f.append(oracle.generate(shape, mode, W, H, xf, overlap=overlap, ec_mode=EC[0], ec_dist=EC[1], stencil=sb))
            s.append(sb)
        f, s = np.stack(f), np.stack(s)
        f.setflags(write=False), s.setflags(write=False)
        _CACHE[k] = (f, s)
    return _CACHE[k]


def assert_same_tiles(what, got, want, idx):
    """got = (tiles, stencil) of the result; want = the same of ALL glyphs of the source (or of the oracle): compared for the selection, every byte."""
    idx = np.asarray(idx, np.int64)
    assert SC.verdict(what+": tiles", got[0], want[0][idx]) is None, SC.verdict(what+": tiles", got[0], want[0][idx])
    if got[1] is not None:
        assert SC.verdict(what+": stencil", got[1], want[1][idx]) is None, SC.verdict(what+": stencil", got[1], want[1][idx])


def test_the_inputs_are_the_ones_described():
    shapes = inputs()[0]
    gco, co = shapes.glyph_contour_offsets, shapes.contour_offsets
    assert (shapes.n_glyphs, shapes.n_contours, shapes.n_edges) == (44, 202, 1249)
    assert (int(np.diff(gco).max()), int((co[gco[1:]]-co[gco[:-1]]).max())) == (20, 128) and gco[44] == gco[43]
    assert shapes.inverse_y[:43].tolist() == [int(g % 3 == 0) for g in range(43)]
    sub = shapes.select(ODD)
    assert (sub.n_glyphs, sub.n_contours, sub.n_edges) == (7, 44, 295)
    draws = selections()["draws"]
    assert len(draws) == 200 and len(set(draws)) < 200 and 43 in draws


@pytest.mark.parametrize("name", list(selections()))
def test_structure(source, name):
    """1: info and download of the result equal ShapeBatch.select(idx); the windings are the source's, gathered by contour."""
    idx = selections()[name]
    shapes = inputs()[0]
    got = source.select(idx)
    check_structure(got, shapes.select(idx), name)
    assert got.windings().tolist() == source.windings()[contours_of(shapes, idx)].tolist()
    got.close()
    check_structure(source, shapes, "the source afterwards")


@pytest.mark.parametrize("mode,overlap", CASES)
def test_rendering(oracle, source, mode, overlap):
    """2: the result's tiles and stencil are the source's tiles of the selected glyphs and the oracle's, bit for bit."""
    xfs = inputs()[1]
    for name, idx in selections().items():
        got = source.select(idx)
        tiles = render(got, mode, overlap, xfs[idx])
        assert tiles[0].shape == (len(idx), H, W, M.CHANNELS[mode])
        assert_same_tiles("%s vs the source's tiles" % name, tiles, source_tiles(source, mode, overlap), idx)
        assert_same_tiles("%s vs the oracle" % name, tiles, oracle_tiles(oracle, mode, overlap), idx)
        got.close()


def test_rendering_sized(oracle, source):
    """2, once through generate_sized with the boxes of tests/test_gpu_sized.py: per glyph the source's packed tile and the oracle's at the glyph's own size."""
    shapes, _, sizes, sized_xfs = inputs()
    cfg = TS.config(3, True, EC)
    out, off = source.generate_sized(3, sizes, sized_xfs, config=cfg)
    whole = out.cpu().numpy()
    got = source.select(ODD)
    out, goff = got.generate_sized(3, sizes[ODD], sized_xfs[ODD], config=cfg)
    flat = out.cpu().numpy()
    assert goff.tolist() == M.GlyphBatch.packed_offsets(sizes[ODD], 3).tolist()
    for k, g in enumerate(ODD):
        w, h = int(sizes[g, 0]), int(sizes[g, 1])
        tile = flat[goff[k]:goff[k+1]]
        assert SC.verdict("glyph %d vs the source's tile" % k, tile, whole[off[g]:off[g+1]]) is None
        want = oracle.generate(shapes.shape(g), 3, w, h, sized_xfs[g], overlap=True, ec_mode=EC[0], ec_dist=EC[1])
        assert SC.verdict("glyph %d vs the oracle" % k, tile, want) is None
    got.close()


def test_instances(oracle, source):
    """3: one glyph taken five times under five transformations -- as framed, mirrored in x, anisotropic, another range, mirrored in y and shifted."""
    g = 5
    shape, xf = inputs()[0].shape(g), inputs()[1][g]
    xfs = np.stack([xf, xf*[-1, 1, 1, 1, 1, 1]+[0, 0, -W/xf[0], 0, 0, 0], xf*[.75, 1.25, 1, 1, 1, 1], xf*[1, 1, 1, 1, 3, 2],
                    xf*[1, -1, 1, 1, 1, 1]+[0, 0, .3, -H/xf[1], 0, 0]])
    got = source.select([g]*5)
    check_structure(got, inputs()[0].select([g]*5), "instances")
    for mode, overlap in ((3, True), (4, False)):
        tiles = render(got, mode, overlap, xfs)
        want = np.stack([oracle.generate(shape, mode, W, H, x, overlap=overlap, ec_mode=EC[0], ec_dist=EC[1]) for x in xfs])
        assert SC.verdict("five instances, mode %d" % mode, tiles[0], want) is None, SC.verdict("five instances, mode %d" % mode, tiles[0], want)
        assert len(SC.equal_glyphs(tiles[0][1:], np.repeat(tiles[0][:1], 4, axis=0), 4)) == 0           # (the transformations do differ)
    got.close()


def test_two_sources_and_fixed_bounds():
    """4: glyphs of a batch of prepared arrays and of a batch prepared from raw outlines (whose bounds were fixed at creation), interleaved. The result's
    bounds are, row by row, the reference's recorded ones for the glyph's source, over the whole matrix of border, miter limit and polarity."""
    z, arrays, raw, prep = BC.golden()
    a = M.GlyphBatch(arrays)
    r = M.GlyphBatch.from_raw(raw, orient_contours=True, seed=BC.SEED)
    source_of, indices = [], []
    for i in range(arrays.n_glyphs):                               # a raw glyph in front of every 41st array glyph, each raw glyph at least once
        if i % 41 == 0:
            source_of.append(1), indices.append((i//41) % raw.n_glyphs)
        source_of.append(0), indices.append(i)
    assert set(range(raw.n_glyphs)) <= {i for s, i in zip(source_of, indices) if s == 1}
    from_raw = np.array(source_of) == 1
    idx = np.array(indices)
    got = M.GlyphBatch.gather([a, r], source_of, indices)
    check_structure(got, ShapeBatch.from_shapes([(r if s else a).shapes.shape(i) for s, i in zip(source_of, indices)]), "two sources")

    def want(array_rows, raw_rows):
        out = np.zeros((len(idx), 4))
        out[~from_raw], out[from_raw] = array_rows[idx[~from_raw]], raw_rows[idx[from_raw]]
        return out
    assert_bit_equal(got.bounds(), want(z["bounds"][:, BC.combo(0., 0., 0)], z["raw_plain"]), "plain bounds")
    for k, (border, limit, polarity) in enumerate(BC.MATRIX):
        assert_bit_equal(got.bounds(border, limit, polarity), want(z["bounds"][:, k], z["raw_bounds"][:, k]), "bounds%s" % ((border, limit, polarity),))
    # without a source of fixed bounds nothing is copied: the result computes the same bits from the arrays it holds
    plain = a.select(list(range(arrays.n_glyphs-1, -1, -1)))
    assert_bit_equal(plain.bounds(), z["bounds"][::-1, BC.combo(0., 0., 0)], "bounds computed on demand")
    k = BC.combo(.125, 4., 0)
    assert_bit_equal(plain.bounds(.125, 4., 0), z["bounds"][::-1, k], "bounds with miters computed on demand")
    for gb in (plain, got, a, r):
        gb.close()


def test_lifetime(oracle):
    """5: the result borrows nothing. The source is closed as soon as select() has returned, and its arrays' memory is handed out again and overwritten."""
    import torch
    shapes, xfs = inputs()[0], inputs()[1]
    src = M.GlyphBatch(shapes)
    idx = selections()["draws"]
    got = src.select(idx)
    src.close()
    del src
    junk = [torch.full((n,), 0x7f, dtype=torch.uint8, device="cuda") for n in (4*45, 4*203, 64*1249, 1249, 1249)]     # (the sizes of the arrays just freed)
    check_structure(got, shapes.select(idx), "after the source is gone")
    tiles = render(got, 3, True, xfs[idx])
    assert_same_tiles("after the source is gone, vs the oracle", tiles, oracle_tiles(oracle, 3, True), idx)
    del junk
    got.close()


def test_stream_order(oracle):
    """6: on one non-default stream: the in-place overwrite of the source's points and colours with variant B, then the gather, then generate. Every glyph of
    the result must be B's; a gather that read its inputs when it was called would deliver A's."""
    import torch
    a, b = SC.variants()["A"], SC.variants()["B"]
    host_a, host_b = ShapeBatch.from_shapes(a["shapes"]), ShapeBatch.from_shapes(b["shapes"])
    assert host_a.contour_offsets.tolist() == host_b.contour_offsets.tolist() and host_a.types.tolist() == host_b.types.tolist()
    idx = [42, 5, 5, 0, 17, 42, 30, 11]
    n = M.CHANNELS[3]
    src = M.GlyphBatch(host_a)
    pts_b = torch.from_numpy(np.ascontiguousarray(host_b.points, np.float64)).to("cuda")
    col_b = torch.from_numpy(np.ascontiguousarray(host_b.colors, np.uint8)).to("cuda")
    mirror = M.GlyphBatch(host_b.select(idx))                      # (only for its descriptors: made on torch's current stream, which is not under test)
    desc = mirror.descriptors(b["xfs"][idx], W, H, n)
    out = torch.full((len(idx), H, W, n), float("nan"), dtype=torch.float32, device="cuda")
    ballast = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for v in range(4):                                         # work in front, so that the overwrite is still pending when the gather is called
            ballast.fill_(v)
        src._pts.copy_(pts_b, non_blocking=True)
        src._colors.copy_(col_b, non_blocking=True)
    got = M.GlyphBatch.gather([src], None, idx, stream=stream)
    got.generate(3, W, H, config=TS.config(3, True, EC), out=out, descriptors=desc, stream=stream)
    stream.synchronize()
    tiles = out.cpu().numpy()
    want_b = oracle_tiles(oracle, 3, True, b["shapes"], b["xfs"], key="B")[0][idx]
    stale = np.stack([oracle.generate(a["shapes"][g], 3, W, H, b["xfs"][g], overlap=True, ec_mode=EC[0], ec_dist=EC[1]) for g in idx])
    assert SC.equal_glyphs(want_b, stale, len(idx)) == []                                               # A's outlines under B's transforms: other bytes for every glyph
    assert SC.equal_glyphs(tiles, want_b, len(idx)) == list(range(len(idx))), SC.verdict("tiles behind the overwrite", tiles, want_b, stale)
    assert SC.equal_glyphs(tiles, stale, len(idx)) == []
    got.shapes = host_b.select(idx)                                # (the host mirror was taken from the source's, which still says A)
    check_structure(got, host_b.select(idx), "the arrays behind the overwrite")
    for gb in (got, mirror, src):
        gb.close()


def test_concat(oracle, source):
    """7: concat([a, b]) equals a batch created from the concatenated host shapes."""
    shapes, xfs = inputs()[0], inputs()[1]
    first, second = list(range(0, 20)), list(range(20, 44))
    a, b = M.GlyphBatch(shapes.select(first)), M.GlyphBatch(shapes.select(second))
    got = M.GlyphBatch.concat([a, b])
    check_structure(got, ShapeBatch.from_shapes(shapes.select(first).shapes()+shapes.select(second).shapes()), "concat")
    check_structure(got, shapes, "concat vs the 44")
    assert got.windings().tolist() == source.windings().tolist()
    for mode, overlap in ((1, True), (3, True), (4, False)):
        tiles = render(got, mode, overlap, xfs)
        assert_same_tiles("concat vs the source's tiles", tiles, source_tiles(source, mode, overlap), range(44))
        assert_same_tiles("concat vs the oracle", tiles, oracle_tiles(oracle, mode, overlap), range(44))
    for gb in (got, a, b):
        gb.close()


def test_refusals_with_a_batch(source):
    """The refusals that read a source (tests/test_gather_plan_host.py has the plan's own and those without a batch): the position is named, nothing is made."""
    lib = L.load()
    ip = C.POINTER(C.c_int32)
    out = C.c_void_p()
    two = (C.c_void_p*2)(source._handle, source._handle)

    def gather(n_sources, source_of, indices):
        so = None if source_of is None else np.ascontiguousarray(source_of, np.int32)
        ix = np.ascontiguousarray(indices, np.int32)
        return lib.msdfhip_batch_gather(C.byref(out), two, n_sources, len(ix), None if so is None else so.ctypes.data_as(ip), ix.ctypes.data_as(ip), None)
    assert gather(1, None, [0, 43, 44]) == L.ERR_INVALID and b"indices[2] = 44" in lib.msdfhip_last_error()
    assert gather(1, None, [0, -1, 44]) == L.ERR_INVALID and b"indices[1] = -1" in lib.msdfhip_last_error()
    assert gather(2, [0, 1, 2], [0, 0, 0]) == L.ERR_INVALID and b"source_of[2] = 2" in lib.msdfhip_last_error()
    assert gather(1, [0, 1], [0, 0]) == L.ERR_INVALID and b"source_of[1] = 1" in lib.msdfhip_last_error()
    assert gather(2, None, [0]) == L.ERR_INVALID and b"source_of is NULL" in lib.msdfhip_last_error()
    assert not out.value
    with pytest.raises(M.MsdfHipError):
        source.select([44])
    # the same batch as both sources is fine
    got = M.GlyphBatch.gather([source, source], [1, 0, 1], [43, 5, 5])
    check_structure(got, inputs()[0].select([43, 5, 5]), "one batch as two sources")
    got.close()
