"""The legacy route on the GPU -- k_distance_legacy, k_ec_legacy and the host flow runGenerateLegacy -- on every framing family (xformcases), every outline
family (geomcases), throughput-shaped batches placed into atlases, every branch of the flow, long outlines and a bounded random sweep, against
legacycases.reference_call: the host build of msdf_legacy.hpp for the raw field and the plain-C oracle for the sign pass and the correction, pinned to
the compiled reference by tests/test_legacy_cases_host.py. Nothing here reads the reference.

Bounds: those of tests/test_gpu_routes.py: check_parity, through test_gpu_sized.Tally -- max |delta| <= 1e-5, values differing bitwise
<= 1e-6 of the values compared (zero at these sizes), stencils exact."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import msdfgen_amd as M
import fuzzlib
import geomcases as GC
import legacycases as LC
import xformcases as XC
from msdfgen_amd import lib as L
from msdfgen_amd import synth
from msdfgen_amd.shape import ShapeBatch, autoframe
from test_gpu_sized import SENTINEL, Tally, atlas_placement
from test_gpu_sized import glyphs as sized_glyphs

pytestmark = pytest.mark.gpu
THE_CASE = "degenerate_edges/cubic_p2_on_p3"          # 12x12, upward shape: under a Y-down bitmap one stencil byte tells the shape's row order from the bitmap's
W, H = 24, 17                                         # nine tiles per glyph
RATIOS = (1.5, 1.3)                                   # min_deviation_ratio, min_improve_ratio: values fuzzlib draws
DEFAULT_RATIOS = (LC.DEFAULT_RATIO, LC.DEFAULT_RATIO)


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return LC.build_host(tmp_path_factory.mktemp("legacy_host"))


class Call:
    """What one legacy call is asked for: mode, ErrorCorrectionConfig::Mode (modes 3, 4), bitmap orientation, the sign pass (LC.SignPass or None), ratios."""

    def __init__(self, mode, ec=2, y_down=False, sign=None, ratios=DEFAULT_RATIOS):
        self.mode, self.ec, self.y_down, self.sign, self.ratios = mode, (ec if mode >= 3 else 0), bool(y_down), sign, ratios
        self.corrects = mode >= 3 and self.ec != 0
        self.key = (mode, self.ec, self.y_down, sign, ratios)

    def ec_config(self):
        return M.ErrorCorrectionConfig(mode=self.ec, min_deviation_ratio=self.ratios[0], min_improve_ratio=self.ratios[1]) if self.mode >= 3 else None

    def c_config(self):
        cfg = L.default_config(ec_mode=self.ec if self.mode >= 3 else M.EC_EDGE_PRIORITY, stencil_y_down=int(self.y_down))
        cfg.min_deviation_ratio, cfg.min_improve_ratio = self.ratios
        if self.sign is not None:
            cfg.sign_correction, cfg.fill_rule, cfg.sdf_zero_value = 1, self.sign.fill_rule, self.sign.zero
        return cfg

    def kwargs(self):
        return dict(config=self.ec_config(), y_orientation=M.Y_DOWNWARD if self.y_down else M.Y_UPWARD, scanline_pass=self.sign is not None,
                    fill_rule=self.sign.fill_rule if self.sign else 0, sdf_zero_value=self.sign.zero if self.sign else .5)


_WANT = {}


def want(host, oracle, name, shape, w, h, xf, call):
    """reference_call of one glyph: computed once per (glyph, call), shared, never written to."""
    key = (name, w, h)+call.key
    if key not in _WANT:
        f, st = LC.reference_call(host, oracle, shape, call.mode, w, h, xf, ec_mode=call.ec, y_down=call.y_down, sign=call.sign, min_dev=call.ratios[0],
                                  min_imp=call.ratios[1])
        f.setflags(write=False)
        if st is not None:
            st.setflags(write=False)
        _WANT[key] = (f, st)
    return _WANT[key]


def single(shape, w, h, xf, call):
    """One msdfhip_generate_legacy call: (bitmap, stencil or None)."""
    out = np.full((h, w, LC.CHANNELS[call.mode]), 3., np.float32)
    stencil = np.full((h, w), 77, np.uint8) if call.corrects else None
    co, pts, types, colors = LC.shape_arrays(shape)
    x6, cfg = LC.xf6(xf), call.c_config()
    flip = int(bool(shape.inverse_y) != call.y_down)
    L.check(L.load().msdfhip_generate_legacy(call.mode, L.ptr(out, L._fp), w, h, out.strides[0]//4, flip, L.ptr(co, L._ip), shape.n_contours, L.ptr(pts, L._dp),
                                             L.ptr(types, L._bp), L.ptr(colors, L._bp), L.ptr(x6, L._dp), C.byref(cfg),
                                             L.ptr(stencil, L._bp) if stencil is not None else None))
    return out, stencil


def batched(shapes, w, h, xfs, call, stream=None, gb=None):
    """GlyphBatch.generate_legacy: ([bitmap per glyph], [stencil per glyph] or None)."""
    own = gb is None
    gb = gb or M.GlyphBatch(ShapeBatch.from_shapes(shapes))
    st = torch.full((len(xfs), h, w), 77, dtype=torch.uint8, device=gb.device) if call.corrects else None
    tiles = gb.generate_legacy(call.mode, w, h, np.stack(xfs), stencil=st, stream=stream, **call.kwargs())
    if stream is not None:
        stream.synchronize()
    tiles = tiles.cpu().numpy()
    st = st.cpu().numpy() if st is not None else None
    if own:
        gb.close()
    return list(tiles), (list(st) if st is not None else None)


def add(tally, what, host, oracle, cases, call, got, got_st):
    ws = [want(host, oracle, c.name, c.shape, c.w, c.h, c.xf, call) for c in cases]
    assert (got_st is not None) == call.corrects
    tally.add(what, got, got_st, [f for f, _ in ws], [s for _, s in ws])


# ---------------------------------------------------------------------------------------------------------- framing families

def test_framing_families_in_single_calls(host, oracle):
    """Every case of xformcases.cases(seeds=(0, 1)) -- mirrored and anisotropic projections, zooms, off-tile glyphs, inverted / huge / tiny / asymmetric
    ranges, all-ones significands, far-off coordinates, bitmaps of 1x1 ... 65x2 -- through msdfhip_generate_legacy in all four modes, under the case's own
    orientations; modes 3 and 4 cycle through the four correction modes, with a stencil wherever a correction runs."""
    cases = XC.cases(seeds=(0, 1))
    assert {c.name.split("/")[0] for c in cases} == set(XC.FAMILIES) and {(c.w, c.h) for c in cases} >= set(XC.TINY_SIZES)
    assert {(bool(c.shape.inverse_y), c.y_down) for c in cases if c.name.split("/")[0] in XC.MIRRORS} == {(False, False), (False, True), (True, False), (True, True)}
    t = Tally()
    seen = set()
    for i, c in enumerate(cases):
        XC.check_premise(c)
        for mode in (1, 2, 3, 4):
            call = Call(mode, ec=(i+mode) % 4, y_down=c.y_down)
            out, st = single(c.shape, c.w, c.h, c.xf, call)
            add(t, (c.name, call.key), host, oracle, [c], call, [out], [st] if st is not None else None)
            seen.add((mode, call.ec))
    assert seen == {(1, 0), (2, 0)} | {(m, e) for m in (3, 4) for e in range(4)}
    t.check()
    assert t.st_compared > 0


# ---------------------------------------------------------------------------------------------------------- outline families

def outline_cases():
    cs = GC.bit_exact(GC.cases())
    assert len(cs) < len(GC.cases()) and not any(GC.base_name(c) in GC.SIGN_NOISE for c in cs)
    return cs


def test_outline_families_in_single_calls(host, oracle):
    """geomcases: lattice ties, texels on the outline, coincident edges, degenerate edges, sparse colourings, scanline hits, slivers -- single calls."""
    t = Tally()
    for i, c in enumerate(outline_cases()):
        for mode in (1, 2, 3, 4):
            for y_down in ((c.y_down,) if mode < 3 else (False, True)):
                call = Call(mode, ec=2 if mode == 3 else 1+(i % 3), y_down=y_down)
                out, st = single(c.shape, c.w, c.h, c.xf, call)
                add(t, (c.name, call.key), host, oracle, [c], call, [out], [st] if st is not None else None)
    t.check()
    assert t.st_compared > 0


def test_outline_families_in_resident_batches(host, oracle):
    """The same cases as resident batches, grouped by bitmap size, every group under both bitmap orientations with stencils. Among them cubic_p2_on_p3
    (an upward shape) under a Y-down bitmap with EDGE_PRIORITY: the stencil byte that a correction along the bitmap's rows gets wrong."""
    groups = {}
    for c in outline_cases():
        groups.setdefault((c.w, c.h), []).append(c)
    t = Tally()
    the_case = 0
    for (w, h), cs in sorted(groups.items()):
        for y_down in (False, True):
            for mode, ec in ((3, 2), (4, 1), (4, 2), (3, 3)):
                call = Call(mode, ec=ec, y_down=y_down)
                got, got_st = batched([c.shape for c in cs], w, h, [c.xf for c in cs], call)
                add(t, ((w, h), call.key), host, oracle, cs, call, got, got_st)
                for k, c in enumerate(cs):
                    if GC.base_name(c) == THE_CASE and (w, h) == (12, 12) and not c.shape.inverse_y and y_down and ec == 2:
                        the_case += 1
                        ws = want(host, oracle, c.name, c.shape, w, h, c.xf, call)[1]
                        assert np.array_equal(got_st[k], ws), (c.name, mode, np.argwhere(got_st[k] != ws).tolist())
    t.check()
    assert the_case >= 2 and t.st_compared > 0


# ---------------------------------------------------------------------------------------------------------- batch shape and placement

def sized_cases():
    """The 43 glyphs of test_gpu_sized.glyphs()'s recipe (every third an inverse-Y one), all framed into 24 x 17."""
    shapes, _, _ = sized_glyphs()
    return [XC.Case("sized/%d" % g, s, W, H, autoframe(s.bounds(), W, H, 2.), False) for g, s in enumerate(shapes)]


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_batch_of_43_packed(host, oracle, mode):
    """43 glyphs x 9 tiles: neither a multiple of 8 (decodeBlock's full groups and its remainder), correction on, both bitmap orientations."""
    cs = sized_cases()
    assert len(cs) == 43 and ((W+7)//8)*((H+7)//8) == 9 and any(c.shape.inverse_y for c in cs) and not all(c.shape.inverse_y for c in cs)
    t = Tally()
    for y_down in (False, True):
        call = Call(mode, ec=2, y_down=y_down)
        got, got_st = batched([c.shape for c in cs], W, H, [c.xf for c in cs], call)
        add(t, call.key, host, oracle, cs, call, got, got_st)
    t.check()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_direct_writes_into_an_atlas(mode):
    """No sign pass and no correction (modes 1, 2; mode 3 with the correction disabled): k_distance_legacy writes the caller's bitmap itself, at
    out_offset + row_stride*row. The boxes go into a sentinel-filled float atlas with gaps, every fourth glyph bottom-up (a negative row stride): every
    rectangle equals the packed result (itself compared with the reference above and below), every other texel keeps its bits."""
    cs = sized_cases()
    shapes, xfs = [c.shape for c in cs], np.stack([c.xf for c in cs])
    n = LC.CHANNELS[mode]
    call = Call(mode, ec=0, y_down=True)
    gb = M.GlyphBatch(ShapeBatch.from_shapes(shapes))
    packed, _ = batched(shapes, W, H, xfs, call, gb=gb)
    sizes = np.tile(np.array([[W, H]], np.int32), (len(cs), 1))
    rows, stride, first, negative = atlas_placement(sizes, n)
    offsets = np.where(negative, first+(H-1)*stride, first)
    strides = np.where(negative, -stride, stride)
    assert negative.sum() >= 10 and offsets.min() >= 0 and (first+(H-1)*stride+W*n).max() <= rows*stride
    # (the atlas lies inside a larger allocation, a glyph's height of rows on either side: a wrong offset or stride sign shows there and stays inside it)
    whole = torch.from_numpy(np.full((rows+2*H)*stride, SENTINEL, np.uint32).view(np.float32)).cuda()
    atlas = whole[H*stride:(H+rows)*stride]
    desc = gb.descriptors(xfs, W, H, n, M.Y_DOWNWARD, out_offsets=offsets, row_stride=strides)
    out = gb.generate_legacy(mode, W, H, descriptors=desc, out=atlas, **call.kwargs())
    assert out is atlas
    everything = whole.cpu().numpy().view(np.uint32).reshape(rows+2*H, stride)
    got = everything[H:H+rows]
    gb.close()
    assert (everything[:H] == SENTINEL).all() and (everything[H+rows:] == SENTINEL).all(), "texels outside the atlas were written"
    written = np.zeros_like(got, bool)
    for g in range(len(cs)):
        r0, x0 = divmod(int(first[g]), stride)
        rect = got[r0:r0+H, x0:x0+W*n]
        rect = rect[::-1] if negative[g] else rect
        assert np.array_equal(rect.reshape(H, W, n), packed[g].view(np.uint32)), "glyph %d (negative stride: %s)" % (g, bool(negative[g]))
        written[r0:r0+H, x0:x0+W*n] = True
    assert (got[~written] == SENTINEL).all() and (~written).sum() > 0 and (got[written] != SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------- every branch of the flow

def flow_calls(mode):
    """(sign pass, correction) each on and off -- modes 1, 2 have no correction -- under both bitmap orientations: every fill rule, a zero level other than
    .5, and the non-default ratios wherever a correction runs."""
    out = []
    for y_down in (False, True):
        for correct in ((False, True) if mode >= 3 else (False,)):
            ec = (2 if y_down else 1) if correct else 0
            out.append(Call(mode, ec=ec, y_down=y_down))
            if correct:
                out.append(Call(mode, ec=2, y_down=y_down, ratios=RATIOS))
            for rule in range(4):
                out.append(Call(mode, ec=ec, y_down=y_down, sign=LC.SignPass(rule, .3 if rule == 2 else .5), ratios=RATIOS if correct and rule == 1 else DEFAULT_RATIOS))
    return out


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_every_branch_of_the_flow(host, oracle, mode):
    """runGenerateLegacy's four branches on a batch of nine that mixes inverse-Y and upward shapes: the field straight to the caller; the sign pass as the
    last stage; the correction along the shape's rows; sign pass then correction on the bitmap as it lies (the reference CLI's flow)."""
    cs = sized_cases()[:9]
    assert {bool(c.shape.inverse_y) for c in cs} == {False, True}
    calls = flow_calls(mode)
    assert {(c.sign is not None, c.corrects) for c in calls} == ({(False, False), (True, False), (False, True), (True, True)} if mode >= 3 else {(False, False), (True, False)})
    assert {c.sign.fill_rule for c in calls if c.sign} == {0, 1, 2, 3} and any(c.sign and c.sign.zero != .5 for c in calls)
    gb = M.GlyphBatch(ShapeBatch.from_shapes([c.shape for c in cs]))
    t = Tally()
    for call in calls:
        got, got_st = batched(None, W, H, [c.xf for c in cs], call, gb=gb)
        add(t, call.key, host, oracle, cs, call, got, got_st)
    gb.close()
    t.check()
    assert mode < 3 or t.st_compared > 0


@pytest.mark.parametrize("own_scratch", [False, True])
def test_c_abi_scratch_and_stream(host, oracle, own_scratch):
    """msdfhip_batch_generate_legacy with d_scratch == NULL (the library's own scratch) and with the caller's, two stages each (sign pass + correction) and
    one stage, on a torch stream that is not the default one."""
    cs = sized_cases()[9:18]
    gb = M.GlyphBatch(ShapeBatch.from_shapes([c.shape for c in cs]))
    stream = torch.cuda.Stream()
    t = Tally()
    for call in (Call(4, ec=2, y_down=True, sign=LC.SignPass(1, .5)), Call(3, ec=1, y_down=False), Call(1, sign=LC.SignPass(0, .5))):
        n = LC.CHANNELS[call.mode]
        stages = int(call.corrects)+int(call.sign is not None)
        desc = gb.descriptors(np.stack([c.xf for c in cs]), W, H, n, M.Y_DOWNWARD if call.y_down else M.Y_UPWARD)
        with torch.cuda.stream(stream):
            out = torch.full((len(cs), H, W, n), 3., dtype=torch.float32, device=gb.device)
            st = torch.full((len(cs), H, W), 77, dtype=torch.uint8, device=gb.device) if call.corrects else None
            scratch = torch.empty(stages*len(cs)*H*W*n, dtype=torch.float32, device=gb.device) if own_scratch else None
        cfg = call.c_config()
        L.check(L.load().msdfhip_batch_generate_legacy(gb._handle, call.mode, W, H, desc.data_ptr(), out.data_ptr(), st.data_ptr() if st is not None else None,
                                                       scratch.data_ptr() if scratch is not None else None, C.byref(cfg), stream.cuda_stream))
        stream.synchronize()
        add(t, (own_scratch, call.key), host, oracle, cs, call, list(out.cpu().numpy()), list(st.cpu().numpy()) if st is not None else None)
    gb.close()
    t.check()


def test_generate_legacy_on_a_side_stream(host, oracle):
    cs = sized_cases()[18:27]
    t = Tally()
    for call in (Call(3, ec=2, y_down=True), Call(4, ec=2, sign=LC.SignPass(3, .5)), Call(2)):
        got, got_st = batched([c.shape for c in cs], W, H, [c.xf for c in cs], call, stream=torch.cuda.Stream())
        add(t, call.key, host, oracle, cs, call, got, got_st)
    t.check()


# ---------------------------------------------------------------------------------------------------------- frame=

@pytest.mark.parametrize("mode", [2, 3])
def test_frame_argument(host, oracle, mode):
    """generate_legacy(frame=FrameConfig(px_range=4)) == generate_legacy on descriptors that GlyphBatch.frame() filled, byte for byte, == the reference on
    those transforms."""
    cs0 = sized_cases()[27:36]
    shapes = [c.shape for c in cs0]
    gb = M.GlyphBatch(ShapeBatch.from_shapes(shapes))
    fc = M.FrameConfig(px_range=4)
    call = Call(mode, ec=2, y_down=True)
    n = LC.CHANNELS[mode]
    st = torch.full((len(shapes), H, W), 77, dtype=torch.uint8, device=gb.device) if call.corrects else None
    framed = gb.generate_legacy(mode, W, H, frame=fc, stencil=st, **call.kwargs()).cpu().numpy()
    desc = gb.descriptors(None, W, H, n, M.Y_DOWNWARD)
    rows = gb.frame(W, H, fc, descriptors=desc)
    explicit = gb.generate_legacy(mode, W, H, descriptors=desc, **call.kwargs()).cpu().numpy()
    gb.close()
    assert np.array_equal(framed.view(np.uint32), explicit.view(np.uint32))
    xfs = [np.array(list(r[:4])+list(LC.range_of(r[4], r[5]))) for r in rows]       # (sx, sy, tx, ty, range): what maps to exactly the device's rows
    assert np.array_equal(rows.view(np.uint64), np.stack([LC.xf6(xf) for xf in xfs]).view(np.uint64))
    auto = np.stack([LC.xf6(autoframe(s.bounds(), W, H, 4)) for s in shapes])
    assert np.allclose(rows, auto, rtol=.5) and (rows[:, 0] > 0).all()             # (-autoframe: near the control-point box's framing, which is not Shape::getBounds')
    cs = [XC.Case("framed/%d" % k, s, W, H, xf, True) for k, (s, xf) in enumerate(zip(shapes, xfs))]
    t = Tally()
    add(t, call.key, host, oracle, cs, call, list(framed), list(st.cpu().numpy()) if st is not None else None)
    t.check()


# ---------------------------------------------------------------------------------------------------------- long walks

def test_long_outlines(host, oracle):
    """A contour of 1000 edges and an outline of 100 contours at 17x9 (the walk is one lane per texel over ALL edges), modes 2 and 4, as single calls and as
    the 5th and 6th glyph of a batch of nine."""
    long_one = synth.random_shape(71, n_contours=1, edges_per_contour=(1000, 1000))
    many = synth.random_shape(72, n_contours=100, edges_per_contour=(3, 5))
    assert long_one.n_edges >= 1000 and many.n_contours >= 100
    w, h = 17, 9
    filler = sized_cases()[36:43]
    shapes = [c.shape for c in filler[:4]]+[long_one, many]+[c.shape for c in filler[4:]]
    cs = [XC.Case("long/%d" % k, s, w, h, autoframe(s.bounds(), w, h, 2.), False) for k, s in enumerate(shapes)]
    assert len(cs) == 9
    t = Tally()
    for mode in (2, 4):
        call = Call(mode, ec=2, y_down=mode == 4)
        for c in cs[4:6]:
            out, st = single(c.shape, w, h, c.xf, call)
            add(t, (c.name, call.key), host, oracle, [c], call, [out], [st] if st is not None else None)
        got, got_st = batched(shapes, w, h, [c.xf for c in cs], call)
        add(t, ("batch", call.key), host, oracle, cs, call, got, got_st)
    t.check()


# ---------------------------------------------------------------------------------------------------------- bounded sweep

def test_bounded_sweep(host, oracle):
    """Seeded groups of 9-43 random outlines at one size per group (1..40 on each axis); modes and correction modes rotate, every second group takes the sign
    pass, every third the non-default ratios. 8 s, at least 4 groups."""
    rng = np.random.default_rng(9043)
    t = Tally()
    t0, groups, deadline, min_groups = time.time(), 0, 8., 4
    while groups < min_groups or time.time()-t0 < deadline:
        n = int(rng.integers(9, 44))
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        cs = []
        for k in range(n):
            s = fuzzlib._shape(rng, (5, 6, 0, 3, 1, 2)[k % 6], int(rng.integers(0, 2**31)))
            s.inverse_y = bool(rng.integers(0, 2))
            cs.append(XC.Case("sweep/%d.%d" % (groups, k), s, w, h, autoframe(s.bounds(), w, h, min(2., .5*min(w, h))), False))
        mode = 1+groups % 4
        sign = LC.SignPass(int(rng.integers(0, 4)), .5) if groups % 2 else None
        call = Call(mode, ec=(groups//4) % 4, y_down=bool(rng.integers(0, 2)), sign=sign, ratios=RATIOS if groups % 3 == 2 else DEFAULT_RATIOS)
        got, got_st = batched([c.shape for c in cs], w, h, [c.xf for c in cs], call)
        add(t, (groups, (w, h), call.key), host, oracle, cs, call, got, got_st)
        groups += 1
        if groups >= 400:
            break
    print("groups:", groups)
    assert groups >= min_groups
    t.check()


# ---------------------------------------------------------------------------------------------------------- k_ec_legacy on crafted fields

def test_legacy_correction_of_crafted_fields_on_host_bitmaps():
    """msdfhip_error_correction_legacy on fields of infinities, NaN, -0, equalized texels and differences at and one ulp around the thresholds, packed and
    as the rows of a wider bitmap walked bottom-up, against the recorded outputs of the reference: bitwise, a NaN equal to a NaN only."""
    recs = LC.crafted_golden()
    assert {(e.n, e.w, e.h) for e in recs} == {(n, w, h) for n in (3, 4) for (w, h) in LC.CRAFTED_SIZES}
    for e in recs:
        what = (e.n, e.w, e.h)
        assert LC.differing(M.msdf_error_correction_legacy(e.field.copy(), (e.tx, e.ty)), e.out) == 0, what
        wide = np.full((e.h, e.w+2, e.n), 5., np.float32)
        view = wide[::-1, :e.w]
        view[...] = e.field
        M.msdf_error_correction_legacy(view, (e.tx, e.ty))
        assert LC.differing(np.ascontiguousarray(view), e.out) == 0, what+("strided",)
        assert (wide[:, e.w:] == 5.).all()


def test_legacy_correction_of_crafted_fields_on_device_tiles(host):
    """The same fields through msdfhip_batch_error_correction_legacy as the 5th of 9 tiles; the others are the same field with its rows, its columns or
    its channels reversed and random ones, checked against the host build of the passes."""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    for e in LC.crafted_golden():
        nine = rng.uniform(0, 1, (9, e.h, e.w, e.n)).astype(np.float32)
        nine[4] = e.field
        nine[3], nine[5] = e.field[::-1], e.field[:, ::-1]
        nine[0][..., :3] = e.field[..., 2::-1]
        wanted = np.stack([LC.host_correction(host, t, e.tx, e.ty) for t in nine])
        assert LC.differing(wanted[4], e.out) == 0
        got = M.error_correction_legacy(torch.from_numpy(nine.copy()).to(dev), (e.tx, e.ty)).cpu().numpy()
        assert LC.differing(got[4], e.out) == 0, (e.n, e.w, e.h)
        assert LC.differing(got, wanted) == 0, (e.n, e.w, e.h, "9 tiles")
