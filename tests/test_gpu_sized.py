"""GlyphBatch.generate_sized: glyph boxes of different sizes in ONE batched generate call (msdfhip_batch_generate_sized), against the oracle per glyph at
that glyph's own size -- the correction and sign passes' behaviour at the box's own borders included --, under the forced launch routes, placed into
atlases, and against the existing uniform call (all sizes equal; one uniform call per distinct size).

43 glyphs (not a multiple of 8: the tail of decodeItem's interleave) whose boxes cycle through BOXES, so the launches have the shape of a 24 x 17 call:
nine tiles per slot, not a multiple of the quad; boxes that end inside a tile on both axes, boxes that end on a tile edge, one that fills the slot."""
import ctypes as C
import functools

import numpy as np
import pytest

import msdfgen_amd as M
import fuzzlib
from msdfgen_amd import lib as L
from msdfgen_amd.shape import ShapeBatch, autoframe
from test_gpu_routes import FORCED

pytestmark = pytest.mark.gpu
TOL = 1e-5                                                                  # the bounds of tests/test_gpu_routes.py: check_parity
BOXES = ((1, 1), (7, 9), (8, 8), (9, 8), (8, 9), (24, 1), (1, 17), (23, 17), (16, 16), (17, 10), (24, 17))
N_GLYPHS = 43
W, H = 24, 17
KINDS = (5, 6, 0, 3, 1, 2)             # fuzzlib's synthesizers: one contour | two | one to three | many (4-11) | cubic | many (CJK-like)
SENTINEL = 0x7fc0dead                  # a NaN payload no kernel writes


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)
    info = M.device_info()
    assert info["arch"].startswith("gfx950"), info
    return info


@functools.lru_cache(maxsize=None)
def glyphs():
    """(shapes, sizes (G, 2), xfs (G, 6)): every glyph framed into its own box; every third shape is an inverse-Y one."""
    rng = np.random.default_rng(4300)
    sizes = np.array([BOXES[g % len(BOXES)] for g in range(N_GLYPHS)], np.int32)
    shapes = []
    for g in range(N_GLYPHS):
        s = fuzzlib._shape(rng, KINDS[g % len(KINDS)], int(rng.integers(0, 2**31)))
        s.inverse_y = g % 3 == 0
        shapes.append(s)
    xfs = np.stack([autoframe(s.bounds(), int(w), int(h), min(2., .5*min(int(w), int(h)))) for s, (w, h) in zip(shapes, sizes)])
    return shapes, sizes, xfs


@functools.lru_cache(maxsize=None)
def batch():
    return M.GlyphBatch(ShapeBatch.from_shapes(glyphs()[0]))


@functools.lru_cache(maxsize=None)
def repeated(reps):
    """The 43 glyphs `reps` times over (same shapes, boxes and transforms: glyph g is glyph g % 43 of the oracle's reference) -> (batch, sizes, xfs)."""
    shapes, sizes, xfs = glyphs()
    return M.GlyphBatch(ShapeBatch.from_shapes(list(shapes)*reps)), np.tile(sizes, (reps, 1)), np.tile(xfs, (reps, 1))


def config(mode, overlap, ec):
    return M.MSDFGeneratorConfig(overlap, M.ErrorCorrectionConfig(ec[0], ec[1])) if mode >= 3 else M.GeneratorConfig(overlap)


def render(mode, overlap, ec, y_down, rule=None, want_stencil=True, gb=None, sizes=None, xfs=None):
    """One generate_sized call -> (per-glyph float arrays (h_g, w_g, N), per-glyph stencils (h_g, w_g) or None, flat float array, route-counter deltas)."""
    import torch
    gb = gb or batch()
    if sizes is None:
        _, sizes, xfs = glyphs()
    n = M.CHANNELS[mode]
    slot = int(sizes[:, 0].max())*int(sizes[:, 1].max())
    st = torch.full((gb.n_glyphs*slot,), 77, dtype=torch.uint8, device="cuda") if want_stencil and mode >= 3 and ec[0] != 0 else None
    before = M.route_counts()
    out, off = gb.generate_sized(mode, sizes, xfs, config=config(mode, overlap, ec), stencil=st, y_orientation=M.Y_DOWNWARD if y_down else M.Y_UPWARD,
                                 scanline_pass=rule is not None, fill_rule=rule or 0)
    flat = out.cpu().numpy()
    routes = fuzzlib._delta(M.route_counts(), before)
    assert off.tolist() == M.GlyphBatch.packed_offsets(sizes, n).tolist() and flat.size == off[-1]
    tiles = [flat[off[g]:off[g+1]].reshape(int(sizes[g, 1]), int(sizes[g, 0]), n) for g in range(len(sizes))]
    stencils = None
    if st is not None:
        s = st.cpu().numpy()
        stencils = [s[g*slot:g*slot+int(sizes[g, 0])*int(sizes[g, 1])].reshape(int(sizes[g, 1]), int(sizes[g, 0])) for g in range(len(sizes))]
        rest = np.concatenate([s[g*slot+int(sizes[g, 0])*int(sizes[g, 1]):(g+1)*slot] for g in range(len(sizes))])
        assert (rest == 77).all(), "stencil bytes behind a glyph's packed box were written"
    return tiles, stencils, flat, routes


_REFERENCE = {}


def reference(oracle, mode, overlap, ec, y_down, rule=None):
    """The oracle's w_g x h_g bitmap (and stencil) of every glyph: computed once per configuration, shared by the tests, never written to."""
    key = (mode, overlap, ec, y_down, rule)
    if key not in _REFERENCE:
        shapes, sizes, xfs = glyphs()
        fields, stencils = [], []
        for s, (w, h), xf in zip(shapes, sizes, xfs):
            w, h = int(w), int(h)
            sb = np.zeros((h, w), np.uint8)
            if rule is None:
                f = oracle.generate(s, mode, w, h, xf, overlap=overlap, ec_mode=ec[0], ec_dist=ec[1], y_down=y_down, stencil=sb)
            else:                                                           # the -scanline flow: field -> sign pass -> correction
                f = oracle.generate(s, mode, w, h, xf, overlap=overlap, ec_mode=0, y_down=y_down)
                f = oracle.sign_correction(s, f, xf, .5, rule, y_down=y_down)
                if mode >= 3 and ec[0] != 0:
                    f = oracle.error_correction(s, f, xf, overlap=overlap, ec_mode=ec[0], ec_dist=ec[1], y_down=y_down, stencil=sb)
            f.setflags(write=False), sb.setflags(write=False)
            fields.append(f), stencils.append(sb)
        _REFERENCE[key] = (fields, stencils)
    return _REFERENCE[key]


class Tally:
    def __init__(self):
        self.compared = self.differing = self.st_compared = self.st_differing = 0
        self.worst, self.worst_case = 0., None

    def add(self, what, got, got_st, want, want_st):
        for g, a in enumerate(got):
            b = want[g % len(want)]                                       # (a batch of repeated(): the reference of the 43)
            assert a.shape == b.shape, (what, g)
            bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
            self.compared += a.size
            self.differing += int(bad.sum())
            if bad.any():
                d = float(np.abs(a.astype(np.float64)-b.astype(np.float64))[bad].max())
                if not d <= self.worst:
                    self.worst, self.worst_case = d, (what, "glyph %d" % g, "box %s" % (a.shape[:2][::-1],), "first at %s" % (np.argwhere(bad)[0].tolist(),))
            if got_st is not None:
                self.st_compared += got_st[g].size
                self.st_differing += int((got_st[g] != want_st[g % len(want_st)]).sum())

    def check(self):
        print({"values_compared": self.compared, "values_differing_bitwise": self.differing, "max_abs_delta": self.worst, "worst_case": self.worst_case,
               "stencil_values_compared": self.st_compared, "stencil_values_differing": self.st_differing})
        assert self.compared > 0
        assert self.worst <= TOL, self.worst_case
        assert self.differing <= self.compared*1e-6, self.worst_case
        assert self.st_differing == 0, self.worst_case


EC_PAIRS = fuzzlib.EC_PAIRS


def test_the_inputs_are_the_ones_described():
    shapes, sizes, xfs = glyphs()
    assert len(shapes) == N_GLYPHS and N_GLYPHS % 8 != 0 and (int(sizes[:, 0].max()), int(sizes[:, 1].max())) == (W, H)
    assert {tuple(b) for b in sizes.tolist()} == set(BOXES) and ((W+7)//8)*((H+7)//8) == 9
    contours = [s.n_contours for s in shapes]
    assert 1 in contours and 2 in contours and max(contours) >= 7 and any((np.asarray(s.types) == 3).all() for s in shapes)
    assert any(s.inverse_y for s in shapes) and not all(s.inverse_y for s in shapes)
    for box in BOXES:                                                       # every box size under both shape orientations
        assert {bool(shapes[g].inverse_y) for g in range(N_GLYPHS) if tuple(sizes[g]) == box} == {False, True}, box


@pytest.mark.parametrize("y_down", [False, True])
@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_box_edge_cases_vs_oracle(oracle, mode, overlap, y_down):
    """Case 1, the small route: every glyph at its own size against the oracle, stencil included; modes 3 and 4 under every (ec_mode, ec_distance_check)."""
    t = Tally()
    for ec in (EC_PAIRS if mode >= 3 else ((0, 0),)):
        got, got_st, _, routes = render(mode, overlap, ec, y_down)
        assert routes["dist_small_overlap" if overlap else "dist_small_simple"] == 1, routes
        want, want_st = reference(oracle, mode, overlap, ec, y_down)
        t.add((mode, overlap, ec, y_down), got, got_st, want, want_st)
    t.check()
    assert mode < 3 or t.st_compared > 0


ROUTE_TABLES = ("quad_classes", "short_classes", "no_lds_class", "persistent_grid", "query_counter")


@pytest.mark.parametrize("name", ROUTE_TABLES)
def test_boxes_under_forced_routes_vs_oracle(oracle, _device, name):
    """Case 2: the same boxes under the MSDFHIP_* tables of fuzzlib.TUNINGS; the route counters prove that the forced route ran (FORCED of
    tests/test_gpu_routes.py). persistent_grid: 40 workgroups walk the queue of the global-scratch class -- an item outside its glyph's box must not end its
    workgroup, or the tiles queued behind it stay unrendered. The planner makes that class persistent from one round of the device's wavefront slots
    (MSDFHIP_PERSISTENT_ROUNDS=1: compute units x 16 one-tile items); the nine glyphs of seven and more contours among the 43 reach that when the 43 are
    repeated some 50 times -- the same glyphs, so the oracle's 43 bitmaps stay the reference."""
    ran, idle, _ = FORCED[name]
    t = Tally()
    total = None
    gb = sizes = xfs = None
    if name == "persistent_grid":
        heavy = sum(s.n_contours >= 7 for s in glyphs()[0])               # msdf: 7 contours x 3 channels x 512 B exceed the 10 KB the LDS class may take
        reps = -(-_device["cus"]*16//(9*heavy))+2
        reps += (N_GLYPHS*reps) % 8 == 0
        gb, sizes, xfs = repeated(reps)
    with fuzzlib.tuned(fuzzlib.TUNINGS[name]):
        for mode in ((3, 4) if name in ("persistent_grid", "query_counter") else (1, 3, 4)):
            for overlap in ((True,) if name == "persistent_grid" else (True, False)):
                for ec in (((1, 1), (2, 2)) if mode >= 3 else ((0, 0),)):
                    y_down = mode == 4
                    got, got_st, _, routes = render(mode, overlap, ec, y_down, gb=gb, sizes=sizes, xfs=xfs)
                    total = routes if total is None else {k: total[k]+routes[k] for k in routes}
                    want, want_st = reference(oracle, mode, overlap, ec, y_down)
                    t.add((name, mode, overlap, ec), got, got_st, want, want_st)
    t.check()
    print(total)
    for alternatives in ran:
        assert sum(total[k] for k in alternatives) > 0, (name, alternatives, total)
    for k in idle:
        assert total[k] == 0, (name, k, total)


def test_boxes_through_the_chunked_sign_pass_vs_oracle(oracle):
    """Case 2, sign_chunked: scanline_pass=True over the four fill rules under MSDFHIP_SIGN_CAP=3 (row lists walked in chunks, tile rows split into spans)."""
    ran, idle, _ = FORCED["sign_chunked"]
    t = Tally()
    total = None
    with fuzzlib.tuned(fuzzlib.TUNINGS["sign_chunked"]):
        for rule in range(4):
            for mode, ec in ((1, (0, 0)), (3, (1, 0)), (4, (3, 2)), (3, (0, 0))):
                overlap, y_down = rule % 2 == 0, rule >= 2
                got, got_st, _, routes = render(mode, overlap, ec, y_down, rule=rule)
                total = routes if total is None else {k: total[k]+routes[k] for k in routes}
                want, want_st = reference(oracle, mode, overlap, ec, y_down, rule)
                t.add(("sign_chunked", rule, mode, ec), got, got_st, want, want_st)
    t.check()
    for alternatives in ran:
        assert sum(total[k] for k in alternatives) > 0, (alternatives, total)


def atlas_placement(sizes, unit):
    """Shelf placement of the boxes into an atlas of 64 texels a row (`unit` = floats or bytes per texel), a texel of gap between boxes and between shelves:
    -> (rows, row stride, per glyph the offset of the rectangle's memory-first row, per glyph whether the box is written bottom-up, i.e. with a negative stride)."""
    aw, x, y, shelf = 64, 1, 1, 0
    first = np.zeros(len(sizes), np.int64)
    for g, (w, h) in enumerate(sizes.tolist()):
        if x+w+1 > aw:
            x, y, shelf = 1, y+shelf+1, 0
        first[g] = (y*aw+x)*unit
        x, shelf = x+w+1, max(shelf, h)
    negative = np.arange(len(sizes)) % 4 == 1
    return y+shelf+1, aw*unit, first, negative


@pytest.mark.parametrize("mode", [3, 1])
def test_placement_into_a_float_atlas(mode):
    """Case 3: the boxes into one float atlas with shared rows, gaps and, for every fourth glyph, a negative row stride. Every texel outside the rectangles keeps
    its bits, every rectangle equals the packed result."""
    import torch
    _, sizes, xfs = glyphs()
    n = M.CHANNELS[mode]
    ec = (1, 1)
    packed, _, _, _ = render(mode, True, ec, False, want_stencil=False)
    rows, stride, first, negative = atlas_placement(sizes, n)
    hs = sizes[:, 1].astype(np.int64)
    offsets = np.where(negative, first+(hs-1)*stride, first)
    strides = np.where(negative, -stride, stride)
    atlas = torch.from_numpy(np.full(rows*stride, SENTINEL, np.uint32).view(np.float32)).cuda()
    gb = batch()
    desc = gb.descriptors_sized(xfs, sizes, n, out_offsets=offsets, row_strides=strides)
    out, _ = gb.generate_sized(mode, sizes, config=config(mode, True, ec), out=atlas, descriptors=desc)
    assert out is atlas
    got = atlas.cpu().numpy().view(np.uint32).reshape(rows, stride)
    untouched = np.ones((rows, stride), bool)
    for g, (w, h) in enumerate(sizes.tolist()):
        r0, c0 = divmod(int(first[g]), stride)
        rect = got[r0:r0+h, c0:c0+w*n].reshape(h, w, n)
        want = packed[g].view(np.uint32)
        assert (rect == (want[::-1] if negative[g] else want)).all(), (g, (w, h), bool(negative[g]))
        untouched[r0:r0+h, c0:c0+w*n] = False
    assert untouched.sum() > 0 and (got[untouched] == SENTINEL).all()


def test_placement_into_a_byte_atlas(oracle):
    """Case 3 through to_bytes_sized: pixelFloatToByte of the packed floats, blitted into a uint8 atlas the same way."""
    import torch
    _, sizes, _ = glyphs()
    n = 3
    packed, _, flat, _ = render(3, True, (1, 1), False, want_stencil=False)
    rows, stride, first, negative = atlas_placement(sizes, n)
    hs = sizes[:, 1].astype(np.int64)
    atlas = torch.full((rows*stride,), 0xA5, dtype=torch.uint8, device="cuda")
    batch().to_bytes_sized(torch.from_numpy(flat).cuda(), sizes, n, atlas, np.where(negative, first+(hs-1)*stride, first), np.where(negative, -stride, stride))
    got = atlas.cpu().numpy().reshape(rows, stride)
    untouched = np.ones((rows, stride), bool)
    for g, (w, h) in enumerate(sizes.tolist()):
        r0, c0 = divmod(int(first[g]), stride)
        want = oracle.pixel_float_to_byte(packed[g]).reshape(h, w, n)
        assert (got[r0:r0+h, c0:c0+w*n].reshape(h, w, n) == (want[::-1] if negative[g] else want)).all(), (g, (w, h))
        untouched[r0:r0+h, c0:c0+w*n] = False
    assert (got[untouched] == 0xA5).all()


@pytest.mark.parametrize("mode,ec,rule", [(3, (1, 1), None), (4, (2, 2), None), (3, (3, 0), 1), (1, (0, 0), 0)])
def test_equal_sizes_give_the_bytes_of_the_uniform_call(mode, ec, rule):
    """Case 4: with all sizes (16, 16) the sized call's floats and stencil are byte-identical to GlyphBatch.generate(16, 16)."""
    import torch
    shapes, _, _ = glyphs()
    sizes = np.full((N_GLYPHS, 2), 16, np.int32)
    xfs = np.stack([autoframe(s.bounds(), 16, 16, 2.) for s in shapes])
    _, stencils, flat, _ = render(mode, True, ec, True, rule=rule, sizes=sizes, xfs=xfs)
    ust = torch.full((N_GLYPHS, 16, 16), 77, dtype=torch.uint8, device="cuda") if stencils is not None else None
    uniform = batch().generate(mode, 16, 16, xfs, config=config(mode, True, ec), stencil=ust, y_orientation=M.Y_DOWNWARD, scanline_pass=rule is not None,
                               fill_rule=rule or 0).cpu().numpy()
    assert (flat.view(np.uint32) == uniform.reshape(-1).view(np.uint32)).all()
    assert (mode >= 3) == (stencils is not None)
    if stencils is not None:
        assert (np.stack(stencils) == ust.cpu().numpy()).all()


@pytest.mark.parametrize("mode,ec,y_down", [(3, (1, 1), False), (4, (2, 2), True), (2, (0, 0), True)])
def test_sized_call_equals_a_uniform_call_per_distinct_size(mode, ec, y_down):
    """Case 5: what a caller had before -- one uniform call per distinct size over that size's glyphs -- gives the sized call's bytes (device results of the
    same arithmetic: exact equality)."""
    import torch
    shapes, sizes, xfs = glyphs()
    got, got_st, _, _ = render(mode, True, ec, y_down)
    y = M.Y_DOWNWARD if y_down else M.Y_UPWARD
    whole = ShapeBatch.from_shapes(shapes)
    for w, h in BOXES:
        pick = [g for g in range(N_GLYPHS) if tuple(sizes[g]) == (w, h)]
        gb = M.GlyphBatch(whole.select(pick))
        st = torch.full((len(pick), h, w), 77, dtype=torch.uint8, device="cuda") if got_st is not None else None
        tiles = gb.generate(mode, w, h, xfs[pick], config=config(mode, True, ec), stencil=st, y_orientation=y).cpu().numpy()
        for k, g in enumerate(pick):
            assert (tiles[k].view(np.uint32) == got[g].view(np.uint32)).all(), (g, (w, h))
            if st is not None:
                assert (st[k].cpu().numpy() == got_st[g]).all(), (g, (w, h))
        gb.close()


def test_bad_sizes_are_refused_with_a_batch():
    """The refusals of msdfhip_batch_generate_sized that need a batch (tests/test_sized_plan_host.py has the others): nothing is written."""
    import torch
    lib, gb = L.load(), batch()
    _, sizes, xfs = glyphs()
    cfg = L.default_config()
    desc = gb.descriptors_sized(xfs, sizes, 3)
    out = torch.zeros(int(M.GlyphBatch.packed_offsets(sizes, 3)[-1]), dtype=torch.float32, device="cuda")
    i32 = C.POINTER(C.c_int32)

    def call(a):
        return lib.msdfhip_batch_generate_sized(gb._handle, 3, None if a is None else a.ctypes.data_as(i32), desc.data_ptr(), out.data_ptr(), None, None, C.byref(cfg), None)
    assert call(None) == L.ERR_INVALID and b"sizes is NULL" in lib.msdfhip_last_error()
    for box in ((0, 3), (3, 0), (-2, 3)):
        bad = sizes.copy()
        bad[17] = box
        assert call(bad) == L.ERR_INVALID and b"glyph 17" in lib.msdfhip_last_error(), box
    with pytest.raises(ValueError):
        gb.generate_sized(3, np.zeros((N_GLYPHS, 2), np.int32), xfs)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()
