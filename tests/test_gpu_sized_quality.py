"""GlyphBatch.estimate_sdf_error_sized and render_sdf_sized: estimateSDFError and renderSDF for glyph boxes of different sizes in ONE call each
(msdfhip_batch_estimate_sdf_error_sized, msdfhip_render_sdf_sized), on the 43 glyphs, boxes and transforms of tests/test_gpu_sized.py: against the oracle per
glyph at that glyph's own size, against the uniform calls (all sizes equal; one uniform call per distinct size), across launch chunks, and under other
placements of the tiles and the results. Every comparison is bitwise."""
import ctypes as C
import functools

import numpy as np
import pytest

import msdfgen_amd as M
import fuzzlib
import sizedqualitycases as Q
from conftest import assert_bit_equal
from msdfgen_amd import lib as L
from msdfgen_amd.shape import ShapeBatch, autoframe
from test_gpu_sized import BOXES, N_GLYPHS, batch, config, glyphs

pytestmark = pytest.mark.gpu
SPR_RULE = ((1, 0), (3, 1), (2, 2))
SENTINEL = 0x7fc0dead                  # a NaN payload no kernel writes
ERR_SENTINEL = -12345.678


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)
    info = M.device_info()
    assert info["arch"].startswith("gfx950"), info
    return info


@functools.lru_cache(maxsize=None)
def tiles_of(mode):
    """generate_sized of the 43 glyphs in `mode` -> (flat device tensor, packed offsets, per-glyph host arrays (h_g, w_g, N))."""
    _, sizes, xfs = glyphs()
    out, off = batch().generate_sized(mode, sizes, xfs, config=config(mode, True, (1, 1)))
    flat = out.cpu().numpy()
    return out, off, [flat[off[g]:off[g+1]].reshape(int(sizes[g, 1]), int(sizes[g, 0]), M.CHANNELS[mode]) for g in range(N_GLYPHS)]


def same_doubles(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, "%s: %s" % (what, [(int(g), float(got[g]), float(want[g])) for g in bad[:8]])


@pytest.mark.parametrize("spr,rule", SPR_RULE)
@pytest.mark.parametrize("mode", [1, 3, 4])
def test_estimate_vs_oracle(oracle, mode, spr, rule):
    """Every glyph at its own size, inverse-Y shapes (every third) included: the oracle's estimateSDFError of the downloaded tile, with no exemption.

    With the math library's acos in the cubic solver (OCML's on the device, < 1 ulp) the (2, 2) cases differed from the oracle by one unit in the last place on
    two glyphs of 43 per mode, in the uniform call exactly as in the sized one: of the 129 arguments these scanlines hand to acos for glyphs 7, 10 and 32, OCML
    and glibc differ on 6, by one ulp, glibc's being the correctly rounded value on every one of them. The estimate's scanlines therefore take acosRounded
    (msdf_device.hpp: acos rounded to nearest, the same operations on the device and in tests/hostemu); glibc's own value is the rounded one but for some
    0.06 % of arguments, so a last-place difference on other inputs is not excluded, only a hundred times rarer than before."""
    shapes, sizes, xfs = glyphs()
    dev, _, host = tiles_of(mode)
    got = batch().estimate_sdf_error_sized(dev, sizes, xfs, spr, rule).cpu().numpy()
    want = np.array([oracle.estimate_sdf_error(shapes[g], host[g], xfs[g], spr, rule) for g in range(N_GLYPHS)])
    print(mode, spr, rule, "differing", int((got.view(np.uint64) != want.view(np.uint64)).sum()), "max |d|", float(np.abs(got-want).max()))
    for g in np.flatnonzero(got.view(np.uint64) != want.view(np.uint64)):
        print("   glyph %d box %s: device %r oracle %r" % (g, tuple(int(v) for v in sizes[g]), float(got[g]), float(want[g])))
    for g in range(N_GLYPHS):
        if tuple(sizes[g]) in ((1, 1), (24, 1), (1, 17)):
            assert got[g].tobytes() == np.float64(0.).tobytes(), (g, got[g])
    assert (got != 0).any()
    same_doubles(got, want, "mode %d spr %d rule %d" % (mode, spr, rule))


def test_estimate_without_scanlines_is_zero():
    """scanlines_per_row < 1: every error is 0 (sdf-error-estimation.cpp:136)."""
    _, sizes, xfs = glyphs()
    dev, _, _ = tiles_of(3)
    for spr in (0, -2):
        assert not batch().estimate_sdf_error_sized(dev, sizes, xfs, spr, 0).cpu().numpy().any()


@pytest.mark.parametrize("mode", [3, 1])
def test_estimate_equals_a_uniform_call_per_distinct_size(mode):
    import torch
    shapes, sizes, xfs = glyphs()
    dev, off, _ = tiles_of(mode)
    n = M.CHANNELS[mode]
    whole = ShapeBatch.from_shapes(shapes)
    for spr, rule in SPR_RULE:
        got = batch().estimate_sdf_error_sized(dev, sizes, xfs, spr, rule).cpu().numpy()
        for w, h in BOXES:
            pick = [g for g in range(N_GLYPHS) if tuple(sizes[g]) == (w, h)]
            gb = M.GlyphBatch(whole.select(pick))
            sub = torch.cat([dev[int(off[g]):int(off[g+1])] for g in pick]).reshape(len(pick), h, w, n).contiguous()
            uniform = gb.estimate_sdf_error(sub, xfs[pick], spr, rule).cpu().numpy()
            same_doubles(got[pick], uniform, "box %dx%d spr %d rule %d" % (w, h, spr, rule))
            gb.close()


@functools.lru_cache(maxsize=None)
def square_tiles(mode):
    shapes, _, _ = glyphs()
    xfs = np.stack([autoframe(s.bounds(), 16, 16, 2.) for s in shapes])
    return batch().generate(mode, 16, 16, xfs, config=config(mode, True, (1, 1))), xfs


@pytest.mark.parametrize("mode", [3, 4, 1])
def test_estimate_with_equal_sizes_equals_the_uniform_call(mode):
    tiles, xfs = square_tiles(mode)
    sizes = np.full((N_GLYPHS, 2), 16, np.int32)
    for spr, rule in SPR_RULE:
        uniform = batch().estimate_sdf_error(tiles, xfs, spr, rule).cpu().numpy()
        got = batch().estimate_sdf_error_sized(tiles.reshape(-1), sizes, xfs, spr, rule).cpu().numpy()
        same_doubles(got, uniform, "mode %d spr %d rule %d" % (mode, spr, rule))
        assert (uniform != 0).any()


def max_edges(gb):
    v = [C.c_int() for _ in range(5)]
    L.check(L.load().msdfhip_batch_info(gb._handle, *[C.byref(x) for x in v]))
    return v[4].value


def test_estimate_across_chunks():
    """MSDFHIP_ERROR_WORKSPACE_MB so small that the 984 scanlines of the batch at 3 per row take at least three launches (the plan restated from its documented
    formula: sizedqualitycases), a last short one included: the bits of the default cap. The uniform call on a 16 x 16 batch under the same cap likewise."""
    _, sizes, xfs = glyphs()
    dev, _, _ = tiles_of(3)
    spr, rule = 3, 1
    items = Q.item_prefix(sizes, spr)[-1]
    assert items == 3*(3*86+70)
    per_lane = Q.lane_bytes(max_edges(batch()), int(sizes[:, 0].max()))
    mb = repr(130*per_lane/float(1 << 20))
    cap = int(float(mb)*(1 << 20))
    lanes = Q.chunk_lanes(items, per_lane, cap)
    assert lanes == 128 and -(-items//lanes) >= 3 and items % lanes != 0, (lanes, items)
    assert Q.chunk_lanes(items, per_lane, 512 << 20) >= items           # the default cap: one launch
    want = batch().estimate_sdf_error_sized(dev, sizes, xfs, spr, rule).cpu().numpy()
    sq, sq_xfs = square_tiles(3)
    sq_items = N_GLYPHS*15*spr
    sq_lane = Q.lane_bytes(max_edges(batch()), 16)
    sq_mb = repr(130*sq_lane/float(1 << 20))
    assert -(-sq_items//Q.chunk_lanes(sq_items, sq_lane, int(float(sq_mb)*(1 << 20)))) >= 3
    sq_want = batch().estimate_sdf_error(sq, sq_xfs, spr, rule).cpu().numpy()
    with fuzzlib.tuned({"MSDFHIP_ERROR_WORKSPACE_MB": mb}):              # (restores the knob and reloads in its finally)
        got = batch().estimate_sdf_error_sized(dev, sizes, xfs, spr, rule).cpu().numpy()
    with fuzzlib.tuned({"MSDFHIP_ERROR_WORKSPACE_MB": sq_mb}):
        sq_got = batch().estimate_sdf_error(sq, sq_xfs, spr, rule).cpu().numpy()
        sq_sized = batch().estimate_sdf_error_sized(sq.reshape(-1), np.full((N_GLYPHS, 2), 16, np.int32), sq_xfs, spr, rule).cpu().numpy()
    same_doubles(got, want, "sized, chunked")
    same_doubles(sq_got, sq_want, "uniform, chunked")
    same_doubles(sq_sized, sq_want, "sized 16 x 16, chunked")
    assert (want != 0).any() and (sq_want != 0).any()


def test_estimate_with_other_placements():
    """Custom tile_offsets: the tiles reversed in memory, gaps of NaN sentinels between them; and d_errors between sentinels (through the C entry point)."""
    import torch
    _, sizes, xfs = glyphs()
    dev, off, _ = tiles_of(3)
    want = batch().estimate_sdf_error_sized(dev, sizes, xfs, 2, 0).cpu().numpy()
    flat = dev.cpu().numpy()
    gap = 5
    total = int(off[-1])+gap*(N_GLYPHS+1)
    moved = np.full(total, SENTINEL, np.uint32).view(np.float32)
    toff = np.zeros(N_GLYPHS, np.int64)
    at = gap
    for g in reversed(range(N_GLYPHS)):
        n = int(off[g+1]-off[g])
        moved[at:at+n] = flat[off[g]:off[g+1]]
        toff[g] = at
        at += n+gap
    assert at == total
    got = batch().estimate_sdf_error_sized(torch.from_numpy(moved).cuda(), sizes, xfs, 2, 0, tile_offsets=toff, channels=3).cpu().numpy()
    same_doubles(got, want, "reversed tiles")
    with pytest.raises(ValueError):
        batch().estimate_sdf_error_sized(dev, sizes, xfs, 2, 0, tile_offsets=toff+int(off[-1]), channels=3)
    # d_errors inside a larger array
    pad = 8
    errors = torch.full((N_GLYPHS+2*pad,), ERR_SENTINEL, dtype=torch.float64, device="cuda")
    d = np.zeros(N_GLYPHS, L.GLYPH_DTYPE)
    d["xf"][:, :4] = xfs[:, :4]
    d["flip"] = batch().shapes.inverse_y.astype(bool).astype(np.int32)
    desc = torch.from_numpy(d.view(np.uint8).reshape(N_GLYPHS, 64)).cuda()
    packed = np.ascontiguousarray(off[:-1], np.int64)
    for spr in (2, 0):                                                  # (0: the zeroing path)
        errors.fill_(ERR_SENTINEL)
        L.check(L.load().msdfhip_batch_estimate_sdf_error_sized(batch()._handle, 3, L.ptr(np.ascontiguousarray(sizes, np.int32), L._ip), packed.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                desc.data_ptr(), dev.data_ptr(), spr, 0, errors.data_ptr()+8*pad, None))
        torch.cuda.synchronize()
        e = errors.cpu().numpy()
        assert (e[:pad] == ERR_SENTINEL).all() and (e[pad+N_GLYPHS:] == ERR_SENTINEL).all()
        same_doubles(e[pad:pad+N_GLYPHS], want if spr else np.zeros(N_GLYPHS), "errors between sentinels, spr %d" % spr)
    # bad arguments with a batch
    assert L.load().msdfhip_batch_estimate_sdf_error_sized(batch()._handle, 2, L.ptr(np.ascontiguousarray(sizes, np.int32), L._ip), packed.ctypes.data_as(C.POINTER(C.c_int64)),
                                                           desc.data_ptr(), dev.data_ptr(), 1, 0, errors.data_ptr(), None) == L.ERR_INVALID
    assert L.load().msdfhip_batch_estimate_sdf_error_sized(batch()._handle, 3, L.ptr(np.ascontiguousarray(sizes, np.int32), L._ip), packed.ctypes.data_as(C.POINTER(C.c_int64)),
                                                           desc.data_ptr(), dev.data_ptr(), 1, 4, errors.data_ptr(), None) == L.ERR_INVALID


@pytest.mark.parametrize("n_out,n_sdf", Q.PAIRS)
def test_render_vs_oracle(oracle, n_out, n_sdf):
    """Every glyph's output against oracle.render_sdf of its field: the channel pairs, output sizes, ranges and thresholds of the host test, one glyph in
    three with a 0 x 0 output; nothing outside the boxes' ranges of `out` is written."""
    import torch
    _, sizes, _ = glyphs()
    dev, _, host = tiles_of(Q.MODE_OF_CHANNELS[n_sdf])
    tail = 64
    compared = 0
    for k in range(Q.N_OUT_SIZES):
        out_sizes = np.array([Q.out_sizes(int(w), int(h))[k] for w, h in sizes], np.int32)
        out_sizes[1::3] = 0
        want = {}
        for lo, hi in Q.RANGES:
            for thr in Q.THRESHOLDS:
                floats = int(M.GlyphBatch.packed_offsets(out_sizes, n_out)[-1])
                out = torch.from_numpy(np.full(floats+tail, SENTINEL, np.uint32).view(np.float32)).cuda()
                got, off = M.render_sdf_sized(dev, sizes, n_sdf, out_sizes, n_out, (lo, hi), thr, out=out)
                assert got is out and off[-1] == floats
                flat = out.cpu().numpy()
                assert (flat[floats:].view(np.uint32) == SENTINEL).all()
                for g in range(N_GLYPHS):
                    ow, oh = (int(v) for v in out_sizes[g])
                    if g % 3 == 1:
                        assert off[g] == off[g+1]
                        continue
                    assert_bit_equal(flat[off[g]:off[g+1]].reshape(oh, ow, n_out), oracle.render_sdf(host[g], ow, oh, n_out, lo, hi, thr),
                                     "glyph %d -> %dx%d range (%g, %g) threshold %g" % (g, ow, oh, lo, hi, thr))
                    compared += ow*oh*n_out
    assert compared > 0


@pytest.mark.parametrize("n_out,n_sdf", [(1, 3), (4, 4), (3, 1)])
def test_render_with_equal_sizes_equals_the_uniform_call(n_out, n_sdf):
    tiles, _ = square_tiles(Q.MODE_OF_CHANNELS[n_sdf])
    sizes = np.full((N_GLYPHS, 2), 16, np.int32)
    for ow, oh in ((32, 32), (23, 9)):
        for (lo, hi), thr in (((-1., 1.), .5), ((0., 0.), .4)):
            uniform = M.render_sdf(tiles, ow, oh, n_out, (lo, hi), thr).cpu().numpy()
            got, _ = M.render_sdf_sized(tiles.reshape(-1), sizes, n_sdf, np.tile(np.array([[ow, oh]], np.int32), (N_GLYPHS, 1)), n_out, (lo, hi), thr)
            assert_bit_equal(got.cpu().numpy().reshape(uniform.shape), uniform, "%dx%d range (%g, %g)" % (ow, oh, lo, hi))


def test_render_by_a_factor_equals_explicit_sizes():
    _, sizes, _ = glyphs()
    dev, _, _ = tiles_of(3)
    a, a_off = M.render_sdf_sized(dev, sizes, 3, 2, 1, 2.)
    b, b_off = M.render_sdf_sized(dev, sizes, 3, 2*sizes, 1, (-1., 1.))
    assert a_off.tolist() == b_off.tolist() == M.GlyphBatch.packed_offsets(2*sizes, 1).tolist()
    assert_bit_equal(a.cpu().numpy(), b.cpu().numpy(), "factor 2")
    none, off = M.render_sdf_sized(dev, sizes, 3, 0, 1, 2.)              # factor 0: no output at all
    assert none.numel() == 0 and off[-1] == 0
    with pytest.raises(ValueError):
        M.render_sdf_sized(dev, sizes, 3, -1, 1, 2.)
    with pytest.raises(M.MsdfHipError):
        M.render_sdf_sized(dev, sizes, 3, 2, 4, 2.)                     # no 4 <- 3 overload


def test_flow_boxes_generate_simulate_estimate(oracle):
    """boxes() -> generate_sized -> simulate_8bit on a clone -> estimate_sdf_error_sized: it runs, the errors are finite and >= 0 and equal the oracle's on the
    same simulated tiles."""
    import torch
    shapes, _, _ = glyphs()
    gb = batch()
    b = gb.bounds()
    scale = 20./float(np.maximum(b[:, 2]-b[:, 0], b[:, 3]-b[:, 1]).max())
    sizes, xf, _ = gb.boxes(M.BoxConfig(scale, px_range=2.))
    sizes = np.maximum(sizes, 1)
    off = M.GlyphBatch.packed_offsets(sizes, 3)
    out = torch.empty(int(off[-1]), dtype=torch.float32, device="cuda")
    tiles, _ = gb.generate_sized(3, sizes, out=out, descriptors=gb.descriptors_sized(None, sizes, 3, raw_xf=xf))
    atlas = M.simulate_8bit(tiles.clone())
    got = gb.estimate_sdf_error_sized(atlas, sizes, raw_xf=xf).cpu().numpy()
    assert np.isfinite(got).all() and (got >= 0).all()
    flat = atlas.cpu().numpy()
    want = np.array([oracle.estimate_sdf_error(shapes[g], flat[off[g]:off[g+1]].reshape(int(sizes[g, 1]), int(sizes[g, 0]), 3), xf[g], 1, 0) for g in range(N_GLYPHS)])
    same_doubles(got, want, "8-bit atlas")
