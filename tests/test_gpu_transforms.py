"""Every generator route under the framings of tests/xformcases.py -- mirrored, anisotropic, zoomed, off-tile, inverted / huge / tiny / asymmetric
ranges, all-ones scale significands, far-off coordinates, bitmaps of 1..7 and 8k+1 texels -- against the oracle, bit for bit. tests/test_xform_cases.py
shows on the CPU that the oracle equals the compiled reference on the same families, so any difference here is a kernel's.

The families reach code the autoframed sweeps do not: the per-tile cull of k_distance with negative and anisotropic scales and tiles deep inside or
outside the glyph, the texel path without divExact (fastXf false), ecDerive with a negative mapScale and ranges far wider or narrower than a texel,
and partial 8x8 tiles in the distance, single-call and correction kernels."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import msdfgen_amd as M
import xformcases as X
from conftest import assert_bit_equal
from msdfgen_amd.shape import ShapeBatch

pytestmark = pytest.mark.gpu

W, H = 41, 27                                                   # 8k+1 wide, ragged high: partial tiles on two sides
FIXED = tuple(f for f in X.FAMILIES if f != "tiny_bitmaps")
EC_PAIRS = [(m, d) for m in range(4) for d in range(3)]
FN = {1: M.generate_sdf, 2: M.generate_psdf, 3: M.generate_msdf, 4: M.generate_mtsdf}


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)
    assert M.device_info()["arch"].startswith("gfx950")


@pytest.fixture(scope="module")
def pool():
    p = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4))
    yield p
    p.shutdown()


@pytest.fixture(scope="module")
def mixed(oracle):
    """Every family but tiny_bitmaps in one W x H batch: the glyphs of one launch have different transforms."""
    cs = X.cases(FIXED, seeds=(0, 1), w=W, h=H)
    for c in cs:
        X.check_premise(c, oracle)
    return cs, ShapeBatch.from_shapes([c.shape for c in cs]), np.stack([c.xf for c in cs])


def tiny_groups(oracle):
    """tiny_bitmaps by size: a batch has one (w, h)."""
    groups = {}
    for c in X.cases(("tiny_bitmaps",), seeds=(0, 1, 2)):
        X.check_premise(c, oracle)
        groups.setdefault((c.w, c.h), []).append(c)
    return groups


def _cfg(mode, ov, ec=2, dc=1, buffer=None):
    return M.MSDFGeneratorConfig(ov, M.ErrorCorrectionConfig(ec, dc, buffer=buffer)) if mode >= 3 else M.GeneratorConfig(ov)


def _batched(oracle, pool, cs, batch, xfs, w, h, mode, ov, ec, dc, y_down):
    import torch
    gb = M.GlyphBatch(batch)
    st = torch.zeros((len(cs), h, w), dtype=torch.uint8, device="cuda")
    yo = M.Y_DOWNWARD if y_down else M.Y_UPWARD
    got = gb.generate(mode, w, h, xfs, config=_cfg(mode, ov, ec, dc), stencil=st if mode >= 3 else None, y_orientation=yo).cpu().numpy()
    gst = st.cpu().numpy()
    gb.close()

    def want(g):
        sb = np.zeros((h, w), np.uint8)
        return oracle.generate(cs[g].shape, mode, w, h, xfs[g], overlap=ov, ec_mode=ec, ec_dist=dc, y_down=y_down, stencil=sb), sb
    for g, (a, sb) in enumerate(pool.map(want, range(len(cs)))):
        what = "%s mode %d overlap %d ec %d/%d y_down %d" % (cs[g].name, mode, ov, ec, dc, y_down)
        assert_bit_equal(got[g], a, what)
        if mode >= 3:
            assert (gst[g] == sb).all(), what+": stencil"


def test_batched_transform_families_all_modes_and_correction(oracle, pool, mixed):
    """GlyphBatch.generate on the mixed batch: sdf / psdf, both combiners; msdf / mtsdf with every EC mode x distance check and the stencil (Y up),
    and a few of them Y down."""
    cs, batch, xfs = mixed
    for ov in (True, False):
        for mode in (1, 2):
            for y_down in (False, True):
                _batched(oracle, pool, cs, batch, xfs, W, H, mode, ov, 0, 0, y_down)
        for mode in (3, 4):
            for ec, dc in EC_PAIRS:
                _batched(oracle, pool, cs, batch, xfs, W, H, mode, ov, ec, dc, False)
            for ec, dc in ((2, 1), (3, 2), (1, 0)):
                _batched(oracle, pool, cs, batch, xfs, W, H, mode, ov, ec, dc, True)


def test_batched_transform_tiny_bitmaps(oracle, pool):
    """Bitmaps of 1..7 and 8k+1 texels: partial 8x8 tiles in k_distance and the correction's 3x3 stencil at both borders at once."""
    for (w, h), cs in tiny_groups(oracle).items():
        batch, xfs = ShapeBatch.from_shapes([c.shape for c in cs]), np.stack([c.xf for c in cs])
        for k, mode in enumerate((1, 2, 3, 4)):
            for ov in (True, False):
                ec, dc = EC_PAIRS[(3*k+5*ov+w+h) % len(EC_PAIRS)] if mode >= 3 else (0, 0)
                _batched(oracle, pool, cs, batch, xfs, w, h, mode, ov, ec, dc, bool((k+ov) & 1))


def test_single_calls_under_transform_families(oracle, mixed):
    """generate_sdf / psdf / msdf / mtsdf, one fused launch per call (msdf_single.hpp), Y_UPWARD and Y_DOWNWARD, with the stencil buffer."""
    cs, _, _ = mixed
    cs = cs+[c for group in tiny_groups(oracle).values() for c in group[:1]]
    for i, c in enumerate(cs):
        for mode in (1, 2, 3, 4):
            for y_down in (False, True):
                ov = bool((i+mode) & 1)
                ec, dc = EC_PAIRS[(i+3*mode+y_down) % len(EC_PAIRS)]
                sa, sb = np.zeros((c.h, c.w), np.uint8), np.zeros((c.h, c.w), np.uint8)
                got = FN[mode](np.zeros((c.h, c.w, M.CHANNELS[mode]), np.float32), c.shape, M.SDFTransformation.from_xf(c.xf), _cfg(mode, ov, ec, dc, sa),
                               M.Y_DOWNWARD if y_down else M.Y_UPWARD)
                want = oracle.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, ec_mode=ec if mode >= 3 else 0, ec_dist=dc, y_down=y_down, stencil=sb)
                what = "%s single mode %d overlap %d ec %d/%d y_down %d" % (c.name, mode, ov, ec, dc, y_down)
                assert_bit_equal(got, want, what)
                if mode >= 3:
                    assert (sa == sb).all(), what+": stencil"


def test_host_pipeline_and_stream_under_transform_families(oracle, pool, mixed):
    """HostBatch.generate_host and generate_stream (CSR) into a float atlas with a gutter and an 8-bit atlas: tiles equal the oracle's, the gutter stays
    untouched, the bytes are pixelFloatToByte of the float tiles. Correction with ALWAYS_CHECK_DISTANCE and without overlap support, so that the
    candidate queues fill up."""
    cs, batch, xfs = mixed
    lib = M.load()
    n = len(cs)
    cols, cw, ch = 8, W+3, H+2
    rows = (n+cols-1)//cols
    offs = np.array([(((g//cols)*ch+1)*cols*cw+(g % cols)*cw+2)*3 for g in range(n)], np.int64)
    offs8 = np.array([((g//cols)*H*cols*W+(g % cols)*W)*3 for g in range(n)], np.int64)
    for ov, ec, dc in ((True, 2, 1), (False, 2, 2), (False, 3, 2)):
        c = _cfg(3, ov, ec, dc)
        want = np.stack(list(pool.map(lambda g: oracle.generate(cs[g].shape, 3, W, H, xfs[g], overlap=ov, ec_mode=ec, ec_dist=dc), range(n))))
        want8 = np.zeros((rows*H, cols*W, 3), np.uint8)
        for g in range(n):
            want8[(g//cols)*H:(g//cols+1)*H, (g % cols)*W:(g % cols+1)*W] = oracle.pixel_float_to_byte(want[g])
        lib.msdfhip_pipeline_overflow_reruns(1)
        hb = M.HostBatch(batch)
        try:
            outs = {}
            atlas = np.full((rows*ch, cols*cw, 3), -5, np.float32)
            outs["generate_host"] = hb.generate_host(3, W, H, xfs, out=atlas, out_offsets=offs, row_stride=cols*cw*3, config=c)
            outs["generate_stream"] = M.generate_stream(batch, 3, W, H, xfs, out=np.full_like(atlas, -5), out_offsets=offs, row_stride=cols*cw*3, config=c)
            for route, a in outs.items():
                for g in range(n):
                    y, x = (g//cols)*ch+1, (g % cols)*cw+2
                    assert_bit_equal(a[y:y+H, x:x+W], want[g], "%s %s overlap %d ec %d/%d" % (route, cs[g].name, ov, ec, dc))
                    a[y:y+H, x:x+W] = -5
                assert (a == -5).all(), route+": texels outside the tiles were written"
            b8 = np.zeros_like(want8)
            hb.generate_bytes_host(3, W, H, xfs, b8, offs8, cols*W*3, config=c)
            assert (b8 == want8).all(), "generate_bytes_host: %d bytes differ" % int((b8 != want8).sum())
            s8 = np.full_like(want8, 77)
            M.generate_stream(batch, 3, W, H, xfs, atlas=s8, out_offsets=offs8, row_stride=cols*W*3, config=c)
            full = n % cols == 0
            assert (s8[:(rows if full else rows-1)*H] == want8[:(rows if full else rows-1)*H]).all(), "generate_stream 8-bit"
            last = s8[(rows-1)*H:]
            k = n-(rows-1)*cols
            assert (last[:, :k*W] == want8[(rows-1)*H:, :k*W]).all() and (last[:, k*W:] == 77).all(), "generate_stream 8-bit, last row of tiles"
        finally:
            hb.close()
        print("overlap %d ec %d/%d: overflow reruns %d" % (ov, ec, dc, lib.msdfhip_pipeline_overflow_reruns(1)))
    # huge_range alone: a range wider than the tile makes every texel a candidate of the distance check, and the correction overflows its candidate
    # segments -- measured on the MI355X: the call takes the overflow rerun (1 rerun; the mixed batch above: 4 with ec 2/2, none with 2/1 or 3/2).
    hr = [g for g, cc in enumerate(cs) if cc.name.startswith("huge_range")]
    sub = batch.select(hr)
    lib.msdfhip_pipeline_overflow_reruns(1)
    got = M.generate_stream(sub, 3, W, H, xfs[hr], config=_cfg(3, False, 2, 2))
    reruns = lib.msdfhip_pipeline_overflow_reruns(1)
    print("huge_range alone: overflow reruns %d" % reruns)
    assert reruns >= 1, "the huge_range glyphs were meant to reach the overflow rerun"

    for k, g in enumerate(hr):
        assert_bit_equal(got[k], oracle.generate(cs[g].shape, 3, W, H, xfs[g], overlap=False, ec_mode=2, ec_dist=2), "stream, "+cs[g].name)


# The one exemption from bit equality: a scanline crossing of a cubic, solved with the kernels' own < 1 ulp cos / cbrt where the oracle
# uses libm's, moves in its last ulp and with it the last ulp of a glyph's error estimate. Only the cases named here, and only where the product's
# device code compiled for the host with the kernels' transcendentals (Emu(lean=True)) gives the GPU's bits exactly.
LAST_ULP = {"zoom_in/0.1"}
_LEAN = []


def _lean():
    if not _LEAN:
        from emu import Emu
        _LEAN.append(Emu(lean=True))
    return _LEAN[0]


def _standalone_cases(oracle, mixed):
    cs, _, _ = mixed
    keep = ("mirror", "aniso", "zoom", "nondivsafe", "far_coords", "neg_range")
    return [c for c in cs if c.name.startswith(keep)]+[group[0] for group in tiny_groups(oracle).values()]


def test_standalone_passes_under_transform_families(oracle, mixed):
    """msdf_error_correction on an uncorrected field, distance_sign_correction and rasterize with every fill rule."""
    for i, c in enumerate(_standalone_cases(oracle, mixed)):
        yo = M.Y_DOWNWARD if c.y_down else M.Y_UPWARD
        xf = M.SDFTransformation.from_xf(c.xf)
        for mode in (3, 4):
            pre = oracle.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
            ov = bool(i & 1)
            for ec, dc in ((2, 1), (1, 2), (3, 0)):
                sa, sb = np.zeros((c.h, c.w), np.uint8), np.zeros((c.h, c.w), np.uint8)
                got = M.msdf_error_correction(pre.copy(), c.shape, xf, _cfg(mode, ov, ec, dc, sa), yo)
                want = oracle.error_correction(c.shape, pre, c.xf, overlap=ov, ec_mode=ec, ec_dist=dc, y_down=c.y_down, stencil=sb)
                what = "%s error_correction mode %d overlap %d ec %d/%d" % (c.name, mode, ov, ec, dc)
                assert_bit_equal(got, want, what)
                assert (sa == sb).all(), what+": stencil"
        for mode in (1, 3):
            field = oracle.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
            for rule in range(4):
                want = oracle.sign_correction(c.shape, field, c.xf, .5, rule, y_down=c.y_down)
                got = M.distance_sign_correction(field.copy(), c.shape, xf, .5, rule, yo)
                assert_bit_equal(got, want, "%s sign correction mode %d rule %d" % (c.name, mode, rule))
        for rule in range(4):
            got = M.rasterize(np.full((c.h, c.w, 1), -3, np.float32), c.shape, xf, rule, yo)
            assert_bit_equal(got, oracle.rasterize(c.shape, c.w, c.h, c.xf, rule, y_down=c.y_down), "%s rasterize rule %d" % (c.name, rule))


def test_scanline_pass_and_error_estimate_under_transform_families(oracle, pool, mixed):
    """The -scanline flow inside GlyphBatch.generate (scanline_pass=True), and GlyphBatch.estimate_sdf_error, on the mirror / aniso / zoom cases and on
    tiny bitmaps."""
    cs = [c for c in _standalone_cases(oracle, mixed) if (c.w, c.h) == (W, H)]
    groups = [(W, H, cs)]+[(w, h, g) for (w, h), g in tiny_groups(oracle).items()]
    for w, h, group in groups:
        batch, xfs = ShapeBatch.from_shapes([c.shape for c in group]), np.stack([c.xf for c in group])
        gb = M.GlyphBatch(batch)
        for mode, rule in ((3, M.FILL_NONZERO), (4, M.FILL_ODD), (1, M.FILL_POSITIVE)):
            c = _cfg(mode, False, 2, 0)
            got = gb.generate(mode, w, h, xfs, config=c, scanline_pass=True, fill_rule=rule).cpu().numpy()

            def want(g):
                s = group[g].shape
                f = oracle.generate(s, mode, w, h, xfs[g], overlap=False, ec_mode=0)
                f = oracle.sign_correction(s, f, xfs[g], .5, rule)
                return oracle.error_correction(s, f, xfs[g], overlap=False, ec_mode=2, ec_dist=0) if mode >= 3 else f
            for g, a in enumerate(pool.map(want, range(len(group)))):
                assert_bit_equal(got[g], a, "%s scanline flow mode %d rule %d" % (group[g].name, mode, rule))
        for mode in (3, 1):
            tiles = gb.generate(mode, w, h, xfs)
            src = tiles.cpu().numpy()
            for spr, rule in ((1, 0), (3, 1)):
                got = gb.estimate_sdf_error(tiles, xfs, spr, rule).cpu().numpy()
                want = np.array([oracle.estimate_sdf_error(group[g].shape, src[g], xfs[g], spr, rule) for g in range(len(group))])
                for g in np.flatnonzero(got.view(np.uint64) != want.view(np.uint64)):
                    what = "estimate_sdf_error %s mode %d spr %d rule %d: %r, oracle %r" % (group[g].name, mode, spr, rule, got[g], want[g])
                    assert group[g].name in LAST_ULP, what
                    lean = _lean().estimate_sdf_error(group[g].shape, src[g], xfs[g], spr, rule)
                    assert np.float64(lean).view(np.uint64) == got[g].view(np.uint64), what+", lean host build %r" % lean
        gb.close()


def test_render_sdf_tiny_and_inverted_range(oracle):
    """renderSDF into 1x1 outputs, from 1-texel-wide fields, and with an inverted sdf_px_range."""
    groups = tiny_groups(oracle)
    for (w, h) in ((1, 9), (1, 64), (9, 1), (1, 1), (17, 9)):
        cs = groups[(w, h)]
        gb = M.GlyphBatch(ShapeBatch.from_shapes([c.shape for c in cs]))
        for mode, n_outs in ((1, (1, 3)), (3, (1, 3)), (4, (1, 4))):
            tiles = gb.generate(mode, w, h, np.stack([c.xf for c in cs]))
            src = tiles.cpu().numpy()
            for n_out in n_outs:
                for ow, oh in ((1, 1), (1, 7), (5, 1), (13, 11)):
                    for lo, hi, thr in ((0, 0, .5), (-2, 2, .5), (2, -2, .5), (1.5, -.5, .4)):
                        got = M.render_sdf(tiles, ow, oh, n_out, (lo, hi), thr).cpu().numpy()
                        for g in range(len(cs)):
                            assert_bit_equal(got[g], oracle.render_sdf(src[g], ow, oh, n_out, lo, hi, thr),
                                             "renderSDF %d<-%d %dx%d from %dx%d range (%g, %g)" % (n_out, src.shape[3], ow, oh, w, h, lo, hi))
        gb.close()
