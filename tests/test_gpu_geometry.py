"""Every generator route on the outline families of tests/geomcases.py -- texel centres tied between edges that are not neighbours, texel centres on the
outline, coincident contours, degenerate edges, channels without an edge, scanlines through vertices, slivers -- against the oracle, bit for bit, NaN
and infinity bit patterns included. tests/test_geom_cases.py shows on the CPU what the oracle equals on the same cases (the reference with uncached
distance queries), so any difference here is a kernel's.

The families reach what random-coordinate blobs do not: the tie-breaks that stand in for visit order (sdReplaces, the survivor compaction of the LDS
class, the cross-wavefront merge of the single call's team, EdgesCooperative in k_ec_query, the per-contour merge of the overlapping combiner), the
exact comparisons of the tile cull, the degenerate branches of the solvers, the selectors' initial values on channels no edge serves, and the
scanline code at exact hits."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fuzzlib
import geomcases as G
import msdfgen_amd as M
from test_gpu_routes import FORCED
from conftest import assert_bit_equal, bits
from msdfgen_amd.shape import FlatShape, ShapeBatch, autoframe, distance_mapping

pytestmark = pytest.mark.gpu

EC_PAIRS = G.EC_PAIRS
FN = {1: M.generate_sdf, 2: M.generate_psdf, 3: M.generate_msdf, 4: M.generate_mtsdf}


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)
    assert M.device_info()["arch"].startswith("gfx950")


@pytest.fixture(scope="module")
def pool():
    p = ThreadPoolExecutor(max_workers=fuzzlib.oracle_threads())
    yield p
    p.shutdown()


def _cfg(mode, ov, ec=2, dc=1, buffer=None):
    return M.MSDFGeneratorConfig(ov, M.ErrorCorrectionConfig(ec, dc, buffer=buffer)) if mode >= 3 else M.GeneratorConfig(ov)


def _groups(cs):
    """Cases by bitmap size: a batch has one (w, h)."""
    groups = {}
    for c in G.bit_exact(cs):
        groups.setdefault((c.w, c.h), []).append(c)
    return groups


def _ordinary(n, w, h, seed=4000):
    """Random-coordinate glyphs of every distance class under autoframe: what pads a batch of hand-built cases."""
    out = []
    for i in range(n):
        s = fuzzlib._shape(np.random.default_rng(seed+i), (5, 6, 2, 0, 4)[i % 5], seed+i)
        out.append(G.Case("ordinary/%d" % i, s, w, h, autoframe(s.bounds(), w, h, 4.), False))
    return out


def _batched(oracle, pool, cs, mode, ov, ec, dc, y_down, cache=None):
    import torch
    w, h = cs[0].w, cs[0].h
    batch, xfs = ShapeBatch.from_shapes([c.shape for c in cs]), np.stack([c.xf for c in cs])
    gb = M.GlyphBatch(batch)
    st = torch.zeros((len(cs), h, w), dtype=torch.uint8, device="cuda")
    yo = M.Y_DOWNWARD if y_down else M.Y_UPWARD
    got = gb.generate(mode, w, h, xfs, config=_cfg(mode, ov, ec, dc), stencil=st if mode >= 3 else None, y_orientation=yo).cpu().numpy()
    gst = st.cpu().numpy()
    gb.close()

    def want(g):
        key = (cs[g].name, mode, ov, ec, dc, y_down)
        if cache is not None and key in cache:
            return cache[key]
        sb = np.zeros((h, w), np.uint8)
        r = oracle.generate(cs[g].shape, mode, w, h, xfs[g], overlap=ov, ec_mode=ec, ec_dist=dc, y_down=y_down, stencil=sb), sb
        if cache is not None:
            cache[key] = r
        return r
    for g, (a, sb) in enumerate(pool.map(want, range(len(cs)))):
        what = "%s mode %d overlap %d ec %d/%d y_down %d" % (cs[g].name, mode, ov, ec, dc, y_down)
        assert_bit_equal(got[g], a, what)
        if mode >= 3:
            assert (gst[g] == sb).all(), what+": stencil"


def _scanline_batched(oracle, pool, cs, mode, rule, cache):
    """The -scanline flow of one batch (distance, sign pass, correction without distance checks) against the oracle's three steps."""
    w, h = cs[0].w, cs[0].h
    batch, xfs = ShapeBatch.from_shapes([c.shape for c in cs]), np.stack([c.xf for c in cs])
    gb = M.GlyphBatch(batch)
    got = gb.generate(mode, w, h, xfs, config=_cfg(mode, False, 2, 0), scanline_pass=True, fill_rule=rule).cpu().numpy()
    gb.close()

    def want(g):
        key = (cs[g].name, mode, "scanline", rule)
        if key not in cache:
            s = cs[g].shape
            f = oracle.generate(s, mode, w, h, xfs[g], overlap=False, ec_mode=0)
            f = oracle.sign_correction(s, f, xfs[g], .5, rule)
            cache[key] = oracle.error_correction(s, f, xfs[g], overlap=False, ec_mode=2, ec_dist=0) if mode >= 3 else f
        return cache[key]
    for g, a in enumerate(pool.map(want, range(len(cs)))):
        assert_bit_equal(got[g], a, "%s scanline flow mode %d rule %d" % (cs[g].name, mode, rule))


@pytest.mark.parametrize("family", G.FAMILIES)
def test_batched_outline_families_all_modes_and_correction(oracle, pool, family):
    """GlyphBatch.generate per family, at the cases' own sizes and at 41x27 and 64x64: sdf / psdf with both combiners and both Y orientations; msdf /
    mtsdf so that all twelve correction settings occur per family and size class, with the stencil."""
    k = 0
    for cs in list(_groups(G.cases((family,))).values())+[G.bit_exact(G.cases((family,), w=w, h=h)) for w, h in G.BIG_SIZES]:
        for c in cs:
            G.check_premise(c, oracle) if c.shape.n_edges <= 32 else None
        for ov in (True, False):
            for mode in (1, 2):
                _batched(oracle, pool, cs, mode, ov, 0, 0, bool(k & 1))
                k += 1
            for mode in (3, 4):
                for j in range(4):
                    ec, dc = EC_PAIRS[(4*k+j) % 12]                      # k advances by one per (combiner, mode): 12 pairs over three of them
                    _batched(oracle, pool, cs, mode, ov, ec, dc, bool((k+j) & 1))
                _batched(oracle, pool, cs, mode, ov, 2, G.ALWAYS_CHECK, False)
                k += 1


def test_mixed_batch_of_all_families_and_ordinary_glyphs(oracle, pool):
    """One launch holds every family at 64x64 and ordinary glyphs of every distance class; with the small-launch route switched off
    (fuzzlib.TUNINGS["short_classes"]) the three classes run side by side, and the route counters show it."""
    cs = G.bit_exact(G.cases(w=64, h=64))+_ordinary(40, 64, 64)
    with fuzzlib.tuned(fuzzlib.TUNINGS["short_classes"]):
        before = M.route_counts()
        for mode, ov, ec, dc in ((3, True, 2, 2), (4, False, 1, 2), (3, False, 3, 1), (1, True, 0, 0), (2, False, 0, 0)):
            _batched(oracle, pool, cs, mode, ov, ec, dc, mode == 4)
        r = fuzzlib._delta(M.route_counts(), before)
    assert r["dist_one_single"] > 0 and r["dist_lds_single"] > 0 and r["dist_global_direct"]+r["dist_global_persistent"] > 0, r
    assert r["dist_small_simple"] == r["dist_small_overlap"] == 0, r


@pytest.mark.parametrize("name", sorted(fuzzlib.TUNINGS))
def test_forced_routes_on_replicated_outline_families(oracle, pool, name):
    """Every table of fuzzlib.TUNINGS on the 64x64 cases of all families plus ordinary glyphs, replicated to at least 256 glyphs and more than 8 192
    tiles, with ALWAYS_CHECK_DISTANCE: the tied texels go through k_ec_query under each query policy (query_counter above all). One oracle tile per
    distinct case."""
    base = G.bit_exact(G.cases(w=64, h=64))+_ordinary(12, 64, 64)
    cs = base*(256//len(base)+1)
    if name == "persistent_grid":
        # The global-scratch class runs persistent only when its launch has at least MSDFHIP_PERSISTENT_ROUNDS (here 1) x resident wavefront slots
        # (CUs x 4 SIMDs x 4 wavefronts) blocks of up to four tiles: the 144-edge grid, of that class by its edge count, as often as that takes.
        heavy = [c for c in base if c.shape.n_edges > 128]
        slots = M.device_info()["cus"]*16
        cs = cs+heavy[:1]*(slots*4//64+1)
    assert len(cs) >= fuzzlib.FULL_MIN_GLYPHS and len(cs)*64 > fuzzlib.FULL_MIN_TILES
    cache = {}
    with fuzzlib.tuned(fuzzlib.TUNINGS[name]):
        before = M.route_counts()
        _batched(oracle, pool, cs, 3, True, 2, G.ALWAYS_CHECK, False, cache)
        _batched(oracle, pool, cs, 4, False, 1, G.ALWAYS_CHECK, True, cache)
        if name == "sign_chunked":                                                # the table's point: the sign pass in chunks, on tied scanlines
            _scanline_batched(oracle, pool, cs, 3, M.FILL_NONZERO, cache)
            _scanline_batched(oracle, pool, cs, 1, M.FILL_ODD, cache)
        r = fuzzlib._delta(M.route_counts(), before)
    print(name, r)
    assert r["dist_small_simple"] == r["dist_small_overlap"] == 0, r              # a launch of this size never takes the small route
    assert r["ec_query_batch"]+r["ec_query_heaviest"] > 0, r
    ran, idle, _ = FORCED[name]                                                   # what tests/test_gpu_routes.py demands of the same table
    for alternatives in ran:
        assert sum(r[k] for k in alternatives) > 0, (name, alternatives, r)
    for k in idle:
        assert r[k] == 0, (name, k, r)


def test_bounded_sweep_of_jittered_outline_families():
    """fuzzlib.run(geometry=...): groups that draw a family and a size and jitter every case on its lattice, batched with the stencil and through
    generate_stream and HostBatch.generate_host, then every glyph through its own call. No value, NaN patterns included, and no stencil byte differs."""
    for single in (False, True):
        r = fuzzlib.run(1200 if not single else 300, 611+single, deadline_s=25, min_groups=8, geometry=list(G.FAMILIES), stencil=not single,
                        paths=not single, single=single)
        print({k: v for k, v in r.items() if k != "group_routes"})
        assert r["groups"] >= 8 and r["values_compared"] > 0
        assert r["values_differing_bitwise"] == 0 and r["max_abs_delta"] == 0, r["worst_case"]
        assert r["stencil_values_differing"] == 0 and r["path_values_differing"] == 0, r
        assert r["framings"] == sorted(G.FAMILIES), r["framings"]


def _single_calls(oracle, cs, label):
    for i, c in enumerate(cs):
        for mode in (1, 2, 3, 4):
            for y_down in (False, True):
                ov = bool((i+mode) & 1)
                ec, dc = EC_PAIRS[(i+3*mode+y_down) % 12]
                sa, sb = np.zeros((c.h, c.w), np.uint8), np.zeros((c.h, c.w), np.uint8)
                got = FN[mode](np.zeros((c.h, c.w, M.CHANNELS[mode]), np.float32), c.shape, M.SDFTransformation.from_xf(c.xf), _cfg(mode, ov, ec, dc, sa),
                               M.Y_DOWNWARD if y_down else M.Y_UPWARD)
                want = oracle.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, ec_mode=ec if mode >= 3 else 0, ec_dist=dc, y_down=y_down, stencil=sb)
                what = "%s %s mode %d overlap %d ec %d/%d y_down %d" % (c.name, label, mode, ov, ec, dc, y_down)
                assert_bit_equal(got, want, what)
                if mode >= 3:
                    assert (sa == sb).all(), what+": stencil"
        if c.shape.n_contours > 1:                                    # the tied texels under the distance check of every texel, both combiners
            for ov in (True, False):
                got = M.generate_msdf(np.zeros((c.h, c.w, 3), np.float32), c.shape, M.SDFTransformation.from_xf(c.xf), _cfg(3, ov, 2, G.ALWAYS_CHECK))
                assert_bit_equal(got, oracle.generate(c.shape, 3, c.w, c.h, c.xf, overlap=ov, ec_mode=2, ec_dist=G.ALWAYS_CHECK),
                                 "%s %s always check, overlap %d" % (c.name, label, ov))


def test_single_calls_on_outline_families(oracle):
    """generate_sdf / psdf / msdf / mtsdf, one fused launch per call with its team of four wavefronts (msdf_single.hpp), on every case at its own size
    and on the 64x64 lattice_ties and coincident cases."""
    _single_calls(oracle, G.bit_exact(G.cases()+G.cases(("lattice_ties", "coincident"), w=64, h=64)), "single")


@pytest.mark.parametrize("env", ("MSDFHIP_NO_ARG_PAYLOAD_SINGLE", "MSDFHIP_NO_ZERO_COPY_SINGLE", "MSDFHIP_NO_FUSED_SINGLE"))
def test_single_calls_with_the_fallbacks_forced(oracle, env):
    """The same calls with the fused launch's other input routes and with the fused launch switched off (the batched sequence)."""
    with fuzzlib.tuned({env: "1"}):
        _single_calls(oracle, G.bit_exact(G.cases()), env)


def test_host_pipeline_stream_and_bytes_on_outline_families(oracle, pool):
    """HostBatch.generate_host, generate_stream and the 8-bit atlas path. The bytes equal pixelFloatToByte of the oracle's floats -- for
    sparse_colours that includes the non-finite values of channels without an edge."""
    for w, h in ((12, 12), (64, 64)):
        cs = [c for c in G.bit_exact(G.cases() if w == 12 else G.cases(w=w, h=h)) if (c.w, c.h) == (w, h)]
        assert any(c.name.startswith("sparse_colours") for c in cs)
        batch, xfs = ShapeBatch.from_shapes([c.shape for c in cs]), np.stack([c.xf for c in cs])
        n = len(cs)
        offs8 = np.array([g*h*w*3 for g in range(n)], np.int64)
        for ov, ec, dc in ((True, 2, 1), (False, 2, 2), (True, 0, 0)):
            c = _cfg(3, ov, ec, dc)
            want = np.stack(list(pool.map(lambda g: oracle.generate(cs[g].shape, 3, w, h, xfs[g], overlap=ov, ec_mode=ec, ec_dist=dc), range(n))))
            if ec == 0:
                sparse = [g for g in range(n) if cs[g].name.startswith("sparse_colours")]
                assert not np.isfinite(want[sparse]).all(), "sparse_colours was meant to put non-finite values into the field"
            want8 = oracle.pixel_float_to_byte(want)
            hb = M.HostBatch(batch)
            try:
                assert_bit_equal(hb.generate_host(3, w, h, xfs, config=c), want, "generate_host %dx%d overlap %d ec %d/%d" % (w, h, ov, ec, dc))
                assert_bit_equal(M.generate_stream(batch, 3, w, h, xfs, config=c), want, "generate_stream %dx%d overlap %d ec %d/%d" % (w, h, ov, ec, dc))
                b8 = np.zeros((n, h, w, 3), np.uint8)
                hb.generate_bytes_host(3, w, h, xfs, b8, offs8, w*3, config=c)
                assert (b8 == want8).all(), "generate_bytes_host: %d bytes differ" % int((b8 != want8).sum())
                s8 = np.full((n, h, w, 3), 77, np.uint8)
                M.generate_stream(batch, 3, w, h, xfs, atlas=s8, out_offsets=offs8, row_stride=w*3, config=c)
                assert (s8 == want8).all(), "generate_stream 8-bit: %d bytes differ" % int((s8 != want8).sum())
            finally:
                hb.close()


def test_scanline_flow_and_standalone_passes_on_outline_families(oracle, pool):
    """The -scanline flow inside GlyphBatch.generate under four fill rules, msdf_error_correction on an uncorrected field, distance_sign_correction,
    rasterize, the error estimate (1 and 3 scanlines per row) and render_sdf (from fields with non-finite channels too), where scanlines run along horizontal edges and through vertices and where a
    channel has no edge."""
    fams = ("scanline_hits", "on_outline", "sparse_colours")
    for (w, h), group in list(_groups(G.cases(fams)).items())+[((41, 27), G.cases(fams, w=41, h=27))]:
        batch, xfs = ShapeBatch.from_shapes([c.shape for c in group]), np.stack([c.xf for c in group])
        gb = M.GlyphBatch(batch)
        for mode, rule in ((3, M.FILL_NONZERO), (4, M.FILL_ODD), (1, M.FILL_POSITIVE), (3, M.FILL_NEGATIVE)):
            got = gb.generate(mode, w, h, xfs, config=_cfg(mode, False, 2, 0), scanline_pass=True, fill_rule=rule).cpu().numpy()

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
                bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
                assert len(bad) == 0, "estimate_sdf_error mode %d spr %d rule %d: %s" % (mode, spr, rule, [(group[g].name, got[g], want[g]) for g in bad])
        for mode, n_outs, ec in ((1, (1, 3), 0), (3, (1, 3), 0), (4, (1, 4), 0), (3, (3,), 2)):      # uncorrected fields keep sparse_colours' non-finite channels
            tiles = gb.generate(mode, w, h, xfs, config=_cfg(mode, True, ec, 1))
            src = tiles.cpu().numpy()
            if ec == 0 and mode >= 3 and any(c.name.startswith("sparse_colours") for c in group):
                assert not np.isfinite(src).all(), "sparse_colours was meant to put non-finite values into the field"
            for n_out in n_outs:
                for ow, oh in ((w, h), (2*w+1, 2*h-1), (7, 5)):
                    for lo, hi, thr in ((0, 0, .5), (-2, 2, .5), (2, -2, .5), (-1, 3, .4)):
                        got = M.render_sdf(tiles, ow, oh, n_out, (lo, hi), thr).cpu().numpy()
                        for g in range(len(group)):
                            assert_bit_equal(got[g], oracle.render_sdf(src[g], ow, oh, n_out, lo, hi, thr),
                                             "%s renderSDF %d<-%d %dx%d range (%g, %g)" % (group[g].name, n_out, src.shape[3], ow, oh, lo, hi))
        gb.close()
        if (w, h) == (41, 27):
            continue
        for i, c in enumerate(group):
            yo = M.Y_DOWNWARD if c.y_down else M.Y_UPWARD
            xf = M.SDFTransformation.from_xf(c.xf)
            pre = oracle.generate(c.shape, 3, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
            for ec, dc in ((2, 1), (1, 2), (3, 0)):
                sa, sb = np.zeros((c.h, c.w), np.uint8), np.zeros((c.h, c.w), np.uint8)
                got = M.msdf_error_correction(pre.copy(), c.shape, xf, _cfg(3, bool(i & 1), ec, dc, sa), yo)
                want = oracle.error_correction(c.shape, pre, c.xf, overlap=bool(i & 1), ec_mode=ec, ec_dist=dc, y_down=c.y_down, stencil=sb)
                assert_bit_equal(got, want, "%s error_correction ec %d/%d" % (c.name, ec, dc))
                assert (sa == sb).all(), c.name+": stencil"
            for mode in (1, 3):
                field = oracle.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
                for rule in range(4):
                    assert_bit_equal(M.distance_sign_correction(field.copy(), c.shape, xf, .5, rule, yo),
                                     oracle.sign_correction(c.shape, field, c.xf, .5, rule, y_down=c.y_down), "%s sign correction mode %d rule %d" % (c.name, mode, rule))
            for rule in range(4):
                assert_bit_equal(M.rasterize(np.full((c.h, c.w, 1), -3, np.float32), c.shape, xf, rule, yo),
                                 oracle.rasterize(c.shape, c.w, c.h, c.xf, rule, y_down=c.y_down), "%s rasterize rule %d" % (c.name, rule))


def _flat(fa):
    return FlatShape(fa.contour_offsets, fa.points, fa.types, fa.colors)


@pytest.mark.parametrize("family", ("degenerate_edges", "coincident", "lattice_ties"))
def test_device_preparation_on_stripped_outlines(oracle, ref, pool, family):
    """The outlines with their colours stripped through the device's shape preparation -- msdfhip_batch_create_prepared (GlyphBatch.from_raw) and
    generate_stream(prepare=...): normalize alone, both colourings, three seeds. Exact 90 and 180 degree corners sit on the angle threshold's
    comparisons, one- and two-edge contours take normalize's split paths, coincident contours tie in the winding walk. The prepared batch equals
    oracle.shape_prepare bit for bit, the tiles of both routes the oracle's tiles of the oracle-prepared shapes. The oriented variant
    (orient_contours, winding guess) against the compiled reference's own sequence (orientcases.ref_prepare_batch)."""
    import orientcases as OC
    for cs in list(_groups(G.cases((family,))).values())+[G.bit_exact(G.cases((family,), w=64, h=64))]:
        w, h = cs[0].w, cs[0].h
        raw = ShapeBatch.from_shapes([G.strip_colours(c.shape) for c in cs], [c.name for c in cs])
        xfs = np.stack([c.xf for c in cs])

        def check(gb, want, prep, what):
            OC.same_batch(gb.shapes, want, what)
            for mode, ov, ec, dc in ((3, True, 2, 1), (4, False, 2, G.ALWAYS_CHECK)):
                tiles = np.stack(list(pool.map(lambda g: oracle.generate(want.shape(g), mode, w, h, xfs[g], overlap=ov, ec_mode=ec, ec_dist=dc), range(len(cs)))))
                got = gb.generate(mode, w, h, xfs, config=_cfg(mode, ov, ec, dc)).cpu().numpy()
                stream = M.generate_stream(raw, mode, w, h, xfs, config=_cfg(mode, ov, ec, dc), prepare=prep)
                for g, c in enumerate(cs):
                    assert_bit_equal(got[g], tiles[g], "%s %s mode %d: prepared batch" % (c.name, what, mode))
                    assert_bit_equal(stream[g], tiles[g], "%s %s mode %d: generate_stream(prepare=)" % (c.name, what, mode))
        for normalize, coloring, seed in ((True, 0, 0), (True, 1, 0), (True, 2, 1), (False, 1, 12345678901), (True, 1, 12345678901), (False, 2, 0)):
            what = "normalize %d colouring %d seed %d" % (normalize, coloring, seed)
            want = ShapeBatch.from_shapes([_flat(oracle.shape_prepare(raw.shape(g), normalize, coloring, 3.0, seed)) for g in range(len(cs))])
            gb = M.GlyphBatch.from_raw(raw, normalize, coloring, 3.0, seed=seed)
            try:
                check(gb, want, M.PrepareConfig(normalize, coloring, 3.0, seed), what)
            finally:
                gb.close()
        for winding in (M.WINDING_GUESS, M.WINDING_REVERSE):
            want = OC.ref_prepare_batch(ref, raw, True, winding, True, 1, 3.0, None)
            gb = M.GlyphBatch.from_raw(raw, True, 1, 3.0, orient_contours=True, winding=winding)
            try:
                check(gb, want, M.PrepareConfig(True, 1, 3.0, 0, orient_contours=True, winding=winding), "oriented, winding %d" % winding)
            finally:
                gb.close()


def test_fold_back_quadratic_follows_the_lean_host_build(oracle):
    """geomcases.SIGN_NOISE, treated exactly as test_backtracking_curves_follow_the_host_build_with_the_devices_own_transcendentals treats its two
    glyphs: the tiles equal the host build with the kernels' own transcendentals bit for bit, and whatever differs from the oracle is a sign flip
    about the mapped zero level, on at most 16 values."""
    from emu import Emu
    emu = Emu(lean=True)
    for c in [c for c in G.cases(("degenerate_edges",)) if G.base_name(c) in G.SIGN_NOISE]:
        for mode in (1, 3):
            for ov in (True, False):
                got = FN[mode](np.zeros((c.h, c.w, M.CHANNELS[mode]), np.float32), c.shape, M.SDFTransformation.from_xf(c.xf), _cfg(mode, ov, 0, 0))
                want = emu.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, ec_mode=0)
                assert (bits(got) == bits(want)).all(), "%s mode %d overlap %d: %d values differ from the lean host build" % (c.name, mode, ov, int((bits(got) != bits(want)).sum()))
                ref = oracle.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, ec_mode=0)
                bad = bits(got) != bits(ref)
                if bad.any():
                    ms, mt = distance_mapping(c.xf[4], c.xf[5])
                    zero = ms*mt
                    assert np.allclose(got[bad].astype(np.float64)-zero, -(ref[bad].astype(np.float64)-zero), atol=1e-5), (c.name, mode, ov)
                assert bad.sum() <= 16, (c.name, mode, ov, int(bad.sum()))
