"""The legacy generators (k_distance_legacy) and the legacy error correction (k_ec_legacy) on the GPU against the recorded reference
(tests/golden/legacy.npz, tools/make_golden_legacy.py): every record through the single-shape C ABI and through resident batches of 9 and of 2 glyphs,
the reference CLI's default -legacy flow, the stencils of the four orientation combinations, both forms of the legacy correction, and what a legacy
call must not do to its neighbours -- to a later modern call on the same batch, and to modern calls grouped next to it. Every comparison is bitwise."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import msdfgen_amd as M
from msdfgen_amd import lib as L
from conftest import assert_bit_equal
import legacycases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return LC.golden()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return LC.build_host(tmp_path_factory.mktemp("legacy_host"))


def config_of(r):
    """The C ABI's config of a record: the correction mode and, for the default flow, the sign pass. (Left at their defaults: overlap support on and the
    distance check at the edges -- the legacy entry points must not read them.)"""
    cfg = L.default_config(ec_mode=r.ec if r.mode >= 3 else M.EC_EDGE_PRIORITY, stencil_y_down=int(r.y_down))
    if r.sign:
        cfg.sign_correction, cfg.fill_rule, cfg.sdf_zero_value = 1, r.fill, r.zero
    return cfg


def single(batch, r):
    """One msdfhip_generate_legacy call: (bitmap, stencil or None)."""
    shape = batch.shape(r.shape)
    out = np.full((r.h, r.w, LC.CHANNELS[r.mode]), 3., np.float32)
    stencil = np.zeros((r.h, r.w), np.uint8) if r.stencil is not None else None
    co, pts, types, colors = LC.shape_arrays(shape)
    xf, cfg = LC.xf6(r.xf), config_of(r)
    flip = int(bool(shape.inverse_y) != r.y_down)
    L.check(L.load().msdfhip_generate_legacy(r.mode, L.ptr(out, L._fp), r.w, r.h, out.strides[0]//4, flip, L.ptr(co, L._ip), shape.n_contours, L.ptr(pts, L._dp),
                                             L.ptr(types, L._bp), L.ptr(colors, L._bp), L.ptr(xf, L._dp), C.byref(cfg),
                                             L.ptr(stencil, L._bp) if stencil is not None else None))
    return out, stencil


def check(r, out, stencil, how):
    assert_bit_equal(out, r.out, "%s (%s)" % (r.name, how))
    if r.stencil is not None:
        assert_bit_equal(stencil, r.stencil, "stencil of %s (%s)" % (r.name, how))


def test_single_calls_equal_the_recorded_reference(gold):
    """Every fixture record, the default flow's included, through msdfhip_generate_legacy."""
    batch, recs, _ = gold
    M.init(0)
    for r in recs:
        check(r, *single(batch, r), "single call")


def test_python_drop_ins_equal_the_recorded_reference(gold):
    """generate_*_legacy(output, shape, range, scale, translate[, error_correction_config]) -- one record per mode, into a bitmap with a row stride."""
    batch, recs, _ = gold
    fns = {1: M.generate_sdf_legacy, 2: M.generate_pseudo_sdf_legacy, 3: M.generate_msdf_legacy, 4: M.generate_mtsdf_legacy}
    for mode in (1, 2, 3, 4):
        r = next(r for r in recs if r.mode == mode and r.w >= 8 and not r.sign)
        wide = np.full((r.h, r.w+3, LC.CHANNELS[mode]), 5., np.float32)
        args = (wide[:, :r.w], batch.shape(r.shape), M.Range(r.xf[4], r.xf[5]), (r.xf[0], r.xf[1]), (r.xf[2], r.xf[3]))
        if mode >= 3:
            args += (M.ErrorCorrectionConfig(mode=r.ec),)
        fns[mode](*args, y_orientation=M.Y_DOWNWARD if r.y_down else M.Y_UPWARD)
        assert_bit_equal(wide[:, :r.w], r.out, r.name)
        assert (wide[:, r.w:] == 5.).all()


def groups_of(recs):
    """Records that one resident batch can render together: everything that is a launch parameter agrees."""
    out = {}
    for r in recs:
        out.setdefault((r.mode, r.w, r.h, r.ec, r.y_down, r.sign, r.fill, r.zero, r.stencil is not None), []).append(r)
    return list(out.values())


def run_batch(batch, members):
    """GlyphBatch.generate_legacy of the members' shapes, each with its own transformation: [(bitmap, stencil or None)] per member."""
    r = members[0]
    gb = M.GlyphBatch(batch.select([m.shape for m in members]))
    stencil = torch.zeros((len(members), r.h, r.w), dtype=torch.uint8, device=gb.device) if r.stencil is not None else None
    tiles = gb.generate_legacy(r.mode, r.w, r.h, np.stack([m.xf for m in members]), config=M.ErrorCorrectionConfig(mode=r.ec) if r.mode >= 3 else None,
                               stencil=stencil, y_orientation=M.Y_DOWNWARD if r.y_down else M.Y_UPWARD, scanline_pass=r.sign, fill_rule=r.fill,
                               sdf_zero_value=r.zero).cpu().numpy()
    st = stencil.cpu().numpy() if stencil is not None else None
    gb.close()
    return [(tiles[k], st[k] if st is not None else None) for k in range(len(members))]


@pytest.mark.parametrize("size", [9, 2])
def test_resident_batches_equal_the_recorded_reference(gold, size):
    """Every record in a batch of 9 glyphs (one full group of eight, dealt glyph by glyph to the XCDs, and a remainder dealt tile by tile: decodeBlock)
    and in a batch of 2 (remainder only); a group of fewer records than the batch holds is repeated round robin."""
    batch, recs, _ = gold
    seen = 0
    for group in groups_of(recs):
        for start in range(0, len(group), size):
            members = [group[(start+i) % len(group)] for i in range(size)]
            for m, (out, st) in zip(members, run_batch(batch, members)):
                check(m, out, st, "batch of %d" % size)
            seen += min(size, len(group)-start)
    assert seen == len(recs)


def test_default_flow_of_the_reference_cli(gold):
    """scanline_pass=True: legacy field -> distanceSignCorrection -> msdfErrorCorrection without the distance check, as `msdfgen -legacy` runs it
    (main.cpp:1223-1298), msdf and mtsdf on BLOBS at 40x32 -- and the sign pass did change the field."""
    batch, recs, _ = gold
    flows = [r for r in recs if r.sign]
    assert [r.mode for r in flows] == [3, 4]
    for r in flows:
        (out, _), = run_batch(batch, [r])
        assert_bit_equal(out, r.out, r.name)
        plain, _ = single(batch, r._replace(sign=False))                       # the same call without the sign pass
        assert (plain.view(np.uint32) != r.out.view(np.uint32)).any()


def test_stencils_of_the_four_orientations(gold):
    """ErrorCorrectionConfig::buffer for inverse_y x y_orientation at 9x7, single calls and one resident batch per bitmap orientation: the stencil's
    rows go upward whatever the bitmap's orientation, and the correction sees a bitmap re-oriented to the shape (msdfgen.cpp:223)."""
    batch, recs, _ = gold
    withst = [r for r in recs if r.stencil is not None]
    assert len(withst) == 4 and all((r.w, r.h) == (9, 7) for r in withst)
    for r in withst:
        check(r, *single(batch, r), "single call")
    for y_down in (False, True):
        members = [r for r in withst if r.y_down == y_down]
        assert len(members) == 2 and {bool(batch.inverse_y[m.shape]) for m in members} == {False, True}
        for m, (out, st) in zip(members, run_batch(batch, members)):
            check(m, out, st, "batch")
    up, down = [next(r for r in withst if not batch.inverse_y[r.shape] and r.y_down == d) for d in (False, True)]
    assert_bit_equal(up.stencil, down.stencil, "the stencil does not depend on the bitmap's orientation")
    assert not np.array_equal(up.stencil, up.stencil[::-1])                   # (and a wrong row order would show)


def test_legacy_route_differs_from_the_modern_one(gold):
    """On the five overlapping contours of BLOBS the minimum over all edges is not what the overlapping contour combiner gives: the recorded legacy MSDF
    (which the legacy entry points reproduce, above) must differ from generate_msdf(overlap_support=True), or the tests would not be looking at the
    legacy route at all."""
    batch, recs, _ = gold
    r = next(r for r in recs if r.name == "blobs/msdf")
    modern = M.generate_msdf(np.zeros((r.h, r.w, 3), np.float32), batch.shape(r.shape), M.SDFTransformation.from_xf(r.xf), M.MSDFGeneratorConfig(overlap_support=True))
    legacy, _ = single(batch, r)
    assert_bit_equal(legacy, r.out, r.name)
    assert int((legacy.view(np.uint32) != modern.view(np.uint32)).sum()) >= 1


def test_legacy_correction_on_host_bitmaps(gold):
    """msdfhip_error_correction_legacy: every recorded field, packed and as the rows of a wider bitmap walked bottom-up (a negative row stride)."""
    _, _, ecs = gold
    for e in ecs:
        what = "legacy correction %dx%dx%d (%g, %g)" % (e.w, e.h, e.n, e.tx, e.ty)
        assert_bit_equal(M.msdf_error_correction_legacy(e.field.copy(), (e.tx, e.ty)), e.out, what)
        wide = np.full((e.h, e.w+2, e.n), 5., np.float32)
        view = wide[::-1, :e.w]
        view[...] = e.field
        M.msdf_error_correction_legacy(view, (e.tx, e.ty))
        assert_bit_equal(np.ascontiguousarray(view), e.out, what+", strided")
        assert (wide[:, e.w:] == 5.).all()


def test_legacy_correction_on_device_tiles(gold, host):
    """msdfhip_batch_error_correction_legacy: every recorded field as one tile, and as the 5th of 9 tiles in one call whose other tiles are fresh random
    fields checked against the host build of the same passes (itself pinned to the reference by test_legacy_host.py)."""
    _, _, ecs = gold
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    for e in ecs:
        what = "legacy correction %dx%dx%d (%g, %g)" % (e.w, e.h, e.n, e.tx, e.ty)
        one = M.error_correction_legacy(torch.from_numpy(e.field[None].copy()).to(dev), (e.tx, e.ty)).cpu().numpy()
        assert_bit_equal(one[0], e.out, what)
        nine = rng.uniform(0, 1, (9, e.h, e.w, e.n)).astype(np.float32)
        nine[4] = e.field
        want = np.stack([LC.host_correction(host, t, e.tx, e.ty) for t in nine])
        assert_bit_equal(want[4], e.out, what+", host")
        assert_bit_equal(M.error_correction_legacy(torch.from_numpy(nine).to(dev), (e.tx, e.ty)).cpu().numpy(), want, what+", 9 tiles")


def linear_batch(gold):
    """Nine fixture shapes without a curve (the modern path is bit-equal to the oracle on those), several of them with more than one contour."""
    batch, _, _ = gold
    pick = [g for g in range(batch.n_glyphs) if batch.shape(g).n_edges and (batch.shape(g).types == 1).all() and not batch.inverse_y[g]][:9]
    assert len(pick) == 9 and sum(batch.shape(g).n_contours > 1 for g in pick) >= 3
    return batch.select(pick)


def test_a_legacy_call_leaves_nothing_on_the_batch(gold, oracle):
    """One resident batch: modern generate -> generate_legacy -> modern generate at another size. Both modern results equal the oracle bit for bit, the
    legacy one equals single legacy calls: no class list, correction constant or scratch of one call is trusted by the next."""
    sub = linear_batch(gold)
    gb = M.GlyphBatch(sub)
    bounds = [sub.shape(g).bounds() for g in range(sub.n_glyphs)]
    sizes = ((32, 32), (40, 32), (24, 40))
    xfs = [np.stack([M.autoframe(b, w, h, 4) for b in bounds]) for (w, h) in sizes]
    first = gb.generate(M.MODE_MSDF, *sizes[0], xfs[0]).cpu().numpy()
    legacy = gb.generate_legacy(M.MODE_MTSDF, *sizes[1], xfs[1]).cpu().numpy()
    second = gb.generate(M.MODE_MSDF, *sizes[2], xfs[2]).cpu().numpy()
    gb.close()
    for g in range(sub.n_glyphs):
        assert_bit_equal(first[g], oracle.generate(sub.shape(g), 3, *sizes[0], xfs[0][g]), "modern call before, glyph %d" % g)
        assert_bit_equal(second[g], oracle.generate(sub.shape(g), 3, *sizes[2], xfs[2][g]), "modern call after, glyph %d" % g)
        want = M.generate_mtsdf_legacy(np.zeros((sizes[1][1], sizes[1][0], 4), np.float32), sub.shape(g), M.Range(xfs[1][g][4], xfs[1][g][5]),
                                       xfs[1][g][:2], xfs[1][g][2:4])
        assert_bit_equal(legacy[g], want, "legacy call between, glyph %d" % g)


def test_legacy_and_modern_calls_are_grouped_apart(gold, oracle):
    """Eight threads of one process issue single-shape calls of one size at once, four legacy and four modern, the modern ones with exactly the config a
    legacy call runs under (no overlap support, no distance check): only the operation tells them apart when the micro-batcher groups the queue
    (sameLaunch). Each result equals its own reference."""
    batch, recs, _ = gold
    w, h = LC.SIZES[-1]
    legacy = [r for r in recs if r.name in ("shape_a/msdf", "cli_teardrop/msdf", "blobs/msdf", "ring65/msdf")]
    assert len(legacy) == 4 and all((r.mode, r.w, r.h, r.ec, r.y_down) == (3, w, h, 2, False) for r in legacy)
    cfg = M.MSDFGeneratorConfig(False, M.ErrorCorrectionConfig(M.EC_EDGE_PRIORITY, M.DO_NOT_CHECK_DISTANCE))
    modern = [(batch.shape(r.shape), r.xf) for r in legacy[:2]]*2                      # shape_a and the CLI test's outline: straight edges only
    want = [oracle.generate(s, 3, w, h, xf, overlap=False, ec_mode=2, ec_dist=0) for s, xf in modern]
    errors, barrier = [], threading.Barrier(8)

    def work(t):
        try:
            barrier.wait()
            for _ in range(4):
                if t < 4:
                    check(legacy[t], *single(batch, legacy[t]), "thread %d" % t)
                else:
                    s, xf = modern[t-4]
                    got = M.generate_msdf(np.zeros((h, w, 3), np.float32), s, M.SDFTransformation.from_xf(xf), cfg)
                    assert_bit_equal(got, want[t-4], "modern call of thread %d" % t)
        except Exception as e:  # noqa: BLE001
            errors.append(e)
            barrier.abort()
    M.microbatch_stats(reset=True)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    assert M.microbatch_stats()["calls"] == 32
