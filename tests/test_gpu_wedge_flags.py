"""The wedge flags of the distance walk on the GPU, bit for bit against the oracle (shapes: tests/wedgecases.py; the CPU side: tests/test_wedge_flags_host.py).

Phase 1 of k_distance stores, per survivor, whether the whole tile lies outside each end's wedge; the per-texel walk then skips that end's perpendicular
distance and its relevance test. A wrong bit drops a perpendicular distance that the reference takes: a different channel value at texels beyond an edge's
end. The crafted outlines (needle corners, corners at a tile's centre and where four tiles meet, zero-length end tangents, contours far outside the bitmap)
and three Latin glyphs at 8 x 8, 16 x 16 and 24 x 16 (anisotropic for the crafted ones; three tiles, not a multiple of the quad), modes psdf / msdf / mtsdf,
both combiners, through every form of the walk: the small route, the three glyph classes in their four-tile and one-tile forms, the persistent
global-scratch class, the per-glyph-box twins with two box sizes in one call, and the fused single-shape launch with its team of wavefronts."""
import functools

import numpy as np
import pytest

import msdfgen_amd as M
import fuzzlib
import wedgecases as W
from msdfgen_amd import synth
from msdfgen_amd.shape import FlatShape, ShapeBatch, autoframe

pytestmark = pytest.mark.gpu
MODES = (2, 3, 4)                                                          # psdf, msdf, mtsdf


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)
    info = M.device_info()
    assert info["arch"].startswith("gfx950"), info
    return info


@functools.lru_cache(maxsize=None)
def glyphs(size):
    """(names, shapes, xfs) at one bitmap size: the crafted outlines in their design framing, the Latin glyphs autoframed, and one CJK-like glyph of many
    contours (msdf: seven contours and more exceed the LDS the combiner scratch may take -- the global-scratch class)."""
    w, h = size
    names, shapes, xfs = [], [], []
    for name, contours in sorted(W.CRAFTED.items()):
        names.append(name), shapes.append(FlatShape.from_contours(contours)), xfs.append(W.design_xf(w, h, pr=min(4., .45*min(w, h))))
    for name, s in W.real_glyphs()+[("cjk", synth.cjk_like_shape(903))]:
        names.append(name), shapes.append(s), xfs.append(autoframe(s.bounds(), w, h, min(4., .45*min(w, h))))
    return names, shapes, np.stack(xfs)


@functools.lru_cache(maxsize=None)
def batch(size):
    return M.GlyphBatch(ShapeBatch.from_shapes(glyphs(size)[1]))


@functools.lru_cache(maxsize=None)
def reference(size, mode, overlap):
    """The oracle's bitmaps of glyphs(size), library-default configuration: computed once, shared, read-only."""
    from oracle.pyoracle import Oracle
    orc = Oracle()
    _, shapes, xfs = glyphs(size)
    out = []
    for s, xf in zip(shapes, xfs):
        f = orc.generate(s, mode, size[0], size[1], xf, overlap=overlap)
        f.setflags(write=False)
        out.append(f)
    return out


def config(mode, overlap):
    return M.MSDFGeneratorConfig(overlap) if mode >= 3 else M.GeneratorConfig(overlap)


def differing(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return int(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).sum())


def check_batch(size, mode, overlap, got, what):
    names = glyphs(size)[0]
    want = reference(size, mode, overlap)
    bad = {names[g]: differing(got[g], want[g]) for g in range(len(names))}
    assert not any(bad.values()), (what, size, mode, overlap, {k: v for k, v in bad.items() if v})


def render(size, mode, overlap):
    _, _, xfs = glyphs(size)
    return batch(size).generate(mode, size[0], size[1], xfs, config=config(mode, overlap)).cpu().numpy()


def test_the_inputs_are_the_ones_described():
    names, shapes, _ = glyphs(W.GPU_SIZES[0])
    assert len(names) == len(W.CRAFTED)+4 and [s.n_contours for s in shapes[-4:-1]] == [3, 5, 2] and shapes[-1].n_contours >= 7
    assert any(s.n_contours == 1 for s in shapes) and sum(s.n_contours == 2 for s in shapes) >= 3


@pytest.mark.parametrize("overlap", [True, False], ids=["overlapping", "simple"])
@pytest.mark.parametrize("size", W.GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_small_route_vs_oracle(size, overlap):
    for mode in MODES:
        before = M.route_counts()
        got = render(size, mode, overlap)
        routes = fuzzlib._delta(M.route_counts(), before)
        assert routes["dist_small_overlap" if overlap else "dist_small_simple"] == 1, routes
        check_batch(size, mode, overlap, got, "small route")


@pytest.mark.parametrize("table,ran", [("quad_classes", ("dist_one_quad", "dist_lds_quad")), ("short_classes", ("dist_one_single", "dist_lds_single"))])
def test_glyph_classes_vs_oracle(table, ran):
    """The launch plan of a throughput-sized call: one-contour glyphs, combiner scratch in LDS (four tiles per wavefront: the benchmark's dominant launch;
    one tile: its short form) and, for the CJK-like glyph, in the global workspace."""
    total = None
    with fuzzlib.tuned(fuzzlib.TUNINGS[table]):
        for size in W.GPU_SIZES:
            for mode in MODES:
                before = M.route_counts()
                got = render(size, mode, True)
                routes = fuzzlib._delta(M.route_counts(), before)
                total = routes if total is None else {k: total[k]+routes[k] for k in routes}
                check_batch(size, mode, True, got, table)
            got = render(size, 3, False)                                   # (quad_classes: the simple combiner's full-size plan)
            check_batch(size, 3, False, got, table+", simple combiner")
    print(total)
    assert all(total[k] > 0 for k in ran) and total["dist_global_direct"]+total["dist_global_persistent"] > 0, total
    assert total["dist_small_overlap"] == 0 and total["dist_small_simple"] == 0, total


def test_persistent_global_scratch_class_vs_oracle(_device):
    """The CJK-like glyph often enough for the planner to make the global-scratch class a persistent launch (one round of the device's wavefront slots under
    MSDFHIP_PERSISTENT_ROUNDS=1: compute units x 16 one-tile items; the glyph has six tiles at 24 x 16): every copy is the oracle's bitmap."""
    size = W.GPU_SIZES[2]
    names, shapes, xfs = glyphs(size)
    g = names.index("cjk")
    reps = -(-_device["cus"]*16//6)+3
    gb = M.GlyphBatch(ShapeBatch.from_shapes([shapes[g]]*reps))
    with fuzzlib.tuned(fuzzlib.TUNINGS["persistent_grid"]):
        for mode in (3, 4):
            before = M.route_counts()
            got = gb.generate(mode, size[0], size[1], np.tile(xfs[g], (reps, 1)), config=config(mode, True)).cpu().numpy()
            routes = fuzzlib._delta(M.route_counts(), before)
            assert routes["dist_global_persistent"] > 0, routes
            want = reference(size, mode, True)[g]
            assert sum(differing(got[k], want) for k in range(reps)) == 0, mode


@pytest.mark.parametrize("table", [None, "quad_classes"], ids=["small_route", "quad_classes"])
def test_two_box_sizes_in_one_call_vs_oracle(table):
    """The per-glyph-box twins (k_distance_sized): glyph g in a 16 x 16 or a 24 x 16 box by turns, each framed for its own box, one generate_sized call."""
    a, b = W.GPU_SIZES[1], W.GPU_SIZES[2]
    names, shapes, xa = glyphs(a)
    xb = glyphs(b)[2]
    sizes = np.array([a if g % 2 == 0 else b for g in range(len(names))], np.int32)
    xfs = np.stack([xa[g] if g % 2 == 0 else xb[g] for g in range(len(names))])
    gb = batch(a)                                                          # (the same shapes at every size)
    with fuzzlib.tuned(fuzzlib.TUNINGS[table] if table else {}):
        for mode in MODES:
            for overlap in (True, False):
                n = M.CHANNELS[mode]
                out, off = gb.generate_sized(mode, sizes, xfs, config=config(mode, overlap))
                flat = out.cpu().numpy()
                bad = {}
                for g in range(len(names)):
                    size = a if g % 2 == 0 else b
                    bad[names[g]] = differing(flat[off[g]:off[g+1]].reshape(size[1], size[0], n), reference(size, mode, overlap)[g])
                assert not any(bad.values()), (mode, overlap, {k: v for k, v in bad.items() if v})


def test_single_shape_calls_vs_oracle():
    """The fused single-shape launch (k_single_call: the leader's survivor lists, bits included, are the team's): a needle of two contours, the Latin B
    and the CJK-like glyph at 24 x 16 through the drop-in signatures."""
    size = W.GPU_SIZES[2]
    names, shapes, xfs = glyphs(size)
    calls = {2: M.generate_psdf, 3: M.generate_msdf, 4: M.generate_mtsdf}
    for name in ("needle_diag", "B", "cjk"):
        g = names.index(name)
        for mode in MODES:
            for overlap in (True, False):
                one = np.zeros((size[1], size[0], M.CHANNELS[mode]), np.float32)
                calls[mode](one, shapes[g], M.SDFTransformation.from_xf(xfs[g]), config(mode, overlap))
                assert differing(one, reference(size, mode, overlap)[g]) == 0, (name, mode, overlap)
