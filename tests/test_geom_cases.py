"""The outline families of tests/geomcases.py on the CPU: their premises, the plain-C oracle against the compiled reference (where oracle/_ref exists),
and the device headers compiled for the host (tests/emu.py) against the oracle. This is what makes the oracle a valid reference for
tests/test_gpu_geometry.py on these inputs.

The oracle equals, bit for bit and under every setting, the reference built with UNCACHED distance queries (oracle/_ref/libmsdfgen_ref_exact.so,
the rules in oracle/Makefile): the distance check of its error correction, and the query of generateDistanceField. The reference as it stands keeps
per-edge caches and the previous minimum in the ShapeDistanceFinder behind both, and on tied or coincident outlines the cached walk returns something
else than a fresh walk: under ALWAYS_CHECK_DISTANCE a few texels per bitmap come out differently; the generator's walk shows on one case (GENERATOR_WALK). tests/golden/geometry_departures.json (tools/make_golden_geometry.py) lists them,
with both builds' bits; the literal comparison below allows exactly that list, and under the other distance-check modes only GENERATOR_WALK's two cases."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import geomcases as G
from conftest import GOLDEN, assert_bit_equal
from msdfgen_amd import synth
from msdfgen_amd.shape import autoframe

EC_PAIRS = G.EC_PAIRS
# The one place where the GENERATOR's cached walk shows, in every mode and setting: the closed one-edge cubic loop at the two larger sizes. One texel
# next to the loop's axis gets, from the reference as it stands, the previous texel's distance widened by 1.001 x the step (the selector's reset())
# because the cubic's own iterated distance there is larger than that bound; the uncached build and the oracle give the cubic's distance.
GENERATOR_WALK = {"degenerate_edges/cubic_loop@41x27", "degenerate_edges/cubic_loop@64x64"}


@pytest.fixture(scope="module")
def emu():
    from emu import Emu
    return Emu()


@pytest.fixture(scope="module")
def exact():
    """The reference with the uncached distance queries. Skipped only where the compiled reference is absent altogether, as `ref` is; an oracle/_ref
    from before this build existed gets it built (where the reference's sources are) or fails."""
    from oracle.pyoracle import Ref
    if not Ref.available() and not Ref.available(exact=True):
        pytest.skip("oracle/_ref/libmsdfgen_ref.so not present")
    return Ref(exact=True)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "geometry_departures.json")) as f:
        doc = json.load(f)["cases"]
    return {name: {key: d["entries"][i] for key, i in d["settings"].items()} for name, d in doc.items()}      # settings with equal lists share an entry


def _ordinary(c, k):
    """The case turned into what every other sweep feeds: a synth glyph under autoframe."""
    s = synth.random_shape(7000+k, n_contours=2+k % 3, kinds=(1, 2, 3), holes=bool(k & 1))
    return c._replace(shape=s, w=32, h=32, xf=autoframe(s.bounds(), 32, 32, 2.))


@pytest.mark.parametrize("family", G.FAMILIES)
def test_family_premises(oracle, family):
    cs = G.cases((family,), seeds=(0, 1, 2))
    assert len(cs) >= 12
    for k, c in enumerate(cs):
        G.check_premise(c, oracle)
        with pytest.raises(AssertionError):                           # the ordinary glyph is not a member of any family
            G.check_premise(_ordinary(c, k), oracle)
    assert {c.y_down for c in cs} == {False, True}
    assert all(G.base_name(c) in G.MIN_COUNT for c in cs) or family in ("degenerate_edges", "sparse_colours", "slivers")


def test_jitter_keeps_the_lattice(oracle):
    """The moves fuzzlib's geometry= applies are exact: the premise count of a jittered case is the count of the case itself."""
    for fam in ("lattice_ties", "on_outline", "scanline_hits"):
        base = {c.name: G.premise_count(c, oracle) for c in G.cases((fam,)) if c.w*c.h <= 1024}
        for sd in (1, 2, 3):
            for c in G.cases((fam,), seeds=(sd,)):
                if G.base_name(c) in base:
                    assert G.premise_count(c, oracle) == base[G.base_name(c)], c.name


def test_geometry_sweep_plan_keeps_the_premises(oracle):
    """fuzzlib.plan(geometry=...): every glyph of every group is still a member of its family after the jitter, all families, all three size classes
    and all twelve correction settings occur, and the default sweep's plan does not change by it (tests/test_fuzz_plan.py pins that one)."""
    import fuzzlib
    groups = list(fuzzlib.plan(900, 7, geometry=list(G.FAMILIES)))
    assert {g["family"] for g in groups} == set(G.FAMILIES) and {g["ec"] for g in groups} == set(fuzzlib.EC_PAIRS)
    assert {(g["w"], g["h"]) for g in groups} >= set(G.BIG_SIZES) and any(g["w"]*g["h"] <= 256 for g in groups)
    for g in groups:
        assert len(g["shapes"]) == g["n"] == len(g["names"]) and g["xfs"].shape == (g["n"], 6)
        for name, s, xf in zip(g["names"], g["shapes"], g["xfs"]):
            assert name.startswith(g["family"]+"/") and G.base_name(G.Case(name, s, 0, 0, xf, False)) not in G.SIGN_NOISE
            if s.n_edges <= 32 and g["w"]*g["h"] <= 41*27:
                G.check_premise(G.Case(name, s, g["w"], g["h"], xf, g["y_down"]), oracle)


def test_larger_bitmaps_keep_the_premises_and_leave_the_single_tile(oracle):
    """Every family at 41x27 and 64x64 with a dyadic scale; among them lattice_ties and coincident cases of six contours and one of more than 128 edges."""
    for w, h in G.BIG_SIZES:
        cs = G.cases(w=w, h=h)
        assert {c.name.split("/")[0] for c in cs} == set(G.FAMILIES)
        for c in cs:
            assert (c.w, c.h) == (w, h)
            s = c.xf[0]
            assert "offgrid" in c.name or (s == c.xf[1] and np.frexp(s)[0] == .5), c.name       # a power of two
            if c.shape.n_edges <= 32:
                G.check_premise(c, oracle)
    big = G.cases(("lattice_ties", "coincident"), w=64, h=64)
    G.check_premise([c for c in big if "grid_6x6" in c.name][0], oracle)
    assert any(c.shape.n_contours >= 6 for c in big if c.name.startswith("lattice_ties"))
    assert any(c.shape.n_contours >= 6 for c in big if c.name.startswith("coincident"))
    assert any(c.shape.n_edges > 128 for c in big)


def _family(cs, family):
    return [c for c in cs if c.name.startswith(family+"/")]


@pytest.mark.parametrize("family", G.FAMILIES)
def test_oracle_matches_reference_on_outline_families(oracle, ref, exact, recorded, family):
    """Four modes, both combiners, Y up and down, all twelve correction settings, stencils compared: the oracle equals the exact-check build everywhere;
    it equals the reference as it stands everywhere but on the recorded texels, all of which are under ALWAYS_CHECK_DISTANCE or in GENERATOR_WALK."""
    seen = 0
    for c in _family(G.reference_cases(), family):
        rec = recorded.get(c.name, {})
        for key, kw in G.settings():
            o, so = G.generate(oracle, c, **kw)
            e, se = G.generate(exact, c, **kw)
            what = "%s %s" % (c.name, key)
            assert_bit_equal(o, e, what+", exact-check reference")
            assert so is None or (so == se).all(), what+": stencil, exact-check reference"
            a, sa = G.generate(ref, c, **kw)
            r = rec.get(key)
            if r is None or (kw["ec_dist"] != G.ALWAYS_CHECK and c.name not in GENERATOR_WALK):
                assert_bit_equal(o, a, what)
                assert so is None or (so == sa).all(), what+": stencil"
                continue
            seen += 1
            at = G.differing(o, a)
            assert at.tolist() == r["at"], what+": the reference departs at %s, recorded %s" % (at.tolist(), r["at"])
            assert a.view(np.uint32).ravel()[at].tolist() == r["literal"] and o.view(np.uint32).ravel()[at].tolist() == r["exact"], what
            if so is None:
                assert not r["stencil_at"], what
                continue
            st = np.flatnonzero(so.ravel() != sa.ravel())
            assert st.tolist() == r["stencil_at"], what+": stencil"
            assert sa.ravel()[st].tolist() == r["stencil_literal"] and so.ravel()[st].tolist() == r["stencil_exact"], what+": stencil"
    assert seen == sum(len(v) for k, v in recorded.items() if k.startswith(family+"/")), "recorded settings that no longer occur"


def test_recorded_departures_are_all_under_always_check_distance(recorded):
    """What DESIGN.md 4 and the README state from this fixture."""
    assert recorded and all(key.endswith("/%d" % G.ALWAYS_CHECK) for name, d in recorded.items() for key in d if name not in GENERATOR_WALK)
    assert GENERATOR_WALK <= set(recorded)
    assert all(1 <= len(v["at"])+len(v["stencil_at"]) for d in recorded.values() for v in d.values())
    assert max(len(v["at"]) for d in recorded.values() for v in d.values()) <= 8        # at most 8 values of one bitmap (grid_6x6)
    assert {k.split("/")[0] for k in recorded} <= set(G.FAMILIES)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_oracle_standalone_passes_match_reference_on_outline_families(oracle, ref, exact, family):
    """msdfErrorCorrection on an uncorrected field, its stages, distanceSignCorrection and rasterize under four fill rules, estimateSDFError with 1 and 3
    scanlines per row, oneShotDistance at the texel centres and vertices, and the contour windings."""
    for i, c in enumerate(_family(G.cases()+G.cases(w=41, h=27), family)):
        for mode in (3, 4):
            pre = oracle.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
            ov = bool(i & 1)
            for ec, dc in ((2, 1), (1, 2), (3, 0), (2, 2)):
                kw = dict(overlap=ov, ec_mode=ec, ec_dist=dc, y_down=c.y_down)
                sa, sb, se = (np.zeros((c.h, c.w), np.uint8) for _ in range(3))
                a = ref.error_correction(c.shape, pre, c.xf, stencil=sa, **kw)
                b = oracle.error_correction(c.shape, pre, c.xf, stencil=sb, **kw)
                e = exact.error_correction(c.shape, pre, c.xf, stencil=se, **kw)
                what = "%s error_correction mode %d ec %d/%d" % (c.name, mode, ec, dc)
                assert_bit_equal(b, e, what+", exact-check reference")
                assert (sb == se).all(), what
                if dc != G.ALWAYS_CHECK:
                    assert_bit_equal(b, a, what)
                    assert (sa == sb).all(), what
                # (under ALWAYS_CHECK_DISTANCE the literal build departs like generate's does; the generate comparison records those texels)
            assert (oracle.ec_stages(c.shape, pre, c.xf, overlap=ov) == ref.ec_stages(c.shape, pre, c.xf, overlap=ov)).all(), c.name+": ec_stages"
        for mode in (1, 3):
            field = oracle.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
            for rule in range(4):
                assert_bit_equal(oracle.sign_correction(c.shape, field, c.xf, .5, rule, y_down=c.y_down),
                                 ref.sign_correction(c.shape, field, c.xf, .5, rule, y_down=c.y_down), "%s sign correction rule %d" % (c.name, rule))
            for spr, rule in ((1, 0), (3, 1)):
                a, b = ref.estimate_sdf_error(c.shape, field, c.xf, spr, rule), oracle.estimate_sdf_error(c.shape, field, c.xf, spr, rule)
                assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64), (c.name, spr, rule, a, b)
        for rule in range(4):
            assert_bit_equal(oracle.rasterize(c.shape, c.w, c.h, c.xf, rule, y_down=c.y_down), ref.rasterize(c.shape, c.w, c.h, c.xf, rule, y_down=c.y_down),
                             "%s rasterize rule %d" % (c.name, rule))
        if family == "sparse_colours" or i % 4 == 0:                  # renderSDF, from uncorrected fields too: channels without an edge are not finite
            for mode, n_outs, ec in ((1, (1, 3), 0), (3, (1, 3), 0), (4, (1, 4), 0), (3, (3,), 2)):
                src = oracle.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=ec)
                for n_out in n_outs:
                    for ow, oh in ((c.w, c.h), (2*c.w+1, 2*c.h-1), (7, 5)):
                        for lo, hi, thr in ((0, 0, .5), (-2, 2, .5), (2, -2, .5), (-1, 3, .4)):
                            assert_bit_equal(oracle.render_sdf(src, ow, oh, n_out, lo, hi, thr), ref.render_sdf(src, ow, oh, n_out, lo, hi, thr),
                                             "%s renderSDF %d<-%d %dx%d (%g, %g)" % (c.name, n_out, mode, ow, oh, lo, hi))
        pts = G.tie_points(c)
        for sel in (1, 2, 3, 4):
            for ov in (True, False):
                assert_bit_equal(oracle.shape_distance(c.shape, sel, ov, pts), ref.shape_distance(c.shape, sel, ov, pts), "%s oneShotDistance %d %d" % (c.name, sel, ov))
        h = ref.shape_from_flat(c.shape)
        want = ref.flatten(h).windings
        ref.free(h)
        assert (oracle.windings(c.shape) == want).all(), c.name+": windings"


@pytest.mark.parametrize("family", G.FAMILIES)
def test_host_build_of_the_kernels_matches_oracle_on_outline_families(oracle, emu, family):
    """The kernels' device headers compiled for the host against the oracle: generate with the tile cull and the correction (every setting over a
    family, stencils), the sign pass, rasterize, the error estimate, the cooperative psdf query in both forms and the shape distance in both forms
    of the overlapping combiner, at the texel centres and vertices. In the larger lattice_ties cases the cull must really drop edges, or its
    exact comparisons at the cull bound are not under test."""
    kept, total = C.c_long(), C.c_long()
    for i, c in enumerate(_family(G.reference_cases(), family)):
        emu.lib.emu_cull_stats(C.byref(kept), C.byref(total), 1)
        native = "@" not in c.name
        for ov in (True, False):
            for mode in (1, 2):
                for yd in (False, True):
                    a = oracle.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, y_down=yd)
                    b = emu.generate(c.shape, mode, c.w, c.h, c.xf, overlap=ov, y_down=yd)
                    assert_bit_equal(b, a, "%s mode %d overlap %d y_down %d" % (c.name, mode, ov, yd))
            for mode in (3, 4):
                pairs = EC_PAIRS if native else [EC_PAIRS[(4*i+3*k+mode+ov) % 12] for k in range(3)]+[(2, 2)]
                for ec, dc in pairs:
                    sa, sb = np.zeros((c.h, c.w), np.uint8), np.zeros((c.h, c.w), np.uint8)
                    kw = dict(overlap=ov, ec_mode=ec, ec_dist=dc, y_down=c.y_down)
                    a = oracle.generate(c.shape, mode, c.w, c.h, c.xf, stencil=sa, **kw)
                    b = emu.generate(c.shape, mode, c.w, c.h, c.xf, stencil=sb, **kw)
                    what = "%s mode %d overlap %d ec %d/%d" % (c.name, mode, ov, ec, dc)
                    assert_bit_equal(b, a, what)
                    assert ((sa[::-1] if c.y_down else sa) == sb).all(), what+": stencil"     # the host build keeps the bitmap's memory rows
        emu.lib.emu_cull_stats(C.byref(kept), C.byref(total), 1)
        assert 0 < kept.value <= total.value
        if family == "lattice_ties" and c.w*c.h >= 41*27:
            print("cull %s: kept %d of %d" % (c.name, kept.value, total.value))
            if c.shape.n_edges >= 16:                               # (a glyph of a few edges next to every tile keeps them all)
                assert kept.value < total.value, (c.name, kept.value, total.value)
            if c.shape.n_edges > 128:
                assert kept.value < .8*total.value, (c.name, kept.value, total.value)     # the bound of test_xform_cases.py
        if not native:
            continue
        for mode in (1, 3):
            field = oracle.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
            for rule in range(4):
                assert_bit_equal(emu.sign_correction(c.shape, field, c.xf, .5, rule, y_down=c.y_down),
                                 oracle.sign_correction(c.shape, field, c.xf, .5, rule, y_down=c.y_down), "%s sign correction rule %d" % (c.name, rule))
            for spr, rule in ((1, 0), (3, 1)):
                a, b = oracle.estimate_sdf_error(c.shape, field, c.xf, spr, rule), emu.estimate_sdf_error(c.shape, field, c.xf, spr, rule)
                assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64), (c.name, spr, rule, a, b)
        for rule in range(4):
            assert_bit_equal(emu.rasterize(c.shape, c.w, c.h, c.xf, rule, y_down=c.y_down), oracle.rasterize(c.shape, c.w, c.h, c.xf, rule, y_down=c.y_down),
                             "%s rasterize rule %d" % (c.name, rule))
        pts = G.tie_points(c)
        if family == "lattice_ties":                                  # the query points are tied points: part of the premise
            assert len(G.tie_texels(oracle, c, pts)) >= G.MIN_COUNT[G.base_name(c)], c.name
        for ov in (True, False):
            want = oracle.shape_distance(c.shape, 2, ov, pts)[:, 0]
            assert_bit_equal(emu.psdf_cooperative(c.shape, ov, pts), want, "%s cooperative psdf overlap %d" % (c.name, ov))
            assert_bit_equal(emu.psdf_cooperative(c.shape, ov, pts, slotted=True), want, "%s slotted cooperative psdf overlap %d" % (c.name, ov))
        for form in (0, 1):
            emu.set_combiner_form(form)
            try:
                for sel in (1, 2, 3, 4):
                    for ov in (True, False):
                        assert_bit_equal(emu.shape_distance(c.shape, sel, ov, pts), oracle.shape_distance(c.shape, sel, ov, pts),
                                         "%s shape distance selector %d overlap %d form %d" % (c.name, sel, ov, form))
                if c.shape.n_contours > 1:
                    assert_bit_equal(emu.generate(c.shape, 3, c.w, c.h, c.xf, ec_mode=0), oracle.generate(c.shape, 3, c.w, c.h, c.xf, ec_mode=0),
                                     "%s msdf, combiner form %d" % (c.name, form))
            finally:
                emu.set_combiner_form(0)


def _same_shape(a, b, what):
    assert (np.asarray(a.contour_offsets) == np.asarray(b.contour_offsets)).all(), what+": contour offsets"
    assert (np.asarray(a.types) == np.asarray(b.types)).all(), what+": edge types"
    assert (np.asarray(a.colors) == np.asarray(b.colors)).all(), what+": colours"
    assert_bit_equal(np.asarray(a.points, np.float64), np.asarray(b.points, np.float64), what+": points")


@pytest.mark.parametrize("family", ("degenerate_edges", "coincident", "lattice_ties"))
def test_shape_preparation_on_outline_families(oracle, ref, emu, family):
    """Shape::normalize and both colourings on the stripped outlines: exact 90 and 180 degree corners sit on the angle threshold's comparisons, and
    one-edge and two-edge contours take normalize's split paths. The oracle against the reference and against the host build of the device's
    lanes = edges form."""
    for c in G.cases((family,)):
        raw = G.strip_colours(c.shape)
        for normalize, coloring in ((True, 0), (True, 1), (True, 2), (False, 1)):
            for seed in (0, 1, 12345678901):
                if coloring == 0 and seed:
                    continue
                for angle in (3.0, 1.0):
                    what = "%s normalize %d colouring %d seed %d angle %g" % (c.name, normalize, coloring, seed, angle)
                    want = oracle.shape_prepare(raw, normalize, coloring, angle, seed)
                    _same_shape(want, ref.shape_prepare(raw, normalize, coloring, angle, seed), what+", reference")
                    _same_shape(want, emu.shape_prepare(raw, normalize, coloring, angle, seed, wave=True), what+", host build")
