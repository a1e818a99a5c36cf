"""The launch routes a batched generate call takes by the size of its launch, against the oracle (tests/fuzzlib.py).

planDistance, planCorrection and planSign (msdfgen_amd/csrc/msdf_launchplan.hpp; msdf_capi.hip's dispatchDistance, launchEc and launchSign execute their plans)
pick the kernels from the size of a launch: up to MSDFHIP_SMALL_LAUNCH_TILES
(8 192) tiles one tile per wavefront, beyond that three glyph classes on concurrent streams (one-contour, LDS scratch, global scratch; four tiles per
wavefront or one; the global class direct or persistent), heaviest-first correction order from 256 glyphs, whole tile rows in the sign pass from
nGlyphs x tilesY >= 4 096. The other sweeps are too small to leave the small route, so here (a) small groups run under MSDFHIP_* tables that force each
large route, and (b) throughput-sized groups run with no knobs at all. Every value is compared with the oracle, the route counters
(msdfhip_debug_route_counts) prove that the route under test ran."""
import numpy as np
import pytest

import msdfgen_amd as M
import fuzzlib

pytestmark = pytest.mark.gpu
TOL = 1e-5
SMALL = ("dist_small_simple", "dist_small_overlap")


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)
    info = M.device_info()
    assert info["arch"].startswith("gfx950"), info
    return info


def check_parity(r):
    print({k: v for k, v in r.items() if k != "group_routes"})
    assert r["max_abs_delta"] <= TOL, r["worst_case"]
    assert r["values_differing_bitwise"] <= r["values_compared"]*1e-6, r["worst_case"]      # the bound of test_fuzz_sweep_vs_oracle
    assert r["stencil_values_differing"] == 0, r
    assert r["path_values_differing"] == 0, r


# table -> (routes that must have run: each entry a tuple of counters of which at least one is nonzero; counters that must stay zero; run() arguments)
FORCED = {
    "quad_classes": ((("dist_one_quad",), ("dist_lds_quad",), ("dist_full_simple",)), SMALL+("dist_one_single", "dist_lds_single"), {}),
    "short_classes": ((("dist_one_single",), ("dist_lds_single",), ("dist_global_direct", "dist_global_persistent")), SMALL+("dist_one_quad", "dist_lds_quad"),
                      {}),
    "lds_class_tpw1": ((("dist_lds_single",), ("dist_one_quad",)), SMALL+("dist_lds_quad", "dist_one_single"), {}),
    "no_lds_class": ((("dist_global_direct", "dist_global_persistent"), ("dist_one_single", "dist_one_quad")), SMALL+("dist_lds_quad", "dist_lds_single"), {}),
    "wide_lds_class": ((("dist_lds_single", "dist_lds_quad"),), SMALL, {}),
    "persistent_grid": ((("dist_global_persistent",),), SMALL, {"scale": "full", "modes": (3, 4), "min_groups": 2, "n_shapes": 2000}),
    "serial_classes": ((("dist_one_single",), ("dist_lds_single",), ("dist_global_direct", "dist_global_persistent")), SMALL, {}),
    "query_lds": ((("ec_query_batch",),), ("ec_wide_slots",), {"modes": (3, 4), "min_groups": 12}),
    "query_policy": ((("ec_query_batch",),), (), {"modes": (3, 4), "min_groups": 12}),
    "query_counter": ((("ec_query_batch",),), (), {"modes": (3, 4), "min_groups": 12}),
    "sign_chunked": ((("sign_chunked",), ("sign_split",)), (), {"scanline": True, "min_groups": 8}),
}


@pytest.mark.parametrize("name", sorted(FORCED))
def test_forced_route_vs_oracle(name):
    """A bounded sweep of mixed-class groups (40-80 glyphs, every error-correction pair, both combiners, Y-down bitmaps, inverse-Y shapes, other
    deviation / improve ratios) under one of fuzzlib.TUNINGS, every value and every stencil byte against the oracle."""
    ran, idle, kw = FORCED[name]
    kw = dict(kw)
    args = {"n_shapes": kw.pop("n_shapes", 1200), "deadline_s": 8, "min_groups": kw.pop("min_groups", 4), "scale": kw.pop("scale", "mixed")}
    r = fuzzlib.run(seed=500+sorted(FORCED).index(name), tuning=fuzzlib.TUNINGS[name], stencil=True, **args, **kw)
    check_parity(r)
    assert r["groups"] >= args["min_groups"], r
    routes = r["routes"]
    for alternatives in ran:
        assert sum(routes[k] for k in alternatives) > 0, (name, alternatives, routes)
    for k in idle:
        assert routes[k] == 0, (name, k, routes)
    if name == "sign_chunked":
        assert r["fill_rules"] == [0, 1, 2, 3], r["fill_rules"]


def test_throughput_sized_groups_vs_oracle():
    """Groups of at least 256 glyphs and more than 8 192 tiles with no knobs: the glyph classes of one launch on their concurrent streams, the
    heaviest-first correction order, and (the scanline groups, nGlyphs x tilesY >= 4 096) the sign pass's whole-row spans, under every fill rule in turn.
    Every tile and stencil byte against the oracle; the same groups through generate_stream and HostBatch.generate_host (the pipeline's batch-order
    chunk views) must give the batch's bytes."""
    r = fuzzlib.run(6000, 601, deadline_s=45, min_groups=4, scale="full", scanline=True, modes=(3, 4), stencil=True, paths=True)
    check_parity(r)
    assert r["groups"] >= 4 and r["min_glyphs_per_group"] >= 256 and r["min_tiles_per_group"] > 8192, r
    routes = r["routes"]
    assert routes["ec_query_heaviest"] > 0 and routes["sign_whole_rows"] > 0, routes
    assert all(g["dist_small_simple"] == g["dist_small_overlap"] == 0 for g in r["group_routes"]), r["group_routes"]
    three = [g for g in r["group_routes"] if g["dist_one_quad"]+g["dist_one_single"] > 0 and g["dist_lds_quad"]+g["dist_lds_single"] > 0 and
             g["dist_global_direct"]+g["dist_global_persistent"] > 0]
    assert three, r["group_routes"]
    assert r["path_values_compared"] > 0 and r["stencil_values_compared"] > 0, r


# sdfZeroValue levels of the sign pass: off the middle, on the edge of and outside [0, 1], and one (1/3 as a float) whose doubling and mirroring round
ZERO_VALUES = (.25, .75, 0., float(np.float32(1/3)), 1.5)


def check_zero_levels(r):
    check_parity(r)
    assert r["zero_values"] == sorted(ZERO_VALUES), r["zero_values"]
    assert r["fill_rules"] == [0, 1, 2, 3], r["fill_rules"]
    assert r["stencil_values_compared"] > 0, r


def test_sign_pass_zero_levels_chunked_and_split_vs_oracle():
    """The -scanline flow with the field's zero level moved off .5 (an asymmetric Range) and that level handed to the sign pass, under MSDFHIP_SIGN_CAP=3:
    the row lists walked in chunks, the tile rows split into spans. k_sign_correction mirrors about zero+zero and votes against zero; a kernel or a
    dispatch path that kept .5 differs from the oracle at every flipped texel."""
    r = fuzzlib.run(1200, 520, min_groups=10, deadline_s=1, scale="mixed", scanline=True, stencil=True, modes=(1, 3, 4), tuning=fuzzlib.TUNINGS["sign_chunked"],
                    zero_values=ZERO_VALUES)
    check_zero_levels(r)
    assert r["routes"]["sign_chunked"] > 0 and r["routes"]["sign_split"] > 0, r["routes"]


def test_sign_pass_zero_levels_whole_rows_vs_oracle():
    """The same with no knobs at the size from which the sign pass keeps whole tile rows per wavefront (nGlyphs x tilesY >= 4 096): the scanline groups
    of the throughput-sized plan, 456-520 glyphs of nine tile rows, the smallest that plan has."""
    r = fuzzlib.run(6000, 602, min_groups=10, deadline_s=1, scale="full", scanline=True, stencil=True, modes=(1, 3, 4), zero_values=ZERO_VALUES)
    check_zero_levels(r)
    assert r["routes"]["sign_whole_rows"] > 0, r["routes"]
    scan = [g for g in r["group_routes"] if g["sign_whole_rows"]+g["sign_split"] > 0]
    assert len(scan) >= len(ZERO_VALUES) and all(g["sign_whole_rows"] > 0 and g["sign_split"] == 0 for g in scan), scan
