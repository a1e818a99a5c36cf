"""The launch plans of msdfgen_amd/csrc/msdf_launchplan.hpp -- what msdf_capi.hip's dispatchDistance, launchEc and launchSign execute -- compiled with the
host compiler (tests/hostemu; binding: tests/launchplan.py): invariants on seeded random glyph ranges under every tuning table, every threshold pinned from
both sides, the routes of the forced tables of tests/test_gpu_routes.py, and the planners in a stand-alone program under the address and
undefined-behaviour sanitizers. No GPU."""
import os
import subprocess

import numpy as np
import pytest

from emu import Emu
import fuzzlib
import launchplan as L
from test_class_plan_host import glyph_set
from test_ec_lazy_host import _sanitizers_link
from test_gpu_routes import FORCED

LDS_LIMIT = 160*1024
NCH = L.CHANNELS
TABLES = dict(fuzzlib.TUNINGS, defaults={})
CLASSES_ON = {"MSDFHIP_SMALL_LAUNCH_TILES": "0"}                              # no launch counts as small: the classes' own thresholds decide


@pytest.fixture(scope="module")
def emu():
    return Emu()


def slots(env, waves):
    return int(L.env_field(env, "cus"))*4*waves


def check_invariants(env, p, n, what):
    limit, budget = L.env_field(env, "ldsLimit"), L.env_field(env, "resLdsBudget")
    launches = p["launches"]
    assert not p["too_complex"], what
    # the culled launches and the list-free one cover the glyphs exactly once
    whole = [l for l in launches if not l["mapped"]]+([p] if p["unculled"] and not p["unculled_mapped"] else [])
    if whole:
        assert len(launches)+p["unculled"] == 1, what
        assert (whole[0]["count"] if launches else p["unculled_count"]) == n, what
    else:
        assert p["order"] is not None and sorted(p["order"].tolist()) == list(range(n)), what
        covered = np.zeros(n, int)
        for l in launches:
            assert l["count"] > 0, what
            covered[l["offset"]:l["offset"]+l["count"]] += 1
        if p["unculled"]:
            assert p["unculled_offset"] == n-p["n_huge"] and p["unculled_count"] == p["n_huge"] > 0, what
            covered[p["unculled_offset"]:p["unculled_offset"]+p["unculled_count"]] += 1
        assert (covered == 1).all(), (what, covered.tolist())
    for l in launches:
        assert l["lds_bytes"] <= limit, (what, l)
        assert (l["overlap"], l["gres"], l["tpw"]) in ((0, 1, 1), (0, 0, 4), (1, 1, 1), (1, 0, 4), (1, 0, 1)), (what, l)   # the instantiations k_distance has
        if l["overlap"] and not l["gres"]:
            assert l["res_bytes"]+l["idx_bytes"] <= budget, (what, l)
        if l["persistent"]:
            assert l["route"] == "dist_global_persistent" and l["chunk"] <= slots(env, 4), (what, l)
            if L.env_field(env, "persistentGrid") > 0:
                assert l["chunk"] <= L.env_field(env, "persistentGrid"), (what, l)
        elif l["gres_bytes"]:
            assert l["chunk"]*l["res_bytes"] <= L.GRES_WORKSPACE_CAP or l["chunk"] == 256, (what, l)
            assert l["route"] != "dist_global_persistent", (what, l)
        if l["route"] in ("dist_lds_quad", "dist_lds_single"):
            assert l["stream"] == L.STREAM_CALLER, (what, l)
    side = [l["stream"] for l in launches if l["stream"] != L.STREAM_CALLER]
    assert len(set(side)) == len(side), (what, side)
    if p["concurrent"]:
        assert not L.env_field(env, "serialClasses") and len(launches) > 1 and side, what
    else:
        assert not side and not p["ec_ahead"] and not p["unculled_after_join"], what
    if p["ec_ahead"]:
        assert L.STREAM_SIDE1 in side, what


@pytest.mark.parametrize("cus", [256, 64])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_distance_plan_invariants_on_random_glyph_ranges(emu, table, cus):
    """Class mixes of test_class_plan_host.glyph_set (every class boundary, oversized glyphs included) and random subsets of them, bitmaps of 1..200 texels a side,
    the four field types, both combiners."""
    env = L.plan_env(emu, TABLES[table], cus=cus)
    rng = np.random.default_rng([sorted(TABLES).index(table), cus])
    concurrent = planned = 0
    for case in range(24):
        mode, overlap = int(rng.integers(1, 5)), bool(case & 1)
        limit = max(L.overlap_class_limit(emu, env, NCH[mode]), 1)
        c, e = glyph_set(limit, int(L.env_field(env, "smallMaxEdges")), LDS_LIMIT, 1000+case)
        keep = rng.permutation(len(c))[:int(rng.choice([1, 2, 7, 60, len(c)]))]
        if case % 3 == 0:                                                     # without the oversized glyphs: every range size also on the culled-only paths
            keep = keep[(e[keep]+4*c[keep]+2)*4 <= LDS_LIMIT]
            if not len(keep):
                continue
        c, e = c[keep], e[keep]
        w, h = int(rng.integers(1, 201)), int(rng.integers(1, 201))
        what = (table, cus, case, mode, overlap, w, h, len(c))
        p = L.plan_distance(emu, env, c, e, w, h, mode, overlap, want_ec_ahead=mode >= 3)
        if p["too_complex"]:                                                  # refused as a whole: the plan names the LDS it would have needed, and launches nothing
            assert p["refused_bytes"] > LDS_LIMIT, what
            continue
        check_invariants(env, p, len(c), what)
        planned += 1
        concurrent += p["concurrent"]
        serial = L.plan_distance(emu, env, c, e, w, h, mode, overlap, serial_batch=True)
        assert not serial["concurrent"] and [l["route"] for l in serial["launches"] if l["route"][:11] != "dist_global"] == \
            [l["route"] for l in p["launches"] if l["route"][:11] != "dist_global"], what
    assert planned >= 12
    if table in ("short_classes", "quad_classes", "wide_lds_class", "persistent_grid"):
        assert concurrent > 0, "no case ran its classes concurrently"
    if table == "serial_classes":
        assert concurrent == 0


def routes(p):
    return [l["route"] for l in p["launches"]]+["dist_unculled"]*p["unculled"]


def test_small_launch_thresholds(emu):
    env = L.plan_env(emu)
    one = lambda n: (np.ones(n, int), np.full(n, 10))
    assert L.launch_shape(emu, env, 128, 1, 10, 64, 64, 3) == {"huge_batch": False, "small_launch": True}      # 128 x 64 tiles = smallLaunchTiles
    assert L.launch_shape(emu, env, 129, 1, 10, 57, 64, 3) == {"huge_batch": False, "small_launch": False}
    assert routes(L.plan_distance(emu, env, *one(128), 64, 64, 3, False)) == ["dist_small_simple"]
    assert routes(L.plan_distance(emu, env, *one(129), 64, 64, 3, False)) == ["dist_full_simple"]
    # the combiner scratch of a small overlapping launch: 8 192 tiles x 16 contours x 512 B = 64 MB
    assert L.launch_shape(emu, env, 128, 16, 99, 64, 64, 1)["small_launch"] and not L.launch_shape(emu, env, 128, 17, 99, 64, 64, 1)["small_launch"]
    assert L.launch_shape(emu, env, 128, 17, 99, 64, 64, 1, bound_scratch=False)["small_launch"]
    c, e = np.array([16]+[2]*127), np.full(128, 99)
    assert routes(L.plan_distance(emu, env, c, e, 64, 64, 1, True)) == ["dist_small_overlap"]
    c[0] = 17
    assert routes(L.plan_distance(emu, env, c, e, 64, 64, 1, True)) == ["dist_global_direct", "dist_lds_single"]
    # the list built ahead of a pipeline chunk: only where the classes will run, and by the tile count alone
    assert L.class_list_limit(emu, env, 128, 17, 99, 64, 64, 1, True) == 15 and L.class_list_limit(emu, env, 128, 17, 99, 64, 64, 1, True, ahead=True) == 0
    assert L.class_list_limit(emu, env, 129, 17, 99, 64, 64, 1, True, ahead=True) == 15
    assert L.class_list_limit(emu, env, 129, 17, 99, 64, 64, 1, False, ahead=True) == L.class_list_limit(emu, env, 129, 1, 99, 64, 64, 1, True) == 0
    assert L.class_list_limit(emu, env, 1, 17, 99, 200, 200, 1, True) == 0


def test_short_and_persistent_round_thresholds(emu):
    env = L.plan_env(emu, CLASSES_ON, cus=64)                                 # 64 CUs: 1 024 slots at 4 waves per SIMD, 1 280 at 5; 64 tiles = 16 quads a glyph
    lds_class = lambda n: L.plan_distance(emu, env, np.full(n, 2), np.full(n, 10), 64, 64, 3, True)["launches"]
    assert [(l["route"], l["tpw"]) for l in lds_class(255)] == [("dist_lds_single", 1)]          # 255 x 16 < shortRounds (4) x 1 024
    assert [(l["route"], l["tpw"]) for l in lds_class(256)] == [("dist_lds_quad", 4)]
    mixed = lambda n: L.plan_distance(emu, env, np.array([1]*n+[2]), np.full(n+1, 10), 64, 64, 3, True)["launches"]
    assert [(l["route"], l["gres"], l["tpw"]) for l in mixed(319)][-1] == ("dist_one_single", 1, 1)   # 319 x 16 < 4 x 1 280
    assert [(l["route"], l["gres"], l["tpw"]) for l in mixed(320)][-1] == ("dist_one_quad", 0, 4)
    rest = lambda n: L.plan_distance(emu, env, np.full(n, 9), np.full(n, 40), 64, 64, 3, True)["launches"]
    (a,), (b,) = rest(127), rest(128)                                         # 128 x 64 tiles = persistentRounds (8) x 1 024
    assert (a["route"], a["persistent"], a["chunk"]) == ("dist_global_direct", 0, 127*64)
    assert (b["route"], b["persistent"], b["chunk"], b["gres_bytes"]) == ("dist_global_persistent", 1, 1024, 1024*9*3*512)


def test_distance_grid(emu):
    env, fixed = L.plan_env(emu), L.plan_env(emu, {"MSDFHIP_PERSISTENT_GRID": "40"})
    grid = lambda *a, e=env: L.plan_distance_grid(emu, e, *a)
    assert grid(5000, 0, 4096) == {"persistent": False, "chunk": 5000, "gres_bytes": 0}
    assert grid(8*4096-1, 1536, 4096)["persistent"] is False and grid(8*4096, 1536, 4096) == {"persistent": True, "chunk": 4096, "gres_bytes": 4096*1536}
    # a share of the slots: only a grid below the slots and below the launch
    assert grid(1000, 1536, 4096, 600) == {"persistent": True, "chunk": 600, "gres_bytes": 600*1536}
    assert not grid(600, 1536, 4096, 600)["persistent"] and not grid(5000, 1536, 4096, 4096)["persistent"] and grid(5000, 1536, 4096, 4095)["persistent"]
    assert grid(1000, 1536, 4096, 600, e=fixed)["chunk"] == 40 and grid(1000, 1536, 4096, 30, e=fixed)["chunk"] == 30
    assert not grid(0xffffffff-8*4096, 1536, 4096)["persistent"] and grid(0xffffffff-8*4096-1, 1536, 4096)["persistent"]
    # direct: pieces of at most 1 GB of workspace, at least 256 workgroups
    assert grid(3000, 1 << 20, 4096)["chunk"] == 1024 and grid(3000, 8 << 20, 4096)["chunk"] == 256 and grid(100, 8 << 20, 4096)["chunk"] == 100


def test_oversized_glyphs(emu):
    env = L.plan_env(emu)
    over = LDS_LIMIT//4                                                       # edges + 4 contours + 2 > over: the survivor lists exceed the LDS
    fits, huge = (3, over-4*3-2), (3, over-4*3-1)
    p = L.plan_distance(emu, env, [fits[0]], [fits[1]], 40, 40, 3, True)
    assert routes(p) == ["dist_small_overlap"] and p["launches"][0]["lds_bytes"] == LDS_LIMIT
    for overlap, contours in ((True, 3), (False, 3), (True, 1)):
        p = L.plan_distance(emu, env, [contours], [huge[1]+8], 40, 40, 3, overlap)
        assert routes(p) == ["dist_unculled"] and not p["unculled_mapped"] and p["unculled_count"] == 1 and p["unculled_overlap"] == (overlap and contours > 1)
    p = L.plan_distance(emu, env, [3, 1, 9], [huge[1], over, over+77], 40, 40, 3, True)          # all oversized
    assert routes(p) == ["dist_unculled"] and not p["unculled_mapped"] and p["unculled_count"] == 3
    # one oversized glyph, and two that fit alone while the maxima of the two (edges of one, contours of the other) do not: the whole batch list-free
    p = L.plan_distance(emu, env, [1, 2000, 1], [over-6, 2000, over+50], 24, 24, 3, True)
    assert routes(p) == ["dist_unculled"] and not p["unculled_mapped"] and p["unculled_count"] == 3 and p["class_limit"] == 5
    p = L.plan_distance(emu, env, [1, 2000, 1], [over-6-8000, 2000, over+50], 24, 24, 3, True)   # ... and do: the oversized one alone, after the others
    assert routes(p) == ["dist_global_direct", "dist_one_single", "dist_unculled"] and p["unculled_mapped"] and (p["unculled_offset"], p["unculled_count"]) == (2, 1)
    assert p["unculled_after_join"] and p["concurrent"]
    check_invariants(env, p, 3, "mixed")
    p = L.plan_distance(emu, env, [1, 1, 1], [30, 20, over+50], 24, 24, 3, False)                # the simple combiner: the culled ones through the map
    assert routes(p) == ["dist_full_simple", "dist_unculled"] and p["launches"][0]["mapped"] and p["launches"][0]["count"] == 2 and not p["unculled_overlap"]


def class_limit_restated(budget, nch, small_max_edges, tpw):
    limit = 0
    while (limit+1)*nch*64*8+tpw*(small_max_edges+(limit+1)+2)*4 <= budget:
        limit += 1
    return limit


def test_overlap_class_limit(emu):
    assert [L.overlap_class_limit(emu, L.plan_env(emu), nch) for nch in (1, 3, 4)] == [15, 5, 3]       # msdf: COST_LDS_MAX_CONTOURS of msdf_classplan.hpp
    for budget in (0, 10240, 53248):
        for table in ({}, {"MSDFHIP_LDS_CLASS_TPW": "1"}, {"MSDFHIP_SMALL_MAX_EDGES": "160"}):
            env = L.plan_env(emu, dict(table, MSDFHIP_RES_LDS_BUDGET=str(budget)))
            for nch in (1, 3, 4):
                want = class_limit_restated(budget, nch, int(L.env_field(env, "smallMaxEdges")), int(L.env_field(env, "ldsClassTpw")))
                assert L.overlap_class_limit(emu, env, nch) == want, (budget, table, nch)
    zero = L.plan_env(emu, {"MSDFHIP_RES_LDS_BUDGET": "0"})
    assert L.overlap_class_limit(emu, zero, 3) == 0 and L.class_list_limit(emu, zero, 60, 4, 40, 99, 99, 3, True) == 1
    assert L.overlap_class_limit(emu, L.plan_env(emu, fuzzlib.TUNINGS["wide_lds_class"]), 3) == 32


def test_correction_plan(emu):
    env = L.plan_env(emu)
    ec = lambda *a, e=env, **k: L.plan_correction(emu, e, *a, **k)
    wide, narrow = ec(255, 3, 500, 32, 32, 3, True), ec(256, 3, 500, 32, 32, 3, True)
    assert (wide["wide_slots"], wide["slot_cap"], wide["merged_cap"]) == (1, 500, 3) and (narrow["wide_slots"], narrow["slot_cap"]) == (0, 160)
    assert wide["query_lds"] == max(3*512, 3*8+503*40) and narrow["query_lds"] == max(3*512, 3*8+163*40)
    forced = ec(255, 3, 500, 32, 32, 3, True, e=L.plan_env(emu, fuzzlib.TUNINGS["query_lds"]))
    assert (forced["wide_slots"], forced["slot_cap"], forced["lpc_max_contours"]) == (0, 16, 2)
    assert ec(255, 3, 2000, 32, 32, 3, True)["slot_cap"] == 1024 and ec(255, 3, 100, 32, 32, 3, True)["wide_slots"] == 0      # (nothing wider than the default to have)
    # the query kernel's LDS against the device's: 8 B per contour + 320 slots of 40 B
    at, beyond = ec(256, 18880, 18880, 32, 32, 3, True), ec(256, 18881, 18881, 32, 32, 3, True)
    assert (at["query_lds"], at["route"], at["gres"]) == (LDS_LIMIT, "normal", 1) and (beyond["query_lds"], beyond["route"]) == (LDS_LIMIT+8, "slow_all")
    assert beyond["slow_lds"] == 0 and beyond["res_bytes"] == 18881*512 and beyond["slow_grid"] == 2048
    assert ec(256, 192, 500, 32, 32, 3, True)["gres"] == 0 and ec(256, 193, 500, 32, 32, 3, True)["gres"] == 1               # 96 KB of scratch per wavefront
    tight = lambda lim: L.plan_env(emu, lds_limit=lim)                        # 100 contours: lane-per-candidate scratch 24 x 512 B, no global scratch
    assert ec(256, 100, 500, 32, 32, 3, True, e=tight(12288))["route"] == "normal" and ec(256, 100, 500, 32, 32, 3, True, e=tight(12287))["route"] == "too_complex"
    assert ec(256, 200, 500, 32, 32, 3, True, e=tight(12287))["route"] == "slow_all"             # with it
    assert ec(256, 200, 500, 32, 32, 3, True, e=tight(5000))["route"] == "too_complex"           # ... but the sweep itself has to fit
    assert ec(256, 200, 500, 32, 32, 3, True, e=tight(5000), stage_limit=2)["route"] == "stage_snapshot"
    # workgroups of the query kernel: a 512th of the texels within [64, 8 192], and no more than the device holds
    blocks = lambda n, **k: ec(n, 2, 20, 64, 64, 3, True, **k)
    assert [blocks(n)["query_blocks"] for n in (1, 8, 9, 1023, 1024, 1025)] == [64, 64, 72, 8184, 8192, 8192]
    assert [blocks(1024, resident=r)["query_blocks_resident"] for r in (0, 100, 8192, 9000)] == [8192, 100, 8192, 8192]
    counter = blocks(1024, resident=100, e=L.plan_env(emu, fuzzlib.TUNINGS["query_counter"]))
    assert (counter["query_blocks_resident"], counter["query_flags"], counter["grid_steps"]) == (8192, 0, 0) and blocks(1)["query_flags"] == 5
    lazy = {(m, d) for m in range(4) for d in range(3) if ec(40, 2, 20, 24, 24, 3, True, ec_mode=m, ec_check=d)["lazy_protect"]}
    assert lazy == {(2, 1)}                                                   # EDGE_PRIORITY with CHECK_DISTANCE_AT_EDGE
    assert ec(1 << 20, 1, 4, 64, 64, 3, False)["too_many_texels"] == 1 and ec((1 << 20)-1, 1, 4, 64, 64, 3, False)["too_many_texels"] == 0
    assert ec(10, 5, 50, 24, 24, 4, False)["res_bytes"] == 0 and ec(10, 5, 50, 24, 24, 4, False)["slot_offset"] == 0


def test_sign_plan(emu):
    env = L.plan_env(emu)
    sign = lambda *a, e=env: L.plan_sign(emu, e, *a)
    whole, split = sign(512, 20, 64, 64), sign(511, 20, 64, 64)              # 8 tile rows: 512 x 8 spans = 4 096
    assert (whole["span"], whole["spans_x"], whole["spans"], whole["blocks"], whole["whole_rows"]) == (8, 1, 8, 4096, 1)
    assert (split["span"], split["spans_x"], split["spans"], split["blocks"], split["whole_rows"]) == (4, 2, 16, 511*16, 0)
    assert sign(1, 20, 64, 64)["span"] == 1 and sign(1, 20, 8, 64)["whole_rows"] == 1
    assert (sign(9, 64, 24, 24)["cap"], sign(9, 64, 24, 24)["chunked"]) == (192, 0) and (sign(9, 65, 24, 24)["cap"], sign(9, 65, 24, 24)["chunked"]) == (192, 1)
    assert sign(9, 64, 24, 24)["lds"] == 10*192*12+40 and sign(9, 0, 24, 24)["cap"] == 3
    low = L.plan_env(emu, fuzzlib.TUNINGS["sign_chunked"])
    assert (sign(9, 1, 24, 24, e=low)["cap"], sign(9, 1, 24, 24, e=low)["chunked"]) == (3, 0) and (sign(9, 2, 24, 24, e=low)["cap"], sign(9, 2, 24, 24, e=low)["chunked"]) == (3, 1)
    assert L.env_field(L.plan_env(emu, {"MSDFHIP_SIGN_CAP": "1"}), "signCap") == 3


@pytest.mark.parametrize("name", sorted(FORCED))
def test_forced_tables_plan_the_routes_the_gpu_test_demands(emu, name):
    """tests/test_gpu_routes.py forces each large route with a table and proves by the route counters that it ran. The same demands on the plans of a
    60-glyph group with all three classes at 40x40 (64 compute units: 1 024 wavefront slots, so that the 45 global-scratch glyphs' 1 125 tiles make a round)."""
    ran, idle, kw = FORCED[name]
    env = L.plan_env(emu, fuzzlib.TUNINGS[name], cus=64)
    rng = np.random.default_rng(7)
    c = np.concatenate([np.ones(7, int), np.full(8, 2), rng.integers(7, 12, 45)])
    e = np.concatenate([rng.integers(3, 25, 7), rng.integers(6, 30, 8), rng.integers(30, 60, 45)])
    total = dict.fromkeys(L.ROUTE_NAMES, 0)
    for mode in kw.get("modes", (1, 2, 3, 4)):
        for overlap in (True, False):
            for scanline in ((False, True) if kw.get("scanline") else (False,)):
                for r in L.planned_routes(emu, env, c, e, 40, 40, mode, overlap, scanline=scanline):
                    total[r] += 1
    for alternatives in ran:
        assert sum(total[k] for k in alternatives) > 0, (name, alternatives, total)
    for k in idle:
        assert total[k] == 0, (name, k, total)


HOST_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_plan_host", "launch_plan_host.cpp")


def test_planners_under_the_sanitizers(tmp_path):
    """tests/launch_plan_host: the planners over seeded random cases in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer
    (host code only). Skipped only where an EMPTY program cannot be built with those flags."""
    if not _sanitizers_link(tmp_path):
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    exe = os.path.join(str(tmp_path), "launch_plan_host_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, HOST_SRC],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("planned ") and int(r.stdout.split()[1]) >= 2000, r.stdout
