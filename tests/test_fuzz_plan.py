"""The randomized sweeps' planner (tests/fuzzlib.py) without a device: the seeds the GPU tests pin keep drawing the groups they always drew, and the
throughput-sized plans really are past the launch-size bounds they exist to cross. Also the route-counter names of the binding against the header."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import fuzzlib
import xformcases
from conftest import GOLDEN, ROOT
from msdfgen_amd import lib as L
from msdfgen_amd.shape import ShapeBatch


def fingerprint(g):
    b = ShapeBatch.from_shapes(g["shapes"])
    hh = hashlib.sha256()
    for a in (b.glyph_contour_offsets, b.contour_offsets, b.points, b.types, b.colors, np.asarray(b.inverse_y, bool), np.ascontiguousarray(g["xfs"], np.float64)):
        hh.update(np.ascontiguousarray(a).tobytes())
    return [g["n"], g["mode"], g["w"], g["h"], g["overlap"], g["ec"][0], g["ec"][1], g["kind"], g["y_down"], g["family"], hh.hexdigest()[:16]]


@pytest.mark.parametrize("seed,n_shapes,framing", [(401, 2000, None), (411, 1500, None), (421, 1500, "all")])
def test_default_plans_are_the_recorded_ones(seed, n_shapes, framing):
    """Seeds 401 / 411 / 421 (test_gpu_parity.py's sweeps) against the groups the sweep drew before plan() and run() were split: sizes, modes,
    combiner, error-correction pair, shape kind, Y orientation, framing and a digest of every shape and transform."""
    with open(os.path.join(GOLDEN, "fuzzlib_default_plans.json")) as f:
        want = json.load(f)[str(seed)]
    got = [fingerprint(g) for g in fuzzlib.plan(n_shapes, seed, framing=list(xformcases.FAMILIES) if framing else None)]
    assert json.loads(json.dumps(got)) == want


def tiles(g):
    return g["n"]*((g["w"]+7)//8)*((g["h"]+7)//8)


@pytest.mark.parametrize("scanline", [False, True])
def test_full_scale_groups_leave_the_small_routes(scanline):
    groups = list(fuzzlib.plan(6000, 5, scale="full", scanline=scanline))
    assert len(groups) >= 12
    for g in groups:
        assert g["n"] >= 256 and tiles(g) > 8192, (g["index"], g["n"], g["w"], g["h"])
        ncont = [s.n_contours for s in g["shapes"]]
        assert min(ncont) <= 1 and 2 in ncont and max(ncont) >= 8, g["index"]        # one-contour, LDS-scratch and global-scratch glyphs in one launch
        if g["scanline"] is not None:
            assert g["n"]*((g["h"]+7)//8) >= 4096                                     # the sign pass's whole-row spans
    assert {g["ec"] for g in groups} == set(fuzzlib.EC_PAIRS)
    assert {g["overlap"] for g in groups} == {False, True} and {g["y_down"] for g in groups} == {False, True}
    assert any(g["min_dev"] != fuzzlib.DEFAULT_RATIO or g["min_imp"] != fuzzlib.DEFAULT_RATIO for g in groups)
    assert any(s.inverse_y for s in groups[0]["shapes"]) and not all(s.inverse_y for s in groups[0]["shapes"])
    if scanline:
        assert {g["scanline"] for g in groups} - {None} == {0, 1, 2, 3}


def test_mixed_scale_groups_hold_every_class_and_every_ec_pair():
    groups = list(fuzzlib.plan(800, 7, scale="mixed", modes=(3, 4)))
    assert {g["ec"] for g in groups} == set(fuzzlib.EC_PAIRS) and {g["mode"] for g in groups} == {3, 4}
    for g in groups:
        ncont = [s.n_contours for s in g["shapes"]]
        assert min(ncont) <= 1 and 2 in ncont and max(ncont) >= 8


def test_tuned_restores_the_environment_even_on_failure():
    os.environ["MSDFHIP_SIGN_CAP"] = "96"
    os.environ.pop("MSDFHIP_SHORT_ROUNDS", None)
    try:
        with pytest.raises(RuntimeError):
            with fuzzlib.tuned({"MSDFHIP_SIGN_CAP": "3", "MSDFHIP_SHORT_ROUNDS": "0"}):
                assert os.environ["MSDFHIP_SIGN_CAP"] == "3" and os.environ["MSDFHIP_SHORT_ROUNDS"] == "0"
                raise RuntimeError("inside")
        assert os.environ["MSDFHIP_SIGN_CAP"] == "96" and "MSDFHIP_SHORT_ROUNDS" not in os.environ
    finally:
        os.environ.pop("MSDFHIP_SIGN_CAP", None)
        L.load().msdfhip_reload_tuning()


def test_every_tuning_table_names_a_parsed_knob():
    src = open(os.path.join(ROOT, "msdfgen_amd", "csrc", "msdf_capi.hip")).read()
    parsed = set(re.findall(r'getenv\("(MSDFHIP_\w+)"\)', src))
    for name, env in fuzzlib.TUNINGS.items():
        assert set(env) <= parsed, (name, set(env)-parsed)


def test_route_counter_names_follow_the_header():
    text = open(os.path.join(ROOT, "include", "msdfgen_hip.h")).read()
    defs = {int(v): k.lower() for k, v in re.findall(r"#define MSDFHIP_ROUTE_(\w+)\s+(\d+)", text) if k != "COUNT"}
    count = int(re.search(r"#define MSDFHIP_ROUTE_COUNT\s+(\d+)", text).group(1))
    assert sorted(defs) == list(range(count)) == list(range(len(L.ROUTE_NAMES)))
    assert tuple(defs[i] for i in range(count)) == L.ROUTE_NAMES
    buf = (L.C.c_ulonglong*count)()
    assert L.load().msdfhip_debug_route_counts(buf, count, 0) == count
    assert L.load().msdfhip_debug_route_counts(buf, 3, 0) == 3
