"""Binds the host-tested launch plans (msdfgen_amd/csrc/msdf_launchplan.hpp, tests/test_launch_plan_host.py) to what the library runs: on one 64-glyph
mixed-class group at 24x24 msdf, under the defaults and under four forcing tables, the increase of the route counters over ONE generate call must be
exactly the routes the host plan lists -- planned through tests/hostemu from the group's contour and edge counts and the device's own compute-unit count
and LDS size.

Every device call is made by one child process (tests/launchplan_gpu_child.py) under a time limit of its own; this process never opens the GPU."""
import json
import os
import subprocess
import sys
from collections import Counter

import pytest

from emu import Emu
import fuzzlib
import launchplan as L
import launchplan_gpu_child as child

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120          # seconds; the child needs a few (torch import and device start included)


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("launch_plan_gpu")), "routes.json")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable]+flags+[child.__file__, out], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def emu():
    return Emu()


def test_the_group_has_every_class(device):
    contours, edges = child.counts(child.group())
    assert (contours, edges) == (device["contours"], device["edges"])
    assert min(contours) == 1 and any(2 <= c <= 5 and e <= 128 for c, e in zip(contours, edges)) and max(contours) > 5


@pytest.mark.parametrize("case", sorted(child.CASES))
def test_one_generate_call_runs_the_planned_routes(device, emu, case):
    table, scanline = child.CASES[case]
    env = L.plan_env(emu, fuzzlib.TUNINGS[table] if table else None, cus=device["device"]["cus"], lds_limit=device["device"]["lds_bytes"])
    w, h = child.SIZE
    planned = Counter(L.planned_routes(emu, env, device["contours"], device["edges"], w, h, 3, True, scanline=scanline))
    ran = Counter({k: v for k, v in device["routes"][case].items() if v})
    print(case, dict(planned))
    assert ran == planned, (case, dict(ran), dict(planned))
