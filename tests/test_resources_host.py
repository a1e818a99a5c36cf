"""msdf_resources.hpp -- the holders of the host runtime's device resources (WorkBuffer, Stream, Event, DevicePool) -- compiled with the host compiler
against a fake HIP runtime that keeps a ledger of live handles, of the device each release ran on and of every call (tests/resources_host/fake).
The program asserts: owned resources are released exactly once and borrowed ones never; moved-from holders are empty; ensure frees before it
allocates and a failed ensure / create leaves the holder empty; an aggregate shaped like a pipeline slot, built with a failure injected at every
creating call in turn, leaves nothing live and releases nothing twice; an aggregate that owns nothing makes no call when it goes; the pool hands out
only objects of the asked device, most recently returned first, gets its object back on every exit of a lease, drains each object on that
object's device and restores the caller's, and leaves an object out on lease alone. No GPU."""
import os
import subprocess

import pytest

from test_ec_lazy_host import _sanitizers_link

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resources_host")
SRC = os.path.join(HERE, "resources_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-I", os.path.join(HERE, "fake")]


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("resources_host: ") and int(r.stdout.split()[1]) >= 100, r.stdout


def test_holders_and_pool_against_the_ledger(tmp_path):
    exe = os.path.join(str(tmp_path), "resources_host")
    subprocess.run(["g++", "-O1"]+FLAGS+["-o", exe, SRC], check=True)
    _run(exe)


def test_holders_and_pool_under_the_sanitizers(tmp_path):
    """The same program under AddressSanitizer (with its leak check: the fake's handles are real blocks) and UndefinedBehaviorSanitizer. Skipped only
    where an EMPTY program cannot be built with those flags."""
    if not _sanitizers_link(tmp_path):
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    exe = os.path.join(str(tmp_path), "resources_host_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]+FLAGS+["-o", exe, SRC],
                   check=True)
    _run(exe)
