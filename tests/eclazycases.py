"""Inputs and the host program (tests/ec_lazy_host) shared by tests/test_ec_lazy_host.py and tests/test_gpu_ec_lazy.py: the fixture glyphs of the lazy
protection order of k_ec_fast (msdf_ec_fast.hpp: ecLazyProtect), their frames at the small sizes, seeded random fields, and the file the program reads."""
import json
import os
import struct
import subprocess

import numpy as np

from msdfgen_amd.shape import autoframe, distance_mapping

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ec_lazy_host", "ec_lazy_host.cpp")

HOST_SIZES = ((16, 16), (23, 17))
GPU_SIZES = ((8, 8), (9, 9), (16, 16), (23, 17))      # a single tile with all its halo outside; partial tiles; 2x2 tiles; 3x3 tiles, the last ones partial
MODES = (1, 2, 3)                                      # EC_INDISCRIMINATE, EC_EDGE_PRIORITY, EC_EDGE_ONLY
DISTANCE_CHECKS = (0, 1, 2)                            # DO_NOT_CHECK_DISTANCE, CHECK_DISTANCE_AT_EDGE, ALWAYS_CHECK_DISTANCE
GROUP_GLYPHS, GROUP_RANDOM, GROUP_BENCH = 0, 1, 2
KINDS = ("conditional_protected_by_edge", "conditional_protected_by_corner", "conditional_unprotected", "error_and_conditional")


def build_host(tmp, sanitize=False):
    """The stand-alone program; sanitize: with AddressSanitizer and UndefinedBehaviorSanitizer (host code only, run as it is)."""
    exe = os.path.join(str(tmp), "ec_lazy_host_san" if sanitize else "ec_lazy_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"]+flags+["-o", exe, SRC], check=True)
    return exe


def fixture_glyphs(n_glyphs, count=40):
    """Evenly spaced glyphs of the Basic-Latin fixture (tests/golden/latin.npz)."""
    return [int(g) for g in np.linspace(0, n_glyphs-1, count).round()]


def frame(bounds, w, h):
    """A range of 2 texels: the widest that fits the 8x8 tile of the GPU test, and one that keeps many texels of these small bitmaps near an edge."""
    return autoframe(bounds, w, h, 2.)


def pack(cases):
    """cases: dicts with w, h, flip, group, shape (FlatShape), xf (sx, sy, tx, ty, range lower, range upper), field float32 (h, w, >= 3)."""
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        s = c["shape"]
        co = np.ascontiguousarray(s.contour_offsets, np.int32)
        ne = int(co[-1])
        ms, mt = distance_mapping(c["xf"][4], c["xf"][5])
        field = np.ascontiguousarray(np.asarray(c["field"], np.float32)[:, :, :3])
        assert field.shape == (c["h"], c["w"], 3)
        blob += [struct.pack("<6i", c["w"], c["h"], int(c["flip"]), int(c["group"]), len(co)-1, ne),
                 np.array([c["xf"][0], c["xf"][1], c["xf"][2], c["xf"][3], ms, mt], np.float64).tobytes(), co.tobytes(),
                 np.ascontiguousarray(s.points, np.float64).reshape(-1, 8)[:ne].tobytes(), np.ascontiguousarray(s.types, np.uint8)[:ne].tobytes(),
                 np.ascontiguousarray(s.colors, np.uint8)[:ne].tobytes(), field.tobytes()]
    return b"".join(blob)


def run_host(exe, cases, tmp, name="cases.bin"):
    """-> (exit status, the program's JSON)."""
    path = os.path.join(str(tmp), name)
    with open(path, "wb") as f:
        f.write(pack(cases))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-4000:])
    return r.returncode, json.loads(r.stdout)


def glyph_cases(batch, bounds, oracle, sizes, glyphs=None, group=GROUP_GLYPHS):
    """Pre-correction msdf fields (the oracle with error correction disabled) of the fixture glyphs at `sizes`, upward and downward rows (flip 0 / 1)."""
    cases = []
    for g in (fixture_glyphs(batch.n_glyphs) if glyphs is None else glyphs):
        s = batch.shape(g)
        for (w, h) in sizes:
            xf = frame(bounds[g], w, h)
            for y_down in (False, True):
                cases.append({"w": w, "h": h, "flip": int(bool(s.inverse_y) != y_down), "group": group, "shape": s, "xf": xf, "glyph": g, "y_down": y_down,
                              "field": oracle.generate(s, 3, w, h, xf, ec_mode=0, y_down=y_down)})
    return cases


def random_cases(batch, bounds, seeds=(1, 2, 3, 4, 5, 6), sizes=HOST_SIZES):
    """Seeded fp32 fields around .5, each under the frame (corners, distance queries) of a fixture glyph, with both flips: per channel a plane wave
    .5+a*sin(fx*x+fy*y+phase) plus white noise. The interpolated median has to leave the range of its end points AND move faster than the span
    allows (0.56 per texel at this range) for a conditional artifact: small white noise alone never does, waves of amplitude <= 0.6 and up to 1.5 rad per
    texel (+-0.05 of noise) do so at a tenth of the texels (odd seeds), and waves of amplitude <= 0.45 and up to 3 rad per texel (+-0.1 of noise) also put
    distance-check candidates behind conditional artifacts of the same diagonal pair (even seeds: the held-back candidates of the lazy order, some of them
    at texels that stay unprotected, where the eager order hands them to nobody)."""
    cases = []
    picks = fixture_glyphs(batch.n_glyphs)
    for seed in seeds:
        rng = np.random.default_rng(1000+seed)
        amp, fmax, noise = (.6, 1.5, .05) if seed%2 else (.45, 3., .1)
        for (w, h) in sizes:
            g = picks[int(rng.integers(len(picks)))]
            s = batch.shape(g)
            yy, xx = np.mgrid[0:h, 0:w]
            field = np.zeros((h, w, 3))
            for k in range(3):
                fx, fy = rng.uniform(-fmax, fmax, 2)
                field[:, :, k] = .5+rng.uniform(.3*amp, amp)*np.sin(fx*xx+fy*yy+rng.uniform(0, 2*np.pi))
            field = (field+rng.uniform(-noise, noise, field.shape)).astype(np.float32)
            for flip in (0, 1):
                cases.append({"w": w, "h": h, "flip": flip, "group": GROUP_RANDOM, "shape": s, "xf": frame(bounds[g], w, h), "glyph": g, "field": field})
    return cases
