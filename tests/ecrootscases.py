"""Inputs and the host program (tests/ec_roots_host) shared by tests/test_ec_roots_host.py, tests/test_gpu_ec_roots.py and tools/ec_root_counts.py: crafted 2x2
cells for the diagonal artifact test of the error-correction sweep (msdf_ec_fast.hpp: diagonalPairFast), embedded in 8x8 and 9x9 fields, and the file the
program reads (the CASES format of tests/eclazycases.py; the program skips the outlines)."""
import json
import os
import subprocess
import types

import numpy as np

import eclazycases as E

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ec_roots_host", "ec_roots_host.cpp")

GROUP_CRAFTED, GROUP_EXTRA = 3, 4
CRAFTED_SIZES = ((8, 8), (9, 9))
XF = (1., 1., 0., 0., -1., 1.)                          # a texel per shape unit, a range of 2 texels (the diagonal span is then 1.11*sqrt(2)/2 per unit of t)
NO_SHAPE = types.SimpleNamespace(contour_offsets=np.zeros(1, np.int32), points=np.zeros((0, 8)), types=np.zeros(0, np.uint8), colors=np.zeros(0, np.uint8))
BARS = ("both_roots", "only_t1", "both_extrema", "error_at_first_of_two", "held_back")       # at least 100 queued items of each
COVERED = ("both_roots", "only_t0", "only_t1", "dscr_zero", "linear_branch", "tex_zero", "tex_one", "both_extrema", "one_extremum", "no_extremum", "q_zero",
           "non_finite")                               # at least one compared pair of each among the crafted cells


def build_host(tmp, sanitize=False):
    """The stand-alone program; sanitize: with AddressSanitizer and UndefinedBehaviorSanitizer (host code only, run as it is)."""
    exe = os.path.join(str(tmp), "ec_roots_host_san" if sanitize else "ec_roots_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"]+flags+["-o", exe, SRC], check=True)
    return exe


def run_host(exe, cases, tmp, name="roots.bin"):
    """-> (exit status, the program's JSON)."""
    path = os.path.join(str(tmp), name)
    with open(path, "wb") as f:
        f.write(E.pack([dict({"flip": 0, "shape": NO_SHAPE, "xf": XF}, **c) for c in cases]))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-4000:])
    return r.returncode, json.loads(r.stdout)


def quadratic_cell(r1, r2, s):
    """Channel differences D = ch1-ch0 at (texel, horizontal, vertical, diagonal neighbour) whose diagonal quadratic is s*(t-r1)*(t-r2): the reference solves
    (dD-dBC+dA)*t^2+(dBC-2*dA)*t+dA with dBC = dB+dC."""
    qa, qb, qc = s, -s*(r1+r2), s*r1*r2
    dA = qc
    dBC = qb+2*dA
    return (dA, .5*dBC, .5*dBC, qa+dBC-dA)


TWO = quadratic_cell(.3, .7, .5)                        # both roots in range
GENERIC = (.4, .45, .55, .6)                            # channel 0: extrema wherever they fall

# name -> (channel 0 at (a, b, c, d), D = channel 1 - channel 0, channel 2: a value, or "ch1" for equal channels)
NAMED_CELLS = {
    "both_roots": (GENERIC, TWO, .5),
    "only_t0": (GENERIC, quadratic_cell(.3, 1.5, .4), .5),               # which index is in range follows the sign of the leading coefficient
    "only_t1": (GENERIC, quadratic_cell(.3, 1.5, -.4), .5),
    "only_first_far": ((.6, .5, .45, .4), quadratic_cell(-.6, .6, .3), .45),
    "dscr_zero": ((.5, .25, .25, .5), (.25, -.25, -.25, .25), .5),       # t^2-t+.25, every value exact in fp32: b*b == 4*a*c
    "a_zero": ((.5, .5, .5, .75), (.25, -.125, -.125, -.5), .5),         # dD-dBC+dA == 0: the linear branch, root 1/3
    "b_dwarfs_a": ((0., 0., 0., 0.), (1e-20, .5, .5, 1.), .5),           # |b| > 1e12*|a| (fp32 coefficients cannot put that branch's root in range)
    "tex_zero": ((.5, .5, .5, .25), TWO, .5),                            # l0 == 0: tEx0 = -0
    "tex_one": ((.5, .25, .25, .25), TWO, .5),                           # l0 == -2*q0: tEx0 == 1
    "q_zero_nan": ((.5, .5, .5, .5), TWO, .5),                           # l0 == q0 == 0: tEx0 is NaN
    "q_zero_inf": ((.5, .25, .25, 0.), TWO, .5),                         # q0 == 0: tEx0 = +inf
    "both_extrema": ((.5, .4, .4, .5), TWO, .5),                         # tEx0 == tEx1 == .5
    "one_extremum": ((.5, .4, .4, .5), quadratic_cell(.3, 1.5, .4), .2),
    "no_extremum": ((.2, .4, .5, .9), quadratic_cell(.4, -2., .2), .5),
    "equal_channels": (GENERIC, TWO, "ch1"),
    "signed_zero": ((0., -0., 0., -0.), TWO, -0.),
    "denormal": ((0., 0., 0., 0.), tuple(np.float32(v)*np.float32(1e-45) for v in (3, -4, -4, 3)), 1e-40),
}
NON_FINITE = (np.nan, np.inf, -np.inf)


def place(field, x0, y0, cell):
    ch0, d, ch2 = cell
    for (dx, dy), v0, dv in zip(((0, 0), (1, 0), (0, 1), (1, 1)), ch0, d):
        t = field[y0+dy, x0+dx]
        t[0] = np.float32(v0)
        t[1] = np.float32(v0)+np.float32(dv)
        t[2] = t[1] if isinstance(ch2, str) else np.float32(ch2)


def background(w, h, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.zeros((h, w, 3))
    for k in range(3):
        fx, fy = rng.uniform(-2., 2., 2)
        f[:, :, k] = .5+rng.uniform(.1, .5)*np.sin(fx*xx+fy*yy+rng.uniform(0, 2*np.pi))
    return (f+rng.uniform(-.05, .05, f.shape)).astype(np.float32)


def cell_origins(w, h):
    """2x2 cells three texels apart: a texel of background between two cells, cells on the bitmap's border and across the 8x8 tile's border (9x9)."""
    return [(x, y) for y in range(0, h-1, 3) for x in range(0, w-1, 3)]


def crafted_cases():
    """Per size: the named cells, each in all four orientations of the 2x2 cell (every texel of it is once the centre of the diagonal test); the
    both-roots cell with one channel of one texel NaN / +inf / -inf; seeded random quadratics with roots in (-.5, 1.5)."""
    cases = []
    for (w, h) in CRAFTED_SIZES:
        origins = cell_origins(w, h)
        cells = []
        for name, (ch0, d, ch2) in NAMED_CELLS.items():
            for perm in ((0, 1, 2, 3), (1, 0, 3, 2), (2, 3, 0, 1), (3, 2, 1, 0)):          # identity, mirrored in x, in y, in both
                cells.append((name, (tuple(ch0[i] for i in perm), tuple(d[i] for i in perm), ch2)))
        for bad in NON_FINITE:
            for texel in range(4):
                for channel in range(3):
                    cells.append(("non_finite", (GENERIC, TWO, .5), (texel, channel, bad)))
        rng = np.random.default_rng(9000+w)
        for i in range(20*len(origins)):
            r1, r2 = rng.uniform(-.5, 1.5, 2)
            cells.append(("random", (tuple(rng.uniform(.2, .8, 4)), quadratic_cell(r1, r2, rng.choice([-1., 1.])*rng.uniform(.1, .8)), float(rng.uniform(.2, .8)))))
        for at in range(0, len(cells), len(origins)):
            field = background(w, h, rng)
            names = []
            for (x0, y0), cell in zip(origins, cells[at:at+len(origins)]):
                place(field, x0, y0, cell[1])
                if len(cell) == 3:
                    texel, channel, bad = cell[2]
                    field[y0+texel//2, x0+texel % 2, channel] = bad
                names.append(cell[0])
            cases.append({"w": w, "h": h, "group": GROUP_CRAFTED, "field": field, "cells": names})
    return cases


def extra_cases(seeds=range(20, 90)):
    """Seeded plane-wave fields like those of eclazycases.random_cases with even seeds (amplitude <= 0.45, up to 3 rad per texel, +-0.1 of noise): fast enough
    for quadratics with both roots in range, with conditional artifacts in front of candidates and ERRORs at a first root. The lazy order meets either in
    one diagonal item of two thousand, hence their number; the first six seeds also at 8x8 and 9x9 (the GPU test's sizes)."""
    cases = []
    for seed in seeds:
        rng = np.random.default_rng(11000+seed)
        for (w, h) in (CRAFTED_SIZES if seed < 26 else ())+E.HOST_SIZES:
            yy, xx = np.mgrid[0:h, 0:w]
            field = np.zeros((h, w, 3))
            for k in range(3):
                fx, fy = rng.uniform(-3., 3., 2)
                field[:, :, k] = .5+rng.uniform(.135, .45)*np.sin(fx*xx+fy*yy+rng.uniform(0, 2*np.pi))
            cases.append({"w": w, "h": h, "group": GROUP_EXTRA, "field": (field+rng.uniform(-.1, .1, field.shape)).astype(np.float32), "seed": seed})
    return cases


def bench_cases(oracle, every, group=E.GROUP_BENCH):
    """Every `every`-th glyph of tests/golden/dejavu8192.npz at 64x64 under the bench step's frames: pre-correction fields by the oracle."""
    from msdfgen_amd.shape import ShapeBatch
    z = np.load(os.path.join(HERE, "golden", "dejavu8192.npz"))
    batch = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                       z["colors"].astype(np.int32), np.zeros(8192, bool), [str(n) for n in z["names"]])
    cases = []
    for g in range(0, batch.n_glyphs, every):
        s = batch.shape(g)
        cases.append({"w": 64, "h": 64, "flip": int(bool(s.inverse_y)), "group": group, "shape": s, "xf": z["xf64"][g], "glyph": g,
                      "field": oracle.generate(s, 3, 64, 64, z["xf64"][g], ec_mode=0)})
    return cases
