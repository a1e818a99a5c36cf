"""Inputs and the host program (tests/ec_hw_median_host) shared by tests/test_ec_hw_median_host.py and tests/test_gpu_ec_hw_median.py: fields for the
hardware-median instantiation of the error-correction sweep and its finiteness vote (msdf_kernels.hpp: ecFastBody, EC_MED3_BOUND; msdf_device.hpp: med3f).
The file format and the special-value fields are those of tests/ecwordscases.py."""
import json
import os
import subprocess

import numpy as np

import ecwordscases as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ec_hw_median_host", "ec_hw_median_host.cpp")

BOUND = np.float32(2.)**100                              # EC_MED3_BOUND
BELOW = np.nextafter(BOUND, np.float32(0), dtype=np.float32)
ABOVE = np.nextafter(BOUND, np.float32(np.inf), dtype=np.float32)


def build_host(tmp, sanitize=False):
    exe = os.path.join(str(tmp), "ec_hw_median_host_san" if sanitize else "ec_hw_median_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"]+flags+["-o", exe, SRC], check=True)
    return exe


def wave_field(w, h, seed):
    """A seeded finite fp32 field (h, w, 3): plane waves around .5 with white noise, as tests/ecwordscases.py: crafted_field before its special texels --
    the channel order changes from texel to texel, so both stages of the sweep have work everywhere."""
    rng = np.random.default_rng(9100+seed)
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.zeros((h, w, 3))
    for k in range(3):
        fx, fy = rng.uniform(-2., 2., 2)
        f[:, :, k] = .5+rng.uniform(.1, .5)*np.sin(fx*xx+fy*yy+rng.uniform(0, 2*np.pi))
    return (f+rng.uniform(-.05, .05, f.shape)).astype(np.float32)


def with_texel(field, x, y, value):
    f = field.copy()
    f[y, x] = np.asarray(value, np.float32)
    return f


def zeros_denormals_bound_field(w, h, seed, outside):
    """A wave field in which a third of the texels hold +0 / -0, denormals and -- one texel each -- a channel just below the vote's bound with either
    sign; outside: one texel more with a channel just above it (the vote of its tile and of the tiles that see it in their halo fails)."""
    rng = np.random.default_rng(9300+seed)
    f = wave_field(w, h, 50+seed)
    tiny = np.float32(1e-45)
    pos = rng.permutation(w*h)
    for i, at in enumerate(pos[:max(4, (w*h)//3)]):
        y, x = divmod(int(at), w)
        kind = i % 4
        if kind == 0:
            f[y, x] = np.array([0., -0., 0.], np.float32)[rng.permutation(3)]
        elif kind == 1:
            f[y, x] = np.array([-0., -0., rng.choice([0., .5])], np.float32)[rng.permutation(3)]
        elif kind == 2:
            f[y, x] = np.float32(rng.choice([0., 1e-39, -3e-40]))+tiny*rng.integers(-3, 4, 3).astype(np.float32)
        else:
            f[y, x, int(rng.integers(3))] = np.float32(rng.choice([0., -0., 1e-42]))
    y, x = divmod(int(pos[-1]), w)
    f[y, x, 0] = BELOW
    y, x = divmod(int(pos[-2]), w)
    f[y, x] = (-BELOW, BELOW, -BELOW)
    if outside:
        y, x = divmod(int(pos[-3]), w)
        f[y, x, 1] = ABOVE
    return f


def bound_field(w, h, seed):
    """Every channel of every texel at the largest magnitudes that pass the vote (just below 2^100, 2^99, with both signs) or an ordinary value: the sums
    a-b-c, -a-abc, d+abc and the interpolations are as large as the vote allows."""
    rng = np.random.default_rng(9500+seed)
    pool = np.array([BELOW, -BELOW, 2.**99, -2.**99, 3*2.**98, .25, .75, 0.], np.float32)
    return pool[rng.integers(0, len(pool), (h, w, 3))]


def host_cases():
    """The special-value fields of tests/ecwordscases.py, finite wave fields, zeros / denormals / bound fields and fields at the bound."""
    cases = W.crafted_cases()
    for i, (w, h) in enumerate(((8, 8), (9, 9), (10, 17), (16, 16), (23, 17))):
        for s in range(6):
            cases.append({"w": w, "h": h, "seed": s, "field": wave_field(w, h, 16*i+s), "ratio": W.RATIOS[s % 2]})
        for s in range(3):
            cases.append({"w": w, "h": h, "seed": s, "field": zeros_denormals_bound_field(w, h, 16*i+s, s == 2)})
            cases.append({"w": w, "h": h, "seed": s, "field": bound_field(w, h, 16*i+s)})
    return cases


def run(exe, args):
    r = subprocess.run([exe]+[str(a) for a in args], capture_output=True, text=True)
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-4000:])
    return r.returncode, json.loads(r.stdout)


def run_sweep(exe, cases, tmp, name="hwmed_cases.bin"):
    path = os.path.join(str(tmp), name)
    with open(path, "wb") as f:
        f.write(W.pack(cases))
    return run(exe, ["sweep", path])


def run_correct(exe, cases, tmp, name="hwmed_correct.bin"):
    """The shapeless error correction of every case by the host walk (exact spelling) -> list of float32 (h, w, 3)."""
    path, out = os.path.join(str(tmp), name), os.path.join(str(tmp), name+".out")
    with open(path, "wb") as f:
        f.write(W.pack(cases))
    status, r = run(exe, ["correct", path, out])
    assert status == 0, r
    flat = np.fromfile(out, np.float32)
    res, at = [], 0
    for c in cases:
        n = c["w"]*c["h"]*3
        res.append(flat[at:at+n].reshape(c["h"], c["w"], 3))
        at += n
    assert at == flat.size
    return res


# ---- the fields of the GPU test: 16x16 and 10x10, one glyph of four tiles each (10x10: partial tiles on two sides)

GPU_SIZES = ((16, 16), (10, 10))


def gpu_cases():
    """name -> field. Tiles are 8x8 and a tile's halo reaches one texel beyond it: tile 0 is columns and rows 0-7, tile 1 starts at column 8, tile 2 at row
    8, tile 3 at both. A texel votes in every tile that holds it or sees it in its halo."""
    cases = {}
    for (w, h) in GPU_SIZES:
        for s in range(3):
            base = wave_field(w, h, 200+10*w+s)
            cases["wave_%dx%d_%d" % (w, h, s)] = base
            # one -inf texel at (7, 7) of tile 0: tiles 1, 2 and 3 hold it in their halo (column / row 7 borders them), so they take the exact path too;
            # at (2, 2) only tile 0 does, the other three run the hardware median in the same launch
            cases["neginf_corner_%dx%d_%d" % (w, h, s)] = with_texel(base, 7, 7, (-np.inf, base[7, 7, 1], base[7, 7, 2]))
            cases["neginf_inner_%dx%d_%d" % (w, h, s)] = with_texel(base, 2, 2, (-np.inf, base[2, 2, 1], base[2, 2, 2]))
            # one -inf texel on the border between tiles 0 and 1: those two and their halo neighbours take the exact path, tile 3 (whose halo starts at
            # column 7, row 7) sees it only if y >= 7
            cases["neginf_edge_%dx%d_%d" % (w, h, s)] = with_texel(base, 7, 3, (base[3, 7, 0], -np.inf, base[3, 7, 2]))
            # two -inf channels in one texel: their difference is a NaN
            cases["nan_difference_%dx%d_%d" % (w, h, s)] = with_texel(base, 7, 3, (-np.inf, -np.inf, base[3, 7, 2]))
            cases["zeros_bound_%dx%d_%d" % (w, h, s)] = zeros_denormals_bound_field(w, h, 300+10*w+s, False)
            cases["zeros_above_bound_%dx%d_%d" % (w, h, s)] = zeros_denormals_bound_field(w, h, 300+10*w+s, True)
    return cases
