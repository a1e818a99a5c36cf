"""Inputs and the host program (tests/ec_emit_mask_host) shared by tests/test_ec_emit_mask_host.py and tests/test_gpu_ec_emit_mask.py: the error-correction
sweep's stage 1 as a mask of surviving tests per texel, appended to the item queue once per tile (msdf_ec_fast.hpp: texelCandidateMask, texelProtectMask,
ecAppendItems; msdf_kernels.hpp: ecFastBody). The file format is that of tests/ecwordscases.py, the host fields those of tests/echwmedcases.py."""
import json
import os
import subprocess

import numpy as np

import echwmedcases as H
import ecwordscases as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ec_emit_mask_host", "ec_emit_mask_host.cpp")


def build_host(tmp, sanitize=False):
    exe = os.path.join(str(tmp), "ec_emit_mask_host_san" if sanitize else "ec_emit_mask_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"]+flags+["-o", exe, SRC], check=True)
    return exe


def run(exe, args):
    r = subprocess.run([exe]+[str(a) for a in args], capture_output=True, text=True)
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-4000:])
    return r.returncode, json.loads(r.stdout)


def run_masks(exe, cases, tmp, name="emit_mask_cases.bin"):
    path = os.path.join(str(tmp), name)
    with open(path, "wb") as f:
        f.write(W.pack(cases))
    return run(exe, ["masks", path])


def host_cases():
    """The 116 fields of tests/test_ec_hw_median_host.py."""
    return H.host_cases()


# ---- the fields of the GPU test: 16x16 and 10x10, one glyph of four 8x8 tiles each (10x10: partial tiles on two sides)

GPU_SIZES = ((16, 16), (10, 10))
KINDS = ("constant", "noise", "one_texel", "wave", "neginf")


def one_texel_field(w, h, at):
    """(.75, .8125, .75) everywhere: channel differences D = (+1/16, -1/16, 0), no test survives. Texel `at` (x, y) holds (1, 1-1/128, 1): D = (-1/128,
    +1/128, 0), opposite in sign to its neighbours', and its deviation .5 exceeds their .25, so it is the texel that reports: its linear and diagonal
    tests of the first two channel pairs survive. Its neighbours do not report against it, and in their diagonal tests that pass over it dBC = 1/16-1/128
    keeps the sign of dA and dD (the third pair: all three zero): exactly one texel has survivors (counted by tests/test_ec_emit_mask_host.py)."""
    f = np.zeros((h, w, 3), np.float32)
    f[:, :] = (.75, .8125, .75)
    f[at[1], at[0]] = (1., 1.-1./128, 1.)
    return f


def gpu_cases():
    """name -> field."""
    cases = {}
    for (w, h) in GPU_SIZES:
        tag = "%dx%d" % (w, h)
        cases["constant_%s_0" % tag] = np.full((h, w, 3), .625, np.float32)
        cases["constant_%s_1" % tag] = np.full((h, w, 3), .5, np.float32)
        for s in range(2):
            rng = np.random.default_rng(9700+10*w+s)
            cases["noise_%s_%d" % (tag, s)] = rng.uniform(0., 1., (h, w, 3)).astype(np.float32)
        cases["one_texel_%s_0" % tag] = one_texel_field(w, h, (3, 4))             # inside tile 0
        cases["one_texel_%s_1" % tag] = one_texel_field(w, h, (8, 7))             # tile 1's first column, last row of the upper tiles: three tiles see it in their halo
        for s in range(2):
            cases["wave_%s_%d" % (tag, s)] = H.wave_field(w, h, 400+10*w+s)
        base = H.wave_field(w, h, 420+10*w)
        cases["neginf_%s_0" % tag] = H.with_texel(base, 7, 7, (-np.inf, base[7, 7, 1], base[7, 7, 2]))     # all four tiles hold it or see it: every vote fails
        cases["neginf_%s_1" % tag] = H.with_texel(base, 2, 2, (base[2, 2, 0], -np.inf, base[2, 2, 2]))     # tile 0 only: the others run the hardware median
    return cases
