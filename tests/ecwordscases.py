"""Inputs and the host program (tests/ec_stage1_words_host) shared by tests/test_ec_stage1_words_host.py and tests/test_gpu_ec_stage1_words.py: crafted
fields for stage 1 of the error-correction sweep (msdf_ec_fast.hpp: ecTexelClassWord, texelCandidatePairs), and the file the program reads."""
import json
import os
import struct
import subprocess

import numpy as np

from msdfgen_amd.shape import distance_mapping

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ec_stage1_words_host", "ec_stage1_words_host.cpp")

# Every combination of bitmap borders that an 8x8 tile (and a texel's 3x3 neighbourhood) can touch: 1x1 touches all four, 1x9 / 9x1 three and two opposite
# ones in a second tile, 2x2 and 8x8 all four from a full tile, 9x9 and 10x17 corners, edges and an interior over several tiles.
CRAFTED_SIZES = ((1, 1), (1, 9), (9, 1), (2, 2), (8, 8), (9, 9), (10, 17))
KINDS = ("equal_channels", "signed_zero", "denormal", "pos_inf", "neg_inf", "nan")
XF = (1., 1., 0., 0., -2., 2.)                          # scale, translate, distance range of the shapeless calls: a texel per shape unit, a range of 4 texels
RATIOS = (1.11111111111111111, 1.0)


def build_host(tmp, sanitize=False):
    """The stand-alone program; sanitize: with AddressSanitizer and UndefinedBehaviorSanitizer (host code only, run as it is)."""
    exe = os.path.join(str(tmp), "ec_stage1_words_host_san" if sanitize else "ec_stage1_words_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"]+flags+["-o", exe, SRC], check=True)
    return exe


def crafted_field(w, h, seed):
    """A seeded fp32 field (h, w, 3): plane waves around .5 with white noise -- channel orders change from texel to texel, so the sign tests fire -- in which
    about four texels in ten are replaced by a special one: all three or two channels equal (differences +0), channels +0 / -0 (differences +0 and -0),
    channels a few denormal steps apart (denormal differences), +inf, -inf or NaN in one to three channels (differences inf, NaN). Each kind is placed at
    least once if the field has texels enough, at seeded positions."""
    rng = np.random.default_rng(7000+seed)
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.zeros((h, w, 3))
    for k in range(3):
        fx, fy = rng.uniform(-2., 2., 2)
        f[:, :, k] = .5+rng.uniform(.1, .5)*np.sin(fx*xx+fy*yy+rng.uniform(0, 2*np.pi))
    f = (f+rng.uniform(-.05, .05, f.shape)).astype(np.float32)
    tiny = np.float32(1e-45)                              # the smallest denormal
    order = rng.permutation(w*h)
    special = order[:max(1, int(round(.4*w*h)))]
    for i, pos in enumerate(special):
        y, x = divmod(int(pos), w)
        kind = i % 8 if len(special) >= 8 else (seed+i) % 8
        t = f[y, x]
        if kind == 0:
            t[:] = t[int(rng.integers(3))]                 # all equal
        elif kind == 1:
            a, b = rng.permutation(3)[:2]
            t[a] = t[b]                                    # two equal
        elif kind == 2:
            t[:] = np.array([0., -0., 0.], np.float32)[rng.permutation(3)]
        elif kind == 3:
            base = np.float32(rng.choice([0., 1e-39, -3e-40]))
            t[:] = base+tiny*rng.integers(-3, 4, 3).astype(np.float32)
        elif kind == 4:
            t[rng.permutation(3)[:int(rng.integers(1, 4))]] = np.inf
        elif kind == 5:
            t[rng.permutation(3)[:int(rng.integers(1, 4))]] = -np.inf
        elif kind == 6:
            t[rng.permutation(3)[:int(rng.integers(1, 4))]] = np.nan
        else:
            t[:] = np.array([np.inf, -np.inf, np.nan], np.float32)[rng.permutation(3)]
    return f


def crafted_cases(seeds=(0, 1, 2, 3, 4, 5, 6, 7)):
    """One field per size and seed; the tiny sizes get every seed so that each kind of special texel meets each border pattern."""
    return [{"w": w, "h": h, "seed": s, "field": crafted_field(w, h, 16*i+s)} for i, (w, h) in enumerate(CRAFTED_SIZES) for s in seeds]


def census(fields):
    """How many texels of each special kind the fields hold (by numpy, from the channel differences stage 1 looks at)."""
    n = dict.fromkeys(KINDS, 0)
    for f in fields:
        with np.errstate(invalid="ignore"):
            d = np.stack([f[:, :, 1]-f[:, :, 0], f[:, :, 2]-f[:, :, 1], f[:, :, 0]-f[:, :, 2]], -1)
        n["equal_channels"] += int(((d == 0) & ~np.signbit(d)).any(-1).sum())
        n["signed_zero"] += int(((d == 0) & np.signbit(d)).any(-1).sum())
        n["denormal"] += int(((d != 0) & (np.abs(d) < np.finfo(np.float32).tiny)).any(-1).sum())
        n["pos_inf"] += int((f[:, :, :3] == np.inf).any(-1).sum())
        n["neg_inf"] += int((f[:, :, :3] == -np.inf).any(-1).sum())
        n["nan"] += int(np.isnan(f[:, :, :3]).any(-1).sum())
    return n


def pack(cases):
    """cases: dicts with w, h, field float32 (h, w, >= 3) and, for the program's `correct`, protect_all, xf (sx, sy, tx, ty, range lower, range upper), ratio."""
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        xf = c.get("xf", XF)
        ms, mt = distance_mapping(xf[4], xf[5])
        field = np.ascontiguousarray(np.asarray(c["field"], np.float32)[:, :, :3])
        assert field.shape == (c["h"], c["w"], 3)
        blob += [struct.pack("<4i", c["w"], c["h"], int(c.get("protect_all", 0)), 0),
                 np.array([xf[0], xf[1], xf[2], xf[3], ms, mt, c.get("ratio", RATIOS[0])], np.float64).tobytes(), field.tobytes()]
    return b"".join(blob)


def run_compare(exe, cases, tmp, name="cases.bin"):
    """-> (exit status, the program's JSON)."""
    path = os.path.join(str(tmp), name)
    with open(path, "wb") as f:
        f.write(pack(cases))
    r = subprocess.run([exe, "compare", path], capture_output=True, text=True)
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-4000:])
    return r.returncode, json.loads(r.stdout)


def run_correct(exe, cases, tmp, name="correct.bin"):
    """The shapeless error correction of every case by the host walk -> list of float32 (h, w, 3)."""
    path, out = os.path.join(str(tmp), name), os.path.join(str(tmp), name+".out")
    with open(path, "wb") as f:
        f.write(pack(cases))
    r = subprocess.run([exe, "correct", path, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    flat = np.fromfile(out, np.float32)
    res, at = [], 0
    for c in cases:
        n = c["w"]*c["h"]*3
        res.append(flat[at:at+n].reshape(c["h"], c["w"], 3))
        at += n
    assert at == flat.size
    return res
