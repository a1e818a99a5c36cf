"""Shared by the framing tests (test_frame_host.py, test_gpu_frame.py): the recorded reference data of tests/golden/frame.npz (tools/make_golden_frame.py)
and the host build of the device's framing helpers (tests/frame_host)."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import load_npz
from msdfgen_amd import lib as L
from msdfgen_amd.shape import ShapeBatch

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((8, 8), (32, 32), (48, 64), (64, 48))
RANGES = ((1, -2., 2.), (1, -1., 3.), (0, -.125, .125))          # -pxrange 4, -apxrange -1 3, -range 0.25 as (range_mode, lower, upper)
LARGE = 1e240                                                   # Shape::getBounds' LARGE_VALUE: the bounds of an empty shape stay at +-LARGE


def golden():
    z = load_npz("frame.npz")
    n = len(z["batch_names"])
    batch = ShapeBatch(z["batch_gco"].astype(np.int32), z["batch_co"].astype(np.int32), z["batch_points"], z["batch_types"].astype(np.int32),
                       z["batch_colors"].astype(np.int32), np.zeros(n, np.uint8), [str(s) for s in z["batch_names"]])
    m = len(z["raw_names"])
    raw = ShapeBatch(z["raw_gco"].astype(np.int32), z["raw_co"].astype(np.int32), z["raw_points"], z["raw_types"].astype(np.int32),
                     np.full(len(z["raw_types"]), 7, np.int32), np.zeros(m, np.uint8), [str(s) for s in z["raw_names"]])
    return z, batch, raw


def build_host(tmp):
    so = os.path.join(str(tmp), "libframe_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "frame_host", "frame_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.bounds_host.argtypes = [C.c_int, L._ip, L._dp, L._bp, L._bp, L._dp]
    lib.frame_host.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, L._dp, L._dp]
    return lib


def host_bounds(lib, shape):
    co = np.ascontiguousarray(shape.contour_offsets, np.int32)
    ne = shape.n_edges
    pts = np.zeros((max(ne, 1), 8))
    pts[:ne] = np.asarray(shape.points, np.float64).reshape(-1, 8)
    types = np.ones(max(ne, 1), np.uint8)
    types[:ne] = shape.types
    cols = np.full(max(ne, 1), 7, np.uint8)
    out = np.zeros(4)
    lib.bounds_host(shape.n_contours, L.ptr(co, L._ip), L.ptr(pts, L._dp), L.ptr(types, L._bp), L.ptr(cols, L._bp), L.ptr(out, L._dp))
    return out


def host_frame(lib, mode, lower, upper, scale, w, h, bounds):
    """frameGlyph of the host build: xf row (sx, sy, tx, ty, mapScale, mapTranslate), or None when the frame cannot fit."""
    b = np.ascontiguousarray(bounds, np.float64)
    xf = np.zeros(6)
    ok = lib.frame_host(mode, int(scale is not None), lower, upper, scale or 1., scale or 1., w, h, L.ptr(b, L._dp), L.ptr(xf, L._dp))
    return xf if ok else None


def frame_matrix():
    """(width, height, range index, given scale or None) of the issue's matrix, in the order of frame.npz's metrics rows per shape."""
    return [(w, h, ri, 20. if scaled else None) for (w, h) in SIZES for ri in range(len(RANGES)) for scaled in (0, 1)]
