"""Binding for tests/devmath (the product's device headers behind one-element-per-lane gfx950 kernels; see devmath.hip). ctypes only: the process that
loads it opens the GPU, so tests/test_gpu_devmath.py does that in a child (tests/devmath_gpu_child.py).

Every method pads its inputs to a multiple of 64 elements (element i = lane i%64 of wavefront i/64) by repeating the last element, and trims the results."""
import ctypes as C
import os
import subprocess

import numpy as np

from msdfgen_amd import build as B

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devmath")
SRC = os.path.join(HERE, "devmath.hip")
SO = os.path.join(HERE, "libdevmath.so")


def build(csrc=B.CSRC, extra=(), so=SO):
    """The product's compiler, exactly its flags, its headers: the helpers compile as they do in the product. csrc / extra / so: for builds against a mutated
    copy of the headers (showing that a test can fail); the tests use the defaults."""
    srcs = [SRC]+[os.path.join(csrc, f) for f in sorted(os.listdir(csrc))]+[os.path.join(B.ROOT, "include", "msdfgen_hip.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([B.hipcc()]+B.HIPCC_FLAGS+list(extra)+["-I", csrc, SRC, "-o", so], check=True)
    return so


def _pad(a, dtype, width=1):
    a = np.ascontiguousarray(a, dtype).reshape(-1, width) if width > 1 else np.ascontiguousarray(a, dtype).reshape(-1)
    n = len(a)
    assert n > 0
    m = -n % 64
    if m:
        a = np.concatenate([a, np.repeat(a[-1:], m, 0)])
    return np.ascontiguousarray(a), n


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class DevMath:
    def __init__(self, so=None):
        self.lib = C.CDLL(so or build())

    def _call(self, name, *args):
        status = getattr(self.lib, name)(*args)
        if status != 0:
            raise RuntimeError("%s: HIP status %d" % (name, status))

    def arch(self):
        buf = C.create_string_buffer(256)
        self._call("devmath_arch", buf, 256)
        return buf.value.decode()

    def sqrt(self, x, compiler=False):
        """msdfSqrt, or the compiler's sqrt. The lane layout is the caller's: x is padded at the END only."""
        x, n = _pad(x, np.float64)
        y = np.zeros(len(x))
        self._call("devmath_sqrt", _p(x), C.c_long(len(x)), int(compiler), _p(y))
        return y[:n]

    def div(self, a, b):
        """(divSafe(b), divExact(a, b, 1/b), a/b), the reciprocal and the quotient by the device's own IEEE division."""
        a, n = _pad(a, np.float64)
        b, _ = _pad(b, np.float64)
        assert len(a) == len(b)
        safe, q, ieee = np.zeros(len(a), np.int32), np.zeros(len(a)), np.zeros(len(a))
        self._call("devmath_div", _p(a), _p(b), C.c_long(len(a)), _p(safe), _p(q), _p(ieee))
        return safe[:n] != 0, q[:n], ieee[:n]

    def cos_thirds(self, t):
        t, n = _pad(t, np.float64)
        c = np.zeros((len(t), 3))
        self._call("devmath_cos_thirds", _p(t), C.c_long(len(t)), _p(c))
        return c[:n]

    def pow_third(self, x):
        x, n = _pad(x, np.float64)
        y = np.zeros(len(x))
        self._call("devmath_pow_third", _p(x), C.c_long(len(x)), _p(y))
        return y[:n]

    def acos(self, x):
        x, n = _pad(x, np.float64)
        y = np.zeros(len(x))
        self._call("devmath_acos", _p(x), C.c_long(len(x)), _p(y))
        return y[:n]

    def solve_quadratic(self, abc):
        abc, n = _pad(abc, np.float64, 3)
        count, roots = np.zeros(len(abc), np.int32), np.zeros((len(abc), 2))
        self._call("devmath_solve_quadratic", _p(abc), C.c_long(len(abc)), _p(count), _p(roots))
        return count[:n], roots[:n]

    def solve_cubic_normed_pre(self, a, b, c):
        """solveCubicNormed(a, b, c) the way sdQuadratic calls it: a*a and a*(1/3.) as buildRecord forms them. -> (count, roots, trigonometric branch taken)"""
        a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
        arg, n = _pad(np.stack([a, a*a, a*(1/3.), b, c], 1), np.float64, 5)
        count, roots, branch = np.zeros(len(arg), np.int32), np.zeros((len(arg), 3)), np.zeros(len(arg), np.int32)
        self._call("devmath_solve_cubic_normed_pre", _p(arg), C.c_long(len(arg)), _p(count), _p(roots), _p(branch))
        return count[:n], roots[:n], branch[:n] != 0

    def signed_distance(self, types, pts, org):
        """-> ((distance, dot, param) per row, the record's REC_* flags)"""
        pts, n = _pad(pts, np.float64, 8)
        org, _ = _pad(org, np.float64, 2)
        types, _ = _pad(types, np.int32)
        out, flags = np.zeros((len(pts), 3)), np.zeros(len(pts), np.int32)
        self._call("devmath_signed_distance", _p(pts), _p(types), _p(org), C.c_long(len(pts)), _p(out), _p(flags))
        return out[:n], flags[:n]

    def map_distance(self, scale, translate, d):
        d, n = _pad(d, np.float64)
        scale, _ = _pad(np.broadcast_to(np.asarray(scale, np.float64), (n,)), np.float64)
        translate, _ = _pad(np.broadcast_to(np.asarray(translate, np.float64), (n,)), np.float64)
        out = np.zeros(len(d), np.float32)
        self._call("devmath_map_distance", _p(scale), _p(translate), _p(d), C.c_long(len(d)), _p(out))
        return out[:n]

    def float_above(self, d):
        d, n = _pad(d, np.float64)
        out = np.zeros(len(d), np.float32)
        self._call("devmath_float_above", _p(d), C.c_long(len(d)), _p(out))
        return out[:n]

    def wave_min(self, v, rows=False):
        """waveMinNonNegative per 64 values (rows: rowMinNonNegative per 16). len(v) must be a multiple of 64: the layout is the test."""
        v = np.ascontiguousarray(v, np.float32).reshape(-1)
        assert len(v) and len(v) % 64 == 0
        out = np.zeros(len(v), np.float32)
        self._call("devmath_wave_min", _p(v), C.c_long(len(v)), int(rows), _p(out))
        return out

    def row_rank(self, keys):
        keys = np.ascontiguousarray(keys, np.uint32).reshape(-1)
        assert len(keys) and len(keys) % 64 == 0
        out = np.zeros(len(keys), np.int32)
        self._call("devmath_row_rank", _p(keys), C.c_long(len(keys)), _p(out))
        return out
