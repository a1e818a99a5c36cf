"""The arithmetic primitives of the device build (msdf_device.hpp, msdf_prep.hpp and the wave helpers of msdf_kernels.hpp), run on gfx950 one element per
lane by the test-only harness tests/devmath and compared with plain high-precision references -- not through glyphs.

msdfSqrt (lean core and voted compiler path), divSafe / divExact, cosThirds, powThird, OCML's acos, solveQuadratic, solveCubicNormedPre, signedDistance of a
record built by buildRecord, mapDistance, floatAbove, waveMinNonNegative, rowMinNonNegative, rowRank; and one product call: texel centres exactly on an edge's
start point (the -0 dividend of divExact) through GlyphBatch.generate against the oracle.

References: np.sqrt and numpy's fp64 + - * / (correctly rounded IEEE operations), np.longdouble (64-bit significand) for the bulk of the transcendental inputs,
mpmath at 200 bits for the hand-picked ones (longdouble if mpmath is missing), tests/golden/kats.npz and the oracle for the solvers and the edge distances,
the host build of the same headers (tests/hostemu, -DMSDF_LEAN_MATH) where bit equality with the device is derivable.

Every device call is made by ONE child process (tests/devmath_gpu_child.py) under a time limit of its own, CHILD_TIMEOUT seconds; this process never opens the
GPU and only compares what the child wrote.

Wall time on one MI355X with 16 CPUs: the child 2.7 s (1.8 s for torch, device start and the product call, 0.35 s for the 30 harness calls on 13 M input values
in all, the rest writing the .npz), plus 7 s once when tests/devmath/libdevmath.so has to be compiled first; each comparison 0.01-0.25 s; the whole file 4-7 s
(3 s of it the host build of the headers, when that is stale)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bit_equal, load_npz
import devmathcases as D
from devmathcases import u64, differs, assert_same, check_division, check_zero_dividends
import devmath_gpu_child as child

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120          # seconds

try:
    import mpmath
    mpmath.mp.prec = 200
except ImportError:          # the hand-picked inputs then take the longdouble reference too
    mpmath = None


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """What the child computed on the GPU. A child that faults, hangs into its limit or returns non-zero fails every test here."""
    out = os.path.join(str(tmp_path_factory.mktemp("devmath_gpu")), "device.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable]+flags+[child.__file__, out], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout.strip())
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def lean_emu():
    from emu import Emu
    return Emu(lean=True)


def ulp_errors(out, args, n_bulk, fn_ld, fn_mp):
    """|out-f(args)| in units of the reference's fp64 ulp: f in longdouble for args[:n_bulk], in mpmath (200 bits) for the hand-picked rest. Only finite
    references count (the callers pin the others exactly)."""
    out, args = np.asarray(out, np.float64), np.asarray(args, np.float64)
    err = np.zeros(out.shape)
    with np.errstate(all="ignore"):
        ref = fn_ld(args.astype(np.longdouble))
        ulp = np.spacing(np.abs(ref.astype(np.float64)))
        ok = np.isfinite(ref) & np.isfinite(out)
        err[ok] = (np.abs(out.astype(np.longdouble)-ref)[ok]/ulp[ok]).astype(np.float64)
        err[~ok & ~(np.isinf(ref) & (out == ref.astype(np.float64)))] = np.inf
    if mpmath is not None:
        flat_o, flat_a, flat_e = out.reshape(-1), args.reshape(-1), err.reshape(-1)
        per = out.size//len(out)
        for i in range(n_bulk*per, out.size):
            if np.isfinite(flat_a[i]) and np.isfinite(flat_o[i]):
                r = fn_mp(mpmath.mpf(float(flat_a[i])))
                flat_e[i] = float(abs(mpmath.mpf(float(flat_o[i]))-r)/mpmath.mpf(float(np.spacing(abs(float(r))))))
    return err


# ------------------------------------------------------------------------------------------------------------------ square root

def test_square_root_is_correctly_rounded_on_both_paths(device):
    """msdfSqrt against np.sqrt (IEEE, correctly rounded), every value bitwise: 4.23 M in-range values in wavefronts that all take leanSqrtCore (random
    significands over the exponents -767..1023, 2^-767 and its upper neighbour, perfect squares and their neighbours from 26- and 53-bit roots, all-ones
    significands, powers of two and their neighbours for every exponent, and 15 818 arguments whose root lies within 2^-44 ulp of a midpoint between two fp64
    values (devmathcases._sqrt_hard_cases: only these tell the core's last Newton correction from its absence -- 4 M random arguments do not), then 12 x 64 wavefronts in which exactly one lane holds a value outside [2^-767, inf) -- 0, -0,
    subnormals, values below 2^-767 (its lower neighbour among them), +inf, NaN, negative numbers: the vote sends all 64 lanes through the compiler's sqrt,
    whose in-range lanes must give the same bits as the lean core does, and whose special lane must give what IEEE gives. The compiler's sqrt alone likewise."""
    x, n_lean = D.sqrt_inputs()
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)
    special = np.zeros(len(x), bool)
    special[n_lean:].reshape(-1, 64, 64)[:, np.arange(64), np.arange(64)] = True
    assert (x[~special] >= D.LEAN_SQRT_MIN).all() and not ((x[special] >= D.LEAN_SQRT_MIN) & (x[special] < np.inf)).any()
    for name in ("sqrt_lean", "sqrt_compiler"):
        got = device[name]
        print("%s: %d of %d differ from np.sqrt (lean-path wavefronts %d, voted wavefronts' in-range lanes %d, special lanes %d)" % (
            name, differs(got, want).sum(), len(x), differs(got[:n_lean], want[:n_lean]).sum(), differs(got[n_lean:], want[n_lean:])[~special[n_lean:]].sum(),
            differs(got, want)[special].sum()))
    assert_same(device["sqrt_lean"][:n_lean], want[:n_lean], "msdfSqrt, wavefronts on the lean path", x[:n_lean])
    assert_same(device["sqrt_lean"][n_lean:], want[n_lean:], "msdfSqrt, wavefronts with one out-of-range lane", x[n_lean:])
    assert_same(device["sqrt_compiler"], want, "the compiler's sqrt", x)
    assert np.isnan(device["sqrt_lean"][special][np.isnan(want[special])]).all()


# -------------------------------------------------------------------------------------------------------------- transcendentals

def test_cos_thirds_is_within_one_ulp_and_equals_the_host_build(device, lean_emu):
    """cosThirds on the device: < 1 ulp against the high-precision cosine of exactly the reference's fp64 arguments (equation-solver.cpp:50-52), and bitwise
    what the host build of the same text gives -- cosKernel / sinKernel / reduceFrom are fixed sequences of fp64 + - * and conversions, so with contraction off
    in both builds equality is derivable; a contracted multiply-add in the device compile breaks it."""
    import ctypes as C
    t, n_bulk = D.cos_thirds_inputs()
    got = device["cos_thirds"]
    third, twopi = np.float64(1)/np.float64(3), np.float64(2)*np.float64(np.pi)
    args = np.stack([third*t, third*(t+twopi), third*(t-twopi)], 1)
    err = ulp_errors(got, args, n_bulk, np.cos, (lambda v: mpmath.cos(v)))
    print("cosThirds max ulp error on the device: %s (bulk), %s (hand-picked, %s)" % (err[:n_bulk].max(0), err[n_bulk:].max(0), "mpmath" if mpmath else "longdouble"))
    host = np.zeros((len(t), 3))
    lean_emu.lib.emu_lean_cos_thirds(t.ctypes.data_as(C.POINTER(C.c_double)), C.c_long(len(t)), host.ctypes.data_as(C.POINTER(C.c_double)))
    print("cosThirds device vs host build: %d of %d values differ" % (differs(got, host).sum(), got.size))
    assert err.max() < 1.0, (err.max(0), t[err.max(1).argmax()])
    assert_same(got, host, "cosThirds, device build vs host build", t.repeat(3))


def test_pow_third_is_within_one_ulp(device, lean_emu):
    """powThird: < 1 ulp against x^(1/3.) with the fp64-rounded exponent (the reference's pow(x, 1/3.)); 0 and +inf exactly. The count of inputs on which the
    device differs from the host build (their fp32 seeds come from OCML's and from glibc's exp2f / log2f) is printed, not asserted: DESIGN.md 4 records it."""
    import ctypes as C
    x, n_bulk = D.pow_third_inputs()
    got = device["pow_third"]
    third = np.float64(1)/np.float64(3)
    err = ulp_errors(got, x, n_bulk, (lambda v: np.power(v, np.longdouble(third))), (lambda v: mpmath.power(v, mpmath.mpf(float(third)))))
    host = np.zeros(len(x))
    lean_emu.lib.emu_lean_pow_third(x.ctypes.data_as(C.POINTER(C.c_double)), C.c_long(len(x)), host.ctypes.data_as(C.POINTER(C.c_double)))
    print("powThird max ulp error on the device: %.4f (bulk), %.4f (hand-picked); device vs host build: %d of %d inputs differ bitwise (%d of the %d bulk ones)" % (
        err[:n_bulk].max(), err[n_bulk:].max(), differs(got, host).sum(), len(x), differs(got, host)[:n_bulk].sum(), n_bulk))
    assert err.max() < 1.0, (err.max(), x[err.argmax()], got[err.argmax()])
    assert got[x == 0][0] == 0 and not np.signbit(got[x == 0][0]) and (got[np.isinf(x)] == np.inf).all()


def test_acos_is_within_one_ulp(device, lean_emu):
    """OCML's acos as the device build of solveCubicNormedPre calls it: < 1 ulp, acos(1) == 0 exactly. The count of inputs on which it differs from this
    machine's libm (what the host build calls) is printed, not asserted: DESIGN.md 4 records it."""
    import ctypes as C
    x, n_bulk = D.acos_inputs()
    got = device["acos"]
    err = ulp_errors(got, x, n_bulk, np.arccos, (lambda v: mpmath.acos(v)))
    host = np.zeros(len(x))
    lean_emu.lib.emu_libm_acos(x.ctypes.data_as(C.POINTER(C.c_double)), C.c_long(len(x)), host.ctypes.data_as(C.POINTER(C.c_double)))
    d = differs(got, host)
    print("acos max ulp error on the device: %.4f (bulk), %.4f (hand-picked); device vs libm: %d of %d inputs differ bitwise (%d of the %d bulk ones), by at most %g ulp" % (
        err[:n_bulk].max(), err[n_bulk:].max(), d.sum(), len(x), d[:n_bulk].sum(), n_bulk, (np.abs(got-host)/np.spacing(np.abs(host)+5e-324)).max()))
    assert err.max() < 1.0, (err.max(), x[err.argmax()], got[err.argmax()])
    assert (got[x == 1] == 0).all() and not np.signbit(got[x == 1]).any()


# ------------------------------------------------------------------------------------------------------------------- division

def test_reciprocal_division_equals_ieee_inside_its_stated_domain(device):
    """divSafe and divExact on the device, the reciprocal RN(1/b) formed there as buildRecord forms it. Families: the host test's own draw; quotients within an
    ulp of a representable value and within 2^-52 ulp of a tie; divisors at both ends of divSafe's range (and just outside); all-ones significands (refused);
    dividends from the subnormals up past 2^-969; dividends in [2^-969, 2^-959) with normal quotients; quotients up to and past overflow; zero dividends of
    either sign over divisors of either sign. The device's own IEEE division is compared with numpy's on all of them as well."""
    fams = D.div_inputs()
    seen_small = False
    for name, (a, b) in fams.items():
        safe, q, ieee_dev = device["div_safe_"+name], device["div_q_"+name], device["div_ieee_"+name]
        with np.errstate(all="ignore"):
            assert_same(ieee_dev, a/b, "the device's IEEE division, family "+name, np.stack([a, b], 1))
        dom, bad_out = check_division(name, a, b, safe, q, print)
        if name == "ones":
            assert not safe.any()
        if name == "host":
            assert not safe[2000:3000].any() and len(a)-1500 < safe.sum() < len(a)
        if name == "small":
            seen_small = bool(bad_out.any())           # the domain's lower edge is not vacuous: below it divExact does depart from IEEE
        if name == "ends":
            assert safe.sum() == len(a)//2 and (dom == safe).all()         # half of the divisors lie just outside divSafe's range, 1e-100 and 1e100 themselves too
        if name in ("edge", "ties", "near_exact", "zero"):
            assert dom.sum() > .9*len(a), name
    assert seen_small
    a, b = fams["zero"]
    check_zero_dividends(lambda aa, bb: np.array([device["div_q_zero"][np.nonzero((u64(a) == u64(x)) & (b == y))[0][0]] for x, y in zip(aa, bb)]))


def test_texels_on_an_edges_start_point_equal_the_oracle(device, oracle):
    """The one place a zero quotient's sign could show: a texel centre exactly ON the start point of a linear, quadratic and cubic edge, running down-left
    (dot(o-p0, ab) = -0) and up-right (-dot(p0-o, direction(0)) = -0), all four modes at 8x8, batched route, against the oracle bit for bit."""
    shapes = D.start_point_glyphs()
    w, h = D.GLYPH_SIZE
    for s in shapes:
        p0 = s.points[0, :2]
        assert (p0-.5 == np.floor(p0)).all() and 0 < p0[0] < w and 0 < p0[1] < h
    for mode in (1, 2, 3, 4):
        want = np.stack([oracle.generate(s, mode, w, h, D.GLYPH_XF) for s in shapes])
        assert_bit_equal(device["tiles_%d" % mode], want, "start-point glyphs, mode %d" % mode)


# -------------------------------------------------------------------------------------------------------------------- solvers

def roots_equal(n_got, x_got, n_want, x_want, what, rows):
    assert (n_got == n_want).all(), (what, np.nonzero(n_got != n_want)[0][:5], rows[n_got != n_want][:5])
    live = np.arange(x_got.shape[1])[None, :] < np.maximum(n_want, 0)[:, None]
    assert_same(np.where(live, x_got, 0), np.where(live, x_want, 0), what, np.repeat(rows, x_got.shape[1], 0))


def test_solve_quadratic_equals_the_reference(device, oracle):
    """Root count and roots bitwise: the recorded answers of the reference (kats.npz) and, on the branch edges (a == 0; |b| at, just above and just below
    1e12|a|; dscr == 0 exactly; b == c == 0) and a random draw, the oracle's."""
    z = load_npz("kats.npz")
    roots_equal(device["quad_kat_n"], device["quad_kat_x"], z["quad_out"][:, 0].astype(np.int32), z["quad_out"][:, 1:], "solveQuadratic, KAT rows", z["cubic_coef"][:, 1:])
    rows = D.quadratic_inputs()
    want_n, want_x = np.zeros(len(rows), np.int32), np.zeros((len(rows), 2))
    for i, r in enumerate(rows):
        want_n[i], want_x[i] = oracle.solve_quadratic(*r)
    print("solveQuadratic fuzz: root counts -1/0/1/2: %s" % [int((want_n == k).sum()) for k in (-1, 0, 1, 2)])
    assert all((want_n == k).sum() > 100 for k in (-1, 0, 1, 2))
    roots_equal(device["quad_n"], device["quad_x"], want_n, want_x, "solveQuadratic, branch edges", rows)


def check_cubic(what, rows, n_got, x_got, trig_got, n_want, x_want):
    """solveCubicNormedPre on the device (OCML's acos, the lean cosines and cube root) against the reference's answers (glibc's acos / cos / pow): all of them
    < 1 ulp functions, so the roots agree up to what two such functions can differ by -- derived from the expressions of equation-solver.cpp:34-61:

    cube-root branch, x = (u+v)-a3 with u = -+powThird(A), v = q/u; A, q and a3 are the same fp64 values on both sides. Two < 1 ulp values of A^(1/3.) differ by
    < 2 ulp(u) <= 2^-51 |u|; v then by < 2^-51 |v| (the divisor's relative change) + 2^-52 |v| (its own rounding); u+v rounds to within an ulp of one another on
    top of that, <= 2^-52 (|u|+|v|); the subtraction of a3 adds an ulp of x. Sum: 1.5*2^-51 (|u|+|v|) + 2^-52 (|u|+|v|) = 2^-50 (|u|+|v|), plus 2^-52 |x|. The
    second root -.5*(u+v)-a3 stays inside the same bound.

    trigonometric branch, x = Q*cos(1/3.*(T+k*2pi))-a3 with Q = -2 sqrt(q) (correctly rounded: the same on both sides) and T = acos(t) in [0, pi], in units of
    2^-53. Two values of T, each < 1 ulp from acos(t), differ by < 2 ulp(T) <= 8 units. The widest chain is k = 1: T+2pi rounds on a grid of 16 units (sums >= 8),
    so the two sums differ by < 8+16, their thirds by < 8, and the product with 1/3. rounds on a grid of 4: the arguments differ by < 12 units and so do their
    cosines (|sin| <= 1); two < 1 ulp cosines of ONE argument differ by < 2 ulp <= 2 units; the product with Q rounds, <= 2 units of |Q|: 16*2^-53 |2 sqrt(q)|,
    plus the ulp of x from the final subtraction, 2^-52 |x|. That figure needs the two acos on opposite sides of the true value at nearly a full ulp each and every
    rounding to fall the same way. ASSERTED is half of it, 8*2^-53 |2 sqrt(q)| + 2^-52 |x|: the two acos measured here differ by one ulp at most (4 units; the acos
    test prints it), which through the same chain gives (4+8)/3+4+2+2 = 12 for sums below 8 and 16 above -- still the worst fall of every rounding -- so 8 is a
    bound a correct kernel can in principle exceed by rounding luck, never by much; the largest ratio seen is printed (0.49 when written), and a ratio between
    1 and 2 would have to be read against the 16-unit derivation before blaming the kernel.

    Where no inexact transcendental enters (A == 0: u = v = 0), the roots must be bitwise equal; the root counts always."""
    a, b, c = rows.T
    q, r, r2, q3 = D.cubic_terms(a, b, c)
    trig = r2 < q3
    assert (trig_got == trig).all(), (what, "the branch the device took", np.nonzero(trig_got != trig)[0][:5])
    assert (n_got == n_want).all(), (what, "root counts", np.nonzero(n_got != n_want)[0][:5], rows[n_got != n_want][:5])
    with np.errstate(all="ignore"):
        A = np.abs(r)+np.sqrt(np.where(trig, 0, r2-q3))
        u = np.power(A.astype(np.longdouble), np.longdouble(np.float64(1)/np.float64(3))).astype(np.float64)
        v = np.where(u == 0, 0, q/np.where(u == 0, 1, u))
        Q = 2*np.sqrt(np.where(trig, q, 0))
    live = np.arange(3)[None, :] < n_want[:, None]
    bound = np.where(trig, 8*2.0**-53*Q, 2.0**-50*(np.abs(u)+np.abs(v)))[:, None]+2.0**-52*np.abs(x_want)
    diff = np.where(live, np.abs(x_got-x_want), 0)
    exact = ~trig & (A == 0)
    ratio = np.where(live & (bound > 0), diff/np.where(bound > 0, bound, 1), 0)
    nd = differs(np.where(live, x_got, 0), np.where(live, x_want, 0))
    print("%s: %d rows (%d trigonometric, %d cube-root, %d with A == 0, %d with r2 == q3, %d two-root exits); roots differing bitwise: %d of %d trigonometric, "
          "%d of %d cube-root; largest |difference|/bound: %.3f trigonometric, %.3f cube-root" % (
              what, len(rows), trig.sum(), (~trig).sum(), exact.sum(), (r2 == q3).sum(), (n_want == 2).sum(), nd[trig].sum(), live[trig].sum(), nd[~trig].sum(),
              live[~trig].sum(), ratio[trig].max(initial=0), ratio[~trig].max(initial=0)))
    assert_same(np.where(live, x_got, 0)[exact], np.where(live, x_want, 0)[exact], what+": no transcendental involved")
    worst = np.unravel_index(ratio.argmax(), ratio.shape)
    assert (diff <= bound).all(), (what, rows[worst[0]], x_got[worst[0]], x_want[worst[0]], ratio.max())
    return trig, q3, r, n_want, exact


def test_solve_cubic_normed_follows_the_reference(device, oracle):
    z = load_npz("kats.npz")
    idx, rows = child.kat_normed_rows(z)
    assert len(idx) > 200
    check_cubic("solveCubicNormedPre, KAT rows", rows, device["cubic_kat_n"], device["cubic_kat_x"], device["cubic_kat_trig"],
                z["cubic_out"][idx, 0].astype(np.int32), z["cubic_out"][idx, 1:])
    rows = D.cubic_inputs()
    want_n, want_x = np.zeros(len(rows), np.int32), np.zeros((len(rows), 3))
    for i, r in enumerate(rows):
        want_n[i], want_x[i] = oracle.solve_cubic(1., *r)            # b/1, c/1, d/1 are exact: solveCubicNormed(a, b, c) itself
    trig, q3, r, n_want, exact = check_cubic("solveCubicNormedPre, branch edges", rows, device["cubic_n"], device["cubic_x"], device["cubic_trig"], want_n, want_x)
    with np.errstate(all="ignore"):
        clamped = trig & (np.abs(r/np.sqrt(q3)) >= 1)
    print("branch edges: %d rows with t clamped at +-1 or exactly there" % clamped.sum())
    assert clamped.sum() >= 10 and (clamped & (r > 0)).any() and (clamped & (r < 0)).any()      # t clamped at +1 and at -1
    assert (r*r == q3).sum() >= 10 and exact.sum() >= 2 and ((n_want == 2) & ~exact).sum() >= 10


def test_signed_distance_of_built_records_equals_the_reference(device):
    """buildRecord + signedDistance on the 3 x 200 recorded rows of the reference: linear and cubic edges use no transcendental, so distance, dot and param are
    bitwise equal; for quadratic edges the count is reported and the mapped distances (mapDistance, what reaches a texel) are equal or adjacent fp32 values.
    mapDistance itself is one fp64 add, one multiply and a conversion: bitwise numpy's."""
    z = load_npz("kats.npz")
    want = np.concatenate([z["sd%d_out" % t] for t in (1, 2, 3)])
    got = device["sd"]
    for k, t in enumerate((1, 2, 3)):
        sl = slice(200*k, 200*k+200)
        print("signedDistance type %d: %d of 200 rows differ bitwise (distance %d, dot %d, param %d); %d records take the reciprocal division" % (
            t, differs(got[sl], want[sl]).any(1).sum(), *differs(got[sl], want[sl]).sum(0), (device["sd_flags"][sl]&16 != 0).sum()))
    assert (device["sd_flags"]&16 != 0).sum() > 500           # REC_FASTDIV: the rows go through divExact
    assert_same(got[:200], want[:200], "signedDistance, linear edges")
    assert_same(got[400:], want[400:], "signedDistance, cubic edges")
    d = np.concatenate([got[:, 0], want[:, 0]])
    for k, (scale, translate) in enumerate(child.MAPPINGS):
        m = device["map_%d" % k]
        assert_bit_equal(m, (np.float64(scale)*(d+np.float64(translate))).astype(np.float32), "mapDistance %d" % k)
        mg, mw = m[200:400], m[800:1000]
        adjacent = (mg == mw) | (np.nextafter(mg, mw) == mw)
        print("mapDistance (scale %g, translate %g) of the quadratic rows: %d of 200 differ" % (scale, translate, (mg != mw).sum()))
        assert adjacent.all(), (k, mg[~adjacent], mw[~adjacent])


# --------------------------------------------------------------------------------------------------------------- wave helpers

def test_wave_minimum_reaches_every_lane_from_every_lane(device):
    """waveMinNonNegative: the unique minimum in each of the 64 lane positions in turn, ties, all +inf, one finite value among +inf, +0 and subnormals, random
    wavefronts: every lane returns the bits of numpy's minimum."""
    v = D.wave_min_inputs()
    want = np.repeat(v.min(1, keepdims=True), 64, 1)
    got = device["wave_min"]
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "waveMinNonNegative: %d wavefronts wrong, first %d: lanes %s got %s want %s (minimum in lane %s)" % (
        bad.any(1).sum(), bad.any(1).argmax(), np.nonzero(bad[bad.any(1).argmax()])[0].tolist(), got[bad.any(1).argmax()][bad[bad.any(1).argmax()]][:4],
        want[bad.any(1).argmax(), 0], v[bad.any(1).argmax()].argmin())


def test_row_minimum_stays_within_its_row(device):
    """rowMinNonNegative: the row's minimum at each of its 16 positions, for each of the 4 rows, with SMALLER values in the other rows: nothing leaks across."""
    v = D.row_min_inputs()
    want = np.repeat(v.reshape(-1, 4, 16).min(2), 16, 1)
    got = device["row_min"]
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "rowMinNonNegative: %d wavefronts wrong, first %d: lanes %s" % (bad.any(1).sum(), bad.any(1).argmax(), np.nonzero(bad[bad.any(1).argmax()])[0].tolist())


def test_row_rank_equals_argsort(device):
    """rowRank: random permutations of 16 unique keys per row, sorted and reversed rows, keys that differ only in their top bits (the compare is unsigned)."""
    keys = D.row_rank_inputs().reshape(-1, 4, 16)
    want = keys.argsort(2).argsort(2).reshape(-1, 64)
    got = device["row_rank"]
    bad = got != want
    assert not bad.any(), "rowRank: %d wavefronts wrong, first %d: lanes %s got %s want %s" % (
        bad.any(1).sum(), bad.any(1).argmax(), np.nonzero(bad[bad.any(1).argmax()])[0].tolist(), got[bad.any(1).argmax()].tolist(), want[bad.any(1).argmax()].tolist())


def test_float_above_is_the_smallest_float_not_below(device):
    """floatAbove(d), d >= 0: values just above and just below fp32 values, fp32 values themselves (subnormal and FLT_MAX too), 0, values below the smallest
    subnormal and above FLT_MAX: the result is >= d, and its lower fp32 neighbour is not."""
    d = D.float_above_inputs()
    got = device["float_above"]
    assert (got.astype(np.float64) >= d).all(), d[~(got.astype(np.float64) >= d)][:5]
    below = np.nextafter(got, np.float32(-np.inf))
    tight = (below.astype(np.float64) < d) | (d == 0)
    assert tight.all(), (d[~tight][:5], got[~tight][:5])
    assert (got[d == 0] == 0).all()
