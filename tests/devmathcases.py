"""Inputs of tests/test_gpu_devmath.py, built the same way by the GPU child (tests/devmath_gpu_child.py) and by the comparing parent; and the division
families that tests/test_device_logic_host.py runs through the host build as well. numpy only, fixed seeds."""
import numpy as np

from msdfgen_amd.shape import FlatShape

LEAN_SQRT_MIN = 2.0**-767            # msdfSqrt: the lean core serves [2^-767, inf)
DIV_MIN_DIVIDEND = 2.0**-969         # divExact's documented domain (msdf_device.hpp)
DIV_MIN_QUOTIENT = 2.0**-1021
DIV_MAX_QUOTIENT = 2.0**1023


def _doubles(rng, n, emin, emax):
    """Random significands, exponents uniform over emin..emax (value in [2^e, 2^(e+1)))."""
    sig = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    exp = rng.integers(emin+1023, emax+1024, n, dtype=np.uint64)
    return (sig | exp << np.uint64(52)).view(np.float64)


def _neighbours(x, k):
    """x and its k fp64 neighbours on either side."""
    x = np.asarray(x, np.float64).reshape(-1)
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------------------------ square root

SQRT_SPECIALS = np.array([0., -0., 5e-324, 2.0**-1060, 2.2250738585072014e-308, 2.0**-1000, 2.0**-768, np.nextafter(LEAN_SQRT_MIN, 0), np.inf, np.nan,
                          -1., -2.0**-800])


def _sqrt_hard_cases():
    """Arguments whose square root lies within ~2^-50 ulp of a MIDPOINT between two fp64 values -- where a result that is accurate to 2^-100 before its final
    rounding can still round the wrong way. For an odd 54-bit s (s/2 is a midpoint of 53-bit integers) with s^2 = x*2^n+rho, n = 54 or 55, x a 53-bit integer
    and rho small: sqrt(x*2^n) = s-rho/(2s), i.e. |rho|*2^-55 ulp off the midpoint, on either side of it by the sign of rho. s^2 = rho (mod 2^n) has four roots
    for every rho = 1 (mod 8), found by lifting them bit by bit. rho = 1 gives the classic pair 1+2^-52 and 1-2^-53."""
    out = []
    for n in (54, 55):
        for rho in range(-2047, 2048, 8):
            roots = {1, 3, 5, 7}
            for k in range(3, n):                       # r*r = rho (mod 2^k), r odd -> exactly one of r, r+2^(k-1) works mod 2^(k+1)
                roots = {(r if (r*r-rho) % (1 << (k+1)) == 0 else r+(1 << (k-1))) % (1 << (k+1)) for r in roots}
                roots |= {(1 << (k+1))-r for r in roots}
            for r in roots:
                x = (r*r-rho) >> n
                if r >> 53 == 1 and x >> 52 == 1:        # a 54-bit midpoint pattern and a 53-bit argument
                    assert (r*r-rho) % (1 << n) == 0
                    out.append(np.ldexp(float(x), n+2*np.arange(-380, 420, 37)))     # scaled by powers of 4: the root's significand stays
    return np.unique(np.concatenate(out))


def sqrt_inputs():
    """-> (x, n_lean): x[:n_lean] are whole wavefronts of in-range values only (every wavefront takes leanSqrtCore); after them, one wavefront per
    (special value, lane): 63 in-range values and the special value in that lane (the vote sends all 64 lanes through the compiler's sqrt)."""
    rng = np.random.default_rng(101)
    y26 = np.ldexp(rng.integers(1 << 25, 1 << 26, 200_000).astype(np.float64), rng.integers(-380, 480, 200_000))    # y*y is exact
    y53 = _doubles(rng, 200_000, -380, 505)
    ones = np.ldexp(2-2.0**-52, np.arange(-767, 1024))                                                              # all-ones significands, even and odd exponents
    fam = [_doubles(rng, 3_000_000, -767, 1023), _neighbours(LEAN_SQRT_MIN, 1)[[0, 2]], np.array([np.nextafter(np.inf, 0), 1., 2., 4., 0.25]),
           y26*y26, np.nextafter(y26*y26, np.inf), np.nextafter(y26*y26, -np.inf), y53*y53, np.nextafter(y53*y53, np.inf), np.nextafter(y53*y53, -np.inf),
           ones, _neighbours(np.ldexp(1., np.arange(-766, 1024)), 2), _sqrt_hard_cases()]
    lean = np.concatenate(fam)
    lean = np.concatenate([lean, _doubles(rng, -len(lean) % 64, -767, 1023)])
    assert len(lean) % 64 == 0 and (lean >= LEAN_SQRT_MIN).all() and np.isfinite(lean).all()
    waves = _doubles(rng, len(SQRT_SPECIALS)*64*64, -767, 1023).reshape(len(SQRT_SPECIALS), 64, 64)
    for s, v in enumerate(SQRT_SPECIALS):
        waves[s, np.arange(64), np.arange(64)] = v                # wavefront (s, lane): the special value in lane `lane`
    return np.concatenate([lean, waves.reshape(-1)]), len(lean)


# -------------------------------------------------------------------------------------------------------------- transcendentals

def cos_thirds_inputs():
    """-> (t, n_bulk): t[n_bulk:] are the hand-picked ones (high-precision reference)."""
    rng = np.random.default_rng(17)
    bulk = rng.uniform(0, np.pi, 400_000)
    picked = np.concatenate([[0., np.pi, np.pi/2, 1e-9],
                             _neighbours(3*np.pi/4, 8),      # 1/3.*t at cosZeroToPi's breakpoint pi/4
                             _neighbours(np.pi/4, 8),        # 1/3.*(t+2pi) at the breakpoint 3pi/4
                             _neighbours(np.pi/2, 8),        # |1/3.*(t-2pi)| within a few ulp of pi/2 (the reduction pi/2-x cancels to its tail)
                             _neighbours(np.nextafter(np.pi, 0), 4)[:5]])
    picked = picked[(picked >= 0) & (picked <= np.pi)]
    return np.concatenate([bulk, picked]), len(bulk)


def pow_third_inputs():
    rng = np.random.default_rng(18)
    bulk = np.exp(rng.uniform(-40, 40, 400_000))
    k = rng.integers(1, 1 << 17, 2000).astype(np.float64)
    cubes = np.ldexp(k*k*k, 3*rng.integers(-100, 100, 2000))                                 # exact cubes (k^3 < 2^53)
    picked = np.concatenate([_neighbours(cubes, 1), np.ldexp(1., np.arange(-1022, 1024)),   # powers of two: every e mod 3, negative exponents too
                             [0., 5e-324, 2.0**-1030, np.finfo(np.float64).max, np.inf, 1., 8., 27., .125]])
    return np.concatenate([bulk, picked]), len(bulk)


def acos_inputs():
    rng = np.random.default_rng(19)
    bulk = rng.uniform(-1, 1, 400_000)
    tiny = np.array([5e-324, 1e-300, 1e-17, 2.0**-27, 2.0**-54, 1e-9])
    picked = np.concatenate([[1., -1., 0., -0., 1-2.0**-53, -1+2.0**-53, .5, -.5], tiny, -tiny, _neighbours([.5, -.5, 2.0**-.5, -2.0**-.5], 2),
                             1-np.ldexp(1., -np.arange(2, 53)), -1+np.ldexp(1., -np.arange(2, 53))])
    return np.concatenate([bulk, picked]), len(bulk)


# ------------------------------------------------------------------------------------------------------------------- division

def div_inputs():
    """-> dict of (a, b) families. 'host' is test_reciprocal_fma_division_is_correctly_rounded's own draw (at a sixth of its size)."""
    fam = {}
    rng = np.random.default_rng(3)
    n = 500_000
    a = rng.standard_normal(n)*np.exp(rng.uniform(-30, 30, n))
    b = rng.standard_normal(n)*np.exp(rng.uniform(-30, 30, n))
    a[:1000] = 0
    a[1000:2000] = b[1000:2000]*rng.integers(1, 9, 1000)                 # exact quotients
    b[2000:3000] = np.ldexp(2-2.0**-52, rng.integers(-20, 20, 1000))     # all-ones significands must be rejected by divSafe
    a[3000:4000] = np.nextafter(b[3000:4000]*3, np.inf)                  # quotients next to ties
    fam["host"] = (a, b)
    fam.update(div_edge_inputs())
    return fam


def div_edge_inputs():
    """The families the host fuzz never drew: quotients next to ties, divisors at both ends of divSafe's range, all-ones significands over that whole range,
    dividends down to the subnormals, dividends at the edge of the documented domain, and zero dividends of either sign."""
    fam = {}
    rng = np.random.default_rng(33)
    n = 200_000
    sgn = lambda m: rng.choice([-1., 1.], m)
    b = sgn(n)*_doubles(rng, n, -300, 300)
    a = b*np.ldexp(rng.integers(1 << 52, 1 << 53, n).astype(np.float64), -52)      # a quotient within an ulp of a representable value, either side
    fam["near_exact"] = (np.concatenate([a, np.nextafter(a, np.inf), np.nextafter(a, -np.inf)]), np.concatenate([b, b, b]))
    # Quotients next to TIES. a/b is never a midpoint of two fp64 values, and a random pair is ~2^-2 ulp away from one; here b is an odd 53-bit integer and
    # x = s*b^-1 mod 2^54 an odd 54-bit integer (a midpoint pattern), so that b*x = a*2^54+s with s in {+-1, +-3}: a/b = (x-s/b)*2^-54, i.e. within
    # 2^-52 ulp of the midpoint x, on either side of it.
    ta, tb = [], []
    for _ in range(2500):
        bi = int(rng.integers(1 << 52, 1 << 53)) | 1
        inv = pow(bi, -1, 1 << 54)
        for s in (1, -1, 3, -3):
            x = s*inv % (1 << 54)
            ai = (bi*x-s) >> 54
            if x >> 53 and ai >> 52:
                assert (bi*x-s) % (1 << 54) == 0 and ai < 1 << 53
                ta.append(float(ai)), tb.append(float(bi))
    ta, tb = np.array(ta), np.array(tb)
    e = rng.integers(-200, 200, (2, len(ta)))
    fam["ties"] = (sgn(len(ta))*np.ldexp(ta, e[0]), sgn(len(ta))*np.ldexp(tb, e[0]+e[1] % 60-30))
    lo, hi = np.nextafter(1e-100, 1), np.nextafter(1e100, 0)            # the smallest and largest divisors divSafe admits
    ends = np.concatenate([_neighbours(lo, 3), _neighbours(hi, 3), _neighbours(1e-100, 0), _neighbours(1e100, 0)])
    ends = np.concatenate([ends, -ends])
    fam["ends"] = (np.tile(sgn(2000)*_doubles(rng, 2000, -300, 300), len(ends)), np.repeat(ends, 2000))
    ones = np.ldexp(2-2.0**-52, np.arange(-332, 332))
    fam["ones"] = (sgn(len(ones))*_doubles(rng, len(ones), -10, 10), ones*sgn(len(ones)))
    # small dividends: |a| from the subnormals up past the domain's edge, divisors over divSafe's whole range
    m = 1_000_000
    fam["small"] = (sgn(m)*np.abs(_bits_uniform(rng, m, 0., 2.0**-940)), sgn(m)*_doubles(rng, m, -331, 331))
    fam["edge"] = (sgn(m)*_doubles(rng, m, -969, -960), sgn(m)*_doubles(rng, m, -331, 52))     # at the edge, normal quotients: |a/b| >= 2^-969-53
    big = _doubles(rng, n, 600, 1022)
    fam["large"] = (sgn(n)*big, sgn(n)*_doubles(rng, n, -331, 331))                            # quotients up to overflow and beyond
    zb = np.concatenate([[3., -3., 1e-99, -1e-99, 1e99, -1e99], sgn(2000)*_doubles(rng, 2000, -331, 331)])
    fam["zero"] = (np.concatenate([np.zeros(len(zb)), -np.zeros(len(zb))]), np.concatenate([zb, zb]))
    return fam


def _bits_uniform(rng, n, lo, hi):
    """Uniform over the BIT PATTERNS of [lo, hi): every binade (and the subnormals) equally likely per value."""
    l, h = np.float64(lo).view(np.uint64), np.float64(hi).view(np.uint64)
    return rng.integers(int(l), int(h), n, dtype=np.uint64).view(np.float64)


def div_in_domain(a, b):
    """divExact's documented domain given divSafe(b): a zero dividend, or 2^-969 <= |a| < inf with 2^-1021 <= |a/b| <= 2^1023."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        q = np.abs(a.astype(np.longdouble)/b.astype(np.longdouble))     # 15-bit exponent: no over/underflow here
    return (a == 0) | ((np.abs(a) >= DIV_MIN_DIVIDEND) & np.isfinite(a) & (q >= DIV_MIN_QUOTIENT) & (q <= DIV_MAX_QUOTIENT))


def div_expected(a, b):
    """IEEE a/b, except the one documented departure: a -0 dividend over a positive divisor gives +0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        q = a/b
    q[(a == 0) & np.signbit(a) & (b > 0)] = 0.
    return q


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def differs(a, b):
    """Bitwise different fp64 values; two NaNs count as equal."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (u64(a) != u64(b)) & ~(np.isnan(a) & np.isnan(b))


def assert_same(got, want, what, inputs=None):
    bad = differs(got, want)
    if bad.any():
        i = np.nonzero(bad.reshape(-1))[0][:5]
        where = "" if inputs is None else " inputs %s" % [np.asarray(inputs).reshape(len(bad.reshape(-1)), -1)[k].tolist() for k in i]
        raise AssertionError("%s: %d of %d values differ, first at %s: got %s want %s%s" % (what, int(bad.sum()), bad.size, i.tolist(),
                             [float.hex(float(v)) for v in np.asarray(got).reshape(-1)[i]], [float.hex(float(v)) for v in np.asarray(want).reshape(-1)[i]], where))


def expected_div_safe(b):
    m = np.abs(np.asarray(b, np.float64))
    return (m > 1e-100) & (m < 1e100) & (np.frexp(m)[0] != 1-2.0**-53)


def check_division(name, a, b, safe, q, report):
    """The statement of divExact's domain (msdf_device.hpp): for every divisor divSafe admits and every dividend inside the domain the result is IEEE a/b, bit
    for bit -- except a -0 dividend over a positive divisor, which gives +0. Outside the domain nothing is promised; what happens there is reported."""
    assert (safe == expected_div_safe(b)).all(), name
    with np.errstate(all="ignore"):
        ieee = a/b
    dom = safe & div_in_domain(a, b)
    out = safe & ~dom
    bad_out = differs(q, ieee) & out
    report("divExact %-10s %8d pairs, %8d safe, %8d in the domain; outside it %d of %d differ from IEEE%s" % (
        name, len(a), safe.sum(), dom.sum(), bad_out.sum(), out.sum(),
        ", the largest such |a| = %s" % float.hex(float(np.abs(a[bad_out]).max())) if bad_out.any() else ""))
    assert_same(q[dom], div_expected(a, b)[dom], "divExact inside its domain, family "+name, np.stack([a, b], 1)[dom])
    return dom, bad_out


def check_zero_dividends(q_of):
    """q_of(a, b) -> divExact. +0/3 = +0, +0/-3 = -0, -0/-3 = +0 as IEEE; -0/3 = +0 where IEEE gives -0 (documented)."""
    q = q_of(np.array([0., 0., -0., -0.]), np.array([3., -3., -3., 3.]))
    assert (q == 0).all() and np.signbit(q).tolist() == [False, True, False, False], q


# -------------------------------------------------------------------------------------------------------------------- solvers

def quadratic_inputs():
    """The branch edges of solveQuadratic (equation-solver.cpp:9-32), then a random draw. Rows (a, b, c)."""
    rng = np.random.default_rng(41)
    rows = []
    z = np.zeros(200)
    u = lambda: rng.uniform(-2, 2, 200)
    rows += [np.stack([z, u(), u()], 1), np.stack([z, z, u()], 1), np.stack([z, z, z], 1), np.stack([z, u(), z], 1), np.stack([-z, u(), u()], 1)]      # a == 0
    a = u()*np.exp(rng.uniform(-20, 5, 200))
    lim = 1e12*np.abs(a)                                                                                                   # |b| against 1e12*|a|
    for bb in (lim, np.nextafter(lim, np.inf), np.nextafter(lim, 0), -lim, -np.nextafter(lim, np.inf), -np.nextafter(lim, 0)):
        rows.append(np.stack([a, bb, u()], 1))
    m, k = rng.integers(1, 1 << 12, 200).astype(np.float64), rng.integers(1, 1 << 12, 200).astype(np.float64)
    rows += [np.stack([m*m, 2*m*k, k*k], 1), np.stack([-m*m, 2*m*k, -k*k], 1), np.stack([m*m, -2*m*k, k*k], 1)]            # dscr == 0 exactly
    rows += [np.stack([u(), z, z], 1), np.stack([u(), -z, z], 1)]                                                           # b == c == 0
    rows += [np.stack([u(), u(), z], 1), np.stack([u(), z, u()], 1)]
    rows.append(rng.uniform(-2, 2, (4000, 3))*np.exp(rng.uniform(-8, 8, (4000, 3))))
    return np.concatenate(rows)


def cubic_inputs():
    """Rows (a, b, c) of solveCubicNormed: x^3+a x^2+b x+c. The edges of its branches, then a random draw."""
    rng = np.random.default_rng(42)
    rows = [np.zeros((1, 3)), np.array([[3., 3., 1.], [-3., 3., -1.], [6., 12., 8.]])]        # u == 0: a triple root
    s = np.concatenate([np.ldexp(1., np.arange(-8, 9)), rng.uniform(.1, 10, 100), -rng.uniform(.1, 10, 100)])
    rows.append(np.stack([0*s, -3*s*s, 2*s*s*s], 1))                                           # (x-s)^2 (x+2s): r2 == q3 when nothing rounds; u == v
    sh = rng.uniform(-2, 2, len(s))
    rows.append(np.stack([3*sh-0*s, 3*sh*sh-3*s*s, sh*sh*sh-3*s*s*sh+2*s*s*s], 1))             # the same double root, shifted (rounds: either side of r2 == q3)
    # around r2 == q3 with a = 0: q = 1/9.*(0-3b), r = 1/54.*(0*(..)+27c); c = +-2*sqrt(q^3) nudged by a few ulp lands on r2 < q3 with |r/sqrt(q3)| rounding
    # to 1 or beyond (the clamp of t), on r2 == q3, and just past it (the cube-root branch with a tiny sqrt(r2-q3)).
    b = -rng.uniform(.01, 30, 3000)
    q = 1/9.*(0-3*b)
    c0 = 2*np.sqrt(q*q*q)
    for k in range(-4, 5):
        ck = c0.copy()
        for _ in range(abs(k)):
            ck = np.nextafter(ck, np.inf if k > 0 else 0)
        rows += [np.stack([0*b, b, ck], 1), np.stack([0*b, b, -ck], 1)]
    rows.append(np.stack([rng.uniform(-3, 3, 2000), rng.uniform(-3, 3, 2000), np.zeros(2000)], 1))     # a root at 0
    rows.append(rng.uniform(-2, 2, (12000, 3)))
    rows.append(rng.uniform(-2, 2, (6000, 3))*np.exp(rng.uniform(-6, 6, (6000, 3))))
    return np.concatenate(rows)


def cubic_terms(a, b, c):
    """q, r, r2, q3 of solveCubicNormedPre, by its own fp64 expressions (numpy: IEEE operations, no contraction)."""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    a2 = a*a
    q = 1/9.*(a2-3*b)
    r = 1/54.*(a*(2*a2-9*b)+27*c)
    return q, r, r*r, q*q*q


# --------------------------------------------------------------------------------------------------------------- wave helpers

def wave_min_inputs():
    """Wavefronts of 64 non-negative floats."""
    rng = np.random.default_rng(51)
    w = []
    base = rng.uniform(1, 100, (64, 64)).astype(np.float32)
    base[np.arange(64), np.arange(64)] = .5                                  # the unique minimum in each lane position in turn
    w.append(base)
    ties = rng.uniform(1, 100, (64, 64)).astype(np.float32)
    ties[np.arange(64), np.arange(64)] = .25
    ties[np.arange(64), (np.arange(64)*7+5) % 64] = .25                       # the minimum twice
    w.append(ties)
    w.append(np.full((1, 64), np.inf, np.float32))
    inf1 = np.full((64, 64), np.inf, np.float32)
    inf1[np.arange(64), np.arange(64)] = 3e38                                 # one finite value among +inf
    w.append(inf1)
    tiny = rng.uniform(1e-44, 1e-38, (64, 64)).astype(np.float32)             # subnormals, +0 the minimum in one lane
    tiny[np.arange(64), np.arange(64)] = 0
    w.append(tiny)
    sub = rng.uniform(1e-30, 1, (64, 64)).astype(np.float32)
    sub[np.arange(64), np.arange(64)] = np.float32(1e-45)                     # the smallest subnormal the minimum
    w.append(sub)
    w.append(np.exp(rng.uniform(-80, 80, (256, 64))).astype(np.float32))
    w.append(np.zeros((1, 64), np.float32))
    return np.concatenate(w)


def row_min_inputs():
    """Wavefronts for rowMinNonNegative: row r (lanes 16r..16r+15) holds values in [10r', ...) with ITS minimum at position p; the other rows hold SMALLER
    values, so a leak across rows shows."""
    rng = np.random.default_rng(52)
    w = []
    for r in range(4):
        for p in range(16):
            v = np.empty((4, 16), np.float32)
            for o in range(4):
                v[o] = rng.uniform(1, 2, 16)*(100 if o == r else 1)          # the other rows: a hundred times smaller
            v[r, p] = 50
            w.append(v.reshape(64))
    w += [np.exp(rng.uniform(-80, 80, 64)).astype(np.float32) for _ in range(128)]
    w.append(np.full(64, np.inf, np.float32))
    x = np.full(64, np.inf, np.float32)
    x[16:32] = 0
    w.append(x)
    return np.stack(w)


def row_rank_inputs():
    rng = np.random.default_rng(53)
    w = []
    for _ in range(256):
        keys = rng.choice(1 << 32, 64, replace=False).astype(np.uint32)       # unique within the wavefront, hence within every row
        w.append(keys)
    small = np.concatenate([rng.permutation(16) for _ in range(4)]).astype(np.uint32)
    w.append(small)
    w.append(np.tile(np.arange(16, dtype=np.uint32), 4))                      # sorted rows
    w.append(np.tile(np.arange(16, dtype=np.uint32)[::-1], 4))                # reversed rows
    hi = np.tile(np.arange(16, dtype=np.uint32)[::-1]*np.uint32(0x10000000)+np.uint32(0xf), 4)    # keys that differ in the top bits (unsigned compare)
    w.append(hi)
    return np.stack(w)


def float_above_inputs():
    rng = np.random.default_rng(54)
    f = np.concatenate([np.exp(rng.uniform(-100, 88, 20000)).astype(np.float32), np.array([1e-45, 1e-40, 1.1754944e-38, 1, 3.4028235e38], np.float32)])
    f64 = f.astype(np.float64)
    big = np.array([3.5e38, 1e39, 1e300, np.inf, 3.4028235e38*(1+1e-9), 0., 1e-46, 1e-60, 5e-324, 7e-46, 2.1e-45])
    return np.concatenate([f64, np.nextafter(f64, np.inf), np.nextafter(f64, 0), np.exp(rng.uniform(-100, 88, 20000)), big])


# ---------------------------------------------------------------------------------------------------- a texel on an edge's start point

GLYPH_SIZE = (8, 8)
GLYPH_XF = np.array([1., 1., 0., 0., -2., 2.])             # identity projection: the texel centre (x+.5, y+.5) is a shape coordinate, exactly


def start_point_glyphs():
    """Closed contours whose first edge is a linear / quadratic / cubic segment STARTING exactly on a texel centre and running down-left, and the same running
    up-right: o-p0 is (+0, +0), so dot(o-p0, ab) is -0 (down-left) and -dot(p0-o, direction(0)) is -0 (up-right) -- the -0 dividends of divExact."""
    def contour(first, t):
        p = np.zeros((3, 8))
        p[0, :2*(t+1)] = np.asarray(first, np.float64).reshape(-1)
        end = p[0, 2*t:2*t+2]
        corner = np.array([end[0]+2.25, end[1]-1.75]) if first[-1][0] < first[0][0] else np.array([end[0]-2.25, end[1]+1.75])
        p[1, :4] = [end[0], end[1], corner[0], corner[1]]
        p[2, :4] = [corner[0], corner[1], p[0, 0], p[0, 1]]
        return p, [t, 1, 1]

    shapes = []
    for flip in (1, -1):
        s = np.array([5.5, 5.5]) if flip == 1 else np.array([2.5, 2.5])
        firsts = {1: [s, s-flip*np.array([3., 2.])],
                  2: [s, s-flip*np.array([1., 2.]), s-flip*np.array([3., 2.5])],
                  3: [s, s-flip*np.array([.5, 1.5]), s-flip*np.array([2., 1.]), s-flip*np.array([3., 3.])]}
        for t in (1, 2, 3):
            pts, types = contour(firsts[t], t)
            shapes.append(FlatShape([0, 3], pts, types, [6, 5, 3]))          # CYAN, MAGENTA, YELLOW: every corner changes colour
    return shapes
