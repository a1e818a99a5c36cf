// msdf_ec_fast.hpp -- the lean, single-sweep form of the error-correction classifier used for ALL texels; the handful of texels whose
// verdict depends on an exact shape-distance query (ShapeDistanceChecker, MSDFErrorCorrection.cpp:58-82; ~0.1 % of texels) are
// deferred to the full per-texel pipeline of msdf_ec.hpp (k_ec_slow).
//
// What is restructured relative to the reference, and why each step is exact:
//  * findErrors(sdf) (:383-410) and findErrors(sdf, shape) (:412-457) enumerate the SAME interpolation candidates (t, xm) -- they
//    differ only in the classifier (protectedFlag, distance check).  One sweep computes each candidate once and derives both
//    verdicts.  The sweep runs in shape orientation: a row flip maps every neighbour test of the native-order sweep onto a test
//    with identical operands (hasDiagonalArtifact always receives (texel, horizontal, vertical, diagonal neighbour)), and the
//    per-texel result is an OR over the tests, so the order does not matter.
//  * The texel's ERROR flag is an OR of side-effect-free predicates, so all cheap predicates are evaluated first; only if none
//    fires and some candidate needs the distance check is the texel deferred (result: identical flag).
//  * Linear pairs: t = dA/(dA-dB) lies in (0,1) only if dA and dB have strictly opposite signs (float subtraction and division are
//    monotone), so the fp64 division is skipped otherwise.
//  * Diagonal pairs: solveQuadratic (sqrt + 2 divisions) is skipped when the quadratic provably has no real root in
//    [0.005, 0.995] (the reference keeps only roots in (0.01, 0.99); the computed roots are within ~1e-4 of the real ones because
//    |b| <= 1e12*|a| in that branch).  The extremum parameters tEx (3 divisions) are computed only when a root survives.
//    A lane visits its in-range roots in the reference's order, but as "first in-range root, second in-range root" rather than by
//    the solver's index (and the in-range extrema likewise: their flags are OR-ed, any order): same tests per lane, and a wavefront
//    runs one copy of the body where its lanes' roots sit at different indices (DiagonalRoots).
//  * Lazy protection (EDGE_PRIORITY with CHECK_DISTANCE_AT_EDGE, the library default): protectAll() precedes the shape pass, so the
//    stencil byte carries PROTECTED whatever protectCorners / protectEdges found, and the shape classifier never reads their bit.
//    The base classifier reads it only for a candidate that is no inversion, lies outside the range of its end points and fails the
//    span test: a CONDITIONAL artifact, an ERROR iff the texel is unprotected.  The sweep therefore runs as if every texel were
//    protected, reports such candidates in a third verdict bit, and only a texel that has one and no unconditional ERROR takes the
//    corner test and the protectEdges pairs afterwards.  Where a diagonal pair would hand a distance-check candidate to the sink at or
//    after a conditional artifact of the same pair (unprotected, the eager order has left the pair by then), the candidate is held
//    back (fourth bit) and handed over in a second visit of that pair once the texel is known to be protected: same candidate set.
//  * Stage 1 (the sign / radius tests that settle nearly all of a texel's 24 + 8 tests) only SAYS which tests survive: one word per texel, a bit per
//    test (texelCandidateMask, texelProtectMask), built from the very predicates with selects and ORs. k_ec_fast hands the survivors of a tile's 64
//    texels to stage 2 in one step (ecAppendItems: popcount, exclusive prefix sum over the wavefront, a walk over the set bits) where every one of the
//    32 emit sites had been a push of its own, an LDS atomic and a wait each. The items are the same set; their order in the queue changes, and with it
//    the order in which a glyph's distance-check candidates reach its segment -- nothing reads either order: verdicts are OR-ed into the texel's word,
//    k_ec_query stores the same median for every candidate that decides a texel, the overflow rule looks at the count. The host walk and every other
//    caller take the tests from texelCandidatePairs / texelProtectPairs, which walk the bits in the order of the emission they replace.
//  * Three template switches that only k_ec_fast turns on (everything else, the host walk included, runs the defaults = the reference's spelling):
//    HWMED, the hardware's median where a wavefront's vote has shown that no operand can be a NaN (msdf_device.hpp: med3f; the consumers of a median
//    and why none sees a zero's sign: at evaluatePair); INDEXED, a test's channels read at computed addresses instead of selected; CORDER, the order
//    and with it the lazy orders' configuration known at compile time. Same floats, same predicates: tests/test_ec_hw_median_host.py.
#pragma once

#include "msdf_ec.hpp"

namespace msdfhip {

enum { EC_DEFER = 0x80 };   // internal: texel must be re-evaluated by the full pipeline (needs a shape-distance query)

// Verdict bits of judge() / evaluatePair() / texelFindFast(). The last two only arise in the lazy order.
enum { EC_V_ERROR = 1,      // ERROR decided
       EC_V_CHECK = 2,      // some candidate needs the distance check
       EC_V_COND = 4,       // conditional artifact: ERROR iff the texel turns out unprotected
       EC_V_HELD = 8 };     // a distance-check candidate was held back behind a conditional artifact of its pair
// Order of a sweep: eager (protection known, `p1`), the lazy first visit (protection assumed), the lazy second visit of a pair of a
// texel now known to be protected (hands over the held-back candidates, nothing else).
enum { EC_ORDER_EAGER = 0, EC_ORDER_LAZY = 1, EC_ORDER_LAZY_HELD = 2 };

// Which of the reference's two findErrors passes apply (core/msdf-error-correction.cpp:36-46).
MSDF_HD bool ecHasBasePass(const EcParams &p) { return p.distanceCheck == EC_DO_NOT_CHECK || (p.distanceCheck == EC_CHECK_AT_EDGE && p.mode != EC_MODE_EDGE_ONLY); }
MSDF_HD bool ecHasShapePass(const EcParams &p) { return p.distanceCheck == EC_ALWAYS_CHECK || p.distanceCheck == EC_CHECK_AT_EDGE; }
// The one configuration in which a texel's protection can be resolved after the sweep (header comment): elsewhere the shape pass
// reads the bit (ALWAYS_CHECK), the stencil shows it (DO_NOT_CHECK) or there is nothing to resolve (EDGE_ONLY, INDISCRIMINATE).
MSDF_HD bool ecLazyProtect(const EcParams &p) { return p.mode == EC_MODE_EDGE_PRIORITY && p.distanceCheck == EC_CHECK_AT_EDGE; }

struct FastCtx {
    double span;
    bool p1;          // protectedFlag of the base pass (and of the shape pass under ALWAYS_CHECK)
    bool pShape;      // protectedFlag of the shape pass
    bool basePass, shapePass;
    int order;        // EC_ORDER_*; the lazy orders run with p1 = pShape = true
};

// rangeTest (:30-40) for both classifiers at once. Returns flags of the base pass in bits 0-1 and of the shape pass in bits 2-3; in the
// lazy order bit 4: the base pass has an artifact here iff its protectedFlag is false (it exists only through `!p1 && outside`).
// HWMED (no operand is a NaN): "both end points above .5" is "the smaller one is" -- one v_min_f32 and a compare for two compares and a mask operation.
template <bool HWMED = false>
MSDF_HD int rangeTest2(const FastCtx &c, double at, double bt, double xt, float am, float bm, float xm) {
    const bool inversion = HWMED ? (med3Lo(am, bm) > .5f && xm <= .5f) || (med3Hi(am, bm) < .5f && xm >= .5f)
                                 : (am > .5f && bm > .5f && xm <= .5f) || (am < .5f && bm < .5f && xm >= .5f);
    const bool outside = medianOf<HWMED>(am, bm, xm) != xm;
    const bool candBase = c.basePass && (inversion || (!c.p1 && outside));
    const bool candShape = c.shapePass && (inversion || (!c.pShape && outside));
    const bool candCond = c.order != EC_ORDER_EAGER && !inversion && outside;
    if (!(candBase || candShape || candCond))
        return 0;
    const double axSpan = (xt-at)*c.span, bxSpan = (bt-xt)*c.span;
    const int f = (xm >= am-axSpan && xm <= am+axSpan && xm >= bm-bxSpan && xm <= bm+bxSpan) ? 1 : 3;
    return (candBase ? f : 0)|(candShape ? f<<2 : 0)|(candCond && f == 3 ? 16 : 0);
}

// EC_V_ERROR: ERROR decided; EC_V_CHECK: needs the distance check; 0: nothing. EC_V_COND rides along from bit 4 of rangeTest2.
MSDF_HD int judge(int flags) {
    const int cond = (flags&16) ? EC_V_COND : 0;
    if (flags&2)
        return EC_V_ERROR|cond;       // base classifier: evaluate() == (flags&ARTIFACT) (:42-44)
    const int fs = (flags>>2)&3;
    if (fs&1)
        return ((fs&2) ? EC_V_ERROR : EC_V_CHECK)|cond;   // shape classifier: artifact already, or candidate -> distance check (:60-64)
    return cond;
}

// Conservative: false only if a*t^2+b*t+c has no real root in [0.005, 0.995] (see header comment). a, b, c as passed to solveQuadratic.
MSDF_HD bool quadraticMayHaveRootInRange(double a, double b, double c) {
    if (a == 0 || fabs(b) > 1e12*fabs(a))
        return true;                                    // linear / degenerate branch of solveQuadratic: let it decide
    const double lo = .005, hi = .995;
    const double mag = fabs(a)+fabs(b)+fabs(c);
    const double eps = 1e-9*mag;
    const double flo = (a*lo+b)*lo+c, fhi = (a*hi+b)*hi+c;
    if (!(flo > eps && fhi > eps) && !(flo < -eps && fhi < -eps))
        return true;                                    // sign change (or too close to call) between the interval ends
    const double s = flo > 0 ? 1. : -1.;                // sign of f at both ends; a root needs an interior extremum of the opposite sign
    const double as = a*s, bs = b*s, cs = c*s;          // as*t^2+bs*t+cs is positive at both ends
    if (as <= 0)
        return false;                                   // concave: minimum over the interval is at an end
    // convex: vertex at -bs/(2*as); inside (lo, hi) iff 2*as*lo < -bs < 2*as*hi
    if (!(-bs > 2*as*lo*(1-1e-9) && -bs < 2*as*hi*(1+1e-9)))
        return false;                                   // monotone on the interval
    return !(4*as*cs-bs*bs > 1e-9*mag*mag);             // minimum value cs-bs^2/(4as) not clearly positive -> may have roots
}

// Cheapest necessary condition for a diagonal candidate, in fp32: along the diagonal the channel difference is the quadratic with
// Bernstein coefficients (dA, dBC/2, dD) on [0, 1] (f(0) = dA, f(1) = dD). If all three have the same sign with a margin that
// dwarfs the rounding of the reference's float coefficients (dD-dBC+dA, dBC-dA-dA: <= 5e-7*M), the quadratic has no real root in
// [0, 1], so solveQuadratic cannot return one in (0.01, 0.99). False = "cannot have a root".
// HWMED (no operand is a NaN -- k_ec_fast behind its vote: differences of finite channels below 2^100): "all three above eps" is "the smallest is", "all
// three below -eps" is "the largest is": v_min3_f32, v_max3_f32 and two compares for six compares and five mask operations. Zeros of either sign compare alike.
template <bool HWMED = false>
MSDF_HD bool bernsteinMayHaveRoot(float dA, float dBC, float dD) {
    const float m = fmaxf(fmaxf(fabsf(dA), fabsf(dBC)), fabsf(dD));
    const float eps = 1e-5f*m;
    const float h = .5f*dBC;
    if (HWMED)
        return !(med3Lo(med3Lo(dA, h), dD) > eps || med3Hi(med3Hi(dA, h), dD) < -eps);
    return !((dA > eps && h > eps && dD > eps) || (dA < -eps && h < -eps && dD < -eps));
}

// edgeBetweenTexelsChannel (MSDFErrorCorrection.cpp:154-168) with the fp64 division skipped when t = (a-.5)/(a-b) cannot lie in
// (0, 1): numerator n = a-.5 (exact in fp64) and denominator d = fl32(a-b) must have the same sign and |n| < |d|; both are
// fp32-derived, so n/d < 1 implies n/d <= 1-2^-26 and the rounded quotient is < 1 as well -- the predicate is exact.
template <bool HWMED = false>
MSDF_HD bool edgeBetweenTexelsChannelFast(const float *a, const float *b, int channel) {
    const double n = a[channel]-.5;
    const double d = a[channel]-b[channel];
    if (!((n > 0 && d > 0 && n < d) || (n < 0 && d < 0 && n > d)))
        return false;
    const double t = n/d;
    if (t > 0 && t < 1) {
        float c[3] = { mixf(a[0], b[0], t), mixf(a[1], b[1], t), mixf(a[2], b[2], t) };
        return medianOf<HWMED>(c[0], c[1], c[2]) == c[channel];
    }
    return false;
}

template <bool HWMED = false>
MSDF_HD int edgeBetweenTexelsFast(const float *a, const float *b) {
    return 1*(int) edgeBetweenTexelsChannelFast<HWMED>(a, b, 0)+2*(int) edgeBetweenTexelsChannelFast<HWMED>(a, b, 1)+4*(int) edgeBetweenTexelsChannelFast<HWMED>(a, b, 2);
}

// The roots of a diagonal pair's quadratic that the reference keeps (those in (0.01, 0.99), :296-298), in the order of solveQuadratic's indices, and the
// extremum parameters of the pair's two channels (:361-365) that lie in (0, 1), likewise in order. Which of x[0] = (-b+sqrt)/(2a) and x[1] = (-b-sqrt)/(2a)
// is the one in range follows the sign of a: written per index, a wavefront runs both copies of everything behind the test although nearly every lane
// has one root in range (4.8 % have two) -- hence this compaction: r0 is a lane's first in-range root whatever its index. The same for the extrema.
struct DiagonalRoots {
    double r0, r1;      // the m in-range roots
    double ex0, ex1;    // the ne in-range extremum parameters
    int m, ne;
};

// qa, qb, qc: as passed to solveQuadratic. False: no root in range (d.m == 0; the extrema, three divisions, are not computed).
MSDF_HD bool diagonalRootsInRange(DiagonalRoots &d, double qa, double qb, double qc, float l0, float q0, float l1, float q1) {
    d.m = 0, d.ne = 0;
    d.r0 = d.r1 = d.ex0 = d.ex1 = 0;
    if (!quadraticMayHaveRootInRange(qa, qb, qc))
        return false;
    double t[2] = { 0, 0 };
    const int solutions = solveQuadratic(t, qa, qb, qc);
    // (no short circuit: all are register values, one branch)
    const bool in0 = (solutions > 0)&(t[0] > MSDF_ARTIFACT_T_EPSILON)&(t[0] < 1-MSDF_ARTIFACT_T_EPSILON);
    const bool in1 = (solutions > 1)&(t[1] > MSDF_ARTIFACT_T_EPSILON)&(t[1] < 1-MSDF_ARTIFACT_T_EPSILON);
    d.m = (int) in0+(int) in1;
    if (!d.m)
        return false;
    d.r0 = in0 ? t[0] : t[1], d.r1 = t[1];
    const double tEx0 = -.5*l0/q0, tEx1 = -.5*l1/q1;               // :361-365 (l, q of the two channels of the pair)
    const bool e0 = (tEx0 > 0)&(tEx0 < 1), e1 = (tEx1 > 0)&(tEx1 < 1);
    d.ne = (int) e0+(int) e1;
    d.ex0 = e0 ? tEx0 : tEx1, d.ex1 = tEx1;
    return true;
}

// One range test of root t (xm: the interpolated median there): over the whole segment, or, for an extremum at tEx, over the part between the
// extremum and the end point on the root's side (:366-377). The results of a root's tests are OR-ed, so their order is free.
template <bool HWMED = false>
MSDF_HD int diagonalUnitFlags(const FastCtx &cx, float am, float dm, const float *a, const float *l, const float *q, double t, double tEx, bool extremum, float xm) {
    if (!extremum)
        return rangeTest2<HWMED>(cx, 0, 1, t, am, dm, xm);
    double tEnd0 = 0, tEnd1 = 1;
    float em0 = am, em1 = dm;
    const float ex = interpolatedMedianQuad<HWMED>(a, l, q, tEx);
    if (tEx > t)
        tEnd1 = tEx, em1 = ex;
    else
        tEnd0 = tEx, em0 = ex;
    return rangeTest2<HWMED>(cx, tEnd0, tEnd1, t, em0, em1, xm);
}

// What the accumulated flags of root t do to the pair's verdict; true: ERROR, the pair is decided (the reference returns there, :300-326).
template <class Sink>
MSDF_HD bool diagonalRootVerdict(const FastCtx &cx, int rangeFlags, double t, int &verdict, Sink &sink) {
    const int v = judge(rangeFlags);
    verdict |= v;
    if (v&EC_V_CHECK) {
        const bool held = (verdict&EC_V_COND) != 0;
        if (held)
            verdict |= EC_V_HELD;
        if (held == (cx.order == EC_ORDER_LAZY_HELD))
            sink(t);
    }
    return (verdict&EC_V_ERROR) != 0;
}

// One diagonal channel pair (:291-327) with lazy extremum parameters. Returns judge() of the accumulated flags, OR-ed over roots;
// candidates that need the distance check are handed to `sink(t)`. Lazy order: a candidate at or after a conditional artifact of this
// pair is held back (EC_V_HELD) -- were the texel unprotected, the eager order would have returned ERROR at that artifact -- and
// handed over by the EC_ORDER_LAZY_HELD visit, which hands over nothing else.
// One pass per in-range root, a lane's roots in index order as before; in a wavefront the first pass is dense and the second runs only if some lane
// has both roots in range. Inside a pass: the first in-range extremum, then the second if a lane has two.
template <bool HWMED = false, class Sink>
MSDF_HD int diagonalPairFast(const FastCtx &cx, float am, float dm, const float *a, const float *l, const float *q,
                             float dA, float dBC, float dD, float l0, float q0, float l1, float q1, Sink &sink) {
    const double qa = dD-dBC+dA, qb = dBC-dA-dA, qc = dA;   // float expressions promoted, exactly as passed at :295
    DiagonalRoots d;
    if (!diagonalRootsInRange(d, qa, qb, qc, l0, q0, l1, q1))
        return 0;
    int verdict = 0;
    MSDF_UNROLL
    for (int i = 0; i < 2; ++i) {
        if (i >= d.m)
            break;
        const double t = i ? d.r1 : d.r0;
        const float xm = interpolatedMedianQuad<HWMED>(a, l, q, t);
        int rangeFlags = diagonalUnitFlags<HWMED>(cx, am, dm, a, l, q, t, 0, false, xm);
        if (d.ne > 0)
            rangeFlags |= diagonalUnitFlags<HWMED>(cx, am, dm, a, l, q, t, d.ex0, true, xm);
        if (d.ne > 1)
            rangeFlags |= diagonalUnitFlags<HWMED>(cx, am, dm, a, l, q, t, d.ex1, true, xm);
        if (diagonalRootVerdict(cx, rangeFlags, t, verdict, sink))
            return verdict;
    }
    return verdict;
}

// 3x3 neighbourhood of a texel in NATIVE row order, loaded once into registers: v[dy+1][dx+1][channel]; valid bit (dy+1)*3+(dx+1).
// dev[dy+1][dx+1] = fabsf(median(v) - .5f) of that texel: both first-level tests (protectEdges' radius test :201, findErrors' "the texel farther from
// the edge reports" :335, :349) compare only these. A texel's value is computed ONCE -- k_ec_fast does it while it stages the halo in LDS (round 6:
// every lane used to recompute the medians of all eight neighbours, twice: 18 medians of 8 instructions per texel, 15 % of the kernel's VALU stream by
// tools/isa_bbcount.py) -- with the reference's own expression, so the comparisons see the same floats.
// cls[dy+1][dx+1] = the texel's class word (ecTexelClassWord; 0 outside the bitmap): everything else the first-level tests derive from ONE texel -- is it
// inside the bitmap, and the signs of its three channel differences -- is likewise computed once per texel (k_ec_fast: next to the deviation, while the halo
// is staged) instead of in each of the up to five lanes that look at it. v and dev of a texel outside the bitmap are unspecified: no test reads them.
struct Neighbourhood {
    float v[3][3][3];
    float dev[3][3];
    unsigned cls[3][3];
    unsigned valid;     // the nine inside bits (host walk; the kernel reads them in cls)
};

template <bool HWMED = false>
MSDF_HD float ecTexelDeviation(const float *t) { return fabsf(medianOf<HWMED>(t[0], t[1], t[2])-.5f); }

// Class word of a texel inside the bitmap. With D[j] = t[j+1 mod 3]-t[j] (channel pair j in the reference's minuend / subtrahend order, the float
// subtraction of hasLinearArtifact / hasDiagonalArtifact): bit j: D[j] > 0, bit 3+j: D[j] < 0, bit 6+j: D[j] == 0 (a NaN sets none of the three),
// bit 15: inside. The bits ARE the outcomes of the comparisons the first-level tests make on this texel's differences.
enum { EC_CLS_INSIDE = 0x8000 };
MSDF_HD unsigned ecTexelClassWord(const float *t) {
    unsigned w = EC_CLS_INSIDE;
    MSDF_UNROLL
    for (int j = 0; j < 3; ++j) {
        const float d = t[j == 2 ? 0 : j+1]-t[j];
        w |= (d > 0 ? 1u<<j : 0u)|(d < 0 ? 8u<<j : 0u)|(d == 0 ? 64u<<j : 0u);
    }
    return w;
}

MSDF_HD unsigned ecValidFromWords(const Neighbourhood &nb) {
    unsigned valid = 0;
    MSDF_UNROLL
    for (int m = 0; m < 9; ++m)
        valid |= (nb.cls[m/3][m%3]&EC_CLS_INSIDE) ? 1u<<m : 0u;
    return valid;
}

MSDF_HD void loadNeighbourhood(Neighbourhood &nb, const SdfView &sdf, int x, int yn) {
    MSDF_UNROLL
    for (int dy = -1; dy <= 1; ++dy) {
        MSDF_UNROLL
        for (int dx = -1; dx <= 1; ++dx) {
            const int nx = x+dx, ny = yn+dy;
            const bool in = nx >= 0 && ny >= 0 && nx < sdf.w && ny < sdf.h;
            const float *t = sdf.native(in ? nx : x, in ? ny : yn);
            nb.v[dy+1][dx+1][0] = t[0], nb.v[dy+1][dx+1][1] = t[1], nb.v[dy+1][dx+1][2] = t[2];
            nb.dev[dy+1][dx+1] = ecTexelDeviation(t);
            nb.cls[dy+1][dx+1] = in ? ecTexelClassWord(t) : 0u;
        }
    }
    nb.valid = ecValidFromWords(nb);
}

// protectEdges (MSDFErrorCorrection.cpp:189-250) as a gather, from the register neighbourhood; see protectedByEdges in msdf_ec.hpp. Two
// stages like findErrors below: stage 1 emits the neighbours m = (dy+1)*3+(dx+1) whose pair passes the radius test (:201, :217, :233),
// stage 2 (evaluateProtectPair) runs edgeBetweenTexels on such a pair -- up to three fp64 divisions -- and is queued by the kernel.
// Stage 1 says WHICH pairs pass, as bit m of one word (texelProtectMask: selects and ORs, no branch per pair); the kernel appends a tile's pairs to its
// queue in one step (ecAppendItems below), everything else walks the bits in ascending m -- the order of the reference's sweeps, as before.
enum { EC_PROTECT_TESTS = 8, EC_PROTECT_MASK = 0x1ef };    // bits 0-8 without the centre
MSDF_HD unsigned texelProtectMask(const Neighbourhood &nb, const EcParams &p) {
    const float sdev = nb.dev[1][1];
    unsigned mask = 0;
    MSDF_UNROLL
    for (int dy = -1; dy <= 1; ++dy) {
        MSDF_UNROLL
        for (int dx = -1; dx <= 1; ++dx) {
            if (!dx && !dy)
                continue;
            const float radius = dy == 0 ? p.radiusH : dx == 0 ? p.radiusV : p.radiusD;
            const float odev = nb.dev[dy+1][dx+1];
            const bool selfIsA = dy > 0 || (dy == 0 && dx > 0);
            const float sum = selfIsA ? sdev+odev : odev+sdev;                     // fabsf(am-.5f)+fabsf(bm-.5f)
            mask |= (((nb.cls[dy+1][dx+1]&EC_CLS_INSIDE) != 0)&(sum < radius)) ? 1u<<((dy+1)*3+(dx+1)) : 0u;
        }
    }
    return mask;
}

template <class Emit>
MSDF_HD void texelProtectPairs(const Neighbourhood &nb, const EcParams &p, Emit &emit) {
    const unsigned mask = texelProtectMask(nb, p);
    for (int m = 0; m < 9; ++m)
        if (mask&(1u<<m))
            emit(m);
}

// Is `self` protected through its pair with neighbour m (`other`)? Pair orientation as the reference's sweeps: `a` is the texel of the
// lower native row (same row: the left one); swapRows: of the higher native row, which is the lower row of a flipped glyph's shape
// (EcParams::shapeRows).
template <bool HWMED = false>
MSDF_HD bool evaluateProtectPair(const float *self, const float *other, int m, bool swapRows = false) {
    const int dy = m/3-1, dx = m%3-1;
    const bool selfIsA = (swapRows ? dy < 0 : dy > 0) || (dy == 0 && dx > 0);
    const int mask = selfIsA ? edgeBetweenTexelsFast<HWMED>(self, other) : edgeBetweenTexelsFast<HWMED>(other, self);
    return extremeChannelInMask(self, medianOf<HWMED>(self[0], self[1], self[2]), mask);
}

MSDF_HD bool protectedByEdgesNb(const Neighbourhood &nb, const EcParams &p, int flip = 0) {
    struct Items {
        unsigned char m[8];
        int n;
        MSDF_HD void operator()(int mm) { m[n++] = (unsigned char) mm; }
    } items;
    items.n = 0;
    texelProtectPairs(nb, p, items);
    for (int i = 0; i < items.n; ++i)
        if (evaluateProtectPair(nb.v[1][1], nb.v[items.m[i]/3][items.m[i]%3], items.m[i], p.shapeRows && flip))
            return true;
    return false;
}

// ---- fused findErrors, in two stages so that a wavefront can COMPACT the expensive part ----------------------------------------------
// A texel is tested against its 8 neighbours x 3 channel pairs. Nearly all of those 24 tests are settled by a sign comparison
// (stage 1); the few survivors need fp64 interpolation / a quadratic solve (stage 2). Run per texel in a wavefront, stage 2 executes
// for a test if ANY of the 64 texels needs it, with a handful of lanes active (measured: 7 of the 24 tests per tile, 37 surviving
// (texel, test) items per tile). The kernel therefore queues the items of all its texels and evaluates them densely, one item per lane.
//
// Neighbour k (native row order): 0..3 = (-1,0), (0,-1), (1,0), (0,1); 4..7 = diagonals (k&1 ? +1 : -1, k&2 ? +1 : -1).
// Channel pair j: (j, j+1 mod 3), i.e. (1,0), (2,1), (0,2) in the reference's (minuend, subtrahend) order.
MSDF_HD int ecNeighbourDx(int k) { return k < 4 ? (k == 0 ? -1 : k == 2 ? 1 : 0) : ((k&1) ? 1 : -1); }
MSDF_HD int ecNeighbourDy(int k) { return k < 4 ? (k == 1 ? -1 : k == 3 ? 1 : 0) : ((k&2) ? 1 : -1); }

// Stage 1: emit(k, j) for every test of the centre texel of `nb` (inside the bitmap) that the cheap conditions cannot settle. Exact skips only:
//  * the neighbour must exist and the centre must be the texel farther from the edge (:335, :349);
//  * linear: t = dA/(dA-dB) lies in (0, 1) only if dA and dB have strictly opposite signs;
//  * diagonal: 0 == 0 has no usable root (equation-solver.cpp:13-17); Bernstein sign test (bernsteinMayHaveRoot).
// What depends on one texel alone comes from the class words (Neighbourhood::cls): whether a neighbour exists, and the signs of dA and dB -- the three
// linear tests of a neighbour are one mask, "positive here and negative there, or the reverse", and one branch on it. The diagonal tests read the
// channels: dBC belongs to no single texel. They are spelled as the reference spells them (dBC left to right); the class words only tell where
// dA == 0 && dD == 0, the one case in which dBC == 0 leaves nothing to solve.
// The survivors are returned as ONE word, test (k, j) = bit 4*k+j (texelCandidateMask): the three linear tests of a neighbour are their mask shifted into
// place, a diagonal test is a select and an OR -- one branch per diagonal neighbour (it skips the channel reads), none per test. Handing a survivor over
// is not stage 1's business: k_ec_fast appends all items of a tile to its queue in one step (ecAppendItems), the host walk and every other caller take
// them from texelCandidatePairs, which walks the bits in ascending order -- k, then j: the order of the emission it replaces.
enum { EC_FIND_TESTS = 24, EC_FIND_MASK = 0x77777777, EC_FIND_LINEAR = 0x7777 };     // 8 neighbours x 3 channel pairs, bit 4*k+3 is no test; k < 4: the linear tests
template <bool HWMED = false>
MSDF_HD unsigned texelCandidateMask(const Neighbourhood &nb) {
    const float *c = nb.v[1][1];
    const float cdev = nb.dev[1][1];
    const unsigned cw = nb.cls[1][1];
    unsigned mask = 0;
    MSDF_UNROLL
    for (int k = 0; k < 4; ++k) {
        const int dx = k == 0 ? -1 : k == 2 ? 1 : 0, dy = k == 1 ? -1 : k == 3 ? 1 : 0;
        const unsigned nw = nb.cls[dy+1][dx+1];
        // bit j: D[j] > 0 here and < 0 there, or < 0 here and > 0 there; none for a neighbour outside the bitmap, whose word is 0
        const unsigned opposite = ((cw&(nw>>3))|((cw>>3)&nw))&7u;
        mask |= cdev >= nb.dev[dy+1][dx+1] ? opposite<<(4*k) : 0u;
    }
    MSDF_UNROLL
    for (int k = 4; k < 8; ++k) {
        const int dx = (k&1) ? 1 : -1, dy = (k&2) ? 1 : -1;
        const unsigned dw = nb.cls[dy+1][dx+1];
        if (!(((dw&EC_CLS_INSIDE) != 0)&(cdev >= nb.dev[dy+1][dx+1])))      // (no short circuit: both are register values, one branch)
            continue;
        const float *d = nb.v[dy+1][dx+1];
        const float *b = nb.v[1][dx+1], *cc = nb.v[dy+1][1];
        const unsigned zeroAD = cw&dw;                          // bit 6+j: dA == 0 and dD == 0
        MSDF_UNROLL
        for (int j = 0; j < 3; ++j) {
            const int i0 = j, i1 = j == 2 ? 0 : j+1;
            const float dA = c[i1]-c[i0], dBC = b[i1]-b[i0]+cc[i1]-cc[i0], dD = d[i1]-d[i0];
            const bool nothingToSolve = ((zeroAD&(64u<<j)) != 0)&(dBC == 0);
            mask |= ((!nothingToSolve)&bernsteinMayHaveRoot<HWMED>(dA, dBC, dD)) ? 1u<<(4*k+j) : 0u;
        }
    }
    return mask;
}

template <class Emit>
MSDF_HD void texelCandidatePairs(const Neighbourhood &nb, Emit &emit) {
    const unsigned mask = texelCandidateMask(nb);
    for (int bit = 0; bit < 32; ++bit)
        if (mask&(1u<<bit))
            emit(bit>>2, bit&3);
}

// ---- one append per tile ---------------------------------------------------------------------------------------------------------------
// A queued item is 16 bits: lane | bit<<6, `bit` the test's place in its mask (find: 4*k+j, so k and j are shifts; protect: m). A lane hands over all
// its survivors at once: it reserves popcount(mask) slots that are this lane's alone (reserve, below; k_ec_fast: an exclusive prefix sum over the
// wavefront; the host test: running counts, lanes in any order) and writes them in a walk over its set bits. Bits outside VALID
// are dropped BEFORE the count is taken, so whatever the mask, a lane takes n <= TESTS slots (64 lanes: the queue's capacity) and the walk makes exactly
// n trips, one per slot: the bound is the loop's own condition, a wrong mask can neither make it spin nor write past the lane's slots. Returns n.
// The order of the items in the queue is free: phase C ORs verdicts into the owning texel's word, and a texel's distance-check candidates reach the
// glyph's segment in any order (k_ec_query writes one value per texel whichever candidate decides it; the overflow rule looks at the count).
// What IS worth keeping of the old order (item by item, site after site: the queue sorted by test): linear items (k < 4) and diagonal ones take different
// paths through stage 2, and a round of 64 items that holds one kind runs one path. So the queue has two parts, the tests of FIRST ahead of the others:
// reserve(nFirst, nOthers, atFirst, atOthers) gives a lane its slots in each part (measured on the bench workload with the kinds mixed lane by lane:
// +36 of stage 2's 408 vector instructions per wavefront).
MSDF_HD int ecItemBit(unsigned item) { return (int) (item>>6); }
template <unsigned VALID, int TESTS, unsigned FIRST, class Reserve>
MSDF_HD int ecAppendItems(unsigned short *queue, unsigned mask, int lane, Reserve &reserve) {
    static_assert(__builtin_popcount(VALID) == TESTS && (FIRST&~VALID) == 0, "a lane's share of the queue is one slot per test");
    mask &= VALID;
    const int n = __builtin_popcount(mask);                 // <= TESTS
    const int nFirst = __builtin_popcount(mask&FIRST);
    int at = 0, atOthers = 0;
    reserve(nFirst, n-nFirst, at, atOthers);
    const int jump = atOthers-(at+nFirst);                  // from the lane's last slot of the first part to its first of the second
    // (rolled: a wavefront makes as many trips as its fullest lane has items, a handful; unrolled by eight the compiler packs the items into 128-bit
    // stores at 2-byte-aligned addresses and every tile with one full lane runs a forty-instruction trip)
    MSDF_NOUNROLL
    for (int i = 0; i < n; ++i) {                           // at most TESTS trips; the mask has exactly n bits, one goes per trip
        queue[at+i+(i >= nFirst ? jump : 0)] = (unsigned short) (lane|__builtin_ctz(mask)<<6);
        mask &= mask-1;
    }
    return n;
}

MSDF_HD float pick3(const float *v, int i) { return i == 0 ? v[0] : i == 1 ? v[1] : v[2]; }
// Channel i of a texel. INDEXED: the texel lies in addressable memory (k_ec_fast: the LDS halo; the host), so v[i] is a read at a computed address
// and costs no compare / select chain; a caller whose texels are register arrays (which an indexed read would send to scratch) keeps pick3. Same float.
template <bool INDEXED>
MSDF_HD float pickChannel(const float *v, int i) { return INDEXED ? v[i] : pick3(v, i); }

// Stage 2: one surviving test. c: centre texel, n: the neighbour k, hb / vc: the horizontal / vertical neighbours on the way to a
// diagonal one (unused for k < 4); any memory (registers, LDS; INDEXED: addressable, see pickChannel). Returns EC_V_* bits (a candidate that needs the
// distance check is also reported as sink(t, dx, dyShape)). Same operands and operations as hasLinearArtifact / hasDiagonalArtifact (:330-381).
// order: EC_ORDER_EAGER with the texel's protection in p1, or one of the lazy orders (only where ecLazyProtect(p); p1 is ignored).
// CORDER >= 0: the order is known where the call is compiled (k_ec_fast's instantiations: `order` must equal it). In a lazy order that settles the
// classifier's configuration as well -- ecLazyProtect(p) means EDGE_PRIORITY with CHECK_AT_EDGE, so both passes run and both see the texel protected --
// and rangeTest2 / judge fold: candBase == candShape == inversion, and nothing of the configuration is carried through the item loop as a scalar mask.
// HWMED: medianOf (msdf_device.hpp). What reads a median here, and why none of it can tell the sign of a zero (values equal the exact spelling's
// for non-NaN operands, which the caller guarantees): cm, nm, xm and the extremum medians go to rangeTest2, which compares them with .5f, with each
// other (`!= xm`: +0 == -0) and, promoted to double, with am +- axSpan (x-s and x+s round to the same double for x = +0 and -0 unless s == 0, and then
// the results are zeros, compared with >= / <=); as operands of the inner median a zero of either sign orders the same. edgeBetweenTexelsChannelFast
// and evaluateProtectPair compare their median with a channel (==, !=), ecTexelDeviation takes fabsf(m-.5f): -.5f for either zero. No median is stored
// -- the apply step of ecFastBody, which does store one, keeps medianf.
template <bool HWMED = false, bool INDEXED = false, int CORDER = -1, class Sink>
MSDF_HD int evaluatePair(const float *c, const float *n, const float *hb, const float *vc, const EcParams &p, bool p1, int flip, int k, int j, Sink &sink,
                         int orderArg = EC_ORDER_EAGER) {
    const int order = CORDER >= 0 ? CORDER : orderArg;
    constexpr bool LAZY_CT = CORDER == EC_ORDER_LAZY || CORDER == EC_ORDER_LAZY_HELD;
    FastCtx cx;
    cx.basePass = LAZY_CT || ecHasBasePass(p);
    cx.shapePass = LAZY_CT || ecHasShapePass(p);
    cx.order = order;
    cx.p1 = order != EC_ORDER_EAGER || p1;
    cx.pShape = (LAZY_CT || p.distanceCheck == EC_CHECK_AT_EDGE) ? true : cx.p1;   // protectAll() precedes the shape pass only in that mode (:38-39, :33)
    const int dx = ecNeighbourDx(k), dy = ecNeighbourDy(k);
    const int i0 = j, i1 = j == 2 ? 0 : j+1;
    const float cm = medianOf<HWMED>(c[0], c[1], c[2]), nm = medianOf<HWMED>(n[0], n[1], n[2]);
    if (k < 4) {
        if (order == EC_ORDER_LAZY_HELD)
            return 0;                                    // one range test per pair: a candidate (inversion) is never conditional as well
        cx.span = dy == 0 ? p.hSpan : p.vSpan;
        const float dA = pickChannel<INDEXED>(c, i1)-pickChannel<INDEXED>(c, i0), dB = pickChannel<INDEXED>(n, i1)-pickChannel<INDEXED>(n, i0);
        const double t = (double) dA/(dA-dB);            // :281
        if (t > MSDF_ARTIFACT_T_EPSILON && t < 1-MSDF_ARTIFACT_T_EPSILON) {
            const float xm = interpolatedMedianLin<HWMED>(c, n, t);
            const int v = judge(rangeTest2<HWMED>(cx, 0, 1, t, cm, nm, xm));
            if (v&EC_V_CHECK)
                sink(t, dx, flip ? -dy : dy);
            return v;
        }
        return 0;
    }
    cx.span = p.dSpan;
    const float *a = c, *b = hb, *cc = vc, *d = n;       // (texel, horizontal, vertical, diagonal neighbour), :404-407
    const float abc[3] = { a[0]-b[0]-cc[0], a[1]-b[1]-cc[1], a[2]-b[2]-cc[2] };
    const float l[3] = { -a[0]-abc[0], -a[1]-abc[1], -a[2]-abc[2] };
    const float q[3] = { d[0]+abc[0], d[1]+abc[1], d[2]+abc[2] };
    const float a3[3] = { a[0], a[1], a[2] };
    struct DirSink {
        Sink &sink;
        int dx, dy;
        MSDF_HD void operator()(double t) { sink(t, dx, dy); }
    } dirSink = { sink, dx, flip ? -dy : dy };
    const float dA = pickChannel<INDEXED>(a, i1)-pickChannel<INDEXED>(a, i0);
    const float dBC = pickChannel<INDEXED>(b, i1)-pickChannel<INDEXED>(b, i0)+pickChannel<INDEXED>(cc, i1)-pickChannel<INDEXED>(cc, i0);
    const float dD = pickChannel<INDEXED>(d, i1)-pickChannel<INDEXED>(d, i0);
    return diagonalPairFast<HWMED>(cx, cm, nm, a3, l, q, dA, dBC, dD, pick3(l, i0), pick3(q, i0), pick3(l, i1), pick3(q, i1), dirSink);   // (l, q: registers)
}

// Both stages for one texel, test after test (host walk; the kernel queues the items instead). Returns EC_V_* bits OR-ed over the tests;
// every candidate that needs the distance check is reported as sink(t, dx, dyShape) (MSDFErrorCorrection.cpp:446-453).
// HWMED: for tests/test_ec_hw_median_host.py, which runs k_ec_fast's second instantiation on the host; the host walk itself never asks for it.
template <bool HWMED = false, class Sink>
MSDF_HD int texelFindFast(const Neighbourhood &nb, const EcParams &p, bool p1, int flip, Sink &sink, int order = EC_ORDER_EAGER) {
    struct Items {
        unsigned char k[24], j[24];
        int n;
        MSDF_HD void operator()(int kk, int jj) { k[n] = (unsigned char) kk, j[n] = (unsigned char) jj; ++n; }
    } items;
    items.n = 0;
    texelCandidatePairs(nb, items);
    int verdict = 0;
    for (int i = 0; i < items.n; ++i) {
        const int k = items.k[i], dx = ecNeighbourDx(k), dy = ecNeighbourDy(k);
        verdict |= evaluatePair<HWMED>(nb.v[1][1], nb.v[dy+1][dx+1], nb.v[1][dx+1], nb.v[dy+1][1], p, p1, flip, k, items.j[i], sink, order);
    }
    return verdict;
}

// Does texel (x, ys) [shape orientation] belong to one of the corner pairs? corners: (l, b) of protectCorners (:131-134).
MSDF_HD bool protectedByCornerList(const int *corners, int nCorners, int x, int ys) {
    for (int i = 0; i < nCorners; ++i) {
        const int l = corners[2*i], b = corners[2*i+1];
        if ((x == l || x == l+1) && (ys == b || ys == b+1))
            return true;
    }
    return false;
}

// Does the lazy first visit leave the texel's protection to be resolved? A conditional artifact decides the texel unless an
// unconditional ERROR already has; a held-back candidate is handed over iff the texel is protected, whatever its verdict.
MSDF_HD bool ecNeedsProtection(int verdict) { return ((verdict&EC_V_COND) && !(verdict&EC_V_ERROR)) || (verdict&EC_V_HELD); }

// Stencil byte of texel (x, yn) [native order] by the fast path: PROTECTED/ERROR as in ecTexelStencil, plus EC_DEFER if the verdict
// hinges on shape-distance checks (each reported through `sink`). corners: (l, b) pairs of protectCorners (:131-134) in shape
// orientation, precomputed per tile. Takes the lazy order where the mode allows it, as the kernel does (allowLazy = false: the eager
// order everywhere; the two are compared by tests/test_ec_lazy_host.py).
template <class Sink>
MSDF_HD int ecTexelFast(const SdfView &sdf, const EcParams &p, const int *corners, int nCorners, int x, int yn, Sink &sink, bool allowLazy = true) {
    const int ys = sdf.flip ? sdf.h-1-yn : yn;
    Neighbourhood nb;
    loadNeighbourhood(nb, sdf, x, yn);
    int st = 0, verdict;
    if (allowLazy && ecLazyProtect(p)) {
        verdict = texelFindFast(nb, p, true, sdf.flip, sink, EC_ORDER_LAZY);
        if (ecNeedsProtection(verdict)) {
            if (!(protectedByCornerList(corners, nCorners, x, ys) || protectedByEdgesNb(nb, p, sdf.flip)))
                verdict |= EC_V_ERROR;                       // (a held-back candidate implies a conditional artifact)
            else if (verdict&EC_V_HELD)
                texelFindFast(nb, p, true, sdf.flip, sink, EC_ORDER_LAZY_HELD);
        }
    } else {
        if (p.mode == EC_MODE_EDGE_PRIORITY) {
            if (protectedByCornerList(corners, nCorners, x, ys) || protectedByEdgesNb(nb, p, sdf.flip))
                st |= EC_PROTECTED;
        } else if (p.mode == EC_MODE_EDGE_ONLY)
            st |= EC_PROTECTED;
        verdict = texelFindFast(nb, p, (st&EC_PROTECTED) != 0, sdf.flip, sink);
    }
    if (ecHasBasePass(p) && p.distanceCheck == EC_CHECK_AT_EDGE)
        st |= EC_PROTECTED;                              // protectAll (:38-39)
    if (verdict&EC_V_ERROR)
        st |= EC_ERROR;
    else if (verdict&EC_V_CHECK)
        st |= EC_DEFER;
    return st;
}

// The distance check of one deferred candidate: ShapeDistanceChecker::ArtifactClassifier::evaluate past its flag tests (:65-79).
// (x, ys): texel in shape orientation; t, (dx, dy): as reported by texelFindFast; query(V2) -> exact PSDF distance at a shape point.
template <class Query>
MSDF_HD bool ecEvaluateCandidate(const SdfView &sdf, const EcParams &p, int x, int ys, double t, int dx, int dy, const Query &query) {
    const float *msd = sdf.shape(x, ys);
    const V2 tVector = t*mk(dx, dy);
    float oldMSD[3], newMSD[3];
    interpolate3(oldMSD, sdf, mk(x+.5, ys+.5)+tVector);
    const double aWeight = (1-fabs(tVector.x))*(1-fabs(tVector.y));
    const float aPSD = medianf(msd[0], msd[1], msd[2]);
    newMSD[0] = (float) (oldMSD[0]+aWeight*(aPSD-msd[0]));
    newMSD[1] = (float) (oldMSD[1]+aWeight*(aPSD-msd[1]));
    newMSD[2] = (float) (oldMSD[2]+aWeight*(aPSD-msd[2]));
    const float oldPSD = medianf(oldMSD[0], oldMSD[1], oldMSD[2]);
    const float newPSD = medianf(newMSD[0], newMSD[1], newMSD[2]);
    const V2 q = unproject(p.t, mk(x+.5, ys+.5))+mk(tVector.x*p.texelX, tVector.y*p.texelY);
    const float refPSD = mapDistance(p.t, query(q));
    return p.minImproveRatio*fabsf(newPSD-refPSD) < (double) fabsf(oldPSD-refPSD);
}

} // namespace msdfhip
