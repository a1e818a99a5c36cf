// TEST TOOLING ONLY -- the diagonal artifact test of the error-correction sweep (msdf_ec_fast.hpp: diagonalPairFast, the stage 2 that k_ec_fast, k_single_call
// and the host walk ecTexelFast share, here compiled for the host with g++) against the form it replaced, and the counts of what a wavefront executes for
// it, for tests/test_ec_roots_host.py, tests/test_gpu_ec_roots.py and tools/ec_root_counts.py. A stand-alone program, so that it can also be built with
// -fsanitize=address,undefined and run as it is. Never loaded by the msdfgen_amd package.
//
//   ec_roots_host CASES        prints one JSON object, returns 1 on any difference
//   CASES: the format of tests/eclazycases.py (int32 n, then per case int32 w, h, flip, group, nC, nE | double xf[6] | int32 co[nC+1] | double points[nE][8]
//          | uint8 types[nE] | uint8 colors[nE] | float field[h][w][3]); the outlines are skipped, stage 2 never reads them.
//
// Compared, for every texel and each of its twelve diagonal (neighbour, channel pair) tests whose neighbour lies inside the bitmap -- a superset of the
// items stage 1 queues -- under EC_ORDER_EAGER with the texel unprotected and protected, EC_ORDER_LAZY and EC_ORDER_LAZY_HELD (EDGE_PRIORITY with
// CHECK_DISTANCE_AT_EDGE, the library default; the eager order also under DO_NOT_CHECK and ALWAYS_CHECK, where the shape pass reads the protection):
//   * evaluatePair, which runs today's diagonalPairFast, against `Before`: the diagonalPairFast of the commit before the in-range-first order, kept here
//     word for word -- the returned verdict bits and the ordered list of sink(t) values, bitwise;
//   * the same for an emulation of the dense form (one lane per (item, root, test) unit, 16-bit descriptors, per-(item, root) flag words, chunks of 64),
//     written with the helpers today's diagonalPairFast is made of (diagonalRootsInRange, diagonalUnitFlags, diagonalRootVerdict).
// Counted per group of cases, on the items stage 1 queues (`items`) and on everything compared (`pairs`), from the root and extremum predicates and the
// lazy order's verdicts; and per round of 64 queued items of an 8x8 tile, queue in push-site order (k outer, j inner), lanes in order: what a wavefront
// executes for the root loop before and after (the table of profiles/ec_root_passes.md).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <vector>

#include "../../msdfgen_amd/csrc/msdf_device.hpp"
#include "../../msdfgen_amd/csrc/msdf_prep.hpp"
#include "../../msdfgen_amd/csrc/msdf_ec.hpp"
#include "../../msdfgen_amd/csrc/msdf_ec_fast.hpp"

using namespace msdfhip;

namespace {

// ---- diagonalPairFast as it was before the in-range roots and extrema came first
namespace Before {

template <class Sink>
MSDF_HD int diagonalPairFast(const FastCtx &cx, float am, float dm, const float *a, const float *l, const float *q,
                             float dA, float dBC, float dD, float l0, float q0, float l1, float q1, Sink &sink) {
    const double qa = dD-dBC+dA, qb = dBC-dA-dA, qc = dA;   // float expressions promoted, exactly as passed at :295
    if (!quadraticMayHaveRootInRange(qa, qb, qc))
        return 0;
    double t[2];
    const int solutions = solveQuadratic(t, qa, qb, qc);
    int verdict = 0;
    for (int i = 0; i < solutions; ++i) {
        if (t[i] > MSDF_ARTIFACT_T_EPSILON && t[i] < 1-MSDF_ARTIFACT_T_EPSILON) {
            const float xm = interpolatedMedianQuad(a, l, q, t[i]);
            int rangeFlags = rangeTest2(cx, 0, 1, t[i], am, dm, xm);
            const double tEx0 = -.5*l0/q0, tEx1 = -.5*l1/q1;               // :361-365 (l, q of the two channels of the pair)
            if (tEx0 > 0 && tEx0 < 1) {
                double tEnd0 = 0, tEnd1 = 1;
                float em0 = am, em1 = dm;
                const float ex = interpolatedMedianQuad(a, l, q, tEx0);
                if (tEx0 > t[i])
                    tEnd1 = tEx0, em1 = ex;
                else
                    tEnd0 = tEx0, em0 = ex;
                rangeFlags |= rangeTest2(cx, tEnd0, tEnd1, t[i], em0, em1, xm);
            }
            if (tEx1 > 0 && tEx1 < 1) {
                double tEnd0 = 0, tEnd1 = 1;
                float em0 = am, em1 = dm;
                const float ex = interpolatedMedianQuad(a, l, q, tEx1);
                if (tEx1 > t[i])
                    tEnd1 = tEx1, em1 = ex;
                else
                    tEnd0 = tEx1, em0 = ex;
                rangeFlags |= rangeTest2(cx, tEnd0, tEnd1, t[i], em0, em1, xm);
            }
            const int v = judge(rangeFlags);
            verdict |= v;
            if (v&EC_V_CHECK) {
                const bool held = (verdict&EC_V_COND) != 0;
                if (held)
                    verdict |= EC_V_HELD;
                if (held == (cx.order == EC_ORDER_LAZY_HELD))
                    sink(t[i]);
            }
            if (verdict&EC_V_ERROR)
                return verdict;
        }
    }
    return verdict;
}

}

struct Case {
    int w, h, flip, group;
    double xf[6];
    std::vector<float> field;
};

template <class T>
bool readN(FILE *f, T *dst, size_t n) { return n == 0 || fread(dst, sizeof(T), n, f) == n; }

bool readCase(FILE *f, Case &c) {
    int32_t head[6];
    if (!readN(f, head, 6))
        return false;
    c.w = head[0], c.h = head[1], c.flip = head[2], c.group = head[3];
    const int nC = head[4], nE = head[5];
    if (c.w < 1 || c.h < 1 || c.w > 4096 || c.h > 4096 || nC < 0 || nE < 0 || nC > (1<<20) || nE > (1<<20) || c.group < 0 || c.group > 7 || (c.flip != 0 && c.flip != 1))
        return false;
    if (!readN(f, c.xf, 6))
        return false;
    std::vector<unsigned char> skipped((size_t) (nC+1)*4+(size_t) nE*(8*8+2));
    if (!readN(f, skipped.data(), skipped.size()))
        return false;
    c.field.assign((size_t) c.w*c.h*3, 0.f);
    return readN(f, c.field.data(), c.field.size());
}

// The operands evaluatePair hands to diagonalPairFast (msdf_ec_fast.hpp, its k >= 4 part), for `Before` and for the units of the dense form.
struct DiagArgs {
    FastCtx cx;
    float cm, nm, a3[3], l[3], q[3], dA, dBC, dD, l0, q0, l1, q1;
};

void diagArgs(DiagArgs &g, const float *c, const float *n, const float *hb, const float *vc, const EcParams &p, bool p1, int j, int order) {
    g.cx.basePass = ecHasBasePass(p);
    g.cx.shapePass = ecHasShapePass(p);
    g.cx.order = order;
    g.cx.p1 = order != EC_ORDER_EAGER || p1;
    g.cx.pShape = (p.distanceCheck == EC_CHECK_AT_EDGE) ? true : g.cx.p1;
    g.cx.span = p.dSpan;
    const int i0 = j, i1 = j == 2 ? 0 : j+1;
    g.cm = medianf(c[0], c[1], c[2]), g.nm = medianf(n[0], n[1], n[2]);
    const float *a = c, *b = hb, *cc = vc, *d = n;
    for (int i = 0; i < 3; ++i) {
        const float abc = a[i]-b[i]-cc[i];
        g.l[i] = -a[i]-abc, g.q[i] = d[i]+abc, g.a3[i] = a[i];
    }
    g.dA = pick3(a, i1)-pick3(a, i0), g.dBC = pick3(b, i1)-pick3(b, i0)+pick3(cc, i1)-pick3(cc, i0), g.dD = pick3(d, i1)-pick3(d, i0);
    g.l0 = pick3(g.l, i0), g.q0 = pick3(g.q, i0), g.l1 = pick3(g.l, i1), g.q1 = pick3(g.q, i1);
}

struct TSink {                      // of Before::diagonalPairFast and the dense form
    std::vector<double> t;
    void operator()(double v) { t.push_back(v); }
};
struct DirTSink {                   // of evaluatePair
    std::vector<double> t;
    int dx, dy, badDir;
    void operator()(double v, int ddx, int ddy) { t.push_back(v); badDir += ddx != dx || ddy != dy; }
};
struct NullSink {
    void operator()(double) { }
};

bool sameBits(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size()*sizeof(double)) == 0);
}

struct Item {                       // one diagonal test: texel (x, yn), neighbour k, channel pair j; lane: the texel's lane in its tile
    int x, yn, k, j, lane;
};

struct Config { int dist, order; bool p1; };
const Config CONFIGS[] = { { EC_CHECK_AT_EDGE, EC_ORDER_EAGER, false }, { EC_CHECK_AT_EDGE, EC_ORDER_EAGER, true }, { EC_CHECK_AT_EDGE, EC_ORDER_LAZY, true },
                           { EC_CHECK_AT_EDGE, EC_ORDER_LAZY_HELD, true }, { EC_DO_NOT_CHECK, EC_ORDER_EAGER, false }, { EC_DO_NOT_CHECK, EC_ORDER_EAGER, true },
                           { EC_ALWAYS_CHECK, EC_ORDER_EAGER, false }, { EC_ALWAYS_CHECK, EC_ORDER_EAGER, true } };
enum { N_CONFIGS = sizeof(CONFIGS)/sizeof(CONFIGS[0]), CONFIG_LAZY = 2 };

struct Texels {
    const SdfView *sdf;
    const float *c, *n, *hb, *vc;
    Texels(const SdfView &s, const Item &it) : sdf(&s) {
        const int dx = ecNeighbourDx(it.k), dy = ecNeighbourDy(it.k);
        c = s.native(it.x, it.yn), n = s.native(it.x+dx, it.yn+dy), hb = s.native(it.x+dx, it.yn), vc = s.native(it.x, it.yn+dy);
    }
};

// What the lazy order's root loop does for one item, from the helpers of today's diagonalPairFast.
struct Analysis {
    bool solve, in0, in1, e0, e1, errorAtFirst, held, dscrZero, linearBranch, tExZero, tExOne, qZero;
    int m, ne;
};

void analyse(Analysis &z, const DiagArgs &g) {
    memset(&z, 0, sizeof(z));
    const double qa = g.dD-g.dBC+g.dA, qb = g.dBC-g.dA-g.dA, qc = g.dA;
    z.solve = quadraticMayHaveRootInRange(qa, qb, qc);
    if (!z.solve)
        return;
    z.linearBranch = qa == 0 || fabs(qb) > 1e12*fabs(qa);
    z.dscrZero = !z.linearBranch && qb*qb-4*qa*qc == 0;
    double t[2] = { 0, 0 };
    const int solutions = solveQuadratic(t, qa, qb, qc);
    z.in0 = solutions > 0 && t[0] > MSDF_ARTIFACT_T_EPSILON && t[0] < 1-MSDF_ARTIFACT_T_EPSILON;
    z.in1 = solutions > 1 && t[1] > MSDF_ARTIFACT_T_EPSILON && t[1] < 1-MSDF_ARTIFACT_T_EPSILON;
    z.m = (int) z.in0+(int) z.in1;
    if (!z.m)
        return;
    const double tEx0 = -.5*g.l0/g.q0, tEx1 = -.5*g.l1/g.q1;
    z.e0 = tEx0 > 0 && tEx0 < 1, z.e1 = tEx1 > 0 && tEx1 < 1;
    z.ne = (int) z.e0+(int) z.e1;
    z.tExZero = tEx0 == 0 || tEx1 == 0, z.tExOne = tEx0 == 1 || tEx1 == 1;
    z.qZero = g.q0 == 0 || g.q1 == 0;
    NullSink none;
    const int all = Before::diagonalPairFast(g.cx, g.cm, g.nm, g.a3, g.l, g.q, g.dA, g.dBC, g.dD, g.l0, g.q0, g.l1, g.q1, none);
    z.held = (all&EC_V_HELD) != 0;
    // did the ERROR come at the first root? Before cannot be asked for one root, so the flags of r0 alone are put together from the pieces of today's
    // form (which main() holds against Before for the whole pair)
    DiagonalRoots d;
    diagonalRootsInRange(d, qa, qb, qc, g.l0, g.q0, g.l1, g.q1);
    const float xm = interpolatedMedianQuad(g.a3, g.l, g.q, d.r0);
    int flags = 0, verdict = 0;
    for (int test = 0; test <= d.ne; ++test)
        flags |= diagonalUnitFlags(g.cx, g.cm, g.nm, g.a3, g.l, g.q, d.r0, test == 1 ? d.ex0 : d.ex1, test != 0, xm);
    z.errorAtFirst = (all&EC_V_ERROR) && diagonalRootVerdict(g.cx, flags, d.r0, verdict, none);
}

struct Categories {
    long compared, solved, rootLanes, bothRoots, onlyT0, onlyT1, bothExtrema, oneExtremum, noExtremum, errorAtFirstOfTwo, held, dscrZero, linearBranch, tExZero,
         tExOne, qZero, nonFinite;
    void add(const Analysis &z, bool nonFiniteTexel) {
        ++compared;
        solved += z.solve, dscrZero += z.dscrZero, linearBranch += z.linearBranch, nonFinite += nonFiniteTexel;
        if (!z.m)
            return;
        ++rootLanes;
        bothRoots += z.m == 2, onlyT0 += z.m == 1 && z.in0, onlyT1 += z.m == 1 && z.in1;
        bothExtrema += z.ne == 2, oneExtremum += z.ne == 1, noExtremum += z.ne == 0;
        errorAtFirstOfTwo += z.m == 2 && z.errorAtFirst, held += z.held;
        tExZero += z.tExZero, tExOne += z.tExOne, qZero += z.qZero;
    }
    void print() const {
        printf("{\"compared\": %ld, \"solved\": %ld, \"root_lanes\": %ld, \"both_roots\": %ld, \"only_t0\": %ld, \"only_t1\": %ld, \"both_extrema\": %ld, "
               "\"one_extremum\": %ld, \"no_extremum\": %ld, \"error_at_first_of_two\": %ld, \"held_back\": %ld, \"dscr_zero\": %ld, \"linear_branch\": %ld, "
               "\"tex_zero\": %ld, \"tex_one\": %ld, \"q_zero\": %ld, \"non_finite\": %ld}", compared, solved, rootLanes, bothRoots, onlyT0, onlyT1, bothExtrema,
               oneExtremum, noExtremum, errorAtFirstOfTwo, held, dscrZero, linearBranch, tExZero, tExOne, qZero, nonFinite);
    }
};

struct RoundCounts {
    long tiles, rounds, items, linearItems, diagonalItems, roundsLinear, roundsSolve, roundsLoop, lanesLoop, onlyT0, onlyT1, bothRoots, body[2], block[2][2],
         lanesEx0, lanesEx1, lanesExBoth, pass[2], passEx1, passEx2, pairs, pairsMax, units, unitsMax, roundsOver64;
};

struct Bad { long verdictA, sinkA, dirA, verdictB, sinkB; };

// The dense form of phase C for the diagonal items of one round (at most 64): every (item, in-range root, test) unit gets a lane.
// verdicts / sinks: per item, to be compared with Before.
void runDense(const SdfView &sdf, const EcParams &p, const Config &cf, const Item *items, int n, int *verdicts, TSink *sinks, long &unitsOut) {
    DiagonalRoots roots[64];
    unsigned short descriptors[64*6];                // source lane | root<<6 | test<<7
    int flagWords[64][2];
    int nUnits = 0;
    for (int s = 0; s < n; ++s) {                    // item lanes: the roots, then the unit counts (a prefix sum on the device)
        const Texels tx(sdf, items[s]);
        DiagArgs g;
        diagArgs(g, tx.c, tx.n, tx.hb, tx.vc, p, cf.p1, items[s].j, cf.order);
        flagWords[s][0] = flagWords[s][1] = 0;
        if (!diagonalRootsInRange(roots[s], g.dD-g.dBC+g.dA, g.dBC-g.dA-g.dA, g.dA, g.l0, g.q0, g.l1, g.q1))
            continue;
        for (int root = 0; root < roots[s].m; ++root)
            for (int test = 0; test <= roots[s].ne; ++test)
                descriptors[nUnits++] = (unsigned short) (s|root<<6|test<<7);
    }
    unitsOut = nUnits;
    for (int base = 0; base < nUnits; base += 64)    // unit lanes, in chunks of 64
        for (int u = base; u < nUnits && u < base+64; ++u) {
            const int s = descriptors[u]&63, root = (descriptors[u]>>6)&1, test = descriptors[u]>>7;
            const Texels tx(sdf, items[s]);
            DiagArgs g;
            diagArgs(g, tx.c, tx.n, tx.hb, tx.vc, p, cf.p1, items[s].j, cf.order);     // re-derived from the halo, as evaluatePair does
            const double r = root ? roots[s].r1 : roots[s].r0;                           // (a lane shuffle on the device)
            const float xm = interpolatedMedianQuad(g.a3, g.l, g.q, r);
            flagWords[s][root] |= diagonalUnitFlags(g.cx, g.cm, g.nm, g.a3, g.l, g.q, r, test == 1 ? roots[s].ex0 : roots[s].ex1, test != 0, xm);
        }
    for (int s = 0; s < n; ++s) {                    // item lanes again: the verdict sequence in root order
        const Texels tx(sdf, items[s]);
        DiagArgs g;
        diagArgs(g, tx.c, tx.n, tx.hb, tx.vc, p, cf.p1, items[s].j, cf.order);
        int verdict = 0;
        for (int root = 0; root < roots[s].m; ++root)
            if (diagonalRootVerdict(g.cx, flagWords[s][root], root ? roots[s].r1 : roots[s].r0, verdict, sinks[s]))
                break;
        verdicts[s] = verdict;
    }
}

struct EmitItems {
    std::vector<Item> *out;
    int x, yn, lane;
    void operator()(int k, int j) { const Item it = { x, yn, k, j, lane }; out->push_back(it); }
};

bool finite3(const float *t) { return std::isfinite(t[0]) && std::isfinite(t[1]) && std::isfinite(t[2]); }

}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    int32_t n = 0;
    if (!f || !readN(f, &n, 1) || n < 0) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    Bad bad;
    memset(&bad, 0, sizeof(bad));
    long badByConfig[N_CONFIGS] = { 0 }, comparisons = 0, sinkCalls = 0;
    Categories items[8], pairs[8];
    RoundCounts rc[8];
    memset(items, 0, sizeof(items));
    memset(pairs, 0, sizeof(pairs));
    memset(rc, 0, sizeof(rc));
    std::vector<long> caseMaxUnits;
    for (int ci = 0; ci < n; ++ci) {
        Case c;
        if (!readCase(f, c)) {
            fprintf(stderr, "case %d of %s is malformed\n", ci, argv[1]);
            return 2;
        }
        SdfView sdf;
        sdf.px = c.field.data(), sdf.w = c.w, sdf.h = c.h, sdf.N = 3, sdf.flip = c.flip;
        EcParams params[3];
        for (int dist = EC_DO_NOT_CHECK; dist <= EC_ALWAYS_CHECK; ++dist) {
            EcParams &p = params[dist];
            const Xform t = { c.xf[0], c.xf[1], c.xf[2], c.xf[3], c.xf[4], c.xf[5] };
            p.t = t;
            p.minDeviationRatio = 1.11111111111111111, p.minImproveRatio = 1.11111111111111111;
            p.mode = EC_MODE_EDGE_PRIORITY, p.distanceCheck = dist, p.overlap = 1, p.stageLimit = 0;
            ecDerive(p);
        }
        long maxUnits = 0;
        for (int ty = 0; ty*8 < c.h; ++ty)
            for (int tx = 0; tx*8 < c.w; ++tx) {
                // ---- every diagonal test of the tile's texels whose neighbour exists (compared), and the tests stage 1 queues (counted, emulated)
                std::vector<Item> all, queued;
                for (int lane = 0; lane < 64; ++lane) {
                    const int x = tx*8+(lane&7), yn = ty*8+(lane>>3);
                    if (x >= c.w || yn >= c.h)
                        continue;
                    for (int k = 4; k < 8; ++k) {
                        const int nx = x+ecNeighbourDx(k), ny = yn+ecNeighbourDy(k);
                        if (nx < 0 || ny < 0 || nx >= c.w || ny >= c.h)
                            continue;
                        for (int j = 0; j < 3; ++j) {
                            const Item it = { x, yn, k, j, lane };
                            all.push_back(it);
                        }
                    }
                    Neighbourhood nb;
                    loadNeighbourhood(nb, sdf, x, yn);
                    EmitItems emit = { &queued, x, yn, lane };
                    texelCandidatePairs(nb, emit);
                }
                // the queue as the wavefront fills it: one push site after the other (k outer, j inner), the lanes of a site in order
                std::stable_sort(queued.begin(), queued.end(), [](const Item &a, const Item &b) { return a.k*3+a.j < b.k*3+b.j; });
                for (int pass = 0; pass < 2; ++pass) {
                    const std::vector<Item> &list = pass ? queued : all;
                    for (size_t base = 0; base < list.size(); base += 64) {
                        const int cnt = (int) std::min<size_t>(64, list.size()-base);
                        Item round[64];
                        int nd = 0;
                        for (int i = 0; i < cnt; ++i)
                            if (list[base+i].k >= 4)
                                round[nd++] = list[base+i];
                        for (int cfi = 0; cfi < N_CONFIGS; ++cfi) {
                            const Config &cf = CONFIGS[cfi];
                            const EcParams &p = params[cf.dist];
                            int denseVerdict[64];
                            TSink denseSink[64];
                            long units = 0;
                            runDense(sdf, p, cf, round, nd, denseVerdict, denseSink, units);
                            if (pass && cfi == CONFIG_LAZY)
                                maxUnits = std::max(maxUnits, units);
                            for (int i = 0; i < nd; ++i) {
                                const Item &it = round[i];
                                const Texels tx4(sdf, it);
                                DiagArgs g;
                                diagArgs(g, tx4.c, tx4.n, tx4.hb, tx4.vc, p, cf.p1, it.j, cf.order);
                                TSink want;
                                const int wantVerdict = Before::diagonalPairFast(g.cx, g.cm, g.nm, g.a3, g.l, g.q, g.dA, g.dBC, g.dD, g.l0, g.q0, g.l1, g.q1, want);
                                const bool vB = denseVerdict[i] != wantVerdict, sB = !sameBits(denseSink[i].t, want.t);
                                bad.verdictB += vB, bad.sinkB += sB;
                                badByConfig[cfi] += vB+sB;
                                if (pass)
                                    continue;                                   // (the queued tests are among `all`)
                                DirTSink got;
                                got.dx = ecNeighbourDx(it.k), got.dy = c.flip ? -ecNeighbourDy(it.k) : ecNeighbourDy(it.k), got.badDir = 0;
                                const int gotVerdict = evaluatePair(tx4.c, tx4.n, tx4.hb, tx4.vc, p, cf.p1, c.flip, it.k, it.j, got, cf.order);
                                const bool vA = gotVerdict != wantVerdict, sA = !sameBits(got.t, want.t);
                                bad.verdictA += vA, bad.sinkA += sA, bad.dirA += got.badDir;
                                badByConfig[cfi] += vA+sA+got.badDir;
                                ++comparisons, sinkCalls += (long) want.t.size();
                            }
                        }
                    }
                }
                // ---- categories (lazy order, library default) and what a wavefront executes per round of the queue
                const EcParams &p = params[EC_CHECK_AT_EDGE];
                const Config &lazy = CONFIGS[CONFIG_LAZY];
                for (int pass = 0; pass < 2; ++pass) {
                    const std::vector<Item> &list = pass ? queued : all;
                    for (size_t i = 0; i < list.size(); ++i) {
                        if (list[i].k < 4)
                            continue;
                        const Texels t4(sdf, list[i]);
                        DiagArgs g;
                        diagArgs(g, t4.c, t4.n, t4.hb, t4.vc, p, lazy.p1, list[i].j, lazy.order);
                        Analysis z;
                        analyse(z, g);
                        (pass ? items : pairs)[c.group].add(z, !(finite3(t4.c) && finite3(t4.n) && finite3(t4.hb) && finite3(t4.vc)));
                    }
                }
                RoundCounts &r = rc[c.group];
                ++r.tiles;
                r.items += (long) queued.size();
                for (size_t base = 0; base < queued.size(); base += 64) {
                    const int cnt = (int) std::min<size_t>(64, queued.size()-base);
                    bool linear = false, solve = false, body[2] = { false, false }, block[2][2] = { { false, false }, { false, false } };
                    bool pass[2] = { false, false }, passEx1[2] = { false, false }, passEx2[2] = { false, false };
                    long pairsHere = 0, unitsHere = 0;
                    for (int i = 0; i < cnt; ++i) {
                        const Item &it = queued[base+i];
                        if (it.k < 4) {
                            linear = true, ++r.linearItems;
                            continue;
                        }
                        ++r.diagonalItems;
                        const Texels t4(sdf, it);
                        DiagArgs g;
                        diagArgs(g, t4.c, t4.n, t4.hb, t4.vc, p, lazy.p1, it.j, lazy.order);
                        Analysis z;
                        analyse(z, g);
                        solve = solve || z.solve;
                        if (!z.m)
                            continue;
                        ++r.lanesLoop;
                        r.onlyT0 += z.m == 1 && z.in0, r.onlyT1 += z.m == 1 && z.in1, r.bothRoots += z.m == 2;
                        r.lanesEx0 += z.e0, r.lanesEx1 += z.e1, r.lanesExBoth += z.e0 && z.e1;
                        const bool second = z.m == 2 && !z.errorAtFirst;                  // the lane is still there for its second root
                        // before: iteration i runs its body where t[i] is in range, its two blocks where tEx0 / tEx1 is
                        const bool it0 = z.in0, it1 = z.in1 && !(z.in0 && z.errorAtFirst);
                        body[0] = body[0] || it0, body[1] = body[1] || it1;
                        block[0][0] = block[0][0] || (it0 && z.e0), block[0][1] = block[0][1] || (it0 && z.e1);
                        block[1][0] = block[1][0] || (it1 && z.e0), block[1][1] = block[1][1] || (it1 && z.e1);
                        // after: pass i over the i-th in-range root, then the first and the second in-range extremum
                        pass[0] = true, pass[1] = pass[1] || second;
                        passEx1[0] = passEx1[0] || z.ne >= 1, passEx2[0] = passEx2[0] || z.ne >= 2;
                        passEx1[1] = passEx1[1] || (second && z.ne >= 1), passEx2[1] = passEx2[1] || (second && z.ne >= 2);
                        pairsHere += z.m, unitsHere += z.m*(1+z.ne);
                    }
                    ++r.rounds;
                    r.roundsLinear += linear, r.roundsSolve += solve, r.roundsLoop += pass[0];
                    for (int i = 0; i < 2; ++i) {
                        r.body[i] += body[i], r.pass[i] += pass[i], r.passEx1 += passEx1[i], r.passEx2 += passEx2[i];
                        r.block[i][0] += block[i][0], r.block[i][1] += block[i][1];
                    }
                    r.pairs += pairsHere, r.pairsMax = std::max(r.pairsMax, pairsHere);
                    r.units += unitsHere, r.unitsMax = std::max(r.unitsMax, unitsHere), r.roundsOver64 += unitsHere > 64;
                }
            }
        caseMaxUnits.push_back(maxUnits);
    }
    fclose(f);
    printf("{\"cases\": %d, \"comparisons\": %ld, \"sink_calls\": %ld, \"bad_verdict\": %ld, \"bad_sink_list\": %ld, \"bad_sink_direction\": %ld, "
           "\"bad_dense_verdict\": %ld, \"bad_dense_sink_list\": %ld,\n \"bad_by_config\": [", (int) n, comparisons, sinkCalls, bad.verdictA, bad.sinkA, bad.dirA,
           bad.verdictB, bad.sinkB);
    for (int i = 0; i < N_CONFIGS; ++i)
        printf("%s[%d, %d, %d, %ld]", i ? ", " : "", CONFIGS[i].dist, CONFIGS[i].order, (int) CONFIGS[i].p1, badByConfig[i]);
    printf("],\n \"case_max_units_per_round\": [");
    for (size_t i = 0; i < caseMaxUnits.size(); ++i)
        printf("%s%ld", i ? ", " : "", caseMaxUnits[i]);
    printf("],\n \"groups\": [");
    for (int g = 0; g < 8; ++g) {
        const RoundCounts &r = rc[g];
        printf("%s{\"items\": ", g ? ",\n  " : "");
        items[g].print();
        printf(", \"pairs\": ");
        pairs[g].print();
        printf(", \"rounds\": {\"tiles\": %ld, \"rounds\": %ld, \"queued_items\": %ld, \"linear_items\": %ld, \"diagonal_items\": %ld, \"rounds_with_linear\": %ld, "
               "\"rounds_reaching_solve\": %ld, \"rounds_reaching_loop\": %ld, \"lanes_reaching_loop\": %ld, \"only_t0\": %ld, \"only_t1\": %ld, \"both_roots\": %ld, "
               "\"before_body\": [%ld, %ld], \"before_extremum_blocks\": [%ld, %ld, %ld, %ld], \"lanes_tex0\": %ld, \"lanes_tex1\": %ld, \"lanes_tex_both\": %ld, "
               "\"after_passes\": [%ld, %ld], \"after_rounds_first_extremum\": %ld, \"after_rounds_second_extremum\": %ld, \"item_root_pairs\": %ld, "
               "\"item_root_pairs_max\": %ld, \"units\": %ld, \"units_max\": %ld, \"rounds_over_64_units\": %ld}}", r.tiles, r.rounds, r.items, r.linearItems,
               r.diagonalItems, r.roundsLinear, r.roundsSolve, r.roundsLoop, r.lanesLoop, r.onlyT0, r.onlyT1, r.bothRoots, r.body[0], r.body[1], r.block[0][0],
               r.block[0][1], r.block[1][0], r.block[1][1], r.lanesEx0, r.lanesEx1, r.lanesExBoth, r.pass[0], r.pass[1], r.passEx1, r.passEx2, r.pairs,
               r.pairsMax, r.units, r.unitsMax, r.roundsOver64);
    }
    printf("]}\n");
    return bad.verdictA || bad.sinkA || bad.dirA || bad.verdictB || bad.sinkB ? 1 : 0;
}
