// TEST TOOLING ONLY -- the hardware-median instantiation of the error-correction sweep (msdf_device.hpp: med3f / medianOf; msdf_ec_fast.hpp: the HWMED,
// INDEXED and CORDER template switches of evaluatePair / texelFindFast, which k_ec_fast turns on behind its finiteness vote) compiled for the host with
// g++, where med3f runs the ISA's definition of v_med3_f32 (med3Model), for tests/test_ec_hw_median_host.py and tests/test_gpu_ec_hw_median.py.
// A stand-alone program, so that it can also be built with -fsanitize=address,undefined and run as it is. Never loaded by the msdfgen_amd package.
//
//   ec_hw_median_host median SEED COUNT     med3Model against medianf: all triples of a set of special values, then COUNT seeded random triples
//                                           (raw bit patterns, and draws from a small pool so that ties occur). Returns 1 if a triple WITHOUT a NaN gives
//                                           two different VALUES (a == b, zeros of either sign equal). Reports, without judging them, the triples whose
//                                           results differ in the sign of a zero and the triples with a NaN whose results differ.
//   ec_hw_median_host sweep CASES           per texel of every case, under every (mode, distance check, order, protection) the sweep runs in: verdict bits
//                                           and the ordered candidate list (t, dx, dy) of texelFindFast<true> against texelFindFast<false>; and per stage-2
//                                           item evaluatePair<true, true, order> (what k_ec_fast's lazy instantiation compiles: hardware median, indexed
//                                           channel reads, configuration folded) against evaluatePair<>. Returns 1 if they differ at a texel where the vote
//                                           passes -- every colour channel of the texels of its 3x3 neighbourhood inside the bitmap below 2^100 in
//                                           magnitude (the kernel votes per tile and halo, which implies this for each of the tile's texels). Texels
//                                           where the vote fails are compared too and only counted: that they do differ is why the kernel votes.
//   ec_hw_median_host correct CASES OUT     the shapeless error correction of every case by the host walk ecTexelFast (exact spelling), as
//                                           ec_stage1_words_host does; OUT: corrected field and stencil-less result, float[h][w][3] per case
//   CASES: int32 n, then per case int32 w, h, protectAll, 0 | double xf[6] (sx, sy, tx, ty, mapScale, mapTranslate) | double minDeviationRatio
//                                 | float field[h][w][3] (rows in memory order)            (the format of tests/ecwordscases.py: pack)
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../msdfgen_amd/csrc/msdf_device.hpp"
#include "../../msdfgen_amd/csrc/msdf_prep.hpp"
#include "../../msdfgen_amd/csrc/msdf_ec.hpp"
#include "../../msdfgen_amd/csrc/msdf_ec_fast.hpp"

using namespace msdfhip;

namespace {

const float VOTE_BOUND = 0x1p100f;          // EC_MED3_BOUND of ecFastBody (msdf_kernels.hpp)

uint32_t bitsOf(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
float floatOf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

struct MedianCounts { long triples, nanTriples, valueMismatch, zeroSignDiffers, nanDiffers; };

void compareMedian(float a, float b, float c, MedianCounts &n) {
    const float want = medianf(a, b, c), got = med3Model(a, b, c);
    ++n.triples;
    if (a != a || b != b || c != c) {
        ++n.nanTriples;
        n.nanDiffers += bitsOf(want) != bitsOf(got) && !(want != want && got != got);
        return;
    }
    if (!(want == got))
        ++n.valueMismatch;
    else if (bitsOf(want) != bitsOf(got))
        ++n.zeroSignDiffers;                // equal as values, different bits: only +0 / -0
}

int runMedian(uint64_t seed, long count) {
    std::vector<float> special;
    const float half = .5f;
    const float positives[] = { 0.f, floatOf(1u), floatOf(0x007fffffu), FLT_MIN, 1.f, FLT_MAX, INFINITY };
    for (float v : positives)
        special.push_back(v), special.push_back(-v);
    special.push_back(half), special.push_back(nextafterf(half, 0.f)), special.push_back(nextafterf(half, 1.f));
    MedianCounts finite = { 0, 0, 0, 0, 0 }, withNan = { 0, 0, 0, 0, 0 }, random = { 0, 0, 0, 0, 0 };
    for (float a : special)
        for (float b : special)
            for (float c : special)
                compareMedian(a, b, c, finite);
    special.push_back(NAN), special.push_back(-NAN);
    for (float a : special)
        for (float b : special)
            for (float c : special)
                if (a != a || b != b || c != c)
                    compareMedian(a, b, c, withNan);
    uint64_t s = seed*0x9e3779b97f4a7c15ull+1;
    const auto next = [&]() { s ^= s<<13, s ^= s>>7, s ^= s<<17; return (uint32_t) (s>>16); };
    for (long i = 0; i < count; ++i) {
        float v[3];
        for (int k = 0; k < 3; ++k) {
            const uint32_t r = next();
            if (i&1)
                v[k] = floatOf(r);                                       // any bit pattern: all exponents, denormals, some NaNs
            else
                v[k] = special[r%17]*(float) (1+(r>>8)%3);                // a small pool: ties, zeros of both signs, overflow to inf
        }
        compareMedian(v[0], v[1], v[2], random);
    }
    printf("{\"special_triples\": %ld, \"special_value_mismatch\": %ld, \"special_zero_sign_differs\": %ld,\n"
           " \"nan_triples\": %ld, \"nan_differs\": %ld,\n"
           " \"random_triples\": %ld, \"random_nan_triples\": %ld, \"random_value_mismatch\": %ld, \"random_zero_sign_differs\": %ld, \"random_nan_differs\": %ld}\n",
           finite.triples, finite.valueMismatch, finite.zeroSignDiffers, withNan.triples, withNan.nanDiffers,
           random.triples, random.nanTriples, random.valueMismatch, random.zeroSignDiffers, random.nanDiffers);
    return finite.valueMismatch || random.valueMismatch ? 1 : 0;
}

struct Case {
    int w, h, protectAll;
    double xf[6], ratio;
    std::vector<float> field;
};

bool readCase(FILE *f, Case &c) {
    int32_t head[4];
    if (fread(head, sizeof(int32_t), 4, f) != 4)
        return false;
    c.w = head[0], c.h = head[1], c.protectAll = head[2];
    if (c.w < 1 || c.h < 1 || c.w > 4096 || c.h > 4096 || (c.protectAll != 0 && c.protectAll != 1) || head[3] != 0)
        return false;
    if (fread(c.xf, sizeof(double), 6, f) != 6 || fread(&c.ratio, sizeof(double), 1, f) != 1)
        return false;
    c.field.assign((size_t) c.w*c.h*3, 0.f);
    return fread(c.field.data(), sizeof(float), c.field.size(), f) == c.field.size();
}

struct Cand {
    double t;
    int dx, dy;
    bool operator==(const Cand &o) const { return memcmp(&t, &o.t, sizeof(t)) == 0 && dx == o.dx && dy == o.dy; }
};
struct VecSink {
    std::vector<Cand> v;
    void operator()(double t, int dx, int dy) { const Cand c = { t, dx, dy }; v.push_back(c); }
};
struct Items {
    unsigned char k[24], j[24];
    int n;
    void operator()(int kk, int jj) { k[n] = (unsigned char) kk, j[n] = (unsigned char) jj; ++n; }
};

bool votePasses(const SdfView &sdf, int x, int yn) {
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int nx = x+dx, ny = yn+dy;
            if (nx < 0 || ny < 0 || nx >= sdf.w || ny >= sdf.h)
                continue;
            const float *t = sdf.native(nx, ny);
            if (!(fabsf(t[0]) < VOTE_BOUND && fabsf(t[1]) < VOTE_BOUND && fabsf(t[2]) < VOTE_BOUND))
                return false;
        }
    return true;
}

struct Config { int mode, check, order; bool p1; };
const Config CONFIGS[] = {
    { EC_MODE_EDGE_PRIORITY, EC_CHECK_AT_EDGE, EC_ORDER_LAZY, true },          // the library default: what k_ec_fast<N, true> runs
    { EC_MODE_EDGE_PRIORITY, EC_CHECK_AT_EDGE, EC_ORDER_LAZY_HELD, true },
    { EC_MODE_EDGE_PRIORITY, EC_CHECK_AT_EDGE, EC_ORDER_EAGER, false },
    { EC_MODE_EDGE_PRIORITY, EC_CHECK_AT_EDGE, EC_ORDER_EAGER, true },
    { EC_MODE_EDGE_PRIORITY, EC_DO_NOT_CHECK, EC_ORDER_EAGER, false },
    { EC_MODE_EDGE_PRIORITY, EC_DO_NOT_CHECK, EC_ORDER_EAGER, true },
    { EC_MODE_EDGE_PRIORITY, EC_ALWAYS_CHECK, EC_ORDER_EAGER, false },
    { EC_MODE_EDGE_PRIORITY, EC_ALWAYS_CHECK, EC_ORDER_EAGER, true },
    { EC_MODE_INDISCRIMINATE, EC_DO_NOT_CHECK, EC_ORDER_EAGER, false },        // the shapeless entries
    { EC_MODE_EDGE_ONLY, EC_DO_NOT_CHECK, EC_ORDER_EAGER, true },
};

struct SweepCounts {
    long texels, voteTexels, comparisons, bad, badOutsideVote, verdictBits[4], candidates, items, linearItems, diagonalItems, foldedComparisons, badFolded, protectComparisons, badProtect,
         badDeviation;
};

// evaluatePair as k_ec_fast's instantiations compile it (order a compile-time constant) against the plain call
template <int CORDER>
void compareFolded(const Neighbourhood &nb, const EcParams &p, const Config &cf, const Items &items, bool vote, SweepCounts &n) {
    for (int i = 0; i < items.n; ++i) {
        const int k = items.k[i], dx = ecNeighbourDx(k), dy = ecNeighbourDy(k);
        VecSink want, got;
        const int wv = evaluatePair(nb.v[1][1], nb.v[dy+1][dx+1], nb.v[1][dx+1], nb.v[dy+1][1], p, cf.p1, 0, k, items.j[i], want, cf.order);
        const int gv = evaluatePair<true, true, CORDER>(nb.v[1][1], nb.v[dy+1][dx+1], nb.v[1][dx+1], nb.v[dy+1][1], p, cf.p1, 0, k, items.j[i], got, CORDER);
        const bool same = wv == gv && want.v == got.v;
        if (vote)
            ++n.foldedComparisons, n.badFolded += !same;
    }
}

int runSweep(const char *path) {
    FILE *f = fopen(path, "rb");
    int32_t nCases = 0;
    if (!f || fread(&nCases, sizeof(nCases), 1, f) != 1 || nCases < 0) {
        fprintf(stderr, "cannot read %s\n", path);
        return 2;
    }
    SweepCounts n;
    memset(&n, 0, sizeof(n));
    for (int i = 0; i < nCases; ++i) {
        Case c;
        if (!readCase(f, c)) {
            fprintf(stderr, "case %d of %s is malformed\n", i, path);
            return 2;
        }
        SdfView sdf;
        sdf.px = c.field.data(), sdf.w = c.w, sdf.h = c.h, sdf.N = 3, sdf.flip = 0;
        const Xform t = { c.xf[0], c.xf[1], c.xf[2], c.xf[3], c.xf[4], c.xf[5] };
        for (int yn = 0; yn < c.h; ++yn)
            for (int x = 0; x < c.w; ++x) {
                Neighbourhood nb;
                loadNeighbourhood(nb, sdf, x, yn);
                const bool vote = votePasses(sdf, x, yn);
                ++n.texels, n.voteTexels += vote;
                Items items;
                items.n = 0;
                texelCandidatePairs(nb, items);
                if (vote) {
                    n.items += items.n;
                    for (int it = 0; it < items.n; ++it)
                        ++(items.k[it] < 4 ? n.linearItems : n.diagonalItems);
                    // the deviation and the protectEdges pairs of the lazy protection round
                    n.badDeviation += bitsOf(ecTexelDeviation<true>(nb.v[1][1])) != bitsOf(ecTexelDeviation<false>(nb.v[1][1]));
                    for (int m = 0; m < 9; ++m)
                        if (m != 4 && (nb.valid&(1u<<m)))
                            for (int swap = 0; swap < 2; ++swap) {
                                ++n.protectComparisons;
                                n.badProtect += evaluateProtectPair<true>(nb.v[1][1], nb.v[m/3][m%3], m, swap != 0) != evaluateProtectPair<false>(nb.v[1][1], nb.v[m/3][m%3], m, swap != 0);
                            }
                }
                for (const Config &cf : CONFIGS) {
                    EcParams p;
                    p.t = t;
                    p.minDeviationRatio = c.ratio, p.minImproveRatio = 1.11111111111111111;
                    p.mode = cf.mode, p.distanceCheck = cf.check, p.overlap = 0, p.stageLimit = 0;
                    ecDerive(p);
                    VecSink want, got;
                    const int wv = texelFindFast<false>(nb, p, cf.p1, 0, want, cf.order);
                    const int gv = texelFindFast<true>(nb, p, cf.p1, 0, got, cf.order);
                    const bool same = wv == gv && want.v == got.v;
                    if (vote) {
                        ++n.comparisons, n.bad += !same;
                        for (int b = 0; b < 4; ++b)
                            n.verdictBits[b] += (wv>>b)&1;
                        n.candidates += (long) want.v.size();
                    } else
                        n.badOutsideVote += !same;
                    if (cf.order == EC_ORDER_LAZY)
                        compareFolded<EC_ORDER_LAZY>(nb, p, cf, items, vote, n);
                    else if (cf.order == EC_ORDER_LAZY_HELD)
                        compareFolded<EC_ORDER_LAZY_HELD>(nb, p, cf, items, vote, n);
                    else
                        compareFolded<EC_ORDER_EAGER>(nb, p, cf, items, vote, n);
                }
            }
    }
    fclose(f);
    printf("{\"cases\": %d, \"texels\": %ld, \"vote_texels\": %ld, \"comparisons\": %ld, \"bad\": %ld, \"differ_outside_vote\": %ld,\n"
           " \"verdict_bits\": [%ld, %ld, %ld, %ld], \"candidates\": %ld, \"items\": %ld, \"linear_items\": %ld, \"diagonal_items\": %ld,\n"
           " \"folded_comparisons\": %ld, \"bad_folded\": %ld, \"protect_comparisons\": %ld, \"bad_protect\": %ld, \"bad_deviation\": %ld}\n",
           (int) nCases, n.texels, n.voteTexels, n.comparisons, n.bad, n.badOutsideVote, n.verdictBits[0], n.verdictBits[1], n.verdictBits[2], n.verdictBits[3],
           n.candidates, n.items, n.linearItems, n.diagonalItems, n.foldedComparisons, n.badFolded, n.protectComparisons, n.badProtect, n.badDeviation);
    return n.bad || n.badFolded || n.badProtect || n.badDeviation ? 1 : 0;
}

struct NoSink {
    long n;
    void operator()(double, int, int) { ++n; }
};

int runCorrect(const char *path, const char *outPath) {
    FILE *f = fopen(path, "rb"), *out = fopen(outPath, "wb");
    int32_t nCases = 0;
    if (!f || !out || fread(&nCases, sizeof(nCases), 1, f) != 1 || nCases < 0) {
        fprintf(stderr, "cannot read %s or write %s\n", path, outPath);
        return 2;
    }
    long corrected = 0, deferred = 0;
    for (int i = 0; i < nCases; ++i) {
        Case c;
        if (!readCase(f, c)) {
            fprintf(stderr, "case %d of %s is malformed\n", i, path);
            return 2;
        }
        SdfView sdf;
        sdf.px = c.field.data(), sdf.w = c.w, sdf.h = c.h, sdf.N = 3, sdf.flip = 0;
        EcParams p;
        const Xform t = { c.xf[0], c.xf[1], c.xf[2], c.xf[3], c.xf[4], c.xf[5] };
        p.t = t;
        p.minDeviationRatio = c.ratio, p.minImproveRatio = 1.11111111111111111;
        p.mode = c.protectAll ? EC_MODE_EDGE_ONLY : EC_MODE_INDISCRIMINATE, p.distanceCheck = EC_DO_NOT_CHECK, p.overlap = 0, p.stageLimit = 0;
        ecDerive(p);
        std::vector<float> res(c.field);
        for (int yn = 0; yn < c.h; ++yn)
            for (int x = 0; x < c.w; ++x) {
                NoSink sink = { 0 };
                const int st = ecTexelFast(sdf, p, (const int *) NULL, 0, x, yn, sink);
                deferred += sink.n+((st&EC_DEFER) != 0);
                if (st&EC_ERROR) {
                    const float *v = sdf.native(x, yn);
                    const float m = medianf(v[0], v[1], v[2]);
                    float *o = res.data()+((size_t) yn*c.w+x)*3;
                    o[0] = m, o[1] = m, o[2] = m;
                    ++corrected;
                }
            }
        if (fwrite(res.data(), sizeof(float), res.size(), out) != res.size())
            return 2;
    }
    fclose(f);
    if (fclose(out) != 0)
        return 2;
    printf("{\"cases\": %d, \"corrected\": %ld, \"deferred\": %ld}\n", (int) nCases, corrected, deferred);
    return deferred ? 1 : 0;                                         // no distance check in these configurations
}

}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "median"))
        return runMedian(strtoull(argv[2], NULL, 10), atol(argv[3]));
    if (argc == 3 && !strcmp(argv[1], "sweep"))
        return runSweep(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "correct"))
        return runCorrect(argv[2], argv[3]);
    fprintf(stderr, "usage: %s median SEED COUNT | sweep CASES | correct CASES OUT\n", argv[0]);
    return 2;
}
