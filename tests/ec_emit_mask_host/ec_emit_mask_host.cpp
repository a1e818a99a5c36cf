// TEST TOOLING ONLY -- stage 1 of the error-correction sweep as a mask of surviving tests per texel and one append per tile (msdf_ec_fast.hpp:
// texelCandidateMask, texelProtectMask, ecAppendItems, and texelCandidatePairs / texelProtectPairs / texelFindFast on top of the masks) compiled for the
// host with g++, for tests/test_ec_emit_mask_host.py. A stand-alone program, so that it can also be built with -fsanitize=address,undefined and run as it
// is. Never loaded by the msdfgen_amd package.
//
//   ec_emit_mask_host masks CASES      per texel of every case: texelCandidateMask against `Plain`, the per-test spelling (one `if` per test, the predicates
//                                      of the form with one emit per test that the masks replaced); the order in which texelCandidatePairs emits; the protect
//                                      mask and texelProtectPairs' order against the plain spelling under the radii of ten configurations (and two stretched
//                                      transforms more); verdict bits and the ordered candidate list of texelFindFast against a walk over the plain items.
//                                      texelCandidateMask<true> (the Bernstein test through min3 / max3, behind the kernel's finiteness vote) gives the same mask
//                                      wherever the vote passes. Returns 1 on any difference.
//   ec_emit_mask_host append SEED N    the append arithmetic (ecAppendItems: popcounts, exclusive offsets in the queue's two parts from a reservation, bounded walk over the set bits)
//                                      for 64 lanes: all masks zero; one lane only; all 24 bits in all 64 lanes (the queue filled to its capacity); the same
//                                      for the protect queue; N seeded random rounds of each queue, lanes reserving in a seeded order (the device's order is
//                                      not the lanes'). The written queue must hold exactly the expected items, no slot written twice, none outside the count,
//                                      the count the sum of the popcounts, the linear tests ahead of the diagonal ones; a mask with bits that are no test writes only its tests. Returns 1 otherwise.
//   CASES: the format of tests/ecwordscases.py: pack
#include <algorithm>
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

// ---- stage 1 with one `if` and one emit per test, from the same Neighbourhood (class words, deviations, channels)
namespace Plain {

template <class Emit>
void texelCandidatePairs(const Neighbourhood &nb, Emit &emit) {
    const float *c = nb.v[1][1];
    const float cdev = nb.dev[1][1];
    const unsigned cw = nb.cls[1][1];
    for (int k = 0; k < 4; ++k) {
        const int dx = k == 0 ? -1 : k == 2 ? 1 : 0, dy = k == 1 ? -1 : k == 3 ? 1 : 0;
        const unsigned nw = nb.cls[dy+1][dx+1];
        const unsigned opposite = ((cw&(nw>>3))|((cw>>3)&nw))&7u;
        const unsigned m = cdev >= nb.dev[dy+1][dx+1] ? opposite : 0u;
        if (m) {
            if (m&1u)
                emit(k, 0);
            if (m&2u)
                emit(k, 1);
            if (m&4u)
                emit(k, 2);
        }
    }
    for (int k = 4; k < 8; ++k) {
        const int dx = (k&1) ? 1 : -1, dy = (k&2) ? 1 : -1;
        const unsigned dw = nb.cls[dy+1][dx+1];
        if (!(((dw&EC_CLS_INSIDE) != 0)&(cdev >= nb.dev[dy+1][dx+1])))
            continue;
        const float *d = nb.v[dy+1][dx+1];
        const float *b = nb.v[1][dx+1], *cc = nb.v[dy+1][1];
        const unsigned zeroAD = cw&dw;
        for (int j = 0; j < 3; ++j) {
            const int i0 = j, i1 = j == 2 ? 0 : j+1;
            const float dA = c[i1]-c[i0], dBC = b[i1]-b[i0]+cc[i1]-cc[i0], dD = d[i1]-d[i0];
            if ((zeroAD&(64u<<j)) && dBC == 0)
                continue;
            if (bernsteinMayHaveRoot(dA, dBC, dD))
                emit(k, j);
        }
    }
}

template <class Emit>
void texelProtectPairs(const Neighbourhood &nb, const EcParams &p, Emit &emit) {
    const float sdev = nb.dev[1][1];
    for (int dy = -1; dy <= 1; ++dy) {
        for (int dx = -1; dx <= 1; ++dx) {
            if (!dx && !dy)
                continue;
            if (!(nb.cls[dy+1][dx+1]&EC_CLS_INSIDE))
                continue;
            const float radius = dy == 0 ? p.radiusH : dx == 0 ? p.radiusV : p.radiusD;
            const float odev = nb.dev[dy+1][dx+1];
            const bool selfIsA = dy > 0 || (dy == 0 && dx > 0);
            const float sum = selfIsA ? sdev+odev : odev+sdev;
            if (sum < radius)
                emit((dy+1)*3+(dx+1));
        }
    }
}

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
    std::vector<int> kj;            // 4*k+j, in the order emitted
    void operator()(int k, int j) { kj.push_back(4*k+j); }
};
struct ProtectItems {
    std::vector<int> m;
    void operator()(int mm) { m.push_back(mm); }
};

struct Config { int mode, check, order; bool p1; };
const Config CONFIGS[] = {                                                      // those of tests/ec_hw_median_host
    { EC_MODE_EDGE_PRIORITY, EC_CHECK_AT_EDGE, EC_ORDER_LAZY, true },
    { EC_MODE_EDGE_PRIORITY, EC_CHECK_AT_EDGE, EC_ORDER_LAZY_HELD, true },
    { EC_MODE_EDGE_PRIORITY, EC_CHECK_AT_EDGE, EC_ORDER_EAGER, false },
    { EC_MODE_EDGE_PRIORITY, EC_CHECK_AT_EDGE, EC_ORDER_EAGER, true },
    { EC_MODE_EDGE_PRIORITY, EC_DO_NOT_CHECK, EC_ORDER_EAGER, false },
    { EC_MODE_EDGE_PRIORITY, EC_DO_NOT_CHECK, EC_ORDER_EAGER, true },
    { EC_MODE_EDGE_PRIORITY, EC_ALWAYS_CHECK, EC_ORDER_EAGER, false },
    { EC_MODE_EDGE_PRIORITY, EC_ALWAYS_CHECK, EC_ORDER_EAGER, true },
    { EC_MODE_INDISCRIMINATE, EC_DO_NOT_CHECK, EC_ORDER_EAGER, false },
    { EC_MODE_EDGE_ONLY, EC_DO_NOT_CHECK, EC_ORDER_EAGER, true },
};
// (the radii follow the transform alone: two more, with a wider range and unequal scales, so that horizontal, vertical and diagonal radius differ)
const double STRETCH[2][2] = { { .5, 2. }, { 3., .75 } };

const float VOTE_BOUND = 0x1p100f;          // EC_MED3_BOUND of ecFastBody (msdf_kernels.hpp)

// every colour channel of the 3x3 texels inside the bitmap below the bound in magnitude: implied by the kernel's vote over tile and halo
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

struct MaskCounts {
    long voteTexels, badVoteMask, differOutsideVote, texels, badMask, badOrder, badBits, tests[32], survivors, fullTexels, emptyTexels, protectComparisons, badProtect, badProtectOrder, protectPairs, protectBits[9],
         findComparisons, badFind, candidates, verdictBits[4];
};

int runMasks(const char *path) {
    FILE *f = fopen(path, "rb");
    int32_t nCases = 0;
    if (!f || fread(&nCases, sizeof(nCases), 1, f) != 1 || nCases < 0) {
        fprintf(stderr, "cannot read %s\n", path);
        return 2;
    }
    MaskCounts n;
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
                ++n.texels;
                // the candidate mask, and the order of the emission built on it
                Items want, got;
                Plain::texelCandidatePairs(nb, want);
                texelCandidatePairs(nb, got);
                unsigned wantMask = 0;
                for (int b : want.kj)
                    wantMask |= 1u<<b;
                const unsigned mask = texelCandidateMask(nb);
                n.badMask += mask != wantMask;
                // the spelling behind the kernel's vote (min3 / max3 in the Bernstein test): the same mask wherever the vote passes
                if (votePasses(sdf, x, yn))
                    ++n.voteTexels, n.badVoteMask += texelCandidateMask<true>(nb) != wantMask;
                else
                    n.differOutsideVote += texelCandidateMask<true>(nb) != wantMask;
                n.badBits += (mask&~(unsigned) EC_FIND_MASK) != 0;
                n.badOrder += want.kj != got.kj;
                n.survivors += (long) want.kj.size();
                n.fullTexels += want.kj.size() >= 12, n.emptyTexels += want.kj.empty();
                for (int b : want.kj)
                    ++n.tests[b];
                for (int cfg = 0; cfg < 12; ++cfg) {
                    const Config &cf = CONFIGS[cfg < 10 ? cfg : 0];
                    EcParams p;
                    p.t = t;
                    if (cfg >= 10)
                        p.t.sx *= STRETCH[cfg-10][0], p.t.sy *= STRETCH[cfg-10][1], p.t.mapScale *= 2.5;
                    p.minDeviationRatio = c.ratio, p.minImproveRatio = 1.11111111111111111;
                    p.mode = cf.mode, p.distanceCheck = cf.check, p.overlap = 0, p.stageLimit = 0;
                    ecDerive(p);
                    // the protect mask
                    ProtectItems wantP, gotP;
                    Plain::texelProtectPairs(nb, p, wantP);
                    texelProtectPairs(nb, p, gotP);
                    unsigned wantPMask = 0;
                    for (int m : wantP.m)
                        wantPMask |= 1u<<m, ++n.protectBits[m];
                    ++n.protectComparisons;
                    n.badProtect += texelProtectMask(nb, p) != wantPMask;
                    n.badProtectOrder += wantP.m != gotP.m;
                    n.protectPairs += (long) wantP.m.size();
                    if (cfg >= 10)
                        continue;
                    // the host walk's two stages against a walk over the plain items
                    VecSink wantS, gotS;
                    int wv = 0;
                    for (int b : want.kj) {
                        const int k = b>>2, dx = ecNeighbourDx(k), dy = ecNeighbourDy(k);
                        wv |= evaluatePair(nb.v[1][1], nb.v[dy+1][dx+1], nb.v[1][dx+1], nb.v[dy+1][1], p, cf.p1, 0, k, b&3, wantS, cf.order);
                    }
                    const int gv = texelFindFast(nb, p, cf.p1, 0, gotS, cf.order);
                    ++n.findComparisons;
                    n.badFind += !(wv == gv && wantS.v == gotS.v);
                    n.candidates += (long) wantS.v.size();
                    for (int b = 0; b < 4; ++b)
                        n.verdictBits[b] += (wv>>b)&1;
                }
            }
    }
    fclose(f);
    printf("{\"vote_texels\": %ld, \"bad_vote_mask\": %ld, \"differ_outside_vote\": %ld,\n ", n.voteTexels, n.badVoteMask, n.differOutsideVote);
    printf("\"cases\": %d, \"texels\": %ld, \"bad_mask\": %ld, \"bad_bits\": %ld, \"bad_order\": %ld, \"survivors\": %ld, \"full_texels\": %ld, \"empty_texels\": %ld,\n \"tests\": [",
           (int) nCases, n.texels, n.badMask, n.badBits, n.badOrder, n.survivors, n.fullTexels, n.emptyTexels);
    for (int b = 0; b < 32; ++b)
        printf("%ld%s", n.tests[b], b < 31 ? ", " : "],\n");
    printf(" \"protect_comparisons\": %ld, \"bad_protect\": %ld, \"bad_protect_order\": %ld, \"protect_pairs\": %ld, \"protect_bits\": [", n.protectComparisons, n.badProtect,
           n.badProtectOrder, n.protectPairs);
    for (int m = 0; m < 9; ++m)
        printf("%ld%s", n.protectBits[m], m < 8 ? ", " : "],\n");
    printf(" \"find_comparisons\": %ld, \"bad_find\": %ld, \"candidates\": %ld, \"verdict_bits\": [%ld, %ld, %ld, %ld]}\n", n.findComparisons, n.badFind, n.candidates,
           n.verdictBits[0], n.verdictBits[1], n.verdictBits[2], n.verdictBits[3]);
    return n.badMask || n.badVoteMask || n.badBits || n.badOrder || n.badProtect || n.badProtectOrder || n.badFind ? 1 : 0;
}

// ---- the append

const int LANES = 64;
const unsigned short UNWRITTEN = 0xffff;                  // no item: an item has 11 bits

// What the device does with a prefix sum, in whatever order the lanes come: a running count per part of the queue, the second part behind the first.
struct Reserve {
    int first, others;
    void operator()(int nFirst, int nOthers, int &atFirst, int &atOthers) { atFirst = first, atOthers = others, first += nFirst, others += nOthers; }
};

struct AppendCounts { long rounds, items, bad, fullRounds; };

// One tile's append of `masks` (lane l reserves at turn order[l]) into a queue of CAP slots with a guard slot of as many on either side.
template <unsigned VALID, int TESTS, unsigned FIRST>
void appendRound(const unsigned *masks, const int *order, AppendCounts &n) {
    const int CAP = LANES*TESTS;
    std::vector<unsigned short> mem(3*CAP, UNWRITTEN);
    unsigned short *queue = mem.data()+CAP;
    int expected = 0, expectedFirst = 0;
    for (int lane = 0; lane < LANES; ++lane)
        expectedFirst += __builtin_popcount(masks[lane]&VALID&FIRST);
    Reserve reserve = { 0, expectedFirst };
    int written = 0;
    for (int turn = 0; turn < LANES; ++turn) {
        const int lane = order[turn];
        written += ecAppendItems<VALID, TESTS, FIRST>(queue, masks[lane], lane, reserve);
    }
    std::vector<unsigned short> want;
    for (int lane = 0; lane < LANES; ++lane)
        for (int b = 0; b < 32; ++b)
            if ((masks[lane]&VALID)&(1u<<b))
                want.push_back((unsigned short) (lane|b<<6)), ++expected;
    const int count = reserve.others;
    bool ok = count == expected && written == expected && count <= CAP && reserve.first == expectedFirst;
    for (int i = 0; ok && i < expected; ++i)                 // the tests of FIRST ahead of the others
        ok = (((FIRST>>ecItemBit(queue[i]))&1u) != 0) == (i < expectedFirst);
    for (int i = 0; i < 3*CAP; ++i) {
        const bool inside = i >= CAP && i < CAP+expected;
        ok = ok && (mem[i] != UNWRITTEN) == inside;         // every slot below the count written (once: the multiset below), nothing else touched
    }
    std::vector<unsigned short> got(queue, queue+std::min(expected, CAP));
    std::sort(got.begin(), got.end()), std::sort(want.begin(), want.end());
    ok = ok && got == want;
    for (size_t i = 0; ok && i < got.size(); ++i)            // and every item decodes to its lane and test
        ok = (got[i]&63) < LANES && ((masks[got[i]&63]&VALID)>>ecItemBit(got[i]))&1u;
    ++n.rounds, n.items += expected, n.bad += !ok, n.fullRounds += expected == CAP;
}

int runAppend(uint64_t seed, int rounds) {
    AppendCounts find = { 0, 0, 0, 0 }, protect = { 0, 0, 0, 0 }, stray = { 0, 0, 0, 0 };
    unsigned masks[LANES];
    int order[LANES];
    for (int l = 0; l < LANES; ++l)
        order[l] = l;
    uint64_t s = seed*0x9e3779b97f4a7c15ull+1;
    const auto next = [&]() { s ^= s<<13, s ^= s>>7, s ^= s<<17; return (uint32_t) (s>>16); };
    // all masks zero
    memset(masks, 0, sizeof(masks));
    appendRound<EC_FIND_MASK, EC_FIND_TESTS, EC_FIND_LINEAR>(masks, order, find), appendRound<EC_PROTECT_MASK, EC_PROTECT_TESTS, EC_PROTECT_MASK>(masks, order, protect);
    // one lane only: each lane in turn, with every test and with one
    for (int l = 0; l < LANES; ++l) {
        memset(masks, 0, sizeof(masks));
        masks[l] = EC_FIND_MASK;
        appendRound<EC_FIND_MASK, EC_FIND_TESTS, EC_FIND_LINEAR>(masks, order, find);
        masks[l] = 1u<<(4*(l&7)+l%3);
        appendRound<EC_FIND_MASK, EC_FIND_TESTS, EC_FIND_LINEAR>(masks, order, find);
        masks[l] = EC_PROTECT_MASK;
        appendRound<EC_PROTECT_MASK, EC_PROTECT_TESTS, EC_PROTECT_MASK>(masks, order, protect);
    }
    // every test of every lane: the queue is full to its last slot
    for (int l = 0; l < LANES; ++l)
        masks[l] = EC_FIND_MASK;
    appendRound<EC_FIND_MASK, EC_FIND_TESTS, EC_FIND_LINEAR>(masks, order, find);
    for (int l = 0; l < LANES; ++l)
        masks[l] = EC_PROTECT_MASK;
    appendRound<EC_PROTECT_MASK, EC_PROTECT_TESTS, EC_PROTECT_MASK>(masks, order, protect);
    // a wrong mask (bits that are no test, all 32 set): only the tests are written, the queue does not overflow
    for (int l = 0; l < LANES; ++l)
        masks[l] = 0xffffffffu;
    appendRound<EC_FIND_MASK, EC_FIND_TESTS, EC_FIND_LINEAR>(masks, order, stray), appendRound<EC_PROTECT_MASK, EC_PROTECT_TESTS, EC_PROTECT_MASK>(masks, order, stray);
    // seeded random masks of three densities, lanes reserving in a seeded order
    for (int r = 0; r < rounds; ++r) {
        for (int l = LANES-1; l > 0; --l)
            std::swap(order[l], order[next()%(unsigned) (l+1)]);
        for (int l = 0; l < LANES; ++l) {
            const uint32_t a = next(), b = next();
            masks[l] = r%3 == 0 ? a : r%3 == 1 ? a&b : ((a|b)&((next()&3) ? ~0u : 0u));
        }
        appendRound<EC_FIND_MASK, EC_FIND_TESTS, EC_FIND_LINEAR>(masks, order, find), appendRound<EC_PROTECT_MASK, EC_PROTECT_TESTS, EC_PROTECT_MASK>(masks, order, protect);
        if (r%8 == 0)
            appendRound<EC_FIND_MASK, EC_FIND_TESTS, EC_FIND_LINEAR>(masks, order, stray);
    }
    printf("{\"find\": {\"rounds\": %ld, \"items\": %ld, \"bad\": %ld, \"full_rounds\": %ld},\n \"protect\": {\"rounds\": %ld, \"items\": %ld, \"bad\": %ld, \"full_rounds\": %ld},\n"
           " \"stray\": {\"rounds\": %ld, \"items\": %ld, \"bad\": %ld, \"full_rounds\": %ld}, \"find_capacity\": %d, \"protect_capacity\": %d}\n",
           find.rounds, find.items, find.bad, find.fullRounds, protect.rounds, protect.items, protect.bad, protect.fullRounds,
           stray.rounds, stray.items, stray.bad, stray.fullRounds, LANES*EC_FIND_TESTS, LANES*EC_PROTECT_TESTS);
    return find.bad || protect.bad || stray.bad ? 1 : 0;
}

}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "masks"))
        return runMasks(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "append"))
        return runAppend(strtoull(argv[2], NULL, 10), atoi(argv[3]));
    fprintf(stderr, "usage: %s masks CASES | append SEED ROUNDS\n", argv[0]);
    return 2;
}
