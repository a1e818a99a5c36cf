// TEST TOOLING ONLY -- the error-correction sweep of msdf_ec_fast.hpp (ecTexelFast: the host walk of k_ec_fast, in its lazy and its eager order) compiled for
// the host with g++ and checked texel by texel against the per-texel pipeline of msdf_ec.hpp (ecTexelStencil), for tests/test_ec_lazy_host.py and
// tests/test_gpu_ec_lazy.py. A stand-alone program: it reads pre-correction fields from a file, prints one JSON object and returns 1 on any mismatch, so
// that it can also be built with -fsanitize=address,undefined and run as it is. Never loaded by the msdfgen_amd package.
//
//   ec_lazy_host CASES            CASES: int32 n, then per case
//                                   int32 w, h, flip, group, nC, nE | double xf[6] (sx, sy, tx, ty, mapScale, mapTranslate) | int32 co[nC+1]
//                                   | double points[nE][8] | uint8 types[nE] | uint8 colors[nE] | float field[h][w][3] (rows in memory order)
//
// Every case runs under all Mode x DistanceCheckMode combinations. Per texel:
//   * stencil byte of the lazy walk and of the eager walk, after their deferred candidates were judged (ecEvaluateCandidate), == ecTexelStencil;
//   * raw byte (EC_DEFER included) and the deferred-candidate set (t, dx, dy) of the lazy walk == those of the eager walk;
//   * where the lazy order applies: "the first visit asks for the texel's protection" (EC_V_COND without EC_V_ERROR) == "the oracle's base pass finds an
//     error iff the texel is unprotected" (texelHasError with protectedFlag false / true).
// Counted per group of cases (so that a test can show it is not vacuous), in the lazy configuration, from the ORACLE's functions: conditional texels protected
// by an edge pair / by a corner / left unprotected; from the first visit's verdict (there is no oracle for it): unconditional ERROR with a conditional bit,
// texels with a held-back candidate, and those of them that stay unprotected. And per 8x8 tile, as k_ec_fast would queue them: the protectEdges pairs of the eager and of the lazy order.
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

struct Case {
    int w, h, flip, group, nC, nE;
    double xf[6];
    std::vector<int32_t> co;
    std::vector<double> points;
    std::vector<uint8_t> types, colors;
    std::vector<float> field;
    std::vector<EdgeRec> recs;
    std::vector<int8_t> windings;
};

template <class T>
bool readN(FILE *f, T *dst, size_t n) { return n == 0 || fread(dst, sizeof(T), n, f) == n; }

bool readCase(FILE *f, Case &c) {
    int32_t head[6];
    if (!readN(f, head, 6))
        return false;
    c.w = head[0], c.h = head[1], c.flip = head[2], c.group = head[3], c.nC = head[4], c.nE = head[5];
    if (c.w < 1 || c.h < 1 || c.w > 4096 || c.h > 4096 || c.nC < 0 || c.nE < 0 || c.nC > (1<<20) || c.nE > (1<<20) || c.group < 0 || c.group > 7)
        return false;
    c.co.assign((size_t) c.nC+1, 0);
    c.points.assign((size_t) 8*(c.nE+1), 0.);
    c.types.assign((size_t) c.nE+1, 1);
    c.colors.assign((size_t) c.nE+1, 7);
    c.field.assign((size_t) c.w*c.h*3, 0.f);
    if (!(readN(f, c.xf, 6) && readN(f, c.co.data(), (size_t) c.nC+1) && readN(f, c.points.data(), (size_t) 8*c.nE) && readN(f, c.types.data(), (size_t) c.nE)
          && readN(f, c.colors.data(), (size_t) c.nE) && readN(f, c.field.data(), c.field.size())))
        return false;
    if (c.co[0] != 0 || c.co[c.nC] != c.nE)
        return false;
    for (int k = 0; k < c.nC; ++k)
        if (c.co[k] > c.co[k+1])
            return false;
    // the records and windings as k_prep_records digests them (tests/hostemu does the same)
    c.recs.resize(c.nE > 0 ? c.nE : 1);
    c.windings.assign(c.nC > 0 ? c.nC : 1, 0);
    for (int slot = 0; slot < c.nE; ++slot) {
        int lo = 0, hi = c.nC-1;
        while (lo < hi) {
            const int mid = (lo+hi+1)>>1;
            if (c.co[mid] <= slot) lo = mid; else hi = mid-1;
        }
        prepRecord(c.recs.data(), slot, lo, c.co.data(), c.points.data(), c.types.data(), c.colors.data());
    }
    for (int k = 0; k < c.nC; ++k)
        c.windings[k] = (int8_t) contourWinding(k, c.co.data(), c.points.data(), c.types.data(), c.colors.data());
    return true;
}

struct HostQuery {
    const Case *c;
    double *res;
    double operator()(V2 q) const {
        double out[1];
        EdgesAll edges;
        edges.coff = c->co.data();
        shapeDistanceOverlap<2>(c->recs.data(), edges, c->windings.data(), c->nC, q, res, 1, out);
        return out[0];
    }
};

struct Cand {
    double t;
    int dx, dy;
    bool operator<(const Cand &o) const { return t != o.t ? t < o.t : dx != o.dx ? dx < o.dx : dy < o.dy; }
    bool operator==(const Cand &o) const { return memcmp(&t, &o.t, sizeof(t)) == 0 && dx == o.dx && dy == o.dy; }
};
struct VecSink {
    std::vector<Cand> v;
    void operator()(double t, int dx, int dy) { const Cand c = { t, dx, dy }; v.push_back(c); }
};
struct CountItems {
    long n;
    void operator()(int) { ++n; }
};

struct Kinds { long byEdge, byCorner, unprotected, errorAndConditional, held, heldUnprotected, texels; };
struct Tiles { long tiles, tilesWithLazyRound, needTexels, eagerItems, lazyItems, cornerTexels; };

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
    long texelsChecked = 0, badLazy = 0, badEager = 0, badRaw = 0, badCands = 0, badCond = 0, deferred = 0;
    long badByConfig[4][3] = { { 0 } };
    Kinds kinds[8];
    Tiles tiles[8];
    memset(kinds, 0, sizeof(kinds));
    memset(tiles, 0, sizeof(tiles));
    for (int i = 0; i < n; ++i) {
        Case c;
        if (!readCase(f, c)) {
            fprintf(stderr, "case %d of %s is malformed\n", i, argv[1]);
            return 2;
        }
        std::vector<double> res((size_t) (c.nC+1)*5);
        const HostQuery q = { &c, res.data() };
        SdfView sdf;
        sdf.px = c.field.data(), sdf.w = c.w, sdf.h = c.h, sdf.N = 3, sdf.flip = c.flip;
        for (int mode = EC_MODE_INDISCRIMINATE; mode <= EC_MODE_EDGE_ONLY; ++mode)
            for (int dist = EC_DO_NOT_CHECK; dist <= EC_ALWAYS_CHECK; ++dist) {
                EcParams p;
                const Xform t = { c.xf[0], c.xf[1], c.xf[2], c.xf[3], c.xf[4], c.xf[5] };
                p.t = t;
                p.minDeviationRatio = 1.11111111111111111, p.minImproveRatio = 1.11111111111111111;
                p.mode = mode, p.distanceCheck = dist, p.overlap = 1, p.stageLimit = 0;
                ecDerive(p);
                std::vector<int> corners;                                     // k_ec_params: protectCorners' texel pairs
                if (mode == EC_MODE_EDGE_PRIORITY)
                    for (int e = 0; e < c.nE; ++e)
                        if (c.recs[e].flags&REC_CORNER) {
                            const V2 pp = project(t, ld(c.recs[e].p0));
                            corners.push_back((int) floor(pp.x-.5));
                            corners.push_back((int) floor(pp.y-.5));
                        }
                const int nCorners = (int) corners.size()/2;
                const bool lazy = ecLazyProtect(p);
                std::vector<unsigned char> needMap((size_t) c.w*c.h, 0);
                for (int yn = 0; yn < c.h; ++yn)
                    for (int x = 0; x < c.w; ++x) {
                        const int ys = c.flip ? c.h-1-yn : yn;
                        const int want = ecTexelStencil(sdf, p, c.recs.data(), c.nE, x, yn, &q);
                        VecSink lazySink, eagerSink;
                        const int rawLazy = ecTexelFast(sdf, p, corners.data(), nCorners, x, yn, lazySink);
                        const int rawEager = ecTexelFast(sdf, p, corners.data(), nCorners, x, yn, eagerSink, false);
                        int gotLazy = rawLazy&~EC_DEFER, gotEager = rawEager&~EC_DEFER;
                        for (size_t k = 0; k < lazySink.v.size(); ++k)
                            if (ecEvaluateCandidate(sdf, p, x, ys, lazySink.v[k].t, lazySink.v[k].dx, lazySink.v[k].dy, q))
                                gotLazy |= EC_ERROR;
                        for (size_t k = 0; k < eagerSink.v.size(); ++k)
                            if (ecEvaluateCandidate(sdf, p, x, ys, eagerSink.v[k].t, eagerSink.v[k].dx, eagerSink.v[k].dy, q))
                                gotEager |= EC_ERROR;
                        deferred += (long) lazySink.v.size();
                        std::sort(lazySink.v.begin(), lazySink.v.end());
                        std::sort(eagerSink.v.begin(), eagerSink.v.end());
                        const bool sameCands = lazySink.v.size() == eagerSink.v.size() && std::equal(lazySink.v.begin(), lazySink.v.end(), eagerSink.v.begin());
                        ++texelsChecked;
                        badLazy += gotLazy != want, badEager += gotEager != want, badRaw += rawLazy != rawEager, badCands += !sameCands;
                        badByConfig[mode][dist] += (gotLazy != want)+(gotEager != want)+(rawLazy != rawEager)+!sameCands;
                        if (!lazy)
                            continue;
                        // the first visit's verdict against the oracle's base pass with the texel protected / unprotected
                        Neighbourhood nb;
                        loadNeighbourhood(nb, sdf, x, yn);
                        VecSink ignored;
                        const int verdict = texelFindFast(nb, p, true, c.flip, ignored, EC_ORDER_LAZY);
                        const bool errorProtected = texelHasError(sdf, p, x, yn, false, true, (const HostQuery *) 0);
                        const bool errorUnprotected = texelHasError(sdf, p, x, yn, false, false, (const HostQuery *) 0);
                        const bool conditional = errorUnprotected && !errorProtected;
                        badCond += conditional != (((verdict&EC_V_COND) && !(verdict&EC_V_ERROR)) != 0);
                        badCond += errorProtected != ((verdict&EC_V_ERROR) != 0);
                        const bool byCorner = protectedByCorners(c.recs.data(), c.nE, p.t, x, ys);
                        const bool byEdge = protectedByEdges(sdf, p, x, yn);
                        Kinds &k = kinds[c.group];
                        ++k.texels;
                        k.byCorner += conditional && byCorner;
                        k.byEdge += conditional && !byCorner && byEdge;
                        k.unprotected += conditional && !byCorner && !byEdge;
                        k.errorAndConditional += (verdict&EC_V_ERROR) && (verdict&EC_V_COND);
                        k.held += (verdict&EC_V_HELD) != 0;
                        k.heldUnprotected += (verdict&EC_V_HELD) && !byCorner && !byEdge;      // the eager order hands these candidates to nobody
                        // what k_ec_fast queues for this texel's protection in either order
                        Tiles &tl = tiles[c.group];
                        const bool need = ecNeedsProtection(verdict);
                        needMap[(size_t) yn*c.w+x] = need;
                        CountItems items = { 0 };
                        if (!byCorner)
                            texelProtectPairs(nb, p, items);
                        tl.cornerTexels += byCorner;
                        tl.eagerItems += items.n;
                        tl.needTexels += need;
                        tl.lazyItems += need ? items.n : 0;
                    }
                if (lazy)
                    for (int ty = 0; ty*8 < c.h; ++ty)
                        for (int tx = 0; tx*8 < c.w; ++tx) {
                            bool any = false;
                            for (int y = ty*8; y < ty*8+8 && y < c.h; ++y)
                                for (int x = tx*8; x < tx*8+8 && x < c.w; ++x)
                                    any = any || needMap[(size_t) y*c.w+x];
                            ++tiles[c.group].tiles;
                            tiles[c.group].tilesWithLazyRound += any;
                        }
            }
    }
    fclose(f);
    printf("{\"cases\": %d, \"texels_checked\": %ld, \"deferred_candidates\": %ld, \"bad_lazy_stencil\": %ld, \"bad_eager_stencil\": %ld, \"bad_raw_byte\": %ld, "
           "\"bad_candidate_set\": %ld, \"bad_conditional_bit\": %ld,\n \"bad_by_config\": [", (int) n, texelsChecked, deferred, badLazy, badEager, badRaw, badCands, badCond);
    for (int mode = 1; mode <= 3; ++mode)
        for (int dist = 0; dist <= 2; ++dist)
            printf("%s[%d, %d, %ld]", mode == 1 && dist == 0 ? "" : ", ", mode, dist, badByConfig[mode][dist]);
    printf("],\n \"groups\": [");
    for (int g = 0; g < 8; ++g)
        printf("%s{\"texels\": %ld, \"conditional_protected_by_edge\": %ld, \"conditional_protected_by_corner\": %ld, \"conditional_unprotected\": %ld, "
               "\"error_and_conditional\": %ld, \"held_back\": %ld, \"held_back_unprotected\": %ld, \"tiles\": %ld, \"tiles_with_lazy_round\": %ld, \"texels_resolved\": %ld, "
               "\"corner_texels\": %ld, \"eager_protect_items\": %ld, \"lazy_protect_items\": %ld}", g ? ",\n  " : "", kinds[g].texels, kinds[g].byEdge, kinds[g].byCorner,
               kinds[g].unprotected, kinds[g].errorAndConditional, kinds[g].held, kinds[g].heldUnprotected, tiles[g].tiles, tiles[g].tilesWithLazyRound, tiles[g].needTexels,
               tiles[g].cornerTexels, tiles[g].eagerItems, tiles[g].lazyItems);
    printf("]}\n");
    return badLazy || badEager || badRaw || badCands || badCond ? 1 : 0;
}
