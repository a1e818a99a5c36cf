// msdf_launchplan.hpp -- which kernels a batched generate call launches, planned on the host over plain integers: the LDS of a distance launch, the
// glyph classes and their streams, persistent or direct grids, the correction pass's query LDS and route, the sign pass's spans.
// Host code only (no HIP): msdf_capi.hip includes it and executes the plans, and tests/hostemu compiles it with the host compiler
// (tests/test_launch_plan_host.py).

#pragma once

#include <cstddef>

#include "../../include/msdfgen_hip.h"
#include "msdf_classplan.hpp"

namespace msdfhip {

// What the plans know of the kernels (msdf_kernels.hpp; msdf_capi.hip asserts that the two agree).
enum { PLAN_TILE = 8, PLAN_WAVE = 64, PLAN_QUAD = 4, PLAN_DISTANCE_WAVES_PER_SIMD = 4, PLAN_SIMPLE_WAVES_PER_SIMD = 5, PLAN_SIGN_ROWS = PLAN_TILE+2,
       PLAN_PB_SLOT_BYTES = 40 };
const size_t GRES_WORKSPACE_CAP = (size_t) 1<<30;   // bound of the global combiner scratch; larger launches are chunked

// The measurement / experiment knobs the launch paths read (msdf_capi.hip: Tuning, readTuning), at their defaults.
struct PlanTuning {
    size_t resLdsBudget = (size_t) 10*1024;   // MSDFHIP_RES_LDS_BUDGET      bytes of LDS per wavefront up to which the combiner scratch stays in LDS
    long persistentRounds = 8;        // MSDFHIP_PERSISTENT_ROUNDS   global-scratch launches of at least this many rounds run persistent; 0 = never
    bool serialClasses = false;       // MSDFHIP_SERIAL_CLASSES      glyph classes one after the other instead of on side streams
    int querySlotCap = 160, queryLpcContours = 24;   // MSDFHIP_QUERY_LDS "slotCap,lpcMaxContours"
    bool hasQueryLds = false;
    bool hasQueryPolicy = false;      // MSDFHIP_QUERY_POLICY        "edgeCost,maxEdges,minCount,wideMaxEdges,wideLoad[,wideMeanCount]"
    int qpEdgeCost = 150, qpMaxEdges = 48, qpMinCount = 0x7fffffff, qpWideMaxEdges = 128;
    float qpWideLoad = 4e8f, qpWideMeanCount = 24.f;
    size_t signCap = 192;             // MSDFHIP_SIGN_CAP            row-list capacity of the sign pass
    int queryStatic = 2;              // MSDFHIP_QUERY_STATIC        2: first ticket dealt, the others from eight counters; 0: k_ec_query draws its tickets from an atomic counter (rounds 2-5) instead of the static serpentine deal
    int queryGridSteps = 16;          // MSDFHIP_QUERY_GRID          grid form of the distance checks: edges a lane may walk per item (0 = off: the two older forms only)
    int queryBatch = 1;               // MSDFHIP_QUERY_BATCH         cooperative distance checks a wavefront of k_ec_query takes per ticket (default 1: more only lengthens the tail)
    // (1.33 since the round-6 refit of glyphCost: the new table prices the global-workspace class at 0.146 of the bench workload where round 3's said 0.195, and
    // the grid that finishes inside the pass is the one the old share gave -- x1.0 / 1.33 / 1.6 / 2.0: 5.22 / 5.00 / 5.04 / 5.03 ms per step, profiles/r06_ab_notes.md)
    double shareGridFactor = 1.33;    // MSDFHIP_SHARE_GRID          the global-scratch class's persistent grid = its share of the batch's cost x this factor of the slots (0: off)
    long persistentGrid = 0;          // MSDFHIP_PERSISTENT_GRID     workgroups of a persistent global-scratch launch (0: one per resident wavefront slot)
    long shortRounds = 4;             // MSDFHIP_SHORT_ROUNDS        LDS-class launches of fewer rounds of four-tile wavefronts take one tile per wavefront
    long smallLaunchTiles = 8192;     // MSDFHIP_SMALL_LAUNCH_TILES  launches of at most this many tiles take one tile per wavefront (latency-shaped form)
    int smallMaxEdges = 128;          // MSDFHIP_SMALL_MAX_EDGES     glyphs of the LDS-scratch class have at most this many edges (128)
    int ldsClassTpw = 4;              // MSDFHIP_LDS_CLASS_TPW       tiles per wavefront of the LDS-scratch class: 4 (default; 1 in short launches) or always 1
};

// What the plans read besides the batch.
struct PlanEnv {
    PlanTuning t;
    size_t ldsLimit;                  // bytes of LDS a workgroup may take (msdfhip_init reads it from the device)
    int cus;                          // compute units (4 SIMDs each): a W-waves-per-SIMD kernel has cus*4*W wavefronts resident at once
    size_t slots(int wavesPerSimd) const { return (size_t) cus*4u*(unsigned) wavesPerSimd; }
    int classTpw() const { return t.ldsClassTpw == 1 ? 1 : (int) PLAN_QUAD; }
};

struct GlyphCounts { int nGlyphs, maxContours, maxEdges; };     // of the glyphs a plan covers

inline int tilesOf(int w, int h) { return ((w+PLAN_TILE-1)/PLAN_TILE)*((h+PLAN_TILE-1)/PLAN_TILE); }

// LDS plan for a launch: bytes of dynamic LDS, the stride of the per-tile survivor lists, and where the combiner scratch lives.
// fits: bytes <= the device limit (else the call is refused as too complex: maxContours / listStride edges).
struct LdsPlan { size_t bytes; bool globalRes; size_t resBytes, ldsBudget, idxBytes; int listStride, maxContours; bool fits; };

// maxContours / maxEdges: of the glyphs this launch covers.
inline LdsPlan planLds(const PlanEnv &env, int nch, bool overlap, int maxContours, int maxEdges, int tilesPerWave = PLAN_QUAD) {
    LdsPlan plan;
    const size_t resBytes = overlap ? (size_t) maxContours*nch*PLAN_WAVE*sizeof(double) : 0;
    const size_t idxOne = tileListBytes(maxEdges, maxContours, false);   // survivor list + per-contour offsets of one tile
    const size_t idxBytes = (size_t) tilesPerWave*idxOne;        // the LDS-scratch variant culls a quad of tiles per wavefront (one in short launches)
    // The combiner scratch lives in LDS only while 16 wavefronts (4 per SIMD, the register-limited occupancy: MSDF_DISTANCE_WAVES_PER_SIMD) fit a CU's
    // 160 KB: beyond 10 KB per wavefront LDS would cap the occupancy (a 20-contour glyph set ran at 1.25 wavefronts/SIMD), so it moves to a
    // global workspace instead -- written and read once per contour with lane-consecutive addresses. (13 KB = 12 wavefronts until round 5.)
    plan.ldsBudget = env.t.resLdsBudget;                         // 10 KB unless MSDFHIP_RES_LDS_BUDGET says otherwise
    plan.resBytes = resBytes;
    plan.globalRes = overlap && resBytes+idxBytes > plan.ldsBudget;
    plan.idxBytes = idxBytes;
    plan.listStride = maxEdges, plan.maxContours = maxContours;
    plan.bytes = plan.globalRes ? tileListBytes(maxEdges, maxContours, true) : resBytes+idxBytes;     // the global-scratch variant takes one tile per wavefront
    plan.fits = plan.bytes <= env.ldsLimit;
    // (Staging the surviving records in LDS instead of reading them with scalar loads was measured slower and is gone.)
    return plan;
}
// `plan` for one tile per wavefront: one survivor list, scratch (if any) in global memory. The small launches (`single`) and the global-scratch
// class (`rest`, sized for the batch's largest glyph) take this form.
inline LdsPlan singleTileLds(LdsPlan plan) {
    plan.globalRes = true;
    plan.bytes = tileListBytes(plan.listStride, plan.maxContours, true);
    return plan;
}
// The one-contour class in its short form: the simple combiner, one tile per wavefront.
inline LdsPlan shortSimpleLds(const PlanEnv &env, int nch, int oneMaxE) {
    LdsPlan plan = planLds(env, nch, false, 1, oneMaxE, 1);
    if (plan.fits)
        plan.bytes = tileListBytes(oneMaxE, 1, true);
    return plan;
}

// Contours up to which a glyph's combiner scratch fits the per-wavefront LDS budget next to the lists of a smallMaxEdges glyph (the LDS class's bound).
inline int overlapClassLimit(const PlanEnv &env, int nch) {
    const size_t perContourLds = (size_t) nch*PLAN_WAVE*sizeof(double);
    int limitAll = 0;
    while ((size_t) (limitAll+1)*perContourLds+(size_t) env.classTpw()*tileListBytes(env.t.smallMaxEdges, limitAll+1, false) <= env.t.resLdsBudget)
        ++limitAll;
    return limitAll;
}

// How the distance pass of a batch at w x h takes its glyphs. hugeBatch: a glyph's survivor lists exceed a CU's LDS. smallLaunch: too few tiles to fill the
// device -- one tile per wavefront, combiner scratch (boundScratch: nch channels per contour, at most 64 MB) in the global workspace.
struct LaunchShape { bool hugeBatch, smallLaunch; };
inline LaunchShape launchShape(const PlanEnv &env, const GlyphCounts &b, int w, int h, int nch, bool boundScratch) {
    const size_t tilesAll = (size_t) b.nGlyphs*(size_t) tilesOf(w, h);
    const size_t gresAll = tilesAll*(size_t) b.maxContours*nch*PLAN_WAVE*sizeof(double);
    LaunchShape l;
    l.hugeBatch = tileListBytes(b.maxEdges, b.maxContours, true) > env.ldsLimit;
    l.smallLaunch = !l.hugeBatch && tilesAll <= (size_t) env.t.smallLaunchTiles && (!boundScratch || gresAll <= ((size_t) 64<<20));
    return l;
}

// The contour limit of the class list (msdf_classplan.hpp) the distance pass will launch from; 0: it needs none (one glyph, or the simple combiner on
// glyphs that all fit the culled kernels).
inline int classListLimit(const PlanEnv &env, const GlyphCounts &b, int w, int h, int nch, bool overlap) {
    const bool huge = launchShape(env, b, w, h, nch, overlap).hugeBatch;
    if (b.nGlyphs <= 1 || !(huge || (overlap && b.maxContours > 1)))
        return 0;
    const int limit = overlapClassLimit(env, nch);
    return limit < 1 ? 1 : limit;
}
// The same for the host-output pipeline, which builds a chunk's list AHEAD of the chunk's turn on the device: only where the classes will run -- a batch
// with an oversized glyph, and a launch of few tiles whatever its combiner scratch (beyond 64 MB of it the call takes the classes, too), build theirs in
// the call, as before.
inline int classListLimitAhead(const PlanEnv &env, const GlyphCounts &b, int w, int h, int nch, bool overlap) {
    const LaunchShape shape = launchShape(env, b, w, h, nch, false);
    return shape.hugeBatch || shape.smallLaunch ? 0 : classListLimit(env, b, w, h, nch, overlap);
}

// Workgroups of a k_distance launch: a wavefront each, tpw tiles of one glyph per wavefront (decodeBlock, msdf_kernels.hpp).
inline size_t distanceBlocks(int nGlyphs, int w, int h, int tpw) { return (size_t) nGlyphs*(size_t) ((tilesOf(w, h)+tpw-1)/tpw); }

// The grid of a launch of `blocks` workgroups whose combiner scratch, resBytes each, lies in the global workspace (0: none -- one direct launch).
struct GridPlan {
    bool persistent;                  // one workgroup per slot draws tiles from a queue and keeps its slice of the workspace
    size_t chunk;                     // workgroups per launch: the grid of the persistent launch; else the launch goes in pieces of this many
    size_t gresBytes;                 // the workspace they need
};
inline GridPlan planDistanceGrid(size_t blocks, size_t resBytes, size_t slots, size_t shareGrid, const PlanEnv &env) {
    GridPlan g = { false, blocks, 0 };
    if (!resBytes)
        return g;
    // More items than resident wavefront slots: a PERSISTENT launch -- one workgroup per slot draws tiles from a queue and keeps
    // its slice of the workspace (3 072 x 30 KB = 92 MB for 20-contour glyphs: Infinity-Cache resident; as one slice per tile the
    // same launch streamed 9 GB through HBM and had to be cut into chunks of 1 GB of workspace).
    // (Only for launches of many rounds: a persistent workgroup never yields its slot, so next to the other glyph classes' launches
    // it freezes the split of the device between them -- measured 2 % slower than the direct mapping at 5 rounds, 12 % faster at 96.)
    const size_t minRounds = (size_t) env.t.persistentRounds;    // 8; MSDFHIP_PERSISTENT_ROUNDS, 0 = never
    // shareGrid (round 4): a class that is a small share of a batch's work runs persistent on that share of the slots -- the launch is no
    // longer (the other classes fill the device, it finishes inside the pass either way: 3.74 vs 3.77 ms) and its few workspace slices, rewritten by
    // one tile after the other, stay in the L2s instead of being written once per tile: HBM bytes of the pass 922 -> 634 MB on the bench workload
    // (2.2x -> 1.5x algorithmic; tools/persistent_grid_traffic.sh)
    const bool byShare = shareGrid > 0 && shareGrid < slots && blocks > shareGrid;
    if (((minRounds && blocks >= minRounds*slots) || byShare) && blocks < 0xffffffffull-8u*slots) {
        g.persistent = true;
        g.chunk = byShare ? shareGrid : slots;
        if (env.t.persistentGrid > 0 && (size_t) env.t.persistentGrid < g.chunk)
            g.chunk = (size_t) env.t.persistentGrid;             // (A/B: a fixed grid)
    } else {
        g.chunk = GRES_WORKSPACE_CAP/resBytes;
        if (g.chunk < 256)
            g.chunk = 256;
        if (g.chunk > blocks)
            g.chunk = blocks;
    }
    g.gresBytes = g.chunk*resBytes;
    return g;
}

enum { PLAN_STREAM_CALLER = 0, PLAN_STREAM_SIDE0 = 1, PLAN_STREAM_SIDE1 = 2 };   // the caller's stream, or one of the batch's two side streams

// One launch of k_distance<SEL, overlap, gres, tpw>.
struct DistanceLaunch {
    bool overlap, gres;
    int tpw;                          // tiles per wavefront
    LdsPlan lds;
    bool mapped;                      // the glyphs [offset, offset+count) of the class list; else the whole batch in its own order
    int offset, count;
    int stream;                       // PLAN_STREAM_*
    size_t shareGrid;                 // planDistanceGrid
    int route;                        // the route counter it bumps (MSDFHIP_ROUTE_*; see routeOf)
};
// (the global-scratch class counts as direct or persistent by what its grid came to)
inline int routeOf(const DistanceLaunch &l, const GridPlan &g) { return l.route == MSDFHIP_ROUTE_DIST_GLOBAL_DIRECT && g.persistent ? MSDFHIP_ROUTE_DIST_GLOBAL_PERSISTENT : l.route; }
inline GridPlan gridOf(const DistanceLaunch &l, int w, int h, const PlanEnv &env) {
    return planDistanceGrid(distanceBlocks(l.count, w, h, l.tpw), l.gres && l.overlap ? l.lds.resBytes : 0, env.slots(PLAN_DISTANCE_WAVES_PER_SIMD), l.shareGrid, env);
}

// The distance pass of one generate call: the culled launches in issue order, then (after their streams have joined) the list-free one.
struct DistancePlan {
    bool tooComplex;                  // `refused` does not fit the device's LDS: no launch
    LdsPlan refused;
    DistanceLaunch launches[4];
    int nLaunches;
    bool concurrent;                  // the classes run on the caller's stream and the side streams at once, forked and joined by events
    bool ecAhead;                     // k_ec_params of the coming correction pass rides ahead of the one-contour class on its side stream
    bool unculled, unculledOverlap;   // a list-free launch (k_distance_unculled) ...
    bool unculledMapped;              // ... of [unculledOffset, +unculledCount) of the class list; else of the whole batch
    int unculledOffset, unculledCount;
    bool unculledAfterJoin;           // it shares the batch's workspace with the global-scratch class: only once the side streams have joined

    void add(bool overlap, bool gres, int tpw, const LdsPlan &lds, int route, int count, bool mapped = false, int offset = 0, int stream = PLAN_STREAM_CALLER,
             size_t shareGrid = 0) {
        const DistanceLaunch l = { overlap, gres, tpw, lds, mapped, offset, count, stream, shareGrid, route };
        launches[nLaunches++] = l;
    }
    bool refuse(const LdsPlan &lds) { tooComplex = !lds.fits, refused = lds; return tooComplex; }
};

// classes: the ClassPlan built for classListLimit() (not read when that is 0). serialBatch: the batch wants its classes one after the other (chunks of
// the host-output pipeline: they overlap with each other instead). wantEcAhead: a correction pass follows whose k_ec_params may run next to this one.
inline DistancePlan planDistance(const PlanEnv &env, const GlyphCounts &b, int w, int h, int nch, bool overlap, bool serialBatch, bool wantEcAhead,
                                 const ClassPlan &classes) {
    DistancePlan p = DistancePlan();
    // A glyph whose survivor lists exceed a CU's LDS takes the list-free kernel (the reference cannot fail on a large shape; neither may this) --
    // alone: in a batch, the OTHER glyphs keep the culled kernels (planClasses puts the oversized ones last in the class list; maxE / maxC below
    // are the maxima of the rest). Round 3 sent the whole batch through the list-free kernel with it.
    const LaunchShape shape = launchShape(env, b, w, h, nch, overlap);
    p.unculledOverlap = overlap && b.maxContours > 1;
    p.unculledCount = b.nGlyphs;
    if (shape.hugeBatch && b.nGlyphs == 1) {
        p.unculled = true;
        return p;
    }
    int maxE = b.maxEdges, maxC = b.maxContours, nHuge = 0;
    const int limit = overlapClassLimit(env, nch);
    if (shape.hugeBatch) {
        nHuge = classes.nHuge;
        maxE = classes.oneMaxE > classes.smallMaxE ? classes.oneMaxE : classes.smallMaxE, maxE = classes.restMaxE > maxE ? classes.restMaxE : maxE;
        maxC = classes.smallMaxC > classes.restMaxC ? classes.smallMaxC : classes.restMaxC, maxC = classes.nOne > 0 && maxC < 1 ? 1 : maxC;
        // (the lists are sized by the two maxima, which may come from different glyphs: if even those do not fit, or nothing is left, the whole batch goes list-free)
        if (nHuge == b.nGlyphs || tileListBytes(maxE, maxC, true) > env.ldsLimit) {
            p.unculled = true;
            return p;
        }
    }
    const int nCulled = b.nGlyphs-nHuge;
    if (nHuge > 0)                                               // the oversized glyphs after the others: they share the batch's workspace
        p.unculled = p.unculledMapped = true, p.unculledOffset = nCulled, p.unculledCount = nHuge;
    LdsPlan plan = planLds(env, nch, overlap, maxC, maxE);
    if (p.refuse(plan))
        return p;
    // A launch too small to fill the device (a single-shape call, a micro-batched group) is latency bound: it takes one tile per
    // wavefront instead of four -- four times the wavefronts, a quarter of the serial work each -- with the combiner scratch in the
    // global workspace (single 64x64 glyph: 19 -> 8 us simple, ~100 -> ~30 us overlapping combiner).
    const LdsPlan single = singleTileLds(plan);
    if (!overlap || maxC <= 1) {
        if (shape.smallLaunch) {
            p.add(false, true, 1, single, MSDFHIP_ROUTE_DIST_SMALL_SIMPLE, b.nGlyphs);
            return p;
        }
        if (overlap && p.refuse(plan = planLds(env, nch, false, maxC, maxE)))
            return p;
        if (!shape.hugeBatch)
            p.add(false, false, PLAN_QUAD, plan, MSDFHIP_ROUTE_DIST_FULL_SIMPLE, b.nGlyphs);
        else if (nCulled > 0)
            p.add(false, false, PLAN_QUAD, plan, MSDFHIP_ROUTE_DIST_FULL_SIMPLE, nCulled, true, 0);
        return p;
    }
    if (b.nGlyphs == 1) {                                        // the class is known, no index map
        if (shape.smallLaunch)
            p.add(true, true, 1, single, MSDFHIP_ROUTE_DIST_SMALL_OVERLAP, 1);
        else if (maxC <= limit && maxE <= env.t.smallMaxEdges && !plan.globalRes)
            p.add(true, false, PLAN_QUAD, plan, MSDFHIP_ROUTE_DIST_LDS_QUAD, 1);
        else
            p.add(true, true, 1, single, MSDFHIP_ROUTE_DIST_GLOBAL_DIRECT, 1);
        return p;
    }
    const int nOne = classes.nOne, nSmall = classes.nSmall, nRest = nCulled-nOne-nSmall;
    if (shape.smallLaunch) {
        if (nOne > 0)
            p.add(false, true, 1, single, MSDFHIP_ROUTE_DIST_SMALL_SIMPLE, nOne, true, 0);
        if (b.nGlyphs > nOne)
            p.add(true, true, 1, single, MSDFHIP_ROUTE_DIST_SMALL_OVERLAP, b.nGlyphs-nOne, true, nOne);
        return p;
    }
    // The classes are disjoint sets of glyphs: their launches run CONCURRENTLY (the long LDS-class launch on the caller's stream, the other
    // two on the batch's side streams, forked and joined by events), so that the tail of one fills with the wavefronts of the others --
    // two processes sharing the GPU had measured 12 % more throughput than one.
    const int nClasses = (nOne > 0)+(nSmall > 0)+(nRest > 0);
    p.concurrent = nClasses > 1 && !env.t.serialClasses && !serialBatch;
    const int sRest = p.concurrent && nRest > 0 && nSmall > 0 ? PLAN_STREAM_SIDE0 : PLAN_STREAM_CALLER;
    const int sOne = p.concurrent && nOne > 0 && (nSmall > 0 || nRest > 0) ? PLAN_STREAM_SIDE1 : PLAN_STREAM_CALLER;
    // the correction pass's per-glyph constants (k_ec_params: 17 us + a dependent launch behind the join, round 6 timeline) depend on nothing the distance
    // pass writes: ahead of the one-contour class on its side stream
    p.ecAhead = wantEcAhead && sOne != PLAN_STREAM_CALLER;
    p.unculledAfterJoin = p.unculled && p.concurrent;
    const int tiles = tilesOf(w, h);
    if (nRest > 0) {                                             // first: few, heavy glyphs -- the longest tail
        size_t shareGrid = 0;
        if (env.t.shareGridFactor > 0 && p.concurrent) {
            shareGrid = (size_t) ((double) env.slots(PLAN_DISTANCE_WAVES_PER_SIMD)*classes.restShare*env.t.shareGridFactor);
            shareGrid = shareGrid < 256 ? 256 : shareGrid;
        }
        p.add(true, true, 1, single, MSDFHIP_ROUTE_DIST_GLOBAL_DIRECT, nRest, true, nOne+nSmall, sRest, shareGrid);
    }
    if (nSmall > 0) {
        // A launch of few rounds of wavefronts (a shard of an atlas: BASELINE config 4 over 8 GPUs leaves 1 024 glyphs per device) ends when its
        // last wavefronts do, and a wavefront of four tiles is four times as long: below shortRounds rounds the class takes one tile per wavefront.
        const bool shortLaunch = env.classTpw() == 1 ||
                                 (size_t) nSmall*(size_t) ((tiles+PLAN_QUAD-1)/PLAN_QUAD) < (size_t) env.t.shortRounds*env.slots(PLAN_DISTANCE_WAVES_PER_SIMD);
        const LdsPlan small = planLds(env, nch, true, classes.smallMaxC, classes.smallMaxE, shortLaunch ? 1 : (int) PLAN_QUAD);
        if (p.refuse(small))
            return p;
        p.add(true, false, shortLaunch ? 1 : (int) PLAN_QUAD, small, shortLaunch ? MSDFHIP_ROUTE_DIST_LDS_SINGLE : MSDFHIP_ROUTE_DIST_LDS_QUAD, nSmall, true, nOne);
    }
    if (nOne > 0) {
        const bool shortLaunch = (size_t) nOne*(size_t) ((tiles+PLAN_QUAD-1)/PLAN_QUAD) < (size_t) env.t.shortRounds*env.slots(PLAN_SIMPLE_WAVES_PER_SIMD);   // as for the LDS class above
        const LdsPlan simple = shortLaunch ? shortSimpleLds(env, nch, classes.oneMaxE) : planLds(env, nch, false, 1, classes.oneMaxE);
        if (p.refuse(simple))
            return p;
        p.add(false, shortLaunch, shortLaunch ? 1 : (int) PLAN_QUAD, simple, shortLaunch ? MSDFHIP_ROUTE_DIST_ONE_SINGLE : MSDFHIP_ROUTE_DIST_ONE_QUAD, nOne, true, 0, sOne);
    }
    return p;
}

// The error-correction pass (k_ec_params, k_ec_fast, k_ec_scan, k_ec_query, k_ec_slow) of nGlyphs bitmaps of w x h texels with n channels.
enum { EC_ROUTE_NORMAL = 0, EC_ROUTE_STAGE_SNAPSHOT, EC_ROUTE_SLOW_ALL, EC_ROUTE_TOO_COMPLEX };
struct EcPlan {
    bool tooManyTexels;               // beyond the pass's 32-bit texel index: refused
    size_t allTexels;
    bool gres;                        // the PSDF distance checks' combiner scratch in the global workspace (k_ec_slow<.., GRES>)
    size_t resBytes, slowLds;
    unsigned slowGrid, snapshotBlocks;
    int route;                        // EC_ROUTE_*
    int slotCap, mergedCap, slotOffset;
    bool wideSlots;
    int lpcMaxContours, lpcEdgeCost, lpcMaxEdges, lpcMinCount, wideMaxEdges;   // EcQueryPolicy (msdf_kernels.hpp), in its order
    float wideLoad, wideMeanCount;
    int gridSteps;
    size_t queryLds, fastLds;
    bool lazyProtect;                 // the sweep's order (msdf_ec_fast.hpp: ecLazyProtect) is fixed per launch: an instantiation each
    unsigned queryBlocks;             // before the clamp to what the device holds at once (residentQueryBlocks)
    bool staticDeal;
    int queryFlags, queryBatch;
    unsigned residentQueryBlocks(unsigned resident) const { return staticDeal && resident && queryBlocks > resident ? resident : queryBlocks; }
};
// ecMode / ecCheck / stageLimit: of the call's config (msdf_ec.hpp: EC_MODE_*, EC_CHECK_*). fastLds: ecFastLdsBytes(b.maxEdges, n) (msdf_kernels.hpp).
inline EcPlan planCorrection(const PlanEnv &env, const GlyphCounts &b, int w, int h, int n, bool overlap, int ecMode, int ecCheck, int stageLimit, size_t fastLds) {
    EcPlan p = EcPlan();
    p.allTexels = (size_t) b.nGlyphs*w*h;
    p.tooManyTexels = p.allTexels >= 0xffffffffull;
    p.gres = overlap && (size_t) b.maxContours*PLAN_WAVE*sizeof(double) > 96*1024;
    p.resBytes = overlap ? (size_t) b.maxContours*PLAN_WAVE*sizeof(double) : 0;   // combiner scratch of the PSDF distance checks
    p.slowLds = p.gres ? 0 : p.resBytes;
    p.slowGrid = (unsigned) (p.allTexels/PLAN_WAVE < 64 ? 64 : p.allTexels/PLAN_WAVE > 2048 ? 2048 : p.allTexels/PLAN_WAVE);   // grid-stride over the texels
    const unsigned cap = p.gres ? p.slowGrid : 16384u;
    p.snapshotBlocks = (unsigned) ((p.allTexels+PLAN_WAVE-1)/PLAN_WAVE < cap ? (p.allTexels+PLAN_WAVE-1)/PLAN_WAVE : cap);
    // k_ec_query parks the single-edge selector states of a glyph in LDS (40 B per edge) when the glyph has at most slotCap edges; its
    // combiner scratch is one double per contour (wave-uniform query point)
    // (both bounded so that the kernel's LDS does not cap its occupancy -- one 543-edge symbol in the batch had cost every wavefront
    // 22 KB; measured: 2.67 -> 2.60 ms of correction on the distinct-glyph set)
    const int slotCapWanted = env.t.querySlotCap, lpcContoursWanted = env.t.queryLpcContours;   // 160, 24 (MSDFHIP_QUERY_LDS)
    p.slotCap = b.maxEdges < slotCapWanted ? (b.maxEdges > 0 ? b.maxEdges : 1) : slotCapWanted;
    // A launch of few glyphs is a latency chain of its largest one (the 926-edge logo: one distance check per wavefront, 40 contours walked one
    // after the other without the slots: correction 0.61 ms, with them 0.39): slots for up to 1024 edges there, LDS permitting.
    if (b.nGlyphs < 256 && !env.t.hasQueryLds) {
        const int wide = b.maxEdges < 1024 ? (b.maxEdges > 0 ? b.maxEdges : 1) : 1024;
        const int wideMerged = b.maxContours < wide ? (b.maxContours > 0 ? b.maxContours : 1) : wide;
        if ((size_t) b.maxContours*sizeof(double)+(size_t) (wide+wideMerged)*PLAN_PB_SLOT_BYTES <= (size_t) 64*1024 && wide > p.slotCap)
            p.slotCap = wide, p.wideSlots = true;
    }
    // LDS of a query wavefront: the lane-per-candidate scratch [maxContours][64], or (cooperative) [maxContours] + the slots -- one or the other
    p.lpcMaxContours = b.maxContours < lpcContoursWanted ? b.maxContours : lpcContoursWanted;     // beyond: cooperative only (one double per contour)
    // Measured on MI355X (post-distance time in ms: Basic-Latin / CJK-like 48x48 / 8192 DejaVu glyphs / 1024x1024 logo):
    //   cooperative only 1.98 / 5.35 / 2.83 / 4.60;  lane-per-candidate wherever the instruction count favours it 1.76 / 3.57 / 4.23 / 10.3;
    //   lane-per-candidate only for glyphs of at most 48 edges 1.75 / 5.40 / 2.67 / 4.62  <- default: a chunk of a large glyph is one long
    //   serial walk that the launch ends up waiting for.
    // Round 2, after the records of the lane-per-candidate walk became scalar loads and the work list heavy-first: with the bound at 128
    // edges for every launch the CJK-like set gains (4.42 -> 2.82) and the DejaVu set loses (2.33 -> 2.73: 55 k candidates are a latency
    // chain, not a load) -- k_ec_scan therefore widens the bound only for launches whose cooperative cost exceeds wideLoad instructions.
    // Round 3, after the chunk walk got batched scalar loads and the cooperative path its register records: the cost of an edge in a chunk
    // relative to a cooperative round re-swept (340 / 200 / 120 / 60): 1.80 / 1.78 / 1.79 / 1.78 ms on the DejaVu set, 1.57 / 1.51 / 1.50 / 1.52 on
    // Basic-Latin -- 150 (profiles/r03_ab_notes.md).
    p.lpcEdgeCost = env.t.qpEdgeCost, p.lpcMaxEdges = env.t.qpMaxEdges, p.lpcMinCount = env.t.qpMinCount;   // 150, 48, never
    p.wideMaxEdges = env.t.qpWideMaxEdges, p.wideLoad = env.t.qpWideLoad, p.wideMeanCount = env.t.qpWideMeanCount;   // 128, 4e8 (MSDFHIP_QUERY_POLICY)
    p.gridSteps = env.t.queryGridSteps;
    const size_t resLanes = overlap ? (size_t) (p.lpcMaxContours > 0 ? p.lpcMaxContours : 1)*PLAN_WAVE*sizeof(double) : 0;
    p.slotOffset = overlap ? (b.maxContours > 0 ? b.maxContours : 1) : 0;
    p.mergedCap = b.maxContours < p.slotCap ? (b.maxContours > 0 ? b.maxContours : 1) : p.slotCap;   // per-contour merged states of a glyph that uses the slots
    const size_t coopLds = (size_t) p.slotOffset*sizeof(double)+(size_t) (p.slotCap+p.mergedCap)*PLAN_PB_SLOT_BYTES;
    p.queryLds = resLanes > coopLds ? resLanes : coopLds;
    p.fastLds = fastLds;
    if (stageLimit != 0)                                         // test hook: stencil snapshots through the full pipeline for every texel
        p.route = EC_ROUTE_STAGE_SNAPSHOT;
    // More contours than k_ec_query's per-contour LDS scratch holds (~19 000): the full per-texel pipeline with its scratch in the global
    // workspace takes every texel -- slow, but a valid shape is corrected instead of refused (the reference cannot fail either).
    else if (p.gres && p.queryLds > env.ldsLimit && fastLds <= env.ldsLimit)
        p.route = EC_ROUTE_SLOW_ALL;
    else if (fastLds > env.ldsLimit || p.queryLds > env.ldsLimit)
        p.route = EC_ROUTE_TOO_COMPLEX;
    p.lazyProtect = ecMode == MSDFHIP_EC_EDGE_PRIORITY && ecCheck == MSDFHIP_CHECK_DISTANCE_AT_EDGE;
    // the query kernel is a pool of wavefronts draining one work list: enough of them to fill the device, no more
    // (a wavefront that finds the list empty leaves after one atomic; still, a single 64x64 glyph should not launch thousands of them)
    const size_t wanted = p.allTexels/512;
    p.queryBlocks = (unsigned) (wanted < 64 ? 64 : wanted > 8192 ? 8192 : wanted);
    // ... dealt out statically (k_ec_query: no ticket counter) to as many workgroups as the device holds at once
    p.staticDeal = env.t.queryStatic != 0;
    p.queryFlags = p.staticDeal ? (env.t.queryStatic == 2 ? 5 : 1) : 0;
    p.queryBatch = env.t.queryBatch;
    return p;
}

// The sign pass (k_sign_correction): a wavefront per span of tiles of one tile row.
struct SignPlan {
    int span, spansX, spans;
    size_t blocks, cap, lds;
    bool wholeRows, chunked;          // its routes: MSDFHIP_ROUTE_SIGN_WHOLE_ROWS or _SPLIT, and _CHUNKED on top
};
inline SignPlan planSign(const PlanEnv &env, int nGlyphs, int maxEdges, int w, int h) {
    SignPlan p;
    const int tilesX = (w+PLAN_TILE-1)/PLAN_TILE, tilesY = (h+PLAN_TILE-1)/PLAN_TILE;
    // Tiles of one tile row share the per-row intersection lists: one wavefront takes `span` of them, as many as still leaves
    // >= 16 wavefronts per CU in the launch (a single huge bitmap keeps span small, an atlas batch takes whole rows).
    p.span = tilesX;
    while (p.span > 1 && (size_t) nGlyphs*tilesY*((tilesX+p.span-1)/p.span) < 4096)
        p.span = (p.span+1)/2;
    p.spansX = (tilesX+p.span-1)/p.span, p.spans = p.spansX*tilesY;
    p.blocks = (size_t) nGlyphs*(size_t) p.spans;
    // Row-list capacity: every edge yields at most 3 intersections per row. Up to capLimit entries per row the lists of the
    // whole shape fit; beyond, the kernel walks the edges in chunks of cap/3.
    const size_t capLimit = env.t.signCap;                       // 192: 23 KB per wavefront at the limit (384: 46 KB = 3 wavefronts per CU; distinct-glyph set 2.95 -> 2.60 ms)
    const size_t all = 3*(size_t) (maxEdges > 0 ? maxEdges : 1);
    p.cap = all > capLimit ? capLimit : all;
    p.lds = PLAN_SIGN_ROWS*p.cap*(sizeof(double)+sizeof(int))+PLAN_SIGN_ROWS*sizeof(int);   // per-row intersection lists
    p.wholeRows = p.span == tilesX, p.chunked = p.cap < all;
    return p;
}

// The legacy generators (k_distance_legacy): a wavefront per tile of every glyph, dealt like k_distance's one-tile launches (decodeBlock).
struct LegacyDistancePlan {
    size_t blocks;
    bool tooManyBlocks;               // beyond the grid limit: refused
};
inline LegacyDistancePlan planLegacyDistance(int nGlyphs, int w, int h) {
    LegacyDistancePlan p;
    p.blocks = distanceBlocks(nGlyphs, w, h, 1);
    p.tooManyBlocks = p.blocks > 0x7fffffffull;
    return p;
}

// The legacy correction (k_ec_legacy) of nGlyphs packed tiles of w x h texels with n channels: two out-of-place passes, tiles -> scratch -> tiles.
enum { PLAN_LEGACY_EC_THREADS = 256, PLAN_LEGACY_EC_MAX_BLOCKS = 65536 };
struct LegacyEcPlan {
    size_t texels, scratchFloats;     // of all tiles; the scratch holds one copy of them
    unsigned blocks;                  // workgroups of PLAN_LEGACY_EC_THREADS threads per pass, grid-stride over the texels (0: nothing to do)
};
inline LegacyEcPlan planLegacyCorrection(int nGlyphs, int w, int h, int n) {
    LegacyEcPlan p;
    p.texels = (size_t) (nGlyphs > 0 ? nGlyphs : 0)*(size_t) w*(size_t) h;
    p.scratchFloats = p.texels*(size_t) n;
    const size_t wanted = (p.texels+PLAN_LEGACY_EC_THREADS-1)/PLAN_LEGACY_EC_THREADS;
    p.blocks = (unsigned) (wanted < PLAN_LEGACY_EC_MAX_BLOCKS ? wanted : PLAN_LEGACY_EC_MAX_BLOCKS);
    return p;
}

} // namespace msdfhip
