// msdf_prepplan.hpp -- the buffers of the raw-outline preparation (msdf_capi.hip: queuePreparation, queueFrame, then k_prep_records), stated once:
// which device buffers a preparation touches under a configuration, how large each is, how they are carved out of one arena, what every slot of a
// streamed call must hold, and which buffer feeds which field of PrepBuffers. msdfhip_batch_create_prepared_oriented allocates the table region by
// region; the streamed generator (StreamFeeder) sizes its slots from the bounds and carves every chunk with its exact counts.
// Host code only (no HIP): msdf_capi.hip includes it, and tests/hostemu compiles it with the host compiler (tests/test_prep_plan_host.py).

#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "msdf_hostplan.hpp"
#include "msdf_shapeprep.hpp"

namespace msdfhip {

enum { PREP_PLAN_WAVE_MAX_EDGES = 2048 };                        // k_prep_colour_wave's large LDS tier (msdf_capi.hip asserts it equal to PREP_WAVE_MAX_EDGES)

// Host side of the preparation's sizes (the same arithmetic wherever raw outlines are prepared): co1 = the contour offsets after normalize, a prefix
// of normalizedCount over the raw contour sizes; *bound2 = the upper bound of the coloured edge count (a contour of n1 < 3 edges may be split into 3*n1);
// *longest = the longest normalized contour (it picks the colouring's LDS tier and says whether the `big` tables are needed).
inline void prepOffsets(const int32_t *co, int nC, bool normalize, int32_t *co1, size_t *bound2, int *longest) {
    size_t b2 = 0;
    int lg = 0;
    co1[0] = 0;
    for (int c = 0; c < nC; ++c) {
        const int n = co[c+1]-co[c];
        const int n1 = normalize ? normalizedCount(n) : n;
        co1[c+1] = co1[c]+n1;
        b2 += n1 < 3 ? 3*(size_t) n1 : (size_t) n1;
        lg = n1 > lg ? n1 : lg;
    }
    *bound2 = b2, *longest = lg;
}

// Does a glyph of maxRawEdges raw edges need k_prep_orient's global hit scratch (3 hits per edge at most)?
inline bool orientHitsBig(long long maxRawEdges) { return 3*maxRawEdges > PREP_ORIENT_LDS_HITS; }

// The device buffers of one preparation (every pointer the caller's: nothing is allocated here).
struct PrepBuffers {
    const int32_t *gco, *co, *co1;        // glyph -> contour offsets, raw contour offsets, contour offsets after normalize (prepOffsets)
    EdgeArrays raw, norm, fin;            // raw edges (colors may be NULL = WHITE); normalized [co1[nC]]; coloured [bound2] (coloring != 0 only)
    int32_t *cusp, *count, *co2;          // [nC+1] each: normalize's cusp flags; coloured edges per contour and their prefix (coloring != 0 only)
    const unsigned long long *seeds;      // one per glyph, or NULL: cfg->seed for every glyph
    ColourTables big;                     // the colouring's tables of contours beyond PREP_WAVE_MAX_EDGES (only when `longest` exceeds it)
    int32_t *votes;                       // [nC] orientContours' votes of glyphs beyond PREP_ORIENT_LDS_CONTOURS contours (orient_contours only)
    double *hitX;                         // [3 nE] + hitTag: scanline hits beyond PREP_ORIENT_LDS_HITS (only when orientHitsBig: see prepOrientScratch)
    int32_t *hitTag;
};

// Every buffer a preparation can touch, in carve order: the part uploaded from the host first, then the device-only part.
enum PrepRegion {
    PREP_GCO, PREP_CO, PREP_RAW_POINTS, PREP_RAW_TYPES, PREP_RAW_COLORS, PREP_CO1, PREP_SEEDS,
    PREP_UPLOADED,                                               // (count of the uploaded regions)
    PREP_CUSP = PREP_UPLOADED, PREP_COUNT, PREP_CO2, PREP_NORM_POINTS, PREP_NORM_TYPES, PREP_NORM_COLORS, PREP_FIN_POINTS, PREP_FIN_TYPES, PREP_FIN_COLORS,
    PREP_BIG_MASK, PREP_BIG_SPLINE, PREP_BIG_EDGE_LENGTH, PREP_BIG_CORNER_LENGTH, PREP_BIG_CORNER_INDEX, PREP_BIG_MINOR, PREP_VOTES, PREP_HIT_X, PREP_HIT_TAG,
    PREP_BOUNDS, PREP_RECS, PREP_WINDINGS,
    PREP_REGIONS
};

// What decides which regions exist. A region is present iff a kernel of the queued sequence reads or writes it under the configuration.
struct PrepPlanConfig {
    bool prepare;                         // false: the edges are prepared already (the streamed generator's plain form) -- the "raw" arrays are final
    int coloring;                         // MsdfHipPrepConfig::coloring (0 keep, 1 simple, 2 ink trap)
    bool seeds, rawColors;                // per-glyph seeds / raw edge colours are given
    bool orient;                          // MsdfHipOrientConfig::orient_contours
    bool hitsBig, longContour;            // orientHitsBig of the largest glyph; a normalized contour beyond PREP_WAVE_MAX_EDGES edges
    bool bounds, records;                 // Shape::getBounds per glyph (k_frame); the records + windings of the final edges (k_prep_records)
};

struct PrepCounts { size_t n, nC, nE, nE1, nE2; };               // glyphs, contours, raw / normalized / coloured edges (nE2: its bound, prepOffsets)

// Bytes of every region; 0: absent.
struct PrepSizes { size_t bytes[PREP_REGIONS]; };
inline PrepSizes prepRegionSizes(const PrepPlanConfig &cfg, const PrepCounts &k) {
    PrepSizes s = PrepSizes();
    size_t *b = s.bytes;
    const size_t e = k.nE ? k.nE : 1, e1 = k.nE1 ? k.nE1 : 1, e2 = k.nE2 ? k.nE2 : 1, offsets = (k.nC+1)*sizeof(int32_t);
    b[PREP_GCO] = (k.n+1)*sizeof(int32_t), b[PREP_CO] = offsets;
    b[PREP_RAW_POINTS] = e*8*sizeof(double), b[PREP_RAW_TYPES] = e, b[PREP_RAW_COLORS] = cfg.rawColors ? e : 0;
    size_t finalEdges = e;
    if (cfg.prepare) {
        b[PREP_CO1] = b[PREP_CUSP] = offsets;
        b[PREP_NORM_POINTS] = e1*8*sizeof(double), b[PREP_NORM_TYPES] = b[PREP_NORM_COLORS] = finalEdges = e1;
        if (cfg.coloring) {
            b[PREP_SEEDS] = cfg.seeds ? k.n*sizeof(uint64_t) : 0;
            b[PREP_COUNT] = b[PREP_CO2] = offsets;
            b[PREP_FIN_POINTS] = e2*8*sizeof(double), b[PREP_FIN_TYPES] = b[PREP_FIN_COLORS] = finalEdges = e2;
            // the colouring's per-contour tables live in LDS; a contour beyond PREP_WAVE_MAX_EDGES edges keeps them in global memory, indexed like the edges
            if (cfg.longContour) {
                b[PREP_BIG_MASK] = sizeof(unsigned long long)*(e1/PREP_WAVE+k.nC+2), b[PREP_BIG_SPLINE] = e1;
                if (cfg.coloring == 2)
                    b[PREP_BIG_EDGE_LENGTH] = b[PREP_BIG_CORNER_LENGTH] = sizeof(double)*e1, b[PREP_BIG_CORNER_INDEX] = sizeof(int)*e1, b[PREP_BIG_MINOR] = e1;
            }
        }
        if (cfg.orient) {                                        // orientContours' scratch: votes of glyphs with many contours, hits beyond the LDS tier
            b[PREP_VOTES] = offsets;
            if (cfg.hitsBig)
                b[PREP_HIT_X] = 3*e*sizeof(double), b[PREP_HIT_TAG] = 3*e*sizeof(int32_t);
        }
        if (cfg.bounds)
            b[PREP_BOUNDS] = 4*(k.n ? k.n : 1)*sizeof(double);
    }
    if (cfg.records)
        b[PREP_RECS] = sizeof(EdgeRec)*finalEdges, b[PREP_WINDINGS] = k.nC ? k.nC : 1;
    return s;
}

// The table as a 256-byte aligned sequential carve of one arena. The first `uploadBytes` are the uploaded regions (they depend on n, nC, nE and the
// call's configuration alone, so a chunk's staging can be filled before its normalized counts are known); a colouring's offsets (co2) come back into
// the pinned staging behind them. deviceBytes: the end of the last region.
struct PrepCarve {
    size_t off[PREP_REGIONS], bytes[PREP_REGIONS];
    size_t uploadBytes, deviceBytes, pinnedBytes;
};
inline PrepCarve prepCarve(const PrepPlanConfig &cfg, const PrepCounts &k) {
    const PrepSizes s = prepRegionSizes(cfg, k);
    PrepCarve c;
    Carver carver;
    c.uploadBytes = c.deviceBytes = 0;
    for (int r = 0; r < PREP_REGIONS; ++r) {
        if (r == PREP_UPLOADED)
            c.uploadBytes = carver.off;
        c.bytes[r] = s.bytes[r], c.off[r] = carver.take(s.bytes[r]);
        if (s.bytes[r])
            c.deviceBytes = c.off[r]+s.bytes[r];
    }
    c.pinnedBytes = c.uploadBytes+s.bytes[PREP_CO2];
    return c;
}

// The one place that knows which region feeds which field of PrepBuffers. ptr[r] == NULL: absent. Without a colouring the final edges are the normalized ones.
inline PrepBuffers bindPrep(void *const ptr[PREP_REGIONS]) {
    PrepBuffers pb;
    pb.gco = (const int32_t *) ptr[PREP_GCO], pb.co = (const int32_t *) ptr[PREP_CO], pb.co1 = (const int32_t *) ptr[PREP_CO1];
    pb.raw.points = (double *) ptr[PREP_RAW_POINTS], pb.raw.types = (uint8_t *) ptr[PREP_RAW_TYPES], pb.raw.colors = (uint8_t *) ptr[PREP_RAW_COLORS];
    pb.norm.points = (double *) ptr[PREP_NORM_POINTS], pb.norm.types = (uint8_t *) ptr[PREP_NORM_TYPES], pb.norm.colors = (uint8_t *) ptr[PREP_NORM_COLORS];
    pb.fin.points = (double *) ptr[PREP_FIN_POINTS], pb.fin.types = (uint8_t *) ptr[PREP_FIN_TYPES], pb.fin.colors = (uint8_t *) ptr[PREP_FIN_COLORS];
    if (!ptr[PREP_FIN_POINTS])
        pb.fin = pb.norm;
    pb.cusp = (int32_t *) ptr[PREP_CUSP], pb.count = (int32_t *) ptr[PREP_COUNT], pb.co2 = (int32_t *) ptr[PREP_CO2];
    pb.seeds = (const unsigned long long *) ptr[PREP_SEEDS];
    pb.big.cornerMask = (unsigned long long *) ptr[PREP_BIG_MASK], pb.big.splineColor = (unsigned char *) ptr[PREP_BIG_SPLINE];
    pb.big.edgeLength = (double *) ptr[PREP_BIG_EDGE_LENGTH], pb.big.cornerLength = (double *) ptr[PREP_BIG_CORNER_LENGTH];
    pb.big.cornerIndex = (int *) ptr[PREP_BIG_CORNER_INDEX], pb.big.minor = (unsigned char *) ptr[PREP_BIG_MINOR];
    pb.votes = (int32_t *) ptr[PREP_VOTES], pb.hitX = (double *) ptr[PREP_HIT_X], pb.hitTag = (int32_t *) ptr[PREP_HIT_TAG];
    return pb;
}

// A region of a carve inside the arena at `base` (NULL: absent), and the whole carve bound.
inline void *prepRegionAt(char *base, const PrepCarve &c, int region) { return c.bytes[region] ? base+c.off[region] : NULL; }
inline PrepBuffers bindPrep(char *base, const PrepCarve &c) {
    void *ptr[PREP_REGIONS];
    for (int r = 0; r < PREP_REGIONS; ++r)
        ptr[r] = prepRegionAt(base, c, r);
    return bindPrep(ptr);
}

// What the slots of a streamed call must hold: the chunks of `lengths` over a list with contours[g] / edges[g] per glyph. A slot is sized before any
// outline is seen, so from upper bounds: a raw contour of one edge becomes three normalized ones and one of two edges at most six coloured ones
// (nE + 2 nC, nE + 4 nC), a glyph of edges + 2 contours > PREP_WAVE_MAX_EDGES may hold a long contour, the largest glyph decides the hit scratch. Every
// region's size grows with each count and with each flag, and the carve is sequential, so a chunk carved with its exact counts (prepOffsets) ends
// inside these. cfg.hitsBig / cfg.longContour are set per chunk here. refused: the first chunk beyond the 32-bit offsets of a batch (-1: none; then
// the chunks up to it are filled and the byte counts are not).
struct StreamChunk {
    int start, length;
    size_t nC, nE;
    bool mayHaveLong, hitsBig;
};
struct StreamPrepPlan {
    std::vector<StreamChunk> chunks;
    size_t pinnedBytes, devBytes;
    int refused;
};
inline StreamPrepPlan planStreamPrep(const int *contours, const int *edges, const std::vector<int> &lengths, PrepPlanConfig cfg) {
    StreamPrepPlan plan;
    plan.pinnedBytes = plan.devBytes = 0, plan.refused = -1;
    int g = 0;
    for (size_t ci = 0; ci < lengths.size(); g += lengths[ci], ++ci) {
        StreamChunk ch = { g, lengths[ci], 0, 0, false, false };
        int maxRaw = 0;
        for (int k = g; k < g+lengths[ci]; ++k) {
            ch.nC += (size_t) contours[k], ch.nE += (size_t) edges[k];
            ch.mayHaveLong |= (long long) edges[k]+2LL*contours[k] > PREP_PLAN_WAVE_MAX_EDGES;
            maxRaw = edges[k] > maxRaw ? edges[k] : maxRaw;
        }
        ch.hitsBig = orientHitsBig(maxRaw);
        plan.chunks.push_back(ch);
        if (ch.nE > 0x7fffffffull/8 || ch.nC > 0x7fffffffull/8 || (cfg.prepare && ch.nE+4*ch.nC > 0x7fffffffull/8)) {
            plan.refused = (int) ci;
            return plan;
        }
        cfg.longContour = ch.mayHaveLong, cfg.hitsBig = ch.hitsBig;
        const PrepCounts bound = { (size_t) lengths[ci], ch.nC, ch.nE, ch.nE+2*ch.nC, ch.nE+4*ch.nC };
        const PrepCarve c = prepCarve(cfg, bound);
        plan.pinnedBytes = c.pinnedBytes > plan.pinnedBytes ? c.pinnedBytes : plan.pinnedBytes;
        plan.devBytes = c.deviceBytes > plan.devBytes ? c.deviceBytes : plan.devBytes;
    }
    return plan;
}

} // namespace msdfhip
