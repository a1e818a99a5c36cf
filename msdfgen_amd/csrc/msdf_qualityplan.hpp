// msdf_qualityplan.hpp -- what the launches of msdfhip_batch_estimate_sdf_error[_sized] and msdfhip_render_sdf[_sized] depend on, over plain integers (and,
// for the render's range mapping, four doubles). Host code that the host compiler builds on its own (tests/sized_quality_host, tests/test_sized_quality_host.py);
// the two searches over a prefix are also what the sized kernels run per lane (msdf_kernels.hpp includes this file: QUALITY_HD).
//
// estimateSDFError (core/sdf-error-estimation.cpp:134-164) walks (h-1)*scanlinesPerRow scanlines of a w x h field, none where w <= 1 or h <= 1 (:136). One
// ITEM is one scanline; the items of a batch are numbered in (glyph, row, subRow) order. renderSDF (core/render-sdf.cpp:14-170) writes ow x oh texels.

#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define QUALITY_HD __host__ __device__ inline
#else
#define QUALITY_HD inline
#endif

namespace msdfhip {

enum { QUALITY_OK = 0, QUALITY_TOO_MANY, QUALITY_BAD_OUTPUT };

// The bound on the items of one estimate and on the output texels of one render: beyond it the per-item results alone would take 2 PiB, and every product
// of a count below it with a per-item byte count below 2^15 stays inside int64.
const int64_t QUALITY_MAX_COUNT = (int64_t) 1<<48;

// itemStart[g+1] = itemStart[g] + (w_g > 1 && h_g > 1 ? (h_g-1)*spr : 0); itemStart: int64[nGlyphs+1]. sizes as sizedLayout validated them (sides >= 1);
// spr >= 1. Refuses (QUALITY_TOO_MANY; itemStart is then unspecified) a total beyond QUALITY_MAX_COUNT.
inline int errorItemPrefix(int nGlyphs, const int32_t *sizes, int spr, int64_t *itemStart) {
    int64_t at = 0;
    itemStart[0] = 0;
    for (int g = 0; g < nGlyphs; ++g) {
        const int64_t w = sizes[2*(size_t) g], h = sizes[2*(size_t) g+1];
        if (w > 1 && h > 1) {
            const int64_t add = (h-1)*(int64_t) spr;             // (< 2^62)
            if (add > QUALITY_MAX_COUNT-at)
                return QUALITY_TOO_MANY;
            at += add;
        }
        itemStart[g+1] = at;
    }
    return QUALITY_OK;
}

// The glyph that holds entry `at` of a prefix (start[0] = 0 <= at < start[n]): the g with start[g] <= at < start[g+1]. Such a glyph has entries of its own,
// so glyphs without any are stepped over wherever they sit. A binary search for the last start[g] <= at.
QUALITY_HD int prefixFind(const int64_t *start, int n, int64_t at) {
    int lo = 0, hi = n;                                          // start[lo] <= at < start[hi]
    while (hi-lo > 1) {
        const int mid = lo+(hi-lo)/2;
        if (start[mid] <= at)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Item -> (glyph, row, subRow).
struct ErrorItem {
    int g, row, subRow;
};
QUALITY_HD ErrorItem errorItemOf(const int64_t *itemStart, int nGlyphs, int spr, int64_t item) {
    ErrorItem it;
    it.g = prefixFind(itemStart, nGlyphs, item);
    const int64_t rem = item-itemStart[it.g];
    it.row = (int) (rem/spr);
    it.subRow = (int) (rem-(int64_t) it.row*spr);
    return it;
}

// The capacities of a lane's two intersection lists: the shape's scanline holds at most 3 per edge, the field's at most 3 per texel column and the two
// of the row's ends (msdf_scanline.hpp). W: the width of the uniform call, the largest w_g of a sized one.
inline size_t errorRefCap(int maxEdges) { return 3*(size_t) (maxEdges > 0 ? maxEdges : 1); }
inline size_t errorSdfCap(int W) { return 3*(size_t) W+2; }
inline size_t errorLaneBytes(size_t refCap, size_t sdfCap) { return (refCap+sdfCap)*(sizeof(double)+sizeof(int)); }

// Lanes per launch under a list workspace of capBytes: at least one wavefront, whole wavefronts, no more than the items need. The launches are then
// [k*lanes, min((k+1)*lanes, items)), k = 0 .. errorChunkCount-1: the last one may be short.
inline size_t errorChunkLanes(int64_t items, size_t laneBytes, size_t capBytes) {
    size_t lanes = capBytes/laneBytes;
    lanes = lanes < 64 ? 64 : lanes/64*64;
    if (lanes > (size_t) items)
        lanes = ((size_t) items+63)/64*64;
    return lanes;
}
inline int64_t errorChunkCount(int64_t items, size_t lanes) { return items > 0 ? (items+(int64_t) lanes-1)/(int64_t) lanes : 0; }

// ---- renderSDF

// outStart[g+1] = outStart[g] + ow_g*oh_g; outSizes: int32[nGlyphs*2] = ow_g, oh_g, each >= 0 (a glyph with a 0 on either side has no texel).
// QUALITY_BAD_OUTPUT with *badGlyph for a negative side, QUALITY_TOO_MANY beyond QUALITY_MAX_COUNT texels.
inline int renderTexelPrefix(int nGlyphs, const int32_t *outSizes, int64_t *outStart, int *badGlyph) {
    int64_t at = 0;
    outStart[0] = 0;
    *badGlyph = -1;
    for (int g = 0; g < nGlyphs; ++g) {
        const int64_t w = outSizes[2*(size_t) g], h = outSizes[2*(size_t) g+1];
        if (w < 0 || h < 0) {
            *badGlyph = g;
            return QUALITY_BAD_OUTPUT;
        }
        const int64_t add = w*h;                                 // (< 2^62)
        if (add > QUALITY_MAX_COUNT-at)
            return QUALITY_TOO_MANY;
        at += add;
        outStart[g+1] = at;
    }
    return QUALITY_OK;
}

// Output texel -> (glyph, x, y).
struct RenderTexel {
    int g, x, y;
};
QUALITY_HD RenderTexel renderTexelOf(const int64_t *outStart, int nGlyphs, const int32_t *outSizes, int64_t texel) {
    RenderTexel t;
    t.g = prefixFind(outStart, nGlyphs, texel);
    const int64_t rem = texel-outStart[t.g];
    const int ow = outSizes[2*(size_t) t.g];
    t.y = (int) (rem/ow);
    t.x = (int) (rem-(int64_t) t.y*ow);
    return t;
}

// What renderSDF derives from the two sizes and the range before its loops (render-sdf.cpp:16-27), in fp64 and in this order: scale = sdf size / output
// size; with a range (lower != upper) the range times (ow+oh)/(sw+sh) and DistanceMapping::inverse of it (DistanceMapping.cpp:6-9). ow, oh >= 1.
struct RenderMapping {
    double scaleX, scaleY, mapScale, mapTranslate;
};
inline RenderMapping renderMapping(int sw, int sh, int ow, int oh, double rangeLower, double rangeUpper) {
    RenderMapping m;
    m.scaleX = (double) sw/ow, m.scaleY = (double) sh/oh;        // render-sdf.cpp:16
    m.mapScale = 1, m.mapTranslate = 0;
    if (!(rangeLower == rangeUpper)) {
        const double f = (double) ((int64_t) ow+oh)/(double) ((int64_t) sw+sh);   // render-sdf.cpp:26: sdfPxRange *= ... (the sums in 64 bits: the same values, no overflow)
        rangeLower *= f, rangeUpper *= f;
        const double rangeWidth = rangeUpper-rangeLower;         // DistanceMapping::inverse(Range), DistanceMapping.cpp:6-9
        m.mapScale = rangeWidth, m.mapTranslate = rangeLower/(rangeWidth ? rangeWidth : 1);
    }
    return m;
}

} // namespace msdfhip
