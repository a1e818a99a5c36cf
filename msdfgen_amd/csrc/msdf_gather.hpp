// msdf_gather.hpp -- the kernels of msdfhip_batch_gather: the CSR arrays of a new batch copied out of resident ones, fed by the table of
// msdf_gatherplan.hpp. Bandwidth-bound copies; the grids cover destination ITEMS (contours, 16-byte pieces of the points), not glyphs, so a glyph of
// 61 440 edges next to thousands of small ones is spread over as many workgroups as its bytes need.
//
// Every kernel here is a template only to be instantiated where it is named (the end of msdf_capi.hip), like k_box.

#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "msdf_device.hpp"

namespace msdfhip {

// The arrays of one source batch, as the kernels read them (a small device table, one row per source: one launch serves any number of sources).
struct GatherSourceArrays {
    const int32_t *contourOffsets;
    const double *points;
    const uint8_t *types, *colors;
    const double *bounds;             // [nGlyphs][4], only read when the result's bounds are fixed
};

// The glyph that owns destination item `item`: the last g with start[g] <= item (start: n+1 ascending entries from 0, start[n] > item; glyphs without items
// share their start with their successor and are stepped over). The wavefront's first and last item are searched wave-uniformly over the whole column
// (scalar loads and branches); a lane then searches only between those two glyphs -- usually one or two candidates.
__device__ __forceinline__ int gatherGlyphUniform(const int32_t *__restrict__ start, int n, int item) {
    int lo = 0, hi = n;               // start[lo] <= item < start[hi]
    while (hi-lo > 1) {
        const int mid = (int) (((unsigned) lo+(unsigned) hi)>>1);
        if (start[mid] <= item)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int gatherGlyphOf(const int32_t *__restrict__ start, int n, int waveFirst, int waveLast, int item) {
    int lo = gatherGlyphUniform(start, n, MSDF_UNIFORM(waveFirst)), hi = gatherGlyphUniform(start, n, MSDF_UNIFORM(waveLast));
    while (lo < hi) {                 // the answer lies in lo..hi
        const int mid = (int) (((unsigned) lo+(unsigned) hi+1u)>>1);
        if (start[mid] <= item)
            lo = mid;
        else
            hi = mid-1;
    }
    return lo;
}

// Lanes are destination contours 0..nContours: dst[c] = the source's offset of that contour, moved from the glyph's first edge in its source to its first
// edge in the result; lane nContours writes the closing entry (the result's edge count). 256 threads; grid = ceil((nContours+1)/256).
template <int WAVE_ = 64>
__global__ void __launch_bounds__(256) k_gather_contours(int32_t *__restrict__ dstContourOffsets, int nGlyphs, int nContours, int nEdges,
                                                         const int32_t *__restrict__ source, const int32_t *__restrict__ srcContour0,
                                                         const int32_t *__restrict__ srcEdge0, const int32_t *__restrict__ dstContour0,
                                                         const int32_t *__restrict__ dstEdge0, const GatherSourceArrays *__restrict__ sources) {
    const long long base = (long long) blockIdx.x*256+(threadIdx.x&~(unsigned) (WAVE_-1));
    const long long c = base+(threadIdx.x&(WAVE_-1));
    if (c >= nContours) {
        if (c == nContours)
            dstContourOffsets[c] = nEdges;
        return;
    }
    const long long last = base+WAVE_-1 < nContours ? base+WAVE_-1 : (long long) nContours-1;
    const int g = gatherGlyphOf(dstContour0, nGlyphs, (int) base, (int) last, (int) c);
    const int32_t *__restrict__ srcOffsets = sources[source[g]].contourOffsets;
    dstContourOffsets[c] = srcOffsets[srcContour0[g]+((int) c-dstContour0[g])]-srcEdge0[g]+dstEdge0[g];
}

// Lanes are 16-byte pieces of the destination points (four per edge, 64 B); the lanes of an edge's first two pieces also copy its type and its colour.
// A piece is read as two doubles -- a caller's points (msdfhip_batch_create_device) need only be aligned as doubles -- which the compiler merges into one
// 16-byte load (the hardware takes global addresses unaligned); the result's own arrays are allocated here and the store is one aligned 16-byte store.
// 256 threads; grid = ceil(4*nEdges/256).
template <int WAVE_ = 64>
__global__ void __launch_bounds__(256) k_gather_edges(double *__restrict__ dstPoints, uint8_t *__restrict__ dstTypes, uint8_t *__restrict__ dstColors, int nGlyphs,
                                                      int nEdges, const int32_t *__restrict__ source, const int32_t *__restrict__ srcEdge0,
                                                      const int32_t *__restrict__ dstEdge0, const GatherSourceArrays *__restrict__ sources) {
    const long long pieces = 4ll*nEdges;
    const long long base = (long long) blockIdx.x*256+(threadIdx.x&~(unsigned) (WAVE_-1));
    const long long p = base+(threadIdx.x&(WAVE_-1));
    if (p >= pieces)
        return;
    const long long lastPiece = base+WAVE_-1 < pieces ? base+WAVE_-1 : pieces-1;
    const int e = (int) (p>>2), part = (int) (p&3);
    const int g = gatherGlyphOf(dstEdge0, nGlyphs, (int) (base>>2), (int) (lastPiece>>2), e);
    const GatherSourceArrays src = sources[source[g]];
    const size_t from = (size_t) (srcEdge0[g]+(e-dstEdge0[g]));
    double2 *__restrict__ dst = reinterpret_cast<double2 *>(dstPoints)+p;
    const double *__restrict__ piece = src.points+8*from+2*part;
    *dst = make_double2(piece[0], piece[1]);
    if (part == 0)
        dstTypes[e] = src.types[from];
    else if (part == 1)
        dstColors[e] = src.colors[from];
}

// Lanes are 16-byte halves of the result's bounds rows (l, b | r, t), copied from the row of the glyph's source. 256 threads; grid = ceil(2*nGlyphs/256).
template <int WAVE_ = 64>
__global__ void __launch_bounds__(256) k_gather_bounds(double *__restrict__ dstBounds, int nGlyphs, const int32_t *__restrict__ source,
                                                       const int32_t *__restrict__ srcGlyph, const GatherSourceArrays *__restrict__ sources) {
    const long long p = (long long) blockIdx.x*256+threadIdx.x;
    if (p >= 2ll*nGlyphs)
        return;
    const int g = (int) (p>>1);
    const double *__restrict__ row = sources[source[g]].bounds+4*(size_t) srcGlyph[g]+2*(p&1);
    reinterpret_cast<double2 *>(dstBounds)[p] = make_double2(row[0], row[1]);
}

} // namespace msdfhip
