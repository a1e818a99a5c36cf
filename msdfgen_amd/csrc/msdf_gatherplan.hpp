// msdf_gatherplan.hpp -- the plan of msdfhip_batch_gather: which glyphs of which resident batches make up the new batch, validated and laid out on the
// host over plain integers. Host code only (no HIP): msdf_capi.hip includes it, and tests/gatherplan_host compiles it with the host compiler
// (tests/test_gather_plan_host.py).
//
// Glyph k of the result is glyph indices[k] of source sourceOf[k] (sourceOf == NULL: source 0). Per source the plan reads the per-glyph contour and edge
// counts; from them come, per destination glyph, where its contours and edges start in its source and in the result (exclusive prefix sums), the totals
// (in 64 bits: one glyph taken many times passes INT32_MAX long before the index arrays do) and the maxima of the SELECTION, which size LDS and the
// class plan of the result. Nothing else derives these numbers.

#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace msdfhip {

enum { GATHER_OK = 0, GATHER_NO_SOURCES, GATHER_BAD_COUNT, GATHER_NO_INDICES, GATHER_NO_SOURCE_OF, GATHER_BAD_SOURCE, GATHER_BAD_INDEX, GATHER_MIXED_DEVICES,
       GATHER_TOO_MANY_CONTOURS, GATHER_TOO_MANY_EDGES };

struct GatherSource {
    int nGlyphs, device;
    const int *contours, *edges;      // per glyph; read by gatherTotals and gatherFill only (gatherCheckArgs needs none: a batch of device arrays fetches them on first need)
};

struct GatherRefusal {
    int position;                     // BAD_SOURCE, BAD_INDEX, TOO_MANY_*: the destination glyph k; MIXED_DEVICES: the source; else -1
    long long value;                  // BAD_SOURCE: sourceOf[k]; BAD_INDEX: indices[k]; MIXED_DEVICES: that source's device; TOO_MANY_*: the total up to and including k
    int limit;                        // BAD_SOURCE: nSources; BAD_INDEX: the glyph count of its source; MIXED_DEVICES: the device of source 0
};

struct GatherTotals {
    long long contours, edges;        // of the selection
    int maxContours, maxEdges;        // per glyph, of the selection
};

// What can be refused before any source is looked at.
inline int gatherCheckCounts(bool haveSources, int nSources, int nGlyphs, const int32_t *sourceOf, const int32_t *indices) {
    if (!haveSources || nSources < 1)
        return GATHER_NO_SOURCES;
    if (nGlyphs < 0)
        return GATHER_BAD_COUNT;
    if (nGlyphs > 0 && !indices)
        return GATHER_NO_INDICES;
    if (nSources > 1 && !sourceOf)
        return GATHER_NO_SOURCE_OF;
    return GATHER_OK;
}

// Everything that can be refused without a contour or edge count per glyph.
inline int gatherCheckArgs(const GatherSource *sources, int nSources, int nGlyphs, const int32_t *sourceOf, const int32_t *indices, GatherRefusal &bad) {
    bad.position = -1, bad.value = 0, bad.limit = 0;
    const int counts = gatherCheckCounts(sources != NULL, nSources, nGlyphs, sourceOf, indices);
    if (counts != GATHER_OK)
        return counts;
    for (int s = 1; s < nSources; ++s)
        if (sources[s].device != sources[0].device) {
            bad.position = s, bad.value = sources[s].device, bad.limit = sources[0].device;
            return GATHER_MIXED_DEVICES;
        }
    for (int k = 0; k < nGlyphs; ++k) {
        const int32_t s = sourceOf ? sourceOf[k] : 0;
        if (s < 0 || s >= nSources) {
            bad.position = k, bad.value = s, bad.limit = nSources;
            return GATHER_BAD_SOURCE;
        }
        if (indices[k] < 0 || indices[k] >= sources[s].nGlyphs) {
            bad.position = k, bad.value = indices[k], bad.limit = sources[s].nGlyphs;
            return GATHER_BAD_INDEX;
        }
    }
    return GATHER_OK;
}

// Totals and maxima of a selection that passed gatherCheckArgs. A total beyond INT32_MAX is refused at the first glyph that passes it.
inline int gatherTotals(const GatherSource *sources, int nGlyphs, const int32_t *sourceOf, const int32_t *indices, GatherTotals &out, GatherRefusal &bad) {
    out.contours = out.edges = 0, out.maxContours = out.maxEdges = 0;
    bad.position = -1, bad.value = 0, bad.limit = INT32_MAX;
    for (int k = 0; k < nGlyphs; ++k) {
        const GatherSource &src = sources[sourceOf ? sourceOf[k] : 0];
        const int c = src.contours[indices[k]], e = src.edges[indices[k]];
        out.contours += c, out.edges += e;
        if (out.contours > INT32_MAX || out.edges > INT32_MAX) {
            bad.position = k, bad.value = out.contours > INT32_MAX ? out.contours : out.edges;
            return out.contours > INT32_MAX ? GATHER_TOO_MANY_CONTOURS : GATHER_TOO_MANY_EDGES;
        }
        out.maxContours = c > out.maxContours ? c : out.maxContours;
        out.maxEdges = e > out.maxEdges ? e : out.maxEdges;
    }
    return GATHER_OK;
}

// The table the gather kernels read, as columns of one int32 block:
//     dstContour0[n+1] | (pad to a multiple of 4) | source[n] | srcGlyph[n] | srcContour0[n] | srcEdge0[n] | dstEdge0[n+1] | (pad to a multiple of 4)
// dstContour0 comes first because it IS the result's glyph_contour_offsets (closing entry included) and is uploaded into that array. The closing entry of
// dstEdge0 is the result's edge count. Every column starts at a multiple of 4 ints only where stated: the two uploads start 16-byte aligned.
struct GatherColumns {
    size_t dstContour0, source, srcGlyph, srcContour0, srcEdge0, dstEdge0, ints;   // offsets in ints; ints = the whole block
};

inline GatherColumns gatherColumns(int nGlyphs) {
    const size_t n = (size_t) (nGlyphs > 0 ? nGlyphs : 0);
    GatherColumns c;
    c.dstContour0 = 0;
    c.source = (n+1+3)&~(size_t) 3;
    c.srcGlyph = c.source+n, c.srcContour0 = c.srcGlyph+n, c.srcEdge0 = c.srcContour0+n, c.dstEdge0 = c.srcEdge0+n;
    c.ints = (c.dstEdge0+n+1+3)&~(size_t) 3;
    return c;
}

// Fills the block (gatherColumns(nGlyphs).ints ints, padding zeroed) and the per-glyph counts of the selection for a selection that passed both checks.
inline void gatherFill(const GatherSource *sources, int nSources, int nGlyphs, const int32_t *sourceOf, const int32_t *indices, int32_t *table, int *selContours,
                       int *selEdges) {
    const GatherColumns col = gatherColumns(nGlyphs);
    for (size_t i = 0; i < col.ints; ++i)
        table[i] = 0;
    // where each glyph of each source starts: exclusive prefix sums of its counts (only of sources the selection names)
    std::vector<std::vector<int32_t> > contour0((size_t) nSources), edge0((size_t) nSources);
    int32_t dstC = 0, dstE = 0;
    for (int k = 0; k < nGlyphs; ++k) {
        const int s = sourceOf ? sourceOf[k] : 0, g = indices[k];
        const GatherSource &src = sources[s];
        if (contour0[(size_t) s].empty()) {
            std::vector<int32_t> &c0 = contour0[(size_t) s], &e0 = edge0[(size_t) s];
            c0.resize((size_t) src.nGlyphs), e0.resize((size_t) src.nGlyphs);
            int32_t c = 0, e = 0;
            for (int i = 0; i < src.nGlyphs; ++i)
                c0[(size_t) i] = c, e0[(size_t) i] = e, c += src.contours[i], e += src.edges[i];
        }
        table[col.source+k] = s, table[col.srcGlyph+k] = g;
        table[col.srcContour0+k] = contour0[(size_t) s][(size_t) g], table[col.srcEdge0+k] = edge0[(size_t) s][(size_t) g];
        table[col.dstContour0+k] = dstC, table[col.dstEdge0+k] = dstE;
        selContours[k] = src.contours[g], selEdges[k] = src.edges[g];
        dstC += src.contours[g], dstE += src.edges[g];
    }
    table[col.dstContour0+(size_t) (nGlyphs > 0 ? nGlyphs : 0)] = dstC, table[col.dstEdge0+(size_t) (nGlyphs > 0 ? nGlyphs : 0)] = dstE;
}

} // namespace msdfhip
