// msdf_hostplan.hpp -- the integer planning of the host-output pipeline (msdf_capi.hip: runPipelineOnce) and of the glyph-sharded entry point:
// how a glyph list is cut into chunks, where a chunk's rectangles lie in the caller's buffer and whether they tile it, how a slot's device
// buffer is laid out, which glyph range each device gets. (A streamed call's INPUT areas -- staging, preparation buffers, records -- are msdf_prepplan.hpp's.)
// Host code only (no HIP): msdf_capi.hip includes it, and tests/hostemu compiles it with the host compiler (tests/test_host_plan.py).

#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/msdfgen_hip.h"
#include "msdf_classplan.hpp"

namespace msdfhip {

struct Carver {                                                  // 256-byte aligned sub-allocation inside an arena
    size_t off;
    Carver() : off(0) { }
    size_t take(size_t bytes) { const size_t at = off; off += (bytes+255)/256*256; return at; }
};

// The automatic chunk: about 96 MB of float tiles, at least 64 glyphs, a multiple of 64.
inline int defaultChunk(size_t tileFloats) {
    int chunk = (int) ((96u<<20)/(tileFloats*sizeof(float) ? tileFloats*sizeof(float) : 1));   // measured on 8192 64x64 glyphs: 512 / 1024 / 2048 / 4096 glyphs per chunk -> 18.6 / 14.6 / 12.7 / 14.7 ms
    return chunk < 64 ? 64 : chunk/64*64;
}

// Chunk lengths: what the pipeline cannot hide is the kernels (streamed calls: also flatten + upload + digest) of the FIRST chunk and the kernels' tail +
// copy of the LAST ones. Round 5 swept the schedule on the streamed end-to-end path (profiles/r05_ab_notes.md, tools/r05_call3.sh; 8 192 glyphs at 64x64):
//   float tiles (copy bound: 403 MB at the link's 57 GB/s are 7.4 ms, the kernels 5.7): HALF chunks with a quarter chunk in front -- the copy engine starts
//     after 512 glyphs' kernels and never waits again: 512, 1 024 x 7, 512 -> 9.29 ms against 10.0-10.2 for 1 024, 2 048 x 3, 1 024;
//   8-bit atlas (kernel bound, a quarter of the bytes): full chunks keep the device fuller; 3/8 of a chunk in front, the remainder in two falling pieces
//     (768, 2 048 x 3, 768, 512 -> 7.25-7.30 ms against 7.34-7.38).
// `chunk` is what every slot holds (clamped to the list's length here as by the caller that sizes the slots): no piece is longer.
inline std::vector<int> chunkSchedule(int nG, int chunk, bool floatOutput) {
    std::vector<int> lengths;
    if (chunk > nG)
        chunk = nG;
    int rem = nG;
    const int unit = floatOutput ? (chunk/2 >= 64 ? chunk/2/64*64 : chunk) : chunk;     // the schedule's full chunk (the slots are sized for `chunk` either way)
    const int first = floatOutput ? (unit/2 >= 64 ? unit/2/64*64 : unit) : (unit*3/8 >= 64 ? unit*3/8/64*64 : unit);
    if (nG >= 2*chunk && first < unit) {
        lengths.push_back(first);
        for (rem -= first; rem > unit+unit/2; rem -= unit)
            lengths.push_back(unit);
        if (!floatOutput && rem > unit/2) {                      // (8-bit) the tail in two falling pieces
            const int a = (rem*3/5+63)/64*64 < rem ? (rem*3/5+63)/64*64 : rem;
            lengths.push_back(a), rem -= a;
        } else if (floatOutput && rem > unit)
            lengths.push_back(unit), rem -= unit;
    } else
        for (; rem > chunk; rem -= chunk)
            lengths.push_back(chunk);
    if (rem > 0)
        lengths.push_back(rem);
    // Every slot (device tiles, descriptors, pinned staging) holds `chunk` glyphs. The schedule's rounded pieces can exceed that when `chunk` is not a
    // multiple of 64 (msdfhip_set_pipeline_chunk(171), 450 glyphs: 64, 171, 192, 23 -- ADVICE r5): an oversized piece is cut, the cut-off part follows it.
    for (size_t i = 0; i < lengths.size(); ++i)
        if (lengths[i] > chunk) {
            lengths.insert(lengths.begin()+(ptrdiff_t) i+1, lengths[i]-chunk);
            lengths[i] = chunk;
        }
    return lengths;
}

// The elements [lo, hi) of the caller's buffer between the first and the last texel of a glyph's w x h rectangle of N channels.
struct RectSpan { long long lo, hi; };
inline RectSpan rectSpan(const MsdfHipGlyph &glyph, int w, int h, int N) {
    const long long o = glyph.out_offset, rs = glyph.row_stride;
    const RectSpan s = { rs >= 0 ? o : o+rs*(h-1), (rs >= 0 ? o+rs*(h-1) : o)+(long long) w*N };
    return s;
}

// dense: the chunk's rectangles exactly tile one contiguous range of the caller's buffer, starting at spanLo (tiles packed in glyph order; whole
// row bands of an atlas) -> the device writes that range in the caller's layout and it goes back as ONE copy.
struct ChunkSpan { long long spanLo; bool dense; };
inline ChunkSpan chunkSpan(const MsdfHipGlyph *glyphs, int n, int w, int h, int N) {
    const size_t tile = (size_t) w*h*N;
    long long spanLo = glyphs[0].out_offset, spanHi = spanLo;
    bool dense = true;
    for (int g = 0; g < n; ++g) {
        dense = dense && glyphs[g].row_stride >= (long long) w*N;
        const RectSpan r = rectSpan(glyphs[g], w, h, N);
        spanLo = r.lo < spanLo ? r.lo : spanLo, spanHi = r.hi > spanHi ? r.hi : spanHi;
    }
    dense = dense && (unsigned long long) (spanHi-spanLo) == (unsigned long long) n*tile;
    // Equal area is an exact tiling only if the rectangles are DISJOINT (two glyphs on one cell + a free cell elsewhere have the same
    // area: the free cell would come back as whatever the device buffer held). Accept the two layouts that make it so by construction:
    // packed tiles in glyph order, or the cells of a grid whose pitch is the common row stride, each used once.
    if (dense) {
        bool packed = true;
        for (int g = 0; g < n && packed; ++g)
            packed = glyphs[g].row_stride == (int64_t) w*N && glyphs[g].out_offset == spanLo+(long long) g*(long long) tile;
        if (!packed) {
            const long long pitch = glyphs[0].row_stride, cellW = (long long) w*N;
            bool grid = pitch > 0 && pitch%cellW == 0 && (long long) n%(pitch/cellW) == 0;
            std::vector<bool> used(grid ? (size_t) n : 0, false);
            for (int g = 0; g < n && grid; ++g) {
                const long long rel = glyphs[g].out_offset-spanLo;
                const long long row = rel/pitch, col = rel%pitch;
                grid = glyphs[g].row_stride == pitch && row%h == 0 && col%cellW == 0;
                if (grid) {
                    const size_t cell = (size_t) ((row/h)*(pitch/cellW)+col/cellW);
                    grid = cell < used.size() && !used[cell];
                    if (grid)
                        used[cell] = true;
                }
            }
            dense = grid;
        }
    }
    const ChunkSpan s = { spanLo, dense };
    return s;
}

// A pipeline slot's device buffer: [descriptors of the generators, of the byte conversion | float tiles | stencil | byte tiles], for `chunk` glyphs.
struct SlotLayout { size_t offGlyphs, offTiles, offStencil, offBytes, devBytes; };
inline SlotLayout slotLayout(int chunk, size_t tileFloats, size_t texels, bool wantStencil, bool bytesOutput) {
    SlotLayout l;
    l.offGlyphs = 0, l.offTiles = (2*(size_t) chunk*sizeof(MsdfHipGlyph)+255)/256*256;
    const size_t tilesBytes = ((size_t) chunk*tileFloats*sizeof(float)+255)/256*256;
    l.offStencil = l.offTiles+tilesBytes;
    const size_t stencilBytes = wantStencil ? ((size_t) chunk*texels+255)/256*256 : 0;
    l.offBytes = l.offStencil+stencilBytes, l.devBytes = l.offBytes+(bytesOutput ? (size_t) chunk*tileFloats : 0)+256;
    return l;
}

// glyphs are independent, so a glyph list is cut into contiguous ranges of equal modelled cost (glyphCost), one range per device:
// device k gets the glyphs [bounds[k], bounds[k+1]).
inline void shardRanges(const int32_t *gco, const int32_t *co, int nGlyphs, int parts, std::vector<int> &bounds) {
    bounds.assign((size_t) parts+1, nGlyphs);
    bounds[0] = 0;
    double total = 0;
    for (int g = 0; g < nGlyphs; ++g)
        total += glyphCost(gco[g+1]-gco[g], co[gco[g+1]]-co[gco[g]]);
    double acc = 0;
    int part = 1;
    for (int g = 0; g < nGlyphs && part < parts; ++g) {
        acc += glyphCost(gco[g+1]-gco[g], co[gco[g+1]]-co[gco[g]]);
        while (part < parts && acc >= total*part/parts)
            bounds[part++] = g+1;
    }
}

} // namespace msdfhip
