// msdf_sizedplan.hpp -- the per-glyph box sizes of msdfhip_batch_generate_sized / msdfhip_tiles_to_bytes_sized, validated and laid out on the host over
// plain integers. Host code only (no HIP): msdf_capi.hip includes it, and tests/sizedplan_host compiles it with the host compiler
// (tests/test_sized_plan_host.py).
//
// sizes: int32[nGlyphs*2] = w_g, h_g, each >= 1. The launches of a sized call keep the shape of a uniform call at W x H = (max w_g) x (max h_g), and every
// per-glyph intermediate buffer keeps SLOTS of W*H texels: glyph g's field is packed [h_g][w_g][N] at the start of slot g.

#pragma once

#include <cstddef>
#include <cstdint>

namespace msdfhip {

enum { SIZED_OK = 0, SIZED_NO_SIZES, SIZED_BAD_BOX, SIZED_TOO_MANY_TEXELS };

struct SizedLayout {
    int W, H;                         // the largest width and the largest height of the batch (not necessarily of one glyph); 0, 0 for no glyphs
    size_t slot;                      // W*H texels
    size_t boxTexels;                 // sum of w_g*h_g: the share boxTexels / (nGlyphs*slot) of the padded grid is real work
    int badGlyph;                     // SIZED_BAD_BOX: the first glyph whose box is not at least 1 x 1
};

// The bound of the launch planners on nGlyphs*W*H (msdf_launchplan.hpp: planCorrection refuses what its 32-bit texel index cannot hold; the candidate
// records of a sized call index slots the same way in every mode).
const size_t SIZED_MAX_SLOT_TEXELS = 0xffffffffull;

inline int sizedLayout(int nGlyphs, const int32_t *sizes, SizedLayout &out) {
    out.W = out.H = 0, out.slot = out.boxTexels = 0, out.badGlyph = -1;
    if (nGlyphs <= 0)
        return SIZED_OK;
    if (!sizes)
        return SIZED_NO_SIZES;
    for (int g = 0; g < nGlyphs; ++g) {
        const int32_t w = sizes[2*(size_t) g], h = sizes[2*(size_t) g+1];
        if (w < 1 || h < 1) {
            out.badGlyph = g;
            return SIZED_BAD_BOX;
        }
        out.W = w > out.W ? w : out.W, out.H = h > out.H ? h : out.H;
        out.boxTexels += (size_t) w*(size_t) h;
    }
    out.slot = (size_t) out.W*(size_t) out.H;
    // (slot < 2^62 and nGlyphs < 2^31: the comparison by division cannot overflow)
    if (out.slot >= SIZED_MAX_SLOT_TEXELS || (size_t) nGlyphs > (SIZED_MAX_SLOT_TEXELS-1)/out.slot)
        return SIZED_TOO_MANY_TEXELS;
    return SIZED_OK;
}

// The default placement of a sized call's output: tiles packed one after another, glyph g at the float offset sum_{k<g} w_k*h_k*channels (its row stride
// is w_g*channels). offsets: int64[nGlyphs+1]; offsets[nGlyphs] = the floats of the whole output.
inline void sizedPackedOffsets(int nGlyphs, const int32_t *sizes, int channels, int64_t *offsets) {
    int64_t at = 0;
    for (int g = 0; g < nGlyphs; ++g) {
        offsets[g] = at;
        at += (int64_t) sizes[2*(size_t) g]*sizes[2*(size_t) g+1]*channels;
    }
    offsets[nGlyphs > 0 ? nGlyphs : 0] = at;
}

} // namespace msdfhip
