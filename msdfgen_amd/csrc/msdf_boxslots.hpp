// msdf_boxslots.hpp -- k_boxes_to_slots: the packed bitmaps of a group of single-shape calls of different sizes (msdf_groupplan.hpp), as one upload
// brought them to the device, spread into the slots the sized passes read their source fields from. A bandwidth-bound copy inside device memory: what it
// saves is the slots' padding on PCIe, about five times the payload at a real font's fill.
//
// A template only to be instantiated where it is named (the end of msdf_capi.hip), like the kernels of msdf_gather.hpp.

#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/msdfgen_hip.h"
#include "msdf_device.hpp"
#include "msdf_groupplan.hpp"

namespace msdfhip {

// Lanes are 16-byte chunks of box blockIdx.y's packed field [h][w][N]: read at the box's packed offset (its descriptor's out_offset: the input region of an
// in-place operation is laid out like its result region, every offset a multiple of 4 floats), written to the start of slot blockIdx.y. The index arithmetic
// is boxChunk's, which the host tests check against a plain per-box copy. A workgroup beyond its box's chunks leaves after one uniform load of the box's two
// dimensions; the last chunk of a box whose float count is no multiple of 4 is copied float by float, and so is a chunk whose destination is not 16-byte
// aligned (slotFloats odd: the slots of such a group start anywhere). 256 threads; grid = (ceil(slotFloats/4/256), n).
template <int WAVE_ = 64>
__global__ void __launch_bounds__(256) k_boxes_to_slots(float *__restrict__ dstSlots, const float *__restrict__ srcPacked, const MsdfHipGlyph *__restrict__ glyphs,
                                                        const int32_t *__restrict__ dims, long long slotFloats, int channels) {
    const int g = (int) blockIdx.y;
    const int w = MSDF_UNIFORM(dims[2*g]), h = MSDF_UNIFORM(dims[2*g+1]);
    const long long firstChunk = (long long) blockIdx.x*256;
    if (4*firstChunk >= (long long) w*h*channels)
        return;
    const long long packedOffset = (long long) glyphs[g].out_offset;   // (a uniform address: a scalar load)
    long long src, dst;
    const int count = boxChunk(w, h, channels, packedOffset, slotFloats, g, firstChunk+threadIdx.x, src, dst);
    if (count == 4 && (dst&3) == 0)
        *reinterpret_cast<float4 *>(dstSlots+dst) = *reinterpret_cast<const float4 *>(srcPacked+src);
    else
        for (int k = 0; k < count; ++k)
            dstSlots[dst+k] = srcPacked[src+k];
}

} // namespace msdfhip
