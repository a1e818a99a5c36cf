// msdf_groupplan.hpp -- which queued single-shape calls one leader of the micro-batcher takes into its group, and how a group of bitmaps of different sizes
// is laid out: decided on the host over plain integers. Host code only (no HIP): msdf_capi.hip includes it, and tests/groupplan_host compiles it with the
// host compiler (tests/test_group_plan_host.py). The one function the device shares with the host (boxChunk, the index arithmetic of k_boxes_to_slots) is
// marked for both where a HIP compiler reads this file.
//
// A group of different sizes runs as ONE sized call (msdf_sizedplan.hpp): its launches are those of a W x H call, W = max w_g, H = max h_g, and every
// intermediate buffer keeps slots of W*H texels. What travels over PCIe stays packed: call g's result (and, for the in-place operations, its input) is
// [h_g][w_g][N] at a float offset of its own, every offset a multiple of 4 floats so that both ends of a 16-byte copy are aligned.

#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "msdf_sizedplan.hpp"

#if defined(__HIPCC__)
#define MSDF_GROUPPLAN_HD __host__ __device__ inline
#else
#define MSDF_GROUPPLAN_HD inline
#endif

namespace msdfhip {

enum SingleOp { OP_GENERATE = 0, OP_ERROR_CORRECTION = 1, OP_SIGN_CORRECTION = 2, OP_RASTERIZE = 3, OP_GENERATE_LEGACY = 4 };   // what a single-shape call does to its bitmap

// What decides whether two calls can share a launch sequence. cfg: the call's whole MsdfHipConfig, compared as bytes.
struct GroupKey {
    int mode, channels, op, w, h;
    const void *cfg;
    size_t cfgBytes;
};

// An operation whose group may hold bitmaps of different sizes. The legacy generators correct along the shape's rows, and that correction has no sized twin.
inline bool groupOpTakesSizes(int op) {
    return op != OP_GENERATE_LEGACY;
}

// Two calls may share a group: everything that is a launch parameter agrees -- for the operations with sized kernels, everything but the size.
inline bool groupCompatible(const GroupKey &a, const GroupKey &b) {
    if (a.mode != b.mode || a.channels != b.channels || a.op != b.op || a.cfgBytes != b.cfgBytes || memcmp(a.cfg, b.cfg, a.cfgBytes) != 0)
        return false;
    return groupOpTakesSizes(a.op) || (a.w == b.w && a.h == b.h);
}

struct GroupSelection {
    int n, W, H;                      // the calls taken; their largest width and largest height (not necessarily of one call)
    size_t slot, boxTexels;           // W*H; sum of w*h of the taken calls
    bool uniform;                     // all taken sizes are equal: the group runs as it always has, without sizes
};

// The leader's walk over the compatible queued calls in arrival order, the leader first. sizes: int32[nCalls*2] = w, h, each >= 1 (singleShape returns
// before it queues an empty bitmap). Call 0 is always taken. A later call is taken iff, with it included (n' calls, W' x H' the maxima, boxTexels' the sum,
// minBox' the smallest w*h),
//     n' <= cap,
//     n'*W'*H'*channels*4 <= byteLimit      (intermediate fields and candidate indices are slots of W*H: the padded size is what the arena pays),
//     n'*W'*H' <= maxPad*boxTexels'         (the group as a whole; compared as fp64: both integers converted, the product rounded once; exact below 2^53,
//                                            i.e. wherever the byte limit is a real one),
//     W'*H' <= maxPad*minBox'               (every member: no call sits in a slot of more than maxPad times its own box, whichever arrived first. The
//                                            bound on the whole group alone depends on the arrival order: it admits a large leader's first small follower,
//                                            2*max <= 2*(max+min), where it refuses the same two kinds arriving the other way round. In exact arithmetic
//                                            this line implies the one above; both are kept, as stated),
// and sizedLayout accepts the n' sizes (the 32-bit texel index of the sized passes; the bound is stated there only; not asked while all sizes are equal:
// such a group runs without sizes). A call passed over stays queued.
// maxPad < 1 (also 0, also not a number): only calls of the leader's own size are taken, which is the grouping of equal sizes exactly.
// taken: uint8[nCalls], set to 1 / 0. scratch: int32[nCalls*2], the taken sizes in order on return.
inline void groupSelect(int nCalls, const int32_t *sizes, int channels, int cap, size_t byteLimit, double maxPad, uint8_t *taken, int32_t *scratch, GroupSelection &out) {
    out.n = 0, out.W = out.H = 0, out.slot = out.boxTexels = 0, out.uniform = true;
    if (nCalls <= 0)
        return;
    size_t minBox = 0;                                           // the smallest w*h taken
    const bool equalOnly = !(maxPad >= 1.);
    const size_t texelLimit = byteLimit/((size_t) (channels > 0 ? channels : 1)*sizeof(float));
    for (int i = 0; i < nCalls; ++i) {
        const int32_t w = sizes[2*(size_t) i], h = sizes[2*(size_t) i+1];
        taken[i] = 0;
        if (i > 0) {
            if (out.n >= cap)
                continue;
            if (equalOnly && (w != sizes[0] || h != sizes[1]))
                continue;
            const int W = w > out.W ? w : out.W, H = h > out.H ? h : out.H;
            const size_t slot = (size_t) W*(size_t) H, n = (size_t) out.n+1, box = out.boxTexels+(size_t) w*(size_t) h;
            if (slot > texelLimit/n)                             // n*slot <= texelLimit, by division: no product that could overflow
                continue;
            if (!equalOnly && !((double) (n*slot) <= maxPad*(double) box))   // (n*slot <= texelLimit < 2^62 here)
                continue;
            const size_t smallest = (size_t) w*(size_t) h < minBox ? (size_t) w*(size_t) h : minBox;
            if (!equalOnly && !((double) slot <= maxPad*(double) smallest))
                continue;
            scratch[2*(size_t) out.n] = w, scratch[2*(size_t) out.n+1] = h;
            if (!(out.uniform && w == sizes[0] && h == sizes[1])) {
                SizedLayout probe;
                if (sizedLayout(out.n+1, scratch, probe) != SIZED_OK)
                    continue;
            }
        } else
            scratch[0] = w, scratch[1] = h;
        taken[i] = 1;
        minBox = i == 0 || (size_t) w*(size_t) h < minBox ? (size_t) w*(size_t) h : minBox;
        out.uniform = out.uniform && w == sizes[0] && h == sizes[1];
        out.W = w > out.W ? w : out.W, out.H = h > out.H ? h : out.H;
        out.boxTexels += (size_t) w*(size_t) h;
        ++out.n;
    }
    out.slot = (size_t) out.W*(size_t) out.H;
}

// The packed placement of a group's tiles in the result region and, for the in-place operations, of its bitmaps in the input region (the two are laid out
// alike): call g at the float offset sum_{k<g} roundUp4(w_k*h_k*channels), rows of w_g*channels floats. offsets: int64[n+1]; offsets[n] = the floats of
// the whole region, itself a multiple of 4.
inline void groupPackedOffsets(int n, const int32_t *sizes, int channels, int64_t *offsets) {
    int64_t at = 0;
    for (int g = 0; g < n; ++g) {
        offsets[g] = at;
        at += ((int64_t) sizes[2*(size_t) g]*sizes[2*(size_t) g+1]*channels+3)&~(int64_t) 3;
    }
    offsets[n > 0 ? n : 0] = at;
}

// k_boxes_to_slots: lane `chunk` of box g copies up to four floats of the box's packed field to the start of slot g. -> the number of floats the lane copies
// (4; 1..3 for the last chunk of a box whose float count is no multiple of 4; 0 beyond the box), from src to dst (float indices).
// packedOffset is a multiple of 4 (groupPackedOffsets), so the source of a full chunk is 16-byte aligned wherever the region is; the destination is only
// where g*slotFloats is a multiple of 4 as well.
MSDF_GROUPPLAN_HD int boxChunk(int w, int h, int channels, long long packedOffset, long long slotFloats, int g, long long chunk, long long &src, long long &dst) {
    const long long floats = (long long) w*h*channels, first = 4*chunk;
    if (first >= floats)
        return 0;
    src = packedOffset+first, dst = (long long) g*slotFloats+first;
    return floats-first < 4 ? (int) (floats-first) : 4;
}

} // namespace msdfhip
