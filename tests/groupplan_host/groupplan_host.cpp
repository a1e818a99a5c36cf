// C binding of msdfgen_amd/csrc/msdf_groupplan.hpp for tests/test_group_plan_host.py: which queued single-shape calls a leader takes, the packed layout of
// a group of different sizes and the index arithmetic of k_boxes_to_slots, compiled with the host compiler (no HIP, no device).
#include "../../msdfgen_amd/csrc/msdf_groupplan.hpp"

#include <vector>

using namespace msdfhip;

extern "C" {

// key: int32[5] = mode, channels, op, w, h; cfg: cfgBytes bytes.
int group_compatible(const int32_t *keyA, const void *cfgA, const int32_t *keyB, const void *cfgB, unsigned long long cfgBytes) {
    const GroupKey a = { keyA[0], keyA[1], keyA[2], keyA[3], keyA[4], cfgA, (size_t) cfgBytes }, b = { keyB[0], keyB[1], keyB[2], keyB[3], keyB[4], cfgB, (size_t) cfgBytes };
    return groupCompatible(a, b) ? 1 : 0;
}

int group_op_takes_sizes(int op) { return groupOpTakesSizes(op) ? 1 : 0; }

int group_legacy_op(void) { return OP_GENERATE_LEGACY; }

// out[0..5] = n, W, H, slot, boxTexels, uniform; taken: uint8[nCalls].
void group_select(int nCalls, const int32_t *sizes, int channels, int cap, unsigned long long byteLimit, double maxPad, uint8_t *taken, long long *out) {
    std::vector<int32_t> scratch(2*(size_t) (nCalls > 0 ? nCalls : 1));
    GroupSelection s;
    groupSelect(nCalls, sizes, channels, cap, (size_t) byteLimit, maxPad, taken, scratch.data(), s);
    out[0] = s.n, out[1] = s.W, out[2] = s.H, out[3] = (long long) s.slot, out[4] = (long long) s.boxTexels, out[5] = s.uniform ? 1 : 0;
}

void group_packed_offsets(int n, const int32_t *sizes, int channels, int64_t *offsets) { groupPackedOffsets(n, sizes, channels, offsets); }

int box_chunk(int w, int h, int channels, long long packedOffset, long long slotFloats, int g, long long chunk, long long *src, long long *dst) {
    return boxChunk(w, h, channels, packedOffset, slotFloats, g, chunk, *src, *dst);
}

// k_boxes_to_slots as its grid walks it: (ceil(slotFloats/4/256), n) workgroups of 256 lanes, a workgroup beyond its box's chunks leaves, every other lane
// copies what boxChunk tells it. Every destination float is written at most once (counted in `writes`, one byte per float of dst); -> 0, or 1 + the first
// float index that is outside its region.
long long boxes_to_slots(int n, const int32_t *sizes, int channels, long long slot, const int64_t *offsets, const float *packed, long long packedFloats, float *dst,
                         uint8_t *writes) {
    const long long slotFloats = slot*channels, groupsX = ((slotFloats+3)/4+255)/256;
    for (int g = 0; g < n; ++g)
        for (long long bx = 0; bx < groupsX; ++bx) {
            const int w = sizes[2*(size_t) g], h = sizes[2*(size_t) g+1];
            if (4*bx*256 >= (long long) w*h*channels)
                continue;
            for (int lane = 0; lane < 256; ++lane) {
                long long s = 0, d = 0;
                const int count = boxChunk(w, h, channels, offsets[g], slotFloats, g, bx*256+lane, s, d);
                for (int k = 0; k < count; ++k) {
                    if (s+k < 0 || s+k >= packedFloats)
                        return 1+s+k;
                    if (d+k < 0 || d+k >= (long long) n*slotFloats)
                        return 1+d+k;
                    dst[d+k] = packed[s+k];
                    ++writes[d+k];
                }
            }
        }
    return 0;
}

}

#if defined(GROUPPLAN_MAIN)
// Stand-alone form for a sanitized build: walks the main cases of the test once more under -fsanitize=address,undefined.
#include <cstdio>
int main() {
    const int32_t boxes[] = { 1, 1, 7, 9, 8, 8, 9, 8, 8, 9, 24, 1, 1, 17, 23, 17, 16, 16, 17, 10, 24, 17 };
    uint8_t taken[11];
    long long out[6];
    group_select(11, boxes, 3, 256, 256ull<<20, 1000., taken, out);
    if (out[0] != 11 || out[1] != 24 || out[2] != 17 || out[3] != 408 || out[4] != 1538 || out[5] != 0)
        return 1;
    group_select(11, boxes, 3, 256, 256ull<<20, 0., taken, out);
    if (out[0] != 1 || out[5] != 1)
        return 2;
    const int32_t huge[] = { 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff };
    group_select(2, huge, 4, 256, ~0ull, 1000., taken, out);
    if (out[0] != 1 || taken[1])
        return 3;
    for (int channels = 1; channels <= 4; channels += channels == 1 ? 2 : 1) {
        int64_t off[12];
        group_packed_offsets(11, boxes, channels, off);
        std::vector<float> packed((size_t) off[11]), dst((size_t) 11*408*channels, -1.f);
        std::vector<uint8_t> writes(dst.size(), 0);
        for (size_t i = 0; i < packed.size(); ++i)
            packed[i] = (float) i;
        if (boxes_to_slots(11, boxes, channels, 408, off, packed.data(), off[11], dst.data(), writes.data()) != 0)
            return 4;
        for (int g = 0; g < 11; ++g)
            for (long long i = 0; i < 408*channels; ++i) {
                const bool inside = i < (long long) boxes[2*g]*boxes[2*g+1]*channels;
                const size_t at = (size_t) g*408*channels+(size_t) i;
                if (writes[at] != (inside ? 1 : 0) || (inside && dst[at] != packed[(size_t) (off[g]+i)]))
                    return 5;
            }
    }
    std::puts("ok");
    return 0;
}
#endif
