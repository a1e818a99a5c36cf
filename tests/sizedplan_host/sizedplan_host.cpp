// C binding of msdfgen_amd/csrc/msdf_sizedplan.hpp for tests/test_sized_plan_host.py: the size validation and the derived quantities of
// msdfhip_batch_generate_sized, compiled with the host compiler (no HIP, no device).
#include "../../msdfgen_amd/csrc/msdf_sizedplan.hpp"

using namespace msdfhip;

extern "C" {

// out[0..5] = W, H, slot, boxTexels, badGlyph, the padded grid's texels (nGlyphs*slot; 0 when refused); returns the SIZED_* code.
int sized_layout(int nGlyphs, const int32_t *sizes, long long *out) {
    SizedLayout l;
    const int rc = sizedLayout(nGlyphs, sizes, l);
    out[0] = l.W, out[1] = l.H, out[2] = (long long) l.slot, out[3] = (long long) l.boxTexels, out[4] = l.badGlyph;
    out[5] = rc == SIZED_OK ? (long long) ((size_t) (nGlyphs > 0 ? nGlyphs : 0)*l.slot) : 0;
    return rc;
}

void sized_packed_offsets(int nGlyphs, const int32_t *sizes, int channels, int64_t *offsets) { sizedPackedOffsets(nGlyphs, sizes, channels, offsets); }

int sized_codes(int which) {
    const int codes[4] = { SIZED_OK, SIZED_NO_SIZES, SIZED_BAD_BOX, SIZED_TOO_MANY_TEXELS };
    return codes[which&3];
}

}

#if defined(SIZEDPLAN_MAIN)
// Stand-alone form for a sanitized build: walks the cases of the test once more under -fsanitize=address,undefined.
#include <cstdio>
#include <vector>
int main() {
    long long out[6];
    const int32_t boxes[] = { 1, 1, 7, 9, 24, 1, 1, 17, 24, 17 };
    if (sized_layout(5, boxes, out) != SIZED_OK || out[0] != 24 || out[1] != 17 || out[2] != 408 || out[3] != 1+63+24+17+408)
        return 1;
    int64_t off[6];
    sized_packed_offsets(5, boxes, 3, off);
    if (off[0] != 0 || off[1] != 3 || off[2] != 192 || off[5] != 3*(1+63+24+17+408))
        return 2;
    const int32_t bad[] = { 4, 4, 0, 3 };
    if (sized_layout(2, bad, out) != SIZED_BAD_BOX || out[4] != 1)
        return 3;
    if (sized_layout(2, NULL, out) != SIZED_NO_SIZES || sized_layout(0, NULL, out) != SIZED_OK)
        return 4;
    std::vector<int32_t> big(2*70000, 256);
    if (sized_layout(70000, big.data(), out) != SIZED_TOO_MANY_TEXELS)
        return 5;
    const int32_t huge[] = { 0x7fffffff, 0x7fffffff };
    if (sized_layout(1, huge, out) != SIZED_TOO_MANY_TEXELS)
        return 6;
    std::puts("ok");
    return 0;
}
#endif
