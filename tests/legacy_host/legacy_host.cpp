// TEST TOOLING ONLY -- the legacy generators' texel function and the legacy correction's clash passes of msdf_legacy.hpp compiled for the host with g++
// and run over one bitmap at a time, so that tests/test_legacy_host.py can check them against the recorded reference (tests/golden/legacy.npz) and the
// compiled reference without a GPU. The records are built by the product's own digest (msdf_prep.hpp: prepRecord), in its own order. Never loaded by
// the msdfgen_amd package. With -DLEGACY_HOST_MAIN it is a stand-alone program (a small self-check to run under a host sanitizer).
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../msdfgen_amd/csrc/msdf_device.hpp"
#include "../../msdfgen_amd/csrc/msdf_prep.hpp"
#include "../../msdfgen_amd/csrc/msdf_legacy.hpp"
#include "../../msdfgen_amd/csrc/msdf_launchplan.hpp"

using namespace msdfhip;

namespace {

template <int MODE>
void generate(float *pixels, int w, int h, int rowStride, int flip, const std::vector<EdgeRec> &recs, const int32_t *co, int nC, const Xform &t) {
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int yn = flip ? h-1-y : y;                        // the kernel's row order (k_distance_legacy)
            legacyTexelMapped<MODE>(recs.data(), co, nC, t, x, y, pixels+(ptrdiff_t) rowStride*yn+(ptrdiff_t) LegacyTraits<MODE>::NCH*x);
        }
}

template <int N>
void correct(float *pixels, int w, int h, double tx, double ty) {
    std::vector<float> scratch((size_t) w*h*N);
    for (int pass = 0; pass < 2; ++pass) {                          // tiles -> scratch -> tiles, as launchLegacyCorrection (msdf_capi.hip)
        const float *src = pass == 0 ? pixels : scratch.data();
        float *dst = pass == 0 ? scratch.data() : pixels;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                legacyClashTexel<N>(src, dst, w, h, x, y, pass, tx, ty);
    }
}

}

extern "C" {

// generate*_legacy WITHOUT the correction that follows in modes 3, 4: mode 1..4, pixels with rowStride floats per memory row, xf6 = sx, sy, tx, ty,
// mapScale, mapTranslate. Returns 0, or -1 for a bad mode.
int legacy_generate_host(int mode, float *pixels, int w, int h, int rowStride, int flip, int nC, const int32_t *co, const double *points, const uint8_t *types,
                         const uint8_t *colors, const double *xf6) {
    const int nE = co[nC];
    std::vector<EdgeRec> recs((size_t) (nE > 0 ? nE : 1));
    for (int c = 0; c < nC; ++c)
        for (int slot = co[c]; slot < co[c+1]; ++slot)
            prepRecord(recs.data(), slot, c, co, points, types, colors);
    Xform t;
    t.sx = xf6[0], t.sy = xf6[1], t.tx = xf6[2], t.ty = xf6[3], t.mapScale = xf6[4], t.mapTranslate = xf6[5];
    switch (mode) {
        case 1: generate<1>(pixels, w, h, rowStride, flip, recs, co, nC, t); return 0;
        case 2: generate<2>(pixels, w, h, rowStride, flip, recs, co, nC, t); return 0;
        case 3: generate<3>(pixels, w, h, rowStride, flip, recs, co, nC, t); return 0;
        case 4: generate<4>(pixels, w, h, rowStride, flip, recs, co, nC, t); return 0;
    }
    return -1;
}

// msdfErrorCorrection_legacy on a packed bitmap [h][w][channels], in place. Returns 0, or -1 for channels other than 3 / 4.
int legacy_correction_host(int channels, float *pixels, int w, int h, double tx, double ty) {
    if (channels == 3)
        correct<3>(pixels, w, h, tx, ty);
    else if (channels == 4)
        correct<4>(pixels, w, h, tx, ty);
    else
        return -1;
    return 0;
}

// The launch plans of the two kernels (msdf_launchplan.hpp): out5 = distance blocks, refused (0 / 1), correction texels, scratch floats, correction blocks.
void legacy_plan_host(int nGlyphs, int w, int h, int channels, unsigned long long *out5) {
    const LegacyDistancePlan d = planLegacyDistance(nGlyphs, w, h);
    const LegacyEcPlan e = planLegacyCorrection(nGlyphs, w, h, channels);
    out5[0] = d.blocks, out5[1] = d.tooManyBlocks ? 1 : 0, out5[2] = e.texels, out5[3] = e.scratchFloats, out5[4] = e.blocks;
}

} // extern "C"

#if defined(LEGACY_HOST_MAIN)
#include <cstdio>

// A triangle with one quadratic and one cubic side, all four modes at 9 x 7, then the correction of the results: exercises every read of the walk.
int main() {
    const int32_t co[2] = { 0, 3 };
    const double points[3*8] = { 1, 1, 8, 1, 0, 0, 0, 0,   8, 1, 7, 5, 4, 6, 0, 0,   4, 6, 2, 6, 0, 4, 1, 1 };
    const uint8_t types[3] = { 1, 2, 3 }, colors[3] = { 3, 6, 5 };
    const double xf[6] = { 1, .8, 0, .5, .25, 2 };
    double sum = 0;
    for (int mode = 1; mode <= 4; ++mode) {
        const int n = mode <= 2 ? 1 : mode, w = 9, h = 7;
        std::vector<float> px((size_t) w*h*n);
        if (legacy_generate_host(mode, px.data(), w, h, w*n, mode&1, 1, co, points, types, colors, xf))
            return 1;
        if (n >= 3 && legacy_correction_host(n, px.data(), w, h, .3, .1))
            return 1;
        for (size_t i = 0; i < px.size(); ++i)
            sum += px[i];
    }
    printf("legacy_host self-check: sum %.9g\n", sum);
    return sum == sum ? 0 : 1;
}
#endif
