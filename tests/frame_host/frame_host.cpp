// TEST TOOLING ONLY -- the framing helpers of msdf_frame.hpp (boundsGlyphWave over edgeBound, frameGlyph) compiled for the host with g++ and run over one
// glyph at a time with a wave context whose 64 lanes take turns between sync points, so that tests/test_frame_host.py can check them against the compiled
// reference and its CLI's recorded metrics without a GPU. Never loaded by the msdfgen_amd package.
#include <cstdint>

#include "../../msdfgen_amd/csrc/msdf_device.hpp"
#include "../../msdfgen_amd/csrc/msdf_prep.hpp"
#include "../../msdfgen_amd/csrc/msdf_scanline.hpp"
#include "../../msdfgen_amd/csrc/msdf_shapeprep.hpp"
#include "../../msdfgen_amd/csrc/msdf_frame.hpp"

using namespace msdfhip;

namespace {
struct HostWave {
    template <class F> void lanes(F f) const { for (int l = 0; l < PREP_WAVE; ++l) f(l); }
    template <class F> void leader(F f) const { f(); }
    void sync() const { }
};
}

extern "C" {

// Shape::getBounds of one normalized glyph (nC contours, offsets co): out4 = l, b, r, t.
void bounds_host(int nC, const int32_t *co, double *points, uint8_t *types, uint8_t *colors, double *out4) {
    EdgeArrays norm = { points, types, colors };
    double part[4*PREP_WAVE], run[4];
    const BoundsScratch s = { part, run };
    boundsGlyphWave(HostWave(), norm, co, 0, nC, s);
    for (int k = 0; k < 4; ++k)
        out4[k] = run[k];
}

// frameGlyph; returns 0 when the frame cannot fit (frameExtent not positive), else 1.
int frame_host(int rangeMode, int scaleSpecified, double lower, double upper, double sx, double sy, int width, int height, const double *bounds4, double *xf6) {
    const FrameParams f = { rangeMode, scaleSpecified, lower, upper, scaleSpecified ? sx : 1., scaleSpecified ? sy : 1. };
    const V2 extent = frameExtent(f, width, height);
    if (extent.x <= 0 || extent.y <= 0)
        return 0;
    frameGlyph(f, width, height, bounds4, xf6);
    return 1;
}

} // extern "C"
