// TEST TOOLING ONLY -- the box helpers of msdf_frame.hpp (mitersGlyphWave on top of boundsGlyphWave, boxGlyph, planBox) compiled for the host with g++ and
// run over one glyph at a time with a wave context whose 64 lanes take turns between sync points, so that tests/test_box_host.py can check them against the
// compiled reference and its recorded bounds without a GPU. Never loaded by the msdfgen_amd package.
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

// Shape::getBounds(border, miterLimit, polarity) of one glyph (nC contours, offsets co) the way k_box takes it: the plain bounds from the edges, or with
// plain4 != NULL those (a batch prepared from raw outlines), then the miters over the edges. out4 = l, b, r, t.
void miters_host(int nC, const int32_t *co, double *points, uint8_t *types, uint8_t *colors, const double *plain4, double border, double miterLimit, int polarity,
                 double *out4) {
    EdgeArrays edges = { points, types, colors };
    double part[4*PREP_WAVE], run[4];
    const BoundsScratch s = { part, run };
    if (plain4)
        for (int k = 0; k < 4; ++k)
            run[k] = plain4[k];
    else
        boundsGlyphWave(HostWave(), edges, co, 0, nC, s);
    mitersGlyphWave(HostWave(), edges, co, 0, nC, border, miterLimit, polarity, s);
    for (int k = 0; k < 4; ++k)
        out4[k] = run[k];
}

// planBox; returns its status (0: the config is good). out4 = s, lo, hi, border.
int plan_box_host(double scale, int rangeMode, double lower, double upper, int alignX, int alignY, double *out4) {
    BoxParams p = { 0., 0., 0., 0, 0 };
    double border = 0;
    const int status = planBox(scale, rangeMode, lower, upper, alignX, alignY, &p, &border);
    out4[0] = p.s, out4[1] = p.lo, out4[2] = p.hi, out4[3] = border;
    return status;
}

// boxGlyph for the parameters planBox makes of a good config.
void box_host(double s, double lo, double hi, int alignX, int alignY, const double *plain4, const double *ext4, int32_t *wh2, double *xf6) {
    const BoxParams p = { s, lo, hi, alignX, alignY };
    boxGlyph(p, plain4, ext4, wh2, xf6);
}

} // extern "C"
