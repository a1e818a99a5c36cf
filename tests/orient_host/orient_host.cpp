// TEST TOOLING ONLY -- the orientation helpers of msdf_shapeprep.hpp (orientGlyphWave, windingGlyphWave) compiled for the host with g++ and run over
// one glyph at a time with a wave context whose 64 lanes take turns between sync points, so that tests/test_cabi_prepare_orient.py can check their
// logic against the compiled reference without a GPU. Never loaded by the msdfgen_amd package.
#include <cstdint>
#include <vector>

#include "../../msdfgen_amd/csrc/msdf_device.hpp"
#include "../../msdfgen_amd/csrc/msdf_prep.hpp"
#include "../../msdfgen_amd/csrc/msdf_scanline.hpp"
#include "../../msdfgen_amd/csrc/msdf_shapeprep.hpp"

using namespace msdfhip;

namespace {
struct HostWave {
    template <class F> void lanes(F f) const { for (int l = 0; l < PREP_WAVE; ++l) f(l); }
    template <class P> unsigned long long ballot(P pred) const {
        unsigned long long m = 0;
        for (int l = 0; l < PREP_WAVE; ++l)
            if (pred(l))
                m |= 1ull<<l;
        return m;
    }
    template <class F> void leader(F f) const { f(); }
    void sync() const { }
};
}

extern "C" {

// Shape::orientContours of one glyph (nC contours, offsets co) in place. colors may be NULL. globalVotes: vote in the global array even for few contours.
void orient_host(int nC, const int32_t *co, double *points, uint8_t *types, uint8_t *colors, int globalVotes) {
    EdgeArrays raw = { points, types, colors };
    const int nE = co[nC];
    std::vector<double> x(PREP_ORIENT_LDS_HITS), bigX(3*(size_t) (nE ? nE : 1));
    std::vector<int> tag(PREP_ORIENT_LDS_HITS), bigTag(3*(size_t) (nE ? nE : 1)), lds(PREP_ORIENT_LDS_CONTOURS), votes(nC ? nC : 1);
    int count = 0;
    const OrientHits hits = { x.data(), tag.data(), bigX.data(), bigTag.data() };
    orientGlyphWave(HostWave(), raw, co, 0, nC, !globalVotes && nC <= PREP_ORIENT_LDS_CONTOURS ? lds.data() : votes.data(), &count, hits);
}

// The winding step (mode 1 reverse, 2 guess) of one normalized glyph in place; returns whether it was reversed.
int winding_host(int nC, const int32_t *co, double *points, uint8_t *types, uint8_t *colors, int mode) {
    EdgeArrays norm = { points, types, colors };
    double lo[2*PREP_WAVE], hi[2*PREP_WAVE], d[PREP_WAVE], dot[PREP_WAVE];
    int idx[PREP_WAVE];
    const WindingScratch s = { lo, hi, d, dot, idx };
    return windingGlyphWave(HostWave(), norm, co, 0, nC, mode, s) ? 1 : 0;
}

} // extern "C"
