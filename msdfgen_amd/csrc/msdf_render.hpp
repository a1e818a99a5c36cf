// msdf_render.hpp -- one output texel of renderSDF (core/render-sdf.cpp:15-170): the body that k_render_sdf and k_render_sdf_sized
// (msdf_kernels.hpp) run per thread, also compilable for the host (tests/sized_quality_host runs it against the oracle without a device).
#pragma once

#include "msdf_ec.hpp"

namespace msdfhip {

// out[0..NO-1] = texel (x, y) of the rendering of the sw x sh field px (row-major [sh][sw][NS], memory rows: the reference does not reorient).
// scaleX, scaleY = sdf size / output size (render-sdf.cpp:16). threshold != 0: sdfPxRange.lower == upper (binary output, :17-24); else mapScale /
// mapTranslate = DistanceMapping::inverse of the range scaled to the output size and sdBias = .5f - sdThreshold (:26-28), all computed by the host
// (msdf_qualityplan.hpp: renderMapping). Channel pairs NO <- NS as the reference's overloads: 1<-1, 3<-1, 1<-3, 3<-3, 1<-4, 4<-4.
template <int NO, int NS>
MSDF_HD void renderSdfTexel(float *o, const float *px, int sw, int sh, int x, int y, double scaleX, double scaleY, int threshold, double mapScale,
                            double mapTranslate, float sdThreshold, float sdBias) {
    V2 pos = mk(scaleX*(x+.5), scaleY*(y+.5));                  // scale*Point2(x+.5, y+.5)
    pos.x = clampd(pos.x, (double) sw);                         // interpolate, bitmap-interpolation.hpp:10-25
    pos.y = clampd(pos.y, (double) sh);
    pos.x -= .5, pos.y -= .5;
    int l = (int) floor(pos.x), b = (int) floor(pos.y);
    int r = l+1, t = b+1;
    const double lr = pos.x-l, bt = pos.y-b;
    l = clampi(l, sw-1), r = clampi(r, sw-1);
    b = clampi(b, sh-1), t = clampi(t, sh-1);
    float sd[NS];
    for (int c = 0; c < NS; ++c)
        sd[c] = mixf(mixf(px[((size_t) b*sw+l)*NS+c], px[((size_t) b*sw+r)*NS+c], lr), mixf(px[((size_t) t*sw+l)*NS+c], px[((size_t) t*sw+r)*NS+c], lr), bt);
    float in[NO];
    if (NO == 1 && NS >= 3)
        in[0] = medianf(sd[0], sd[NS >= 3 ? 1 : 0], sd[NS >= 3 ? 2 : 0]);
    else
        for (int c = 0; c < NO; ++c)
            in[c] = sd[c < NS ? c : 0];
    for (int c = 0; c < NO; ++c) {
        if (threshold)
            o[c] = (float) (in[c] >= sdThreshold);
        else {                                                  // distVal, render-sdf.cpp:11-13
            const double v = mapScale*((double) (in[c]+sdBias)+mapTranslate)+.5;
            o[c] = (float) (v >= 0 && v <= 1 ? v : (double) (v > 0));
        }
    }
}

} // namespace msdfhip
