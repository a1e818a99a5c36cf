// msdf_frame.hpp -- framing on the device: Shape::getBounds (core/Shape.cpp:104-115) of a normalized glyph and the reference CLI's -autoframe
// (main.cpp:1153-1183) from those bounds, so that a caller hands over outlines and a tile size and never walks the geometry on the host.
//
// The bounds are taken where the CLI takes them: after Shape::normalize (main.cpp:1125-1132), before the colouring (which moves no point, but may split a
// short teardrop contour into thirds -- the extrema of the parts do not round like those of the whole edge, so the coloured arrays are NOT the input).
// One wavefront per glyph, lanes = edges (boundsGlyphWave, k_frame); lane 0 then frames the glyph (frameGlyph) and writes xf[0..5] of its MsdfHipGlyph.
// All arithmetic is the reference's, operation for operation (fp64, no contraction, division stays division).
#pragma once

#include "msdf_shapeprep.hpp"

namespace msdfhip {

// MsdfHipFrameConfig as checked by the host (checkFrameConfig in msdf_capi.hip).
struct FrameParams {
    int rangeMode;                // 0 unit range (-range / -arange), 1 pixel range (-pxrange / -apxrange)
    int scaleSpecified;           // 0: autoframe picks the scale, 1: centre the glyph at (sx, sy)
    double lower, upper;          // the range's ends
    double sx, sy;
};

// The frame of main.cpp:1155-1161 -- (width, height), plus 2*pxRange.lower for a pixel range without a given scale. A frame that is not positive in both
// directions is the CLI's "Cannot fit the specified pixel range." (main.cpp:1164-1165); it depends on nothing per glyph, so the host refuses it up front.
MSDF_HD V2 frameExtent(const FrameParams &f, int width, int height) {
    V2 frame = mk((double) width, (double) height);
    if (!f.scaleSpecified && f.rangeMode == 1)
        frame = frame+mk(2*f.lower, 2*f.lower);
    return frame;
}

// main.cpp:1153-1183 with autoFrame set, then SDFTransformation(Projection(scale, translate), range) (main.cpp:1218, DistanceMapping.cpp:13).
// bounds: l, b, r, t of Shape::getBounds. xf: sx, sy, tx, ty, mapScale, mapTranslate.
MSDF_HD void frameGlyph(const FrameParams &f, int width, int height, const double *bounds, double *xf) {
    double l = bounds[0], b = bounds[1], r = bounds[2], t = bounds[3];
    const V2 frame = frameExtent(f, width, height);
    if (!f.scaleSpecified && f.rangeMode == 0)
        l += f.lower, b += f.lower, r -= f.lower, t -= f.lower;
    if (l >= r || b >= t)                                                             // also an empty glyph: its bounds stay at +-1e240
        l = 0, b = 0, r = 1, t = 1;
    const V2 dims = mk(r-l, t-b);
    V2 scale = mk(f.sx, f.sy), translate;
    if (f.scaleSpecified)
        translate = mk(.5*(frame.x/scale.x-dims.x)-l, .5*(frame.y/scale.y-dims.y)-b);
    else {
        if (dims.x*frame.y < dims.y*frame.x) {
            translate = mk(.5*(frame.x/frame.y*dims.y-dims.x)-l, -b);
            scale.x = scale.y = frame.y/dims.y;
        } else {
            translate = mk(-l, .5*(frame.y/frame.x*dims.x-dims.y)-b);
            scale.x = scale.y = frame.x/dims.x;
        }
    }
    if (f.rangeMode == 1 && !f.scaleSpecified)
        translate = mk(translate.x-f.lower/scale.x, translate.y-f.lower/scale.y);
    double lower = f.lower, upper = f.upper;
    if (f.rangeMode == 1) {                                                           // range = pxRange/min(scale.x, scale.y); min: arithmetics.hpp:10-13
        const double m = scale.y < scale.x ? scale.y : scale.x;
        lower = f.lower/m, upper = f.upper/m;
    }
    xf[0] = scale.x, xf[1] = scale.y, xf[2] = translate.x, xf[3] = translate.y;
    xf[4] = 1/(upper-lower), xf[5] = -lower;
}

// Memory the wavefront shares: the lanes' bounds of one pass, and the glyph's running bounds.
struct BoundsScratch {
    double *part;                 // [4*64]: l, b, r, t per lane
    double *run;                  // [4]
};

// Shape::getBounds of the glyph whose contours are [c0, c1) (offsets co into `norm`), lanes = edges, 64 edges per pass. pointBounds (edge-segments.cpp:405-410)
// compares strictly, so what the reference's walk over the edges leaves in l is the FIRST point in its order that is smaller than everything before it: a
// NaN never enters, and of a +0 and a -0 the earlier one stays. Strict comparisons over the same order give the same doubles: a lane folds its edge from
// +-1e240 (edgeBound), lanes 0..3 then fold the 64 lanes' l / b / r / t in lane order into the running value, pass after pass -- edge order throughout.
// The result is in s.run for every lane once this returns.
template <class Ctx>
MSDF_HD void boundsGlyphWave(const Ctx &ctx, const EdgeArrays &norm, const int32_t *co, int c0, int c1, const BoundsScratch &s) {
    const int e0 = co[c0], e1 = co[c1];
    ctx.leader([&]() { s.run[0] = s.run[1] = 1e240, s.run[2] = s.run[3] = -1e240; });  // Shape::getBounds' LARGE_VALUE
    ctx.sync();
    for (int base = e0; base < e1; base += PREP_WAVE) {
        ctx.lanes([&](int lane) {
            V2 lo = mk(1e240, 1e240), hi = mk(-1e240, -1e240);
            if (base+lane < e1)
                edgeBound(loadEdge(norm, base+lane), lo, hi);
            s.part[4*lane] = lo.x, s.part[4*lane+1] = lo.y, s.part[4*lane+2] = hi.x, s.part[4*lane+3] = hi.y;
        });
        ctx.sync();
        ctx.lanes([&](int lane) {
            if (lane < 4) {
                double v = s.run[lane];
                for (int k = 0; k < PREP_WAVE; ++k) {
                    const double p = s.part[4*k+lane];
                    if (lane < 2 ? p < v : p > v)
                        v = p;
                }
                s.run[lane] = v;
            }
        });
        ctx.sync();
    }
}

} // namespace msdfhip
