// msdf_frame.hpp -- framing on the device: Shape::getBounds (core/Shape.cpp:104-115) of a normalized glyph and the reference CLI's -autoframe
// (main.cpp:1153-1183) from those bounds, so that a caller hands over outlines and a tile size and never walks the geometry on the host.
//
// The bounds are taken where the CLI takes them: after Shape::normalize (main.cpp:1125-1132), before the colouring (which moves no point, but may split a
// short teardrop contour into thirds -- the extrema of the parts do not round like those of the whole edge, so the coloured arrays are NOT the input).
// One wavefront per glyph, lanes = edges (boundsGlyphWave, k_frame); lane 0 then frames the glyph (frameGlyph) and writes xf[0..5] of its MsdfHipGlyph.
// All arithmetic is the reference's, operation for operation (fp64, no contraction, division stays division).
// Further down: Shape::getBounds(border, miterLimit, polarity) and the box sizes of a packed atlas from it (mitersGlyphWave, boxGlyph, k_box).
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

// ------------------------------------------------------------------------------------------------------ box sizes (k_box)
//
// Shape::getBounds(border, miterLimit, polarity) (core/Shape.cpp:104-115) and, from it, the box an atlas generator gives the glyph at one common scale:
// its size in texels and the transformation that puts the glyph into it. Two parts, and which arrays each reads:
//   the plain bounds   those of msdfhip_batch_bounds: of the arrays the batch holds, or -- a batch prepared from raw outlines -- the ones fixed after its
//                      normalize, before the colouring (boundsFixed);
//   the miters         Shape::boundMiters (core/Shape.cpp:99-102, core/Contour.cpp:39-55) over the edges the batch HOLDS: for such a batch the oriented,
//                      coloured edges.
// Together that is what a caller gets who keeps getBounds() from load time and calls boundMiters on the shape it is about to render; for a batch made from
// prepared arrays it is exactly getBounds(border, miterLimit, polarity) of those arrays.

// Shape::boundMiters of the glyph whose contours are [c0, c1) (offsets co into `edges`) on top of its plain bounds: s.run holds l, b, r, t of Shape::getBounds
// when this is called (visible to every lane) and the bounds with border and miters when it returns. The reference's gates stay (Shape.cpp:108-113): nothing
// changes unless border > 0, no join is visited unless also miterLimit > 0. Lanes = joins, 64 per pass: lane i takes its own edge and the cyclic previous
// edge of the same contour -- a contour's first edge pairs with its last, which may lie in a later pass or be the edge itself -- and computes the miter point
// operation for operation as Contour.cpp:42-53. boundPoint (Contour.cpp:27-32) compares strictly like pointBounds, so the fold is boundsGlyphWave's: lanes
// 0..3 fold the 64 points' x / y / x / y in lane order into the running value, pass after pass, which is contour order, then edge order. A join that fails
// the polarity test contributes +-infinity, which no strict comparison lets in.
template <class Ctx>
MSDF_HD void mitersGlyphWave(const Ctx &ctx, const EdgeArrays &edges, const int32_t *co, int c0, int c1, double border, double miterLimit, int polarity,
                             const BoundsScratch &s) {
    if (!(border > 0))
        return;
    ctx.leader([&]() { s.run[0] -= border, s.run[1] -= border, s.run[2] += border, s.run[3] += border; });
    ctx.sync();
    if (!(miterLimit > 0))
        return;
    const int e0 = co[c0], e1 = co[c1];
    for (int base = e0; base < e1; base += PREP_WAVE) {
        ctx.lanes([&](int lane) {
            const double inf = __builtin_huge_val();
            V2 lo = mk(inf, inf), hi = mk(-inf, -inf);
            const int e = base+lane;
            if (e < e1) {
                int a = c0, b = c1-1;                                                 // the contour of e: the first c with co[c+1] > e (empty contours fall out)
                while (a < b) {
                    const int m = (a+b)/2;
                    if (co[m+1] > e) b = m; else a = m+1;
                }
                const PrepEdge edge = loadEdge(edges, e);
                const PrepEdge prev = e == co[a] ? loadEdge(edges, co[a+1]-1) : loadEdge(edges, e-1);
                const V2 prevDir = normalize(edgeDirection(prev, 1), true);
                const V2 dir = -normalize(edgeDirection(edge, 0), true);
                if ((double) polarity*cross(prevDir, dir) >= 0) {
                    double miterLength = miterLimit;
                    const double q = .5*(1-dot(prevDir, dir));
                    if (q > 0) {
                        const double m = 1/sqrt(q);
                        miterLength = miterLimit < m ? miterLimit : m;                // min(1/sqrt(q), miterLimit), arithmetics.hpp:10-13
                    }
                    lo = hi = edgePoint(edge, 0)+(border*miterLength)*normalize(prevDir+dir, true);
                }
            }
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

// MsdfHipBoxConfig as checked by the host (checkBoxConfig in msdf_capi.hip). lo, hi: the distance range in shape units (a pixel range divided by s).
struct BoxParams {
    double s;                     // texels per shape unit, both axes
    double lo, hi;
    int alignX, alignY;           // put the shape's origin on a texel corner along that axis
};

enum { BOX_MAX_SIDE = 1 << 30 };  // a side beyond it (or a NaN one) is stored as -1: the host answers MSDFHIP_ERR_INVALID

// The fields of an MsdfHipBoxConfig, checked on the host before the device is touched (checkBoxConfig): BOX_CONFIG_OK, or the first bad field.
// out: the kernel's parameters; *border = -lo, the border of Shape::getBounds that keeps the whole distance range inside the box.
enum { BOX_CONFIG_OK = 0, BOX_CONFIG_SCALE, BOX_CONFIG_RANGE_MODE, BOX_CONFIG_RANGE, BOX_CONFIG_ALIGN };

inline int planBox(double scale, int rangeMode, double lower, double upper, int alignX, int alignY, BoxParams *out, double *border) {
    const double finite = scale-scale+(lower-lower)+(upper-upper);                    // 0, or NaN when one of them is infinite or NaN
    if (!(scale > 0 && scale-scale == 0))
        return BOX_CONFIG_SCALE;
    if (rangeMode < 0 || rangeMode > 1)
        return BOX_CONFIG_RANGE_MODE;
    if (!(finite == 0 && lower < upper && lower <= 0))
        return BOX_CONFIG_RANGE;
    if (alignX < 0 || alignX > 1 || alignY < 0 || alignY > 1)
        return BOX_CONFIG_ALIGN;
    out->s = scale;
    out->lo = rangeMode == 1 ? lower/scale : lower, out->hi = rangeMode == 1 ? upper/scale : upper;
    out->alignX = alignX, out->alignY = alignY;
    const double width = out->hi-out->lo;
    if (!(width > 0 && width-width == 0))                                             // (a pixel range over a scale so small that the division overflows)
        return BOX_CONFIG_RANGE;
    *border = -out->lo;
    return BOX_CONFIG_OK;
}

// One axis of the box: the extended bounds [l, r] at scale s -> the side in texels (as a double, not yet checked) and the translation.
//   aligned    the texel grid passes through the shape's origin: the box runs from floor(s*l - .5) to ceil(s*r + .5)
//   otherwise  the glyph is centred in ceil(s*(r-l)) + 1 texels
MSDF_HD void boxAxis(double s, double l, double r, int aligned, double &side, double &translate) {
    if (aligned) {
        const double sl = floor(s*l-.5), sr = ceil(s*r+.5);
        side = sr-sl;
        translate = -sl/s;
    } else {
        const double d = s*(r-l);
        side = ceil(d)+1;
        translate = -l+(.5*(side-d))/s;
    }
}

// plain4: l, b, r, t of Shape::getBounds; ext4: the same with border = -lo and the miters. wh: the box, 0 x 0 when the glyph has none (an empty glyph, a lone
// horizontal or vertical line: nothing to render), -1 for a side that is NaN or beyond BOX_MAX_SIDE. xf: sx, sy, tx, ty, mapScale, mapTranslate
// (DistanceMapping.cpp:13) -- a texel centre (x+.5, y+.5) of the box is the shape point (x+.5)/s - tx, (y+.5)/s - ty.
MSDF_HD void boxGlyph(const BoxParams &p, const double *plain4, const double *ext4, int32_t *wh, double *xf6) {
    double w = 0, h = 0, tx = 0, ty = 0;
    if (plain4[0] < plain4[2] && plain4[1] < plain4[3]) {
        boxAxis(p.s, ext4[0], ext4[2], p.alignX, w, tx);
        boxAxis(p.s, ext4[1], ext4[3], p.alignY, h, ty);
    }
    wh[0] = w >= 0 && w <= (double) BOX_MAX_SIDE ? (int32_t) w : -1;                   // (a NaN fails the comparison)
    wh[1] = h >= 0 && h <= (double) BOX_MAX_SIDE ? (int32_t) h : -1;
    xf6[0] = p.s, xf6[1] = p.s, xf6[2] = tx, xf6[3] = ty;
    xf6[4] = 1/(p.hi-p.lo), xf6[5] = -p.lo;
}

} // namespace msdfhip
