// msdf_legacy.hpp -- the reference's legacy generators and legacy error correction, per texel: generateSDF_legacy / generatePSDF_legacy /
// generateMSDF_legacy / generateMTSDF_legacy (core/msdfgen.cpp:166-333) and msdfErrorCorrection_legacy (core/msdf-error-correction.cpp:115-181).
//
// The legacy field is the true minimum over ALL edges of the shape in shape order: no contour combiner, no windings, no per-contour selectors. A texel
// keeps one SignedDistance (modes 1 and 4) and, per channel, the nearest edge with its parameter (modes 2..4); after the walk every channel that found an
// edge converts its distance on that one edge (distanceToPerpendicularDistance). Replacement is the strict `<` of SignedDistance.hpp:22-24, so of two
// edges that tie in distance and alignment the FIRST in shape order stays -- the walk below therefore visits the edges in the shape's own order, which is
// not the order the records are stored in (msdf_prep.hpp: a contour's records start with its last edge).
// All arithmetic is the reference's, operation for operation (fp64, no contraction, division stays division). The kernels over these functions are
// k_distance_legacy and k_ec_legacy (msdf_kernels.hpp); tests/legacy_host compiles this header with the host compiler.
#pragma once

#include "msdf_device.hpp"

namespace msdfhip {

template <int MODE> struct LegacyTraits { enum { NCH = MODE <= 2 ? 1 : MODE, NNEAR = MODE == 1 ? 0 : MODE == 2 ? 1 : 3, TRUE_SD = MODE == 1 || MODE == 4 }; };

// minDistance / nearEdge / nearParam of one channel (msdfgen.cpp:197-199, 231-237).
struct LegacyNear {
    SD sd;
    int slot;                     // record of the nearest edge; -1: none yet (nearEdge == NULL)
    double param;
};

MSDF_HD SD legacyFarthest() { SD r = { -DBL_MAX, 0 }; return r; }              // SignedDistance(), SignedDistance.hpp:17

MSDF_HD void legacyOffer(LegacyNear &n, SD distance, int slot, double param) {
    if (sdLess(distance, n.sd))
        n.sd = distance, n.slot = slot, n.param = param;
}

// The record slot of the i-th edge (shape order) of a contour of n edges whose records start at `start`: the inverse of visitToEdge (msdf_prep.hpp).
MSDF_HD int legacySlot(int start, int n, int i) { return start+(i+1 == n ? 0 : i+1); }

// One texel of generate*_legacy at the shape-space point p: out[0..NCH) are the distances BEFORE the distance mapping. recs: the batch's records;
// coff: the glyph's C+1 contour offsets (global record indices). Every read of coff and recs inside the walk is the same for all texels.
template <int MODE>
MSDF_HD void legacyTexel(const EdgeRec *recs, const int32_t *coff, int C, V2 p, double *out) {
    enum { NNEAR = LegacyTraits<MODE>::NNEAR, TRUE_SD = LegacyTraits<MODE>::TRUE_SD };
    SD minDistance = legacyFarthest();
    LegacyNear ch[3];
    for (int k = 0; k < 3; ++k)
        ch[k].sd = legacyFarthest(), ch[k].slot = -1, ch[k].param = 0;
    for (int c = 0; c < C; ++c) {
        const int start = coff[c], n = coff[c+1]-start;
        MSDF_NOUNROLL
        for (int i = 0; i < n; ++i) {
            const int slot = legacySlot(start, n, i);
            const EdgeRec &e = recs[slot];
            double param;
            const SD distance = signedDistance(e, p, param);
            if (TRUE_SD && sdLess(distance, minDistance))
                minDistance = distance;
            if (NNEAR == 1)
                legacyOffer(ch[0], distance, slot, param);
            if (NNEAR == 3) {
                const int color = e.Color();
                if (color&1)
                    legacyOffer(ch[0], distance, slot, param);
                if (color&2)
                    legacyOffer(ch[1], distance, slot, param);
                if (color&4)
                    legacyOffer(ch[2], distance, slot, param);
            }
        }
    }
    // The nearest edge differs from texel to texel: its record is fetched per texel (on the device: per lane), once per channel.
    for (int k = 0; k < NNEAR; ++k) {
        if (ch[k].slot >= 0)
            distanceToPerpendicular(recs[ch[k].slot], ch[k].sd, p, ch[k].param);
        out[k] = ch[k].sd.d;
    }
    if (TRUE_SD)
        out[NNEAR] = minDistance.d;
}

// generate*_legacy's texel (x, y) in the SHAPE's row order (the bitmap was re-oriented to it, msdfgen.cpp:168): NCH floats.
template <int MODE>
MSDF_HD void legacyTexelMapped(const EdgeRec *recs, const int32_t *coff, int C, const Xform &t, int x, int y, float *out) {
    double d[LegacyTraits<MODE>::NCH];
    legacyTexel<MODE>(recs, coff, C, unproject(t, mk(x+.5, y+.5)), d);             // Vector2(x+.5, y+.5)/scale-translate
    for (int k = 0; k < LegacyTraits<MODE>::NCH; ++k)
        out[k] = mapDistance(t, d[k]);                                               // float(distanceMapping(d)): a channel without an edge maps -DBL_MAX
}

// ------------------------------------------------------------------------------------------------- legacy correction

// detectClash (msdf-error-correction.cpp:115-135): the channel pairs ordered by |b-a|, largest first; a clash when the middle difference reaches the
// threshold, b is not an equalized texel and a is the farther of the two from the edge. Float arithmetic stays float; the threshold compares in double.
MSDF_HD bool legacyDetectClash(const float *a, const float *b, double threshold) {
    float a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2], tmp;
    if (fabsf(b0-a0) < fabsf(b1-a1)) {
        tmp = a0, a0 = a1, a1 = tmp;
        tmp = b0, b0 = b1, b1 = tmp;
    }
    if (fabsf(b1-a1) < fabsf(b2-a2)) {
        tmp = a1, a1 = a2, a2 = tmp;
        tmp = b1, b1 = b2, b2 = tmp;
        if (fabsf(b0-a0) < fabsf(b1-a1)) {
            tmp = a0, a0 = a1, a1 = tmp;
            tmp = b0, b0 = b1, b1 = tmp;
        }
    }
    return (double) fabsf(b1-a1) >= threshold && !(b0 == b1 && b0 == b2) && fabsf(a2-.5f) >= fabsf(b2-.5f);
}

// One texel of one pass of msdfErrorCorrectionInner_legacy, OUT OF PLACE: every detection of a pass reads the bitmap as it was before the pass (the
// reference collects the clashes first and equalizes afterwards), so a pass reads `src` and writes `dst`; pass 1 (diagonal neighbours, threshold
// tx+ty) runs on what pass 0 (axial neighbours, tx / ty) wrote. src / dst: one tile, packed [h][w][N]. Neighbours outside the bitmap do not exist.
// The fourth channel of an MTSDF is copied, never equalized.
template <int N>
MSDF_HD void legacyClashTexel(const float *src, float *dst, int w, int h, int x, int y, int pass, double tx, double ty) {
    const float *a = src+((size_t) y*w+x)*N;
    const ptrdiff_t right = N, up = (ptrdiff_t) w*N;
    bool clash;
    if (pass == 0)
        clash = (x > 0 && legacyDetectClash(a, a-right, tx)) || (x < w-1 && legacyDetectClash(a, a+right, tx)) ||
                (y > 0 && legacyDetectClash(a, a-up, ty)) || (y < h-1 && legacyDetectClash(a, a+up, ty));
    else {
        const double t = tx+ty;
        clash = (x > 0 && y > 0 && legacyDetectClash(a, a-right-up, t)) || (x < w-1 && y > 0 && legacyDetectClash(a, a+right-up, t)) ||
                (x > 0 && y < h-1 && legacyDetectClash(a, a-right+up, t)) || (x < w-1 && y < h-1 && legacyDetectClash(a, a+right+up, t));
    }
    float *o = dst+((size_t) y*w+x)*N;
    if (clash)
        o[0] = o[1] = o[2] = medianf(a[0], a[1], a[2]);
    else
        o[0] = a[0], o[1] = a[1], o[2] = a[2];
    if (N == 4)
        o[3] = a[3];
}

} // namespace msdfhip
