// msdf_classplan.hpp -- the glyph classes of the distance pass, planned on the host from the per-glyph contour and edge counts.
// Host code only (no HIP): msdf_capi.hip includes it, and tests/hostemu compiles it with the host compiler.

#pragma once

#include <algorithm>
#include <cstddef>

namespace msdfhip {

// LDS of k_distance's phase 1 per tile: survivor list [maxEdges], list offsets per contour [C+1] (+1 spare) and, in the global-scratch
// form, the per-contour channel bounds [C][3] (the LDS form keeps those in the combiner scratch's region)
inline size_t tileListBytes(int maxEdges, int maxContours, bool withBounds) { return ((size_t) maxEdges+(withBounds ? 4 : 1)*(size_t) maxContours+2)*sizeof(int); }

const int SMALL_MAX_EDGES = 128;                    // cost model only: the edge bound of the LDS-scratch class (PlanTuning::smallMaxEdges is what the launches use)
const int COST_LDS_MAX_CONTOURS = 5;                // cost model only: the LDS class's contour bound at the default LDS budget, msdf (msdf_launchplan.hpp: overlapClassLimit derives the real one per launch)

// Cost of one glyph in microseconds at 64x64 (only the ratios matter): a + b*E + c*C + d*E*C per kernel class, fitted to measured kernel
// times (tools/fit_cost_model.py, profiles/r06_cost_model.json: refitted in round 6; the same table as msdfgen_amd/shard.py: COST_MODEL).
inline double glyphCost(int contours, int edges) {
    static const double kOne[4] = { 0.25625, 0.01190, 0.00000, 0.00000 }, kLds[4] = { 0.38398, 0.00846, -0.02755, 0.003446 }, kGlobal[4] = { 1.11611, 0.015776, -0.05039, 0.000681 };
    const double *k = contours <= 1 ? kOne : (contours <= COST_LDS_MAX_CONTOURS && edges <= SMALL_MAX_EDGES) ? kLds : kGlobal;
    const double c = k[0]+k[1]*edges+k[2]*contours+k[3]*(double) edges*contours;
    return c > k[0] ? c : k[0];                                  // never below the class's intercept (the fit's negative contour terms are local to the measured range)
}

// The class list of a glyph range is [nOne][nSmall][rest][nHuge] glyph indices, heaviest first inside each of the first three:
//   one    <= 1 contour: the combiner reduces to the simple one (contour-combiners.cpp:104-133 with a single selector) -- these run the
//          simple-combiner kernel, which needs 95 VGPRs instead of ~150 and therefore runs 5 instead of 3 wavefronts per SIMD;
//   small  2..limit contours and at most smallMaxEdges edges: per-contour distances in LDS;
//   rest   more: per-contour distances in the global workspace;
//   huge   survivor lists beyond a CU's LDS (edges + 4 contours > ~40 000), whatever the contour count: the list-free kernel -- ALONE: round 3
//          sent the whole batch there with it.
struct ClassPlan {
    int nOne = 0, nSmall = 0, nHuge = 0;
    int oneMaxE = 0, smallMaxC = 0, smallMaxE = 0, restMaxC = 0, restMaxE = 0;   // maxima of the three culled classes
    float restShare = 1.f;            // the global-scratch class's share of the range's modelled cost (glyphCost): sizes its persistent launch
};

// order[n] receives the class list.
inline ClassPlan planClasses(const int *contours, const int *edges, int n, int limit, int smallMaxEdges, size_t ldsLimit, int *order) {
    auto classOf = [=](int g) {
        if (tileListBytes(edges[g], contours[g], true) > ldsLimit)
            return 3;
        return contours[g] <= 1 ? 0 : contours[g] <= limit && edges[g] <= smallMaxEdges ? 1 : 2;
    };
    int end[4], maxC[4] = { 0, 0, 0, 0 }, maxE[4] = { 0, 0, 0, 0 }, at = 0;
    for (int k = 0; k < 4; ++k) {
        for (int g = 0; g < n; ++g)
            if (classOf(g) == k) {
                order[at++] = g;
                maxC[k] = std::max(maxC[k], contours[g]), maxE[k] = std::max(maxE[k], edges[g]);
            }
        end[k] = at;
    }
    // Heaviest glyphs first inside each class (longest-processing-time order: a launch is ~26 rounds of workgroups, its tail is the last round's
    // heaviest glyph; the output does not depend on the order -- a glyph writes its own tiles).
    auto heavier = [=](int x, int y) { return (long long) edges[x]*std::max(contours[x], 1) > (long long) edges[y]*std::max(contours[y], 1); };
    for (int k = 0; k < 3; ++k)
        std::stable_sort(order+(k ? end[k-1] : 0), order+end[k], heavier);
    double all = 0, rest = 0;
    for (int g = 0; g < n; ++g)
        all += glyphCost(contours[g], edges[g]);
    for (int k = end[1]; k < end[2]; ++k)
        rest += glyphCost(contours[order[k]], edges[order[k]]);
    ClassPlan p;
    p.nOne = end[0], p.nSmall = end[1]-end[0], p.nHuge = end[3]-end[2];
    p.oneMaxE = maxE[0], p.smallMaxC = maxC[1], p.smallMaxE = maxE[1], p.restMaxC = maxC[2], p.restMaxE = maxE[2];
    p.restShare = all > 0 ? (float) (rest/all) : 1.f;
    return p;
}

} // namespace msdfhip
