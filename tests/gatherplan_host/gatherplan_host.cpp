// C binding of msdfgen_amd/csrc/msdf_gatherplan.hpp for tests/test_gather_plan_host.py: the validation, the totals and the table of msdfhip_batch_gather,
// compiled with the host compiler (no HIP, no device).
#include "../../msdfgen_amd/csrc/msdf_gatherplan.hpp"

using namespace msdfhip;

namespace {

// Sources as the test passes them: nSources, then per source nGlyphs, device and a pointer pair into the flat count arrays.
std::vector<GatherSource> sourcesOf(int nSources, const int *nGlyphs, const int *devices, const int *contours, const int *edges) {
    std::vector<GatherSource> src((size_t) (nSources > 0 ? nSources : 0));
    size_t at = 0;
    for (size_t s = 0; s < src.size(); ++s) {
        const GatherSource one = { nGlyphs[s], devices ? devices[s] : 0, contours ? contours+at : NULL, edges ? edges+at : NULL };
        src[s] = one;
        at += (size_t) (nGlyphs[s] > 0 ? nGlyphs[s] : 0);
    }
    return src;
}

} // namespace

extern "C" {

int gather_codes(int which) {
    const int codes[10] = { GATHER_OK, GATHER_NO_SOURCES, GATHER_BAD_COUNT, GATHER_NO_INDICES, GATHER_NO_SOURCE_OF, GATHER_BAD_SOURCE, GATHER_BAD_INDEX,
                            GATHER_MIXED_DEVICES, GATHER_TOO_MANY_CONTOURS, GATHER_TOO_MANY_EDGES };
    return codes[which%10];
}

// The whole plan as msdfhip_batch_gather runs it: gatherCheckArgs, then gatherTotals, then (with `table`) gatherFill. contours / edges: the per-glyph counts
// of all sources, one source after the other (NULL with nGlyphsOf == NULL: "sources is NULL").
// refusal[0..2] = position, value, limit; totals[0..3] = contours, edges, maxContours, maxEdges; columns[0..6] = the column offsets and the block's ints.
// table: NULL or gatherColumns(n).ints ints; selContours / selEdges: n ints each.
int gather_plan(int nSources, const int *nGlyphsOf, const int *devices, const int *contours, const int *edges, int nGlyphs, const int32_t *sourceOf,
                const int32_t *indices, long long *refusal, long long *totals, long long *columns, int32_t *table, int *selContours, int *selEdges) {
    const std::vector<GatherSource> src = sourcesOf(nGlyphsOf ? nSources : 0, nGlyphsOf, devices, contours, edges);
    GatherRefusal bad;
    int rc = gatherCheckArgs(nGlyphsOf ? src.data() : NULL, nSources, nGlyphs, sourceOf, indices, bad);
    GatherTotals t = { 0, 0, 0, 0 };
    if (rc == GATHER_OK)
        rc = gatherTotals(src.data(), nGlyphs, sourceOf, indices, t, bad);
    refusal[0] = bad.position, refusal[1] = bad.value, refusal[2] = bad.limit;
    totals[0] = t.contours, totals[1] = t.edges, totals[2] = t.maxContours, totals[3] = t.maxEdges;
    const GatherColumns col = gatherColumns(nGlyphs);
    columns[0] = (long long) col.dstContour0, columns[1] = (long long) col.source, columns[2] = (long long) col.srcGlyph, columns[3] = (long long) col.srcContour0;
    columns[4] = (long long) col.srcEdge0, columns[5] = (long long) col.dstEdge0, columns[6] = (long long) col.ints;
    if (rc == GATHER_OK && table)
        gatherFill(src.data(), nSources, nGlyphs, sourceOf, indices, table, selContours, selEdges);
    return rc;
}

}

#if defined(GATHERPLAN_MAIN)
// Stand-alone form for a sanitized build: walks cases of the test once more under -fsanitize=address,undefined.
#include <cstdio>
int main() {
    long long refusal[3], totals[4], columns[7];
    // source 0: glyphs of (2 contours, 7 edges), (0, 0), (1, 3); source 1: (3, 9), (1, 4)
    const int nGlyphsOf[2] = { 3, 2 }, devices[2] = { 0, 0 }, contours[5] = { 2, 0, 1, 3, 1 }, edges[5] = { 7, 0, 3, 9, 4 };
    const int32_t sourceOf[5] = { 1, 0, 0, 1, 0 }, indices[5] = { 1, 2, 1, 0, 0 };
    if (gather_plan(2, nGlyphsOf, devices, contours, edges, 5, sourceOf, indices, refusal, totals, columns, NULL, NULL, NULL) != GATHER_OK)
        return 1;
    if (totals[0] != 7 || totals[1] != 23 || totals[2] != 3 || totals[3] != 9)
        return 2;
    std::vector<int32_t> table((size_t) columns[6], -1);
    int selC[5], selE[5];
    if (gather_plan(2, nGlyphsOf, devices, contours, edges, 5, sourceOf, indices, refusal, totals, columns, table.data(), selC, selE) != GATHER_OK)
        return 3;
    const int32_t dstC[6] = { 0, 1, 2, 2, 5, 7 }, dstE[6] = { 0, 4, 7, 7, 16, 23 }, srcC[5] = { 3, 2, 2, 0, 0 }, srcE[5] = { 9, 7, 7, 0, 0 };
    for (int k = 0; k <= 5; ++k)
        if (table[(size_t) columns[0]+k] != dstC[k] || table[(size_t) columns[5]+k] != dstE[k])
            return 4;
    for (int k = 0; k < 5; ++k)
        if (table[(size_t) columns[1]+k] != sourceOf[k] || table[(size_t) columns[2]+k] != indices[k] || table[(size_t) columns[3]+k] != srcC[k] ||
            table[(size_t) columns[4]+k] != srcE[k])
            return 5;
    const int32_t badIndex[2] = { 0, 3 };
    if (gather_plan(1, nGlyphsOf, devices, contours, edges, 2, NULL, badIndex, refusal, totals, columns, NULL, NULL, NULL) != GATHER_BAD_INDEX || refusal[0] != 1)
        return 6;
    // one glyph of 2^20 edges 2 048 times: one too many
    const int oneGlyph[1] = { 1 }, oneContour[1] = { 1 }, bigEdges[1] = { 1<<20 };
    std::vector<int32_t> many(2048, 0);
    if (gather_plan(1, oneGlyph, devices, oneContour, bigEdges, 2048, NULL, many.data(), refusal, totals, columns, NULL, NULL, NULL) != GATHER_TOO_MANY_EDGES ||
        refusal[0] != 2047)
        return 7;
    if (gather_plan(1, oneGlyph, devices, oneContour, bigEdges, 2047, NULL, many.data(), refusal, totals, columns, NULL, NULL, NULL) != GATHER_OK ||
        totals[1] != 2047ll<<20)
        return 8;
    if (gather_plan(1, oneGlyph, devices, oneContour, bigEdges, 0, NULL, NULL, refusal, totals, columns, table.data(), selC, selE) != GATHER_OK || table[0] != 0)
        return 9;
    std::puts("ok");
    return 0;
}
#endif
