// C binding of msdfgen_amd/csrc/msdf_qualityplan.hpp and of the render texel function of msdf_render.hpp for tests/test_sized_quality_host.py: what the
// launches of msdfhip_batch_estimate_sdf_error_sized / msdfhip_render_sdf_sized depend on, and the per-texel body of the render kernels, compiled with the
// host compiler (no HIP, no device).
#include "../../msdfgen_amd/csrc/msdf_qualityplan.hpp"
#include "../../msdfgen_amd/csrc/msdf_render.hpp"

using namespace msdfhip;

// renderSDF of one sw x sh field into out[oh][ow][no], as msdfhip_render_sdf[_sized] does it: renderMapping on the "host", renderSdfTexel per output texel.
template <int NO, int NS>
static void renderAll(float *out, int ow, int oh, const float *sdf, int sw, int sh, double lo, double hi, float thr) {
    const RenderMapping m = renderMapping(sw, sh, ow, oh, lo, hi);
    const int threshold = lo == hi;
    const float sdBias = threshold ? 0.f : .5f-thr;
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < ow; ++x)
            renderSdfTexel<NO, NS>(out+((size_t) y*ow+x)*NO, sdf, sw, sh, x, y, m.scaleX, m.scaleY, threshold, m.mapScale, m.mapTranslate, thr, sdBias);
}

extern "C" {

int sq_codes(int which) {
    const int codes[3] = { QUALITY_OK, QUALITY_TOO_MANY, QUALITY_BAD_OUTPUT };
    return codes[which%3];
}

long long sq_max_count() { return (long long) QUALITY_MAX_COUNT; }

int sq_item_prefix(int nGlyphs, const int32_t *sizes, int spr, int64_t *itemStart) { return errorItemPrefix(nGlyphs, sizes, spr, itemStart); }

// out[0..2] = glyph, row, subRow of `item`
void sq_item_of(const int64_t *itemStart, int nGlyphs, int spr, long long item, int *out) {
    const ErrorItem it = errorItemOf(itemStart, nGlyphs, spr, (int64_t) item);
    out[0] = it.g, out[1] = it.row, out[2] = it.subRow;
}

// out[0..2] = refCap, sdfCap, bytes per lane
void sq_caps(int maxEdges, int W, long long *out) {
    const size_t refCap = errorRefCap(maxEdges), sdfCap = errorSdfCap(W);
    out[0] = (long long) refCap, out[1] = (long long) sdfCap, out[2] = (long long) errorLaneBytes(refCap, sdfCap);
}

// out[0..1] = lanes per launch, launches
void sq_chunks(long long items, long long laneBytes, long long capBytes, long long *out) {
    const size_t lanes = errorChunkLanes((int64_t) items, (size_t) laneBytes, (size_t) capBytes);
    out[0] = (long long) lanes, out[1] = (long long) errorChunkCount((int64_t) items, lanes);
}

int sq_texel_prefix(int nGlyphs, const int32_t *outSizes, int64_t *outStart, int *badGlyph) { return renderTexelPrefix(nGlyphs, outSizes, outStart, badGlyph); }

// out[0..2] = glyph, x, y of output texel `texel`
void sq_texel_of(const int64_t *outStart, int nGlyphs, const int32_t *outSizes, long long texel, int *out) {
    const RenderTexel t = renderTexelOf(outStart, nGlyphs, outSizes, (int64_t) texel);
    out[0] = t.g, out[1] = t.x, out[2] = t.y;
}

// acosRounded (msdf_device.hpp): what the error estimate's cubic solver takes for acos
void sq_acos_rounded(const double *x, long n, double *y) {
    for (long i = 0; i < n; ++i)
        y[i] = acosRounded(x[i]);
}

int sq_render(int no, int ns, float *out, int ow, int oh, const float *sdf, int sw, int sh, double lo, double hi, float thr) {
    if (no == 1 && ns == 1) renderAll<1, 1>(out, ow, oh, sdf, sw, sh, lo, hi, thr);
    else if (no == 3 && ns == 1) renderAll<3, 1>(out, ow, oh, sdf, sw, sh, lo, hi, thr);
    else if (no == 1 && ns == 3) renderAll<1, 3>(out, ow, oh, sdf, sw, sh, lo, hi, thr);
    else if (no == 3 && ns == 3) renderAll<3, 3>(out, ow, oh, sdf, sw, sh, lo, hi, thr);
    else if (no == 1 && ns == 4) renderAll<1, 4>(out, ow, oh, sdf, sw, sh, lo, hi, thr);
    else if (no == 4 && ns == 4) renderAll<4, 4>(out, ow, oh, sdf, sw, sh, lo, hi, thr);
    else return 1;
    return 0;
}

}

#if defined(SIZED_QUALITY_MAIN)
// Stand-alone form for a sanitized build: walks the plan over the boxes of the test and renders a synthetic field of every box under every channel pair,
// output size, range and threshold of the test, under -fsanitize=address,undefined.
#include <cstdio>
#include <vector>
int main() {
    const int32_t boxes[] = { 1, 1, 7, 9, 8, 8, 9, 8, 8, 9, 24, 1, 1, 17, 23, 17, 16, 16, 17, 10, 24, 17 };
    const int n = 11;
    for (int spr = 1; spr <= 3; spr += 2) {
        std::vector<int64_t> start(n+1);
        if (sq_item_prefix(n, boxes, spr, start.data()) != QUALITY_OK || start[n] != (102-16)*spr)     // the sum of h-1 less that of the 1 x 17 box
            return 1;
        int64_t seen = 0;
        for (int g = 0; g < n; ++g)
            for (int row = 0; boxes[2*g] > 1 && row < boxes[2*g+1]-1; ++row)
                for (int sub = 0; sub < spr; ++sub, ++seen) {
                    int got[3];
                    sq_item_of(start.data(), n, spr, seen, got);
                    if (got[0] != g || got[1] != row || got[2] != sub)
                        return 2;
                }
        if (seen != start[n])
            return 3;
    }
    long long chunks[2];
    sq_chunks(306, 100, 12800, chunks);
    if (chunks[0] != 128 || chunks[1] != 3)
        return 4;
    sq_chunks(129, 100, 12800, chunks);                          // a last chunk of one lane
    if (chunks[0] != 128 || chunks[1] != 2)
        return 5;
    const int32_t outs[] = { 0, 5, 3, 2, 4, 0, 0, 0, 1, 1 };
    std::vector<int64_t> outStart(6);
    int bad;
    if (sq_texel_prefix(5, outs, outStart.data(), &bad) != QUALITY_OK || outStart[5] != 7)
        return 6;
    for (long long t = 0; t < 7; ++t) {
        int got[3];
        sq_texel_of(outStart.data(), 5, outs, t, got);
        if (got[0] != (t < 6 ? 1 : 4) || got[1] != (t < 6 ? (int) (t%3) : 0) || got[2] != (t < 6 ? (int) (t/3) : 0))
            return 7;
    }
    const int32_t negative[] = { 2, 2, 3, -1 };
    if (sq_texel_prefix(2, negative, outStart.data(), &bad) != QUALITY_BAD_OUTPUT || bad != 1)
        return 8;
    const int32_t huge[] = { 0x7fffffff, 0x7fffffff };
    std::vector<int64_t> hugeStart(2);
    if (sq_item_prefix(1, huge, 0x7fffffff, hugeStart.data()) != QUALITY_TOO_MANY || sq_texel_prefix(1, huge, hugeStart.data(), &bad) != QUALITY_TOO_MANY)
        return 9;
    const int pairs[6][2] = { { 1, 1 }, { 3, 1 }, { 1, 3 }, { 3, 3 }, { 1, 4 }, { 4, 4 } };
    const double ranges[3][2] = { { -1, 1 }, { 2, -1 }, { 0, 0 } };
    for (int g = 0; g < n; ++g) {
        const int w = boxes[2*g], h = boxes[2*g+1];
        const int sizes[4][2] = { { 2*w, 2*h }, { w, h }, { 1, 1 }, { 3*w+1, h/2 > 1 ? h/2 : 1 } };
        for (const auto &p : pairs) {
            std::vector<float> sdf((size_t) w*h*p[1]);
            for (size_t i = 0; i < sdf.size(); ++i)
                sdf[i] = (float) ((i*37)%101)/100.f;
            for (const auto &s : sizes)
                for (const auto &r : ranges)
                    for (int k = 0; k < 2; ++k) {
                        std::vector<float> out((size_t) s[0]*s[1]*p[0], -1.f);
                        if (sq_render(p[0], p[1], out.data(), s[0], s[1], sdf.data(), w, h, r[0], r[1], k ? .4f : .5f))
                            return 10;
                        for (float v : out)
                            if (!(v >= 0.f && v <= 1.f))
                                return 11;
                    }
        }
    }
    std::puts("ok");
    return 0;
}
#endif
