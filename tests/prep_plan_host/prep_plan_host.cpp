// The slot sizing of msdf_prepplan.hpp against real memory (tests/test_prep_plan_host.py builds this with -fsanitize=address,undefined): for seeded random
// streamed calls, an arena of exactly the planned slot size is allocated, every chunk is carved with its exact counts, and every present region is
// written over its full size. A chunk carving past its slot is an AddressSanitizer report. Host code only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../msdfgen_amd/csrc/msdf_prepplan.hpp"

using namespace msdfhip;

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {                                // xorshift64*, [0, n)
    state ^= state >> 12, state ^= state << 25, state ^= state >> 27;
    return (uint32_t) ((state*0x2545f4914f6cdd1dull) >> 33)%n;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "case %d: %s\n", cases, #cond); return 1; } } while (0)

int main() {
    int cases = 0;
    size_t chunksCarved = 0;
    for (; cases < 600; ++cases) {
        // glyphs: contours per glyph and edges per contour. kind: 0 mixed, 1 single-edge contours (nE1 = nE + 2 nC), 2 two-edge contours (nE2 up to nE + 4 nC),
        // 3 glyphs around the colouring's and the orientation's tiers
        const int kind = (int) rnd(4), nG = 1+(int) rnd(40);
        std::vector<int> contours, edges, co(1, 0);
        for (int g = 0; g < nG; ++g) {
            int nC = rnd(5) == 0 ? 0 : 1+(int) rnd(6), nE = 0;
            for (int c = 0; c < nC; ++c) {
                int n = kind == 1 ? 1 : kind == 2 ? 2 : (int) rnd(9);
                if (kind == 3 && c == 0) {
                    const int special[] = { 341, 342, 2046, 2047, 2048, 2049, 2100 };
                    n = special[rnd(7)];
                }
                nE += n;
                co.push_back(co.back()+n);
            }
            contours.push_back(nC), edges.push_back(nE);
        }
        std::vector<int> lengths;
        for (int left = nG; left > 0;) {
            const int len = 1+(int) rnd(rnd(3) ? 4 : (uint32_t) left);
            lengths.push_back(len < left ? len : left);
            left -= lengths.back();
        }
        const bool prepare = rnd(8) != 0, normalize = rnd(2) != 0;
        const PrepPlanConfig cfg = { prepare, prepare ? (int) rnd(3) : 0, rnd(2) != 0, true, rnd(2) != 0, false, false, prepare && rnd(2), true };

        const StreamPrepPlan plan = planStreamPrep(contours.data(), edges.data(), lengths, cfg);
        CHECK(plan.refused < 0 && plan.chunks.size() == lengths.size());
        char *dev = (char *) malloc(plan.devBytes), *pinned = (char *) malloc(plan.pinnedBytes);
        CHECK(dev && pinned);
        size_t c0 = 0;
        for (size_t ci = 0; ci < plan.chunks.size(); ++ci) {
            const StreamChunk &ch = plan.chunks[ci];
            std::vector<int32_t> rel(ch.nC+1), co1(ch.nC+1);
            for (size_t c = 0; c <= ch.nC; ++c)
                rel[c] = co[c0+c]-co[c0];
            c0 += ch.nC;
            CHECK((size_t) rel[ch.nC] == ch.nE);
            size_t bound2 = 0;
            int longest = 0, maxRaw = 0;
            if (prepare)
                prepOffsets(rel.data(), (int) ch.nC, normalize, co1.data(), &bound2, &longest);
            for (int g = ch.start; g < ch.start+ch.length; ++g)
                maxRaw = edges[(size_t) g] > maxRaw ? edges[(size_t) g] : maxRaw;
            PrepPlanConfig exact = cfg;
            exact.longContour = longest > PREP_PLAN_WAVE_MAX_EDGES, exact.hitsBig = orientHitsBig(maxRaw);
            CHECK((!exact.longContour || ch.mayHaveLong) && exact.hitsBig == ch.hitsBig);
            const PrepCounts counts = { (size_t) ch.length, ch.nC, ch.nE, prepare ? (size_t) co1[ch.nC] : 0, bound2 };
            const PrepCarve cv = prepCarve(exact, counts);
            for (int r = 0; r < PREP_REGIONS; ++r)
                if (cv.bytes[r]) {
                    memset(dev+cv.off[r], 0x5a, cv.bytes[r]);
                    if (r < PREP_UPLOADED)
                        memset(pinned+cv.off[r], 0x5a, cv.bytes[r]);
                }
            if (cfg.coloring)                                    // the coloured offsets come back behind the uploaded part
                memset(pinned+cv.uploadBytes, 0x5a, (ch.nC+1)*sizeof(int32_t));
            const PrepBuffers pb = bindPrep(dev, cv);
            CHECK(pb.gco == (const int32_t *) dev && (cfg.coloring ? pb.fin.points != pb.norm.points : pb.fin.points == pb.norm.points));
            ++chunksCarved;
        }
        free(dev), free(pinned);
    }
    printf("planned %d calls, carved %zu chunks\n", cases, chunksCarved);
    return 0;
}
