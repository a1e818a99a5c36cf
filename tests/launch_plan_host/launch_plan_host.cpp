// TEST TOOLING ONLY -- the launch planners of msdfgen_amd/csrc/msdf_launchplan.hpp (and planClasses, which feeds them) over seeded random glyph ranges, as
// a stand-alone program: tests/test_launch_plan_host.py builds it with -fsanitize=address,undefined and runs it. The checks here are the memory-shaped ones
// (every planned range lies inside the class list and covers it once); the arithmetic is pinned by the Python tests through tests/hostemu.
// Prints "planned <cases>" and returns 0, or reports the first violated check and returns 1.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "../../msdfgen_amd/csrc/msdf_launchplan.hpp"

using namespace msdfhip;

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t draw(uint32_t n) {                                // xorshift64*: [0, n)
    state ^= state>>12, state ^= state<<25, state ^= state>>27;
    return (uint32_t) ((state*0x2545f4914f6cdd1dull)>>33)%n;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "case %d: %s (line %d)\n", cases, #cond, __LINE__); return 1; } } while (0)

int main() {
    int cases = 0;
    for (int round = 0; round < 2400; ++round, ++cases) {
        PlanEnv env;
        env.ldsLimit = draw(8) ? 160*1024 : 1200+draw(60000);
        env.cus = draw(2) ? 256 : 64;
        env.t.smallLaunchTiles = draw(2) ? 0 : 8192;
        env.t.shortRounds = draw(3) ? 4 : 0;
        env.t.resLdsBudget = draw(4) ? 10*1024 : draw(2) ? 0 : 53248;
        env.t.smallMaxEdges = draw(4) ? 128 : 160;
        env.t.ldsClassTpw = draw(4) ? 4 : 1;
        env.t.persistentRounds = draw(3) ? 8 : draw(2);
        env.t.persistentGrid = draw(4) ? 0 : 40;
        env.t.serialClasses = draw(6) == 0;
        env.t.signCap = draw(4) ? 192 : 3;
        env.t.hasQueryLds = draw(6) == 0;
        const int n = 1+(int) draw(draw(2) ? 6 : 300), nch = draw(2) ? 3 : draw(2) ? 1 : 4;
        const int w = 1+(int) draw(200), h = 1+(int) draw(200);
        const bool overlap = draw(2) != 0;
        std::vector<int> contours((size_t) n), edges((size_t) n), order((size_t) n, -1);
        GlyphCounts b = { n, 0, 0 };
        for (int g = 0; g < n; ++g) {
            contours[g] = (int) draw(draw(8) ? 12 : 3000);
            edges[g] = contours[g] ? contours[g]+(int) draw(draw(40) ? 400 : 60000) : 0;
            b.maxContours = std::max(b.maxContours, contours[g]), b.maxEdges = std::max(b.maxEdges, edges[g]);
        }
        const int limit = classListLimit(env, b, w, h, nch, overlap);
        CHECK(classListLimitAhead(env, b, w, h, nch, overlap) == 0 || classListLimitAhead(env, b, w, h, nch, overlap) == limit);
        ClassPlan classes;
        if (limit)
            classes = planClasses(contours.data(), edges.data(), n, limit, env.t.smallMaxEdges, env.ldsLimit, order.data());
        const DistancePlan p = planDistance(env, b, w, h, nch, overlap, draw(5) == 0, draw(2) != 0, classes);
        if (!p.tooComplex) {
            std::vector<int> covered((size_t) n, 0);
            CHECK(p.nLaunches >= 0 && p.nLaunches <= 4);
            for (int k = 0; k < p.nLaunches; ++k) {
                const DistanceLaunch &l = p.launches[k];
                CHECK(l.count > 0 && l.offset >= 0 && l.offset+l.count <= n && (l.mapped ? limit != 0 : l.offset == 0 && l.count == n));
                CHECK(l.lds.bytes <= env.ldsLimit && l.stream >= PLAN_STREAM_CALLER && l.stream <= PLAN_STREAM_SIDE1);
                const GridPlan g = gridOf(l, w, h, env);
                CHECK(g.chunk > 0 && g.chunk <= distanceBlocks(l.count, w, h, l.tpw) && g.gresBytes == (l.gres && l.overlap ? g.chunk*l.lds.resBytes : 0));
                CHECK(routeOf(l, g) >= 0 && routeOf(l, g) < MSDFHIP_ROUTE_COUNT);
                for (int i = l.offset; i < l.offset+l.count; ++i)
                    ++covered[i];
            }
            if (p.unculled) {
                CHECK(p.unculledCount > 0 && p.unculledOffset >= 0 && p.unculledOffset+p.unculledCount <= n && (p.unculledMapped ? limit != 0 : p.unculledCount == n));
                for (int i = p.unculledOffset; i < p.unculledOffset+p.unculledCount; ++i)
                    ++covered[i];
            }
            for (int g = 0; g < n; ++g)
                CHECK(covered[g] == 1);
        }
        const size_t fastLds = 100*nch*sizeof(float)+68*sizeof(int)+2048*sizeof(unsigned short);
        const EcPlan ec = planCorrection(env, b, w, h, nch == 4 ? 4 : 3, overlap, (int) draw(4), (int) draw(3), draw(9) ? 0 : 1+(int) draw(4), fastLds);
        CHECK(ec.route != EC_ROUTE_NORMAL || (ec.queryLds <= env.ldsLimit && ec.fastLds <= env.ldsLimit));
        CHECK(ec.slotCap >= 1 && ec.mergedCap >= 1 && ec.mergedCap <= ec.slotCap && ec.queryBlocks >= 64 && ec.queryBlocks <= 8192 && ec.slowGrid >= 64 && ec.slowGrid <= 2048);
        CHECK(ec.residentQueryBlocks(draw(9000)) <= ec.queryBlocks);
        const SignPlan s = planSign(env, n, b.maxEdges, w, h);
        CHECK(s.span >= 1 && s.spansX*s.span >= (w+7)/8 && (s.spansX-1)*s.span < (w+7)/8 && s.cap >= 3 && s.cap <= env.t.signCap && s.blocks == (size_t) n*s.spans);
    }
    printf("planned %d\n", cases);
    return 0;
}
