// The wedge flags of the distance walk without a GPU: phase 1's "the whole tile lies outside this end's wedge" bits (msdf_cull.hpp: cullWedgeOutside), carried
// by a survivor's list entry into the per-texel walk (msdf_device.hpp: selEdgeRelevantWedges, selAddEdge skip a flagged end). Compiled from the product headers.
//
//   wedge_flags_host <cases.bin>      -> one JSON object on stdout; exit status 0 if every check held, 1 otherwise
//
// cases.bin: int32 nCases; per case int32 w, h, nC, nE; f64 sx, sy, tx, ty; int32 co[nC+1]; f64 points[nE][8]; u8 types[nE]; u8 colors[nE].
// For every case, both combiners and SEL 2, 3, 4, tile by tile (8x8 texels, the texels inside the bitmap are the lanes):
//   * phase 1 as k_distance runs it (bounds as floats rounded up, rows of 16 consecutive edges, nearest first inside a contour's segment of a row), which
//     also yields the two bits per survivor;
//   * the domain check: a set bit (of ANY edge of the glyph, survivor or not) -> no texel of the tile passes that end's domain test, evaluated with the
//     per-texel expressions of selAddEdge (add > 0 && ts > 0 / bdd > 0 && ts > 0);
//   * three lockstep walks of the survivors, contour by contour, with the kernel's two votes (box, then wedges) over the lanes: the records as they are in
//     memory (no bits: the walk of the parent commit), the records with their bits, and the records with BOTH bits forced on. After every contour the
//     selectors of the first two must be equal bit for bit in every lane and so must every vote; the third is there to show that the comparison can fail.
// The counts of the run (tests that reach the wedge stage, evaluated edges, how many of them with the tile outside) are printed per combiner.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>

#include "../../msdfgen_amd/csrc/msdf_device.hpp"
#include "../../msdfgen_amd/csrc/msdf_prep.hpp"
#include "../../msdfgen_amd/csrc/msdf_cull.hpp"

using namespace msdfhip;

namespace {

enum { T = 8 };

// A survivor's record as the walk sees it: the record plus the two bits of its list entry (the kernel's EdgeRegs reads them from the packed entry).
struct FlaggedRec : EdgeRec {
    int outside;
    FlaggedRec(const EdgeRec &e, int bits) : EdgeRec(e), outside(bits) { }
    bool OutsideA() const { return (outside&CULL_OUTSIDE_A) != 0; }
    bool OutsideB() const { return (outside&CULL_OUTSIDE_B) != 0; }
};

struct Case {
    int w, h, nC, nE;
    Xform t;
    std::vector<int32_t> co;
    std::vector<double> points;
    std::vector<uint8_t> types, colors;
    std::vector<EdgeRec> recs;
    std::vector<int> contourOf;
};

struct Entry { int edge, outside; };
struct TileLists { std::vector<Entry> list; std::vector<int> cstart; };

struct Counts {
    long tiles, survivors, wedgeStage, wedgeBoth, wedgeOne, wedgeRelevant, evaluated, endsOutside, bothEndsOutside;
    long bitsSet, bitsChecked, domainViolations, selectorMismatches, voteMismatches, forcedMismatches, lanesCompared;
};

bool sameBits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

template <int SEL>
bool sameSelector(const Selector<SEL> &a, const Selector<SEL> &b) {
    bool same = sameBits(a.m.d, b.m.d) && sameBits(a.m.dot, b.m.dot) && a.idx[0] == b.idx[0];
    for (int i = 0; i < (int) SelTraits<SEL>::NPB; ++i)
        same = same && sameBits(a.c[i].td, b.c[i].td) && sameBits(a.c[i].tdot, b.c[i].tdot) && sameBits(a.c[i].perp, b.c[i].perp) &&
               sameBits(a.c[i].neg, b.c[i].neg) && sameBits(a.c[i].pos, b.c[i].pos) && a.idx[i] == b.idx[i];
    return same;
}

// Tile centre and radius as distanceBody computes them (reciprocal scale; only accurate to within the cull's slack, which is the point of the domain check).
void tileGeometry(const Xform &t, int tx, int ty, V2 &tc, double &tr) {
    const double rsx = 1/t.sx, rsy = 1/t.sy;
    const double hx = (.5*T-.5)*fabs(rsx), hy = (.5*T-.5)*fabs(rsy);
    tr = sqrt(hx*hx+hy*hy);
    tc = mk((tx*T+.5*T)*rsx-t.tx, (ty*T+.5*T)*rsy-t.ty);
}

template <int SEL>
TileLists cullTile(const Case &k, bool overlap, V2 tc, double tr, std::vector<int> &outsideOfEdge) {
    TileLists out;
    const int nE = k.nE, nC = k.nC;
    std::vector<float> U((size_t) (nC > 0 ? nC : 1)*3, INFINITY);
    for (int i = 0; i < nE; ++i) {
        const int mask = cullMask<SEL>(k.recs[i]);
        const float ub = cullUpperFromSample2(cullNearestSample2(k.recs[i], tc));
        float *mine = &U[(size_t) (overlap ? k.contourOf[i] : 0)*3];
        for (int ch = 0; ch < 3; ++ch)
            if ((mask>>ch)&1)
                mine[ch] = ub < mine[ch] ? ub : mine[ch];
    }
    outsideOfEdge.assign((size_t) (nE > 0 ? nE : 1), 0);
    std::vector<int> perContour((size_t) nC+1, 0);
    for (int group = 0; group < nE; group += 16) {
        std::vector<std::pair<std::pair<int, unsigned>, int> > keyed;
        for (int i = group; i < nE && i < group+16; ++i) {
            const int mask = cullMask<SEL>(k.recs[i]);
            if (!mask)
                continue;
            const float *mine = &U[(size_t) (overlap ? k.contourOf[i] : 0)*3];
            double umax = 0;
            for (int ch = 0; ch < 3; ++ch)
                if ((mask>>ch)&1)
                    umax = dmax(umax, (double) mine[ch]);
            const int outside = cullWedgeOutside(k.recs[i], tc, tr);
            outsideOfEdge[i] = outside;
            const bool keep = cullEdgeSurvives<true>(k.recs[i], tc, tr, umax, outside);
            if (keep != cullEdgeSurvives<true>(k.recs[i], tc, tr, umax))                   // the four-argument form is the same verdict
                outsideOfEdge[i] |= 0x100;
            if (keep)
                keyed.push_back(std::make_pair(std::make_pair(k.contourOf[i], cullOrderKey(k.recs[i], tc, i-group)), i));
        }
        std::sort(keyed.begin(), keyed.end());
        for (size_t j = 0; j < keyed.size(); ++j) {
            Entry e = { keyed[j].second, outsideOfEdge[keyed[j].second]&3 };
            out.list.push_back(e);
            ++perContour[keyed[j].first.first];
        }
    }
    int at = 0;
    for (int c = 0; c < nC; ++c) {
        out.cstart.push_back(at);
        at += perContour[c];
    }
    out.cstart.push_back(at);
    return out;
}

// One survivor, one walk: the kernel's two votes over the lanes, then the evaluation in every lane. Returns 0 not relevant, 1 by the box, 2 by the wedges.
template <int SEL, class Rec>
int walkEdge(Selector<SEL> *sel, const Rec &r, int idx, const V2 *p, int lanes, bool skipWedgeVote) {
    double bound2[64];
    bool relevant = false;
    for (int l = 0; l < lanes; ++l)
        relevant = selEdgeRelevantBox(sel[l], r, p[l], bound2[l]) || relevant;
    int how = relevant ? 1 : 0;
    if (!relevant && !skipWedgeVote) {
        for (int l = 0; l < lanes; ++l)
            relevant = selEdgeRelevantWedges<SEL>(r, p[l], bound2[l]) || relevant;
        how = relevant ? 2 : 0;
    }
    if (relevant)
        for (int l = 0; l < lanes; ++l)
            selAddEdge(sel[l], r, idx, p[l]);
    return how;
}

template <int SEL>
void runCase(const Case &k, bool overlap, Counts &n) {
    for (int ty = 0; ty*T < k.h; ++ty)
        for (int tx = 0; tx*T < k.w; ++tx) {
            V2 tc;
            double tr;
            tileGeometry(k.t, tx, ty, tc, tr);
            V2 p[64];
            int lanes = 0;
            for (int l = 0; l < 64; ++l) {
                const int x = tx*T+(l&7), y = ty*T+(l>>3);
                if (x < k.w && y < k.h)
                    p[lanes++] = unproject(k.t, mk(x+.5, y+.5));
            }
            std::vector<int> outsideOfEdge;
            const TileLists lists = cullTile<SEL>(k, overlap, tc, tr, outsideOfEdge);
            ++n.tiles;
            n.survivors += (long) lists.list.size();
            // the domain check, over every edge of the glyph
            for (int i = 0; i < k.nE; ++i) {
                const EdgeRec &e = k.recs[i];
                if (outsideOfEdge[i]&0x100)
                    ++n.domainViolations;
                for (int end = 0; end < 2; ++end) {
                    if (!(outsideOfEdge[i]&(end ? CULL_OUTSIDE_B : CULL_OUTSIDE_A)))
                        continue;
                    ++n.bitsSet;
                    for (int l = 0; l < lanes; ++l) {
                        ++n.bitsChecked;
                        bool inside;
                        if (end == 0) {
                            const V2 ap = p[l]-e.P0();
                            inside = dot(ap, e.NA()) > 0 && dot(ap, -e.ADirN()) > 0;
                        } else {
                            const V2 bp = p[l]-e.PE();
                            inside = -dot(bp, e.NB()) > 0 && dot(bp, e.BDirN()) > 0;
                        }
                        if (inside)
                            ++n.domainViolations;
                    }
                }
            }
            // the three walks
            Selector<SEL> plain[64], flagged[64], forced[64];
            for (int l = 0; l < 64; ++l)
                selInit(plain[l]), selInit(flagged[l]), selInit(forced[l]);
            for (int c = 0; c < k.nC; ++c) {
                if (overlap)
                    for (int l = 0; l < 64; ++l)
                        selInit(plain[l]), selInit(flagged[l]), selInit(forced[l]);
                for (int j = lists.cstart[c]; j < lists.cstart[c+1]; ++j) {
                    const Entry &en = lists.list[j];
                    const EdgeRec &rec = k.recs[en.edge];
                    const FlaggedRec fr(rec, en.outside), all(rec, CULL_OUTSIDE_A|CULL_OUTSIDE_B);
                    const int a = walkEdge<SEL>(plain, rec, en.edge, p, lanes, false);
                    const int b = walkEdge<SEL>(flagged, fr, en.edge, p, lanes, fr.OutsideA() && fr.OutsideB());
                    walkEdge<SEL>(forced, all, en.edge, p, lanes, true);
                    if (a != b)
                        ++n.voteMismatches;
                    const int ends = (en.outside&1)+((en.outside>>1)&1);
                    if (b != 1) {
                        ++n.wedgeStage;
                        n.wedgeBoth += ends == 2, n.wedgeOne += ends == 1, n.wedgeRelevant += b == 2;
                    }
                    if (b) {
                        ++n.evaluated;
                        n.endsOutside += ends, n.bothEndsOutside += ends == 2;
                    }
                }
                for (int l = 0; l < lanes; ++l) {
                    ++n.lanesCompared;
                    if (!sameSelector(plain[l], flagged[l]))
                        ++n.selectorMismatches;
                    if (!sameSelector(plain[l], forced[l]))
                        ++n.forcedMismatches;
                }
            }
        }
}

bool readCases(const char *path, std::vector<Case> &cases) {
    FILE *f = fopen(path, "rb");
    if (!f)
        return false;
    int32_t nCases = 0;
    bool ok = fread(&nCases, 4, 1, f) == 1 && nCases >= 0 && nCases < (1<<20);
    for (int i = 0; ok && i < nCases; ++i) {
        Case k;
        int32_t head[4];
        double xf[4];
        ok = fread(head, 4, 4, f) == 4 && fread(xf, 8, 4, f) == 4;
        if (!ok)
            break;
        k.w = head[0], k.h = head[1], k.nC = head[2], k.nE = head[3];
        ok = k.w > 0 && k.h > 0 && k.w <= 4096 && k.h <= 4096 && k.nC >= 0 && k.nC < (1<<20) && k.nE >= 0 && k.nE < (1<<20);
        if (!ok)
            break;
        k.t.sx = xf[0], k.t.sy = xf[1], k.t.tx = xf[2], k.t.ty = xf[3], k.t.mapScale = 1, k.t.mapTranslate = 0;
        k.co.resize((size_t) k.nC+1), k.points.resize((size_t) k.nE*8+1), k.types.resize((size_t) k.nE+1), k.colors.resize((size_t) k.nE+1);
        ok = fread(k.co.data(), 4, (size_t) k.nC+1, f) == (size_t) k.nC+1 && fread(k.points.data(), 8, (size_t) k.nE*8, f) == (size_t) k.nE*8 &&
             fread(k.types.data(), 1, (size_t) k.nE, f) == (size_t) k.nE && fread(k.colors.data(), 1, (size_t) k.nE, f) == (size_t) k.nE;
        ok = ok && k.co[0] == 0 && k.co[k.nC] == k.nE;
        for (int c = 0; ok && c < k.nC; ++c)
            ok = k.co[c] <= k.co[c+1];
        for (int e = 0; ok && e < k.nE; ++e)
            ok = k.types[e] >= 1 && k.types[e] <= 3;
        if (!ok)
            break;
        k.recs.resize((size_t) (k.nE > 0 ? k.nE : 1));
        k.contourOf.assign((size_t) (k.nE > 0 ? k.nE : 1), 0);
        for (int c = 0; c < k.nC; ++c)
            for (int slot = k.co[c]; slot < k.co[c+1]; ++slot) {
                k.contourOf[slot] = c;
                prepRecord(k.recs.data(), slot, c, k.co.data(), k.points.data(), k.types.data(), k.colors.data());
            }
        cases.push_back(k);
    }
    fclose(f);
    return ok;
}

void printCounts(const char *name, const Counts &n, bool last) {
    printf("\"%s\": {\"tiles\": %ld, \"survivors\": %ld, \"wedge_stage\": %ld, \"wedge_outside_both\": %ld, \"wedge_outside_one\": %ld, \"wedge_relevant\": %ld, "
           "\"evaluated\": %ld, \"ends_outside\": %ld, \"both_ends_outside\": %ld, \"bits_set\": %ld, \"bits_checked\": %ld, \"domain_violations\": %ld, "
           "\"selector_mismatches\": %ld, \"vote_mismatches\": %ld, \"forced_mismatches\": %ld, \"lanes_compared\": %ld}%s\n",
           name, n.tiles, n.survivors, n.wedgeStage, n.wedgeBoth, n.wedgeOne, n.wedgeRelevant, n.evaluated, n.endsOutside, n.bothEndsOutside, n.bitsSet, n.bitsChecked,
           n.domainViolations, n.selectorMismatches, n.voteMismatches, n.forcedMismatches, n.lanesCompared, last ? "" : ",");
}

}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    std::vector<Case> cases;
    if (!readCases(argv[1], cases)) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    static const char *names[2][3] = { { "simple_sel2", "simple_sel3", "simple_sel4" }, { "overlap_sel2", "overlap_sel3", "overlap_sel4" } };
    long bad = 0, zeroDir = 0;
    for (size_t i = 0; i < cases.size(); ++i)
        for (int e = 0; e < cases[i].nE; ++e)
            zeroDir += (cases[i].recs[e].flags&(REC_A_ZERO|REC_B_ZERO)) != 0;
    printf("{\"cases\": %ld, \"zero_direction_edges\": %ld,\n", (long) cases.size(), zeroDir);
    for (int overlap = 0; overlap < 2; ++overlap)
        for (int s = 0; s < 3; ++s) {
            Counts n;
            memset(&n, 0, sizeof(n));
            for (size_t i = 0; i < cases.size(); ++i) {
                if (s == 0)
                    runCase<2>(cases[i], overlap != 0, n);
                else if (s == 1)
                    runCase<3>(cases[i], overlap != 0, n);
                else
                    runCase<4>(cases[i], overlap != 0, n);
            }
            bad += n.domainViolations+n.selectorMismatches+n.voteMismatches;
            printCounts(names[overlap][s], n, overlap == 1 && s == 2);
        }
    printf("}\n");
    return bad ? 1 : 0;
}
