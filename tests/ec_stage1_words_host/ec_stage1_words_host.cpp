// TEST TOOLING ONLY -- stage 1 of the error-correction sweep (msdf_ec_fast.hpp: ecTexelClassWord, loadNeighbourhood, texelCandidatePairs -- the classifier
// k_ec_fast runs per texel, here compiled for the host with g++) against the form it replaced, for tests/test_ec_stage1_words_host.py and
// tests/test_gpu_ec_stage1_words.py. A stand-alone program, so that it can also be built with -fsanitize=address,undefined and run as it is. Never loaded by
// the msdfgen_amd package.
//
//   ec_stage1_words_host compare CASES        prints one JSON object, returns 1 on any difference
//   ec_stage1_words_host correct CASES OUT    the shapeless error correction (findErrors(sdf) + apply) of every case by the host walk ecTexelFast;
//                                             OUT: the corrected fields, float[h][w][3] per case, one after the other
//   CASES: int32 n, then per case int32 w, h, protectAll, 0 | double xf[6] (sx, sy, tx, ty, mapScale, mapTranslate) | double minDeviationRatio
//                                 | float field[h][w][3] (rows in memory order)
//
// compare: for every texel, the set of (neighbour k, channel pair j) tests that the word-based stage 1 emits and the inside bits of the 3x3 neighbourhood
// against `Before`: the stage 1 of the commit before the class words, kept here word for word -- every lane derives everything from the channel values
// and the coordinates. Counted so that a test can show it is not vacuous: how often each of the 24 tests is emitted, and how many texels of each border
// pattern (bit 0: x == 0, bit 1: x == w-1, bit 2: y == 0, bit 3: y == h-1) were compared.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../msdfgen_amd/csrc/msdf_device.hpp"
#include "../../msdfgen_amd/csrc/msdf_prep.hpp"
#include "../../msdfgen_amd/csrc/msdf_ec.hpp"
#include "../../msdfgen_amd/csrc/msdf_ec_fast.hpp"

using namespace msdfhip;

namespace {

// ---- stage 1 as it was before the class words
namespace Before {

struct Neighbourhood {
    float v[3][3][3];
    float dev[3][3];
    unsigned valid;
};

void loadNeighbourhood(Neighbourhood &nb, const SdfView &sdf, int x, int yn) {
    nb.valid = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        for (int dx = -1; dx <= 1; ++dx) {
            const int nx = x+dx, ny = yn+dy;
            const bool in = nx >= 0 && ny >= 0 && nx < sdf.w && ny < sdf.h;
            const float *t = sdf.native(in ? nx : x, in ? ny : yn);
            nb.v[dy+1][dx+1][0] = t[0], nb.v[dy+1][dx+1][1] = t[1], nb.v[dy+1][dx+1][2] = t[2];
            nb.dev[dy+1][dx+1] = ecTexelDeviation(t);
            if (in)
                nb.valid |= 1u<<((dy+1)*3+(dx+1));
        }
    }
}

template <class Emit>
void texelCandidatePairs(const Neighbourhood &nb, Emit &emit) {
    const float *c = nb.v[1][1];
    const float cdev = nb.dev[1][1];
    for (int k = 0; k < 4; ++k) {
        const int dx = k == 0 ? -1 : k == 2 ? 1 : 0, dy = k == 1 ? -1 : k == 3 ? 1 : 0;
        if (!(nb.valid&(1u<<((dy+1)*3+(dx+1)))))
            continue;
        const float *b = nb.v[dy+1][dx+1];
        if (!(cdev >= nb.dev[dy+1][dx+1]))
            continue;
        for (int j = 0; j < 3; ++j) {
            const int i0 = j, i1 = j == 2 ? 0 : j+1;
            const float dA = c[i1]-c[i0], dB = b[i1]-b[i0];
            if ((dA > 0 && dB < 0) || (dA < 0 && dB > 0))
                emit(k, j);
        }
    }
    for (int k = 4; k < 8; ++k) {
        const int dx = (k&1) ? 1 : -1, dy = (k&2) ? 1 : -1;
        if (!(nb.valid&(1u<<((dy+1)*3+(dx+1)))))
            continue;
        const float *d = nb.v[dy+1][dx+1];
        if (!(cdev >= nb.dev[dy+1][dx+1]))
            continue;
        const float *b = nb.v[1][dx+1], *cc = nb.v[dy+1][1];
        for (int j = 0; j < 3; ++j) {
            const int i0 = j, i1 = j == 2 ? 0 : j+1;
            const float dA = c[i1]-c[i0], dBC = b[i1]-b[i0]+cc[i1]-cc[i0], dD = d[i1]-d[i0];
            if (dA == 0 && dBC == 0 && dD == 0)
                continue;
            if (bernsteinMayHaveRoot(dA, dBC, dD))
                emit(k, j);
        }
    }
}

}

struct Case {
    int w, h, protectAll;
    double xf[6], ratio;
    std::vector<float> field;
};

bool readCase(FILE *f, Case &c) {
    int32_t head[4];
    if (fread(head, sizeof(int32_t), 4, f) != 4)
        return false;
    c.w = head[0], c.h = head[1], c.protectAll = head[2];
    if (c.w < 1 || c.h < 1 || c.w > 4096 || c.h > 4096 || (c.protectAll != 0 && c.protectAll != 1) || head[3] != 0)
        return false;
    if (fread(c.xf, sizeof(double), 6, f) != 6 || fread(&c.ratio, sizeof(double), 1, f) != 1)
        return false;
    c.field.assign((size_t) c.w*c.h*3, 0.f);
    return fread(c.field.data(), sizeof(float), c.field.size(), f) == c.field.size();
}

struct MaskOfTests {
    unsigned mask;                  // bit 3*k+j
    int emitted;
    void operator()(int k, int j) { mask |= 1u<<(3*k+j); ++emitted; }
};

struct NoSink {
    long n;
    void operator()(double, int, int) { ++n; }
};

}

int main(int argc, char **argv) {
    const bool compare = argc == 3 && !strcmp(argv[1], "compare"), correct = argc == 4 && !strcmp(argv[1], "correct");
    if (!compare && !correct) {
        fprintf(stderr, "usage: %s compare CASES | correct CASES OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[2], "rb");
    int32_t n = 0;
    if (!f || fread(&n, sizeof(n), 1, f) != 1 || n < 0) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 2;
    }
    FILE *out = correct ? fopen(argv[3], "wb") : NULL;
    if (correct && !out) {
        fprintf(stderr, "cannot write %s\n", argv[3]);
        return 2;
    }
    long texels = 0, badTests = 0, badValid = 0, badCount = 0, emitted[24] = { 0 }, border[16] = { 0 }, deferred = 0, corrected = 0;
    for (int i = 0; i < n; ++i) {
        Case c;
        if (!readCase(f, c)) {
            fprintf(stderr, "case %d of %s is malformed\n", i, argv[2]);
            return 2;
        }
        SdfView sdf;
        sdf.px = c.field.data(), sdf.w = c.w, sdf.h = c.h, sdf.N = 3, sdf.flip = 0;
        if (compare) {
            for (int yn = 0; yn < c.h; ++yn)
                for (int x = 0; x < c.w; ++x) {
                    Before::Neighbourhood was;
                    Before::loadNeighbourhood(was, sdf, x, yn);
                    MaskOfTests want = { 0, 0 }, got = { 0, 0 };
                    Before::texelCandidatePairs(was, want);
                    Neighbourhood nb;
                    loadNeighbourhood(nb, sdf, x, yn);
                    texelCandidatePairs(nb, got);
                    ++texels;
                    badTests += got.mask != want.mask;
                    badCount += got.emitted != want.emitted;              // (a test emitted twice would be evaluated twice)
                    badValid += nb.valid != was.valid || ecValidFromWords(nb) != was.valid;
                    for (int t = 0; t < 24; ++t)
                        emitted[t] += (got.mask>>t)&1;
                    ++border[(x == 0 ? 1 : 0)|(x == c.w-1 ? 2 : 0)|(yn == 0 ? 4 : 0)|(yn == c.h-1 ? 8 : 0)];
                }
            continue;
        }
        // msdfFastDistanceErrorCorrection / msdfFastEdgeErrorCorrection as the device entry runs them: the general pass on an empty shape, mode
        // INDISCRIMINATE resp. EDGE_ONLY, no distance check
        EcParams p;
        const Xform t = { c.xf[0], c.xf[1], c.xf[2], c.xf[3], c.xf[4], c.xf[5] };
        p.t = t;
        p.minDeviationRatio = c.ratio, p.minImproveRatio = 1.11111111111111111;
        p.mode = c.protectAll ? EC_MODE_EDGE_ONLY : EC_MODE_INDISCRIMINATE, p.distanceCheck = EC_DO_NOT_CHECK, p.overlap = 0, p.stageLimit = 0;
        ecDerive(p);
        std::vector<float> res(c.field);
        for (int yn = 0; yn < c.h; ++yn)
            for (int x = 0; x < c.w; ++x) {
                NoSink sink = { 0 };
                const int st = ecTexelFast(sdf, p, (const int *) NULL, 0, x, yn, sink);
                deferred += sink.n+((st&EC_DEFER) != 0);
                if (st&EC_ERROR) {
                    const float *v = sdf.native(x, yn);
                    const float m = medianf(v[0], v[1], v[2]);
                    float *o = res.data()+((size_t) yn*c.w+x)*3;
                    o[0] = m, o[1] = m, o[2] = m;
                    ++corrected;
                }
                ++texels;
            }
        if (fwrite(res.data(), sizeof(float), res.size(), out) != res.size()) {
            fprintf(stderr, "cannot write %s\n", argv[3]);
            return 2;
        }
    }
    fclose(f);
    if (out && fclose(out) != 0)
        return 2;
    if (correct) {
        printf("{\"cases\": %d, \"texels\": %ld, \"corrected\": %ld, \"deferred\": %ld}\n", (int) n, texels, corrected, deferred);
        return deferred ? 1 : 0;                                     // no distance check in these configurations
    }
    printf("{\"cases\": %d, \"texels_compared\": %ld, \"bad_test_set\": %ld, \"bad_test_count\": %ld, \"bad_valid_mask\": %ld,\n \"emitted\": [", (int) n, texels, badTests,
           badCount, badValid);
    for (int t = 0; t < 24; ++t)
        printf("%s%ld", t ? ", " : "", emitted[t]);
    printf("],\n \"border_patterns\": [");
    for (int b = 0; b < 16; ++b)
        printf("%s%ld", b ? ", " : "", border[b]);
    printf("]}\n");
    return badTests || badCount || badValid ? 1 : 0;
}
