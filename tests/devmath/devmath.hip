// devmath.hip -- test-only harness: the arithmetic primitives of the PRODUCT's device headers (msdfgen_amd/csrc), each behind a one-element-per-lane kernel,
// so that tests/test_gpu_devmath.py can compare the gfx950 build of that text with high-precision references. Nothing is reimplemented here and no product
// binary is involved: tests/devmath.py compiles this file with the product's own compiler flags.
//
// Element i is lane i%64 of wavefront i/64: n must be a multiple of 64 (the callers pad), blocks are 256 lanes, so every wavefront that runs has all 64 lanes
// active -- which msdfSqrt's wave vote is tested through and which the DPP helpers require.
// Every entry point takes HOST pointers, allocates, copies, launches, synchronises, copies back, frees, and returns the HIP status (0 = hipSuccess).
#include <hip/hip_runtime.h>

#include <vector>

#include "msdf_device.hpp"
#include "msdf_prep.hpp"
#include "msdf_kernels.hpp"     // the wave helpers (waveMinNonNegative, rowMinNonNegative, rowRank, floatAbove); no kernel of it is launched

using namespace msdfhip;

namespace {

enum { BLOCK = 256 };

struct Dev {
    hipError_t err = hipSuccess;
    std::vector<void *> owned;
    struct Back { void *host; const void *dev; size_t bytes; };
    std::vector<Back> backs;

    explicit Dev(long n) {
        if (n <= 0 || n%64)
            err = hipErrorInvalidValue;
    }
    void *alloc(size_t bytes) {
        void *d = nullptr;
        if (err == hipSuccess)
            err = hipMalloc(&d, bytes);
        if (err == hipSuccess)
            owned.push_back(d);
        return err == hipSuccess ? d : nullptr;
    }
    template <class T> const T *in(const T *host, size_t count) {
        void *d = alloc(count*sizeof(T));
        if (err == hipSuccess)
            err = hipMemcpy(d, host, count*sizeof(T), hipMemcpyHostToDevice);
        return static_cast<const T *>(d);
    }
    template <class T> T *out(T *host, size_t count) {
        void *d = alloc(count*sizeof(T));
        if (err == hipSuccess)
            err = hipMemset(d, 0xff, count*sizeof(T));
        if (err == hipSuccess)
            backs.push_back(Back { host, d, count*sizeof(T) });
        return static_cast<T *>(d);
    }
    bool ok() const { return err == hipSuccess; }
    int finish() {
        if (err == hipSuccess)
            err = hipGetLastError();
        if (err == hipSuccess)
            err = hipDeviceSynchronize();
        for (const Back &b : backs)
            if (err == hipSuccess)
                err = hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost);
        for (void *p : owned)
            (void) hipFree(p);
        return (int) err;
    }
};

inline dim3 gridFor(long n) { return dim3((unsigned) ((n+BLOCK-1)/BLOCK)); }
__device__ inline long element() { return (long) blockIdx.x*BLOCK+threadIdx.x; }

// which: 0 msdfSqrt (lean core unless a lane of the wavefront is out of range), 1 the compiler's sqrt
__global__ void k_sqrt(const double *x, long n, int which, double *y) {
    const long i = element();
    if (i < n)
        y[i] = which ? sqrt(x[i]) : msdfSqrt(x[i]);
}

// The reciprocal is formed on the device with the division buildRecord uses (msdf_prep.hpp: 1/r.k[0]).
__global__ void k_div(const double *a, const double *b, long n, int32_t *safe, double *viaRcp, double *ieee) {
    const long i = element();
    if (i < n) {
        const double y = 1/b[i];
        safe[i] = divSafe(b[i]) ? 1 : 0;
        viaRcp[i] = divExact(a[i], b[i], y);
        ieee[i] = a[i]/b[i];
    }
}

__global__ void k_cos_thirds(const double *t, long n, double *c) {
    const long i = element();
    if (i < n)
        cosThirds(t[i], c[3*i], c[3*i+1], c[3*i+2]);
}

__global__ void k_pow_third(const double *x, long n, double *y) {
    const long i = element();
    if (i < n)
        y[i] = powThird(x[i]);
}

__global__ void k_acos(const double *x, long n, double *y) {
    const long i = element();
    if (i < n)
        y[i] = acos(x[i]);
}

__global__ void k_solve_quadratic(const double *abc, long n, int32_t *count, double *roots) {
    const long i = element();
    if (i < n) {
        double x[2] = { 0, 0 };
        count[i] = solveQuadratic(x, abc[3*i], abc[3*i+1], abc[3*i+2]);
        roots[2*i] = x[0], roots[2*i+1] = x[1];
    }
}

// in: a, a*a, a*(1/3.), b, c per element. branch: 1 the trigonometric branch (r2 < q3), 0 the cube-root branch -- from solveCubicNormedPre's own expressions.
__global__ void k_solve_cubic_normed_pre(const double *in, long n, int32_t *count, double *roots, int32_t *branch) {
    const long i = element();
    if (i < n) {
        const double a = in[5*i], a2 = in[5*i+1], a3 = in[5*i+2], b = in[5*i+3], c = in[5*i+4];
        double x[3] = { 0, 0, 0 };
        count[i] = solveCubicNormedPre(x, a, a2, a3, b, c);
        roots[3*i] = x[0], roots[3*i+1] = x[1], roots[3*i+2] = x[2];
        const double q = 1/9.*(a2-3*b);
        const double r = 1/54.*(a*(2*a2-9*b)+27*c);
        const double r2 = r*r;
        const double q3 = q*q*q;
        branch[i] = r2 < q3 ? 1 : 0;
    }
}

// One edge (its own cyclic neighbour: prev and next only enter the corner bisectors, which signedDistance does not read) digested by buildRecord.
__global__ void k_signed_distance(const double *pts, const int32_t *type, const double *org, long n, double *out, int32_t *flags) {
    const long i = element();
    if (i < n) {
        RawEdge e;
        for (int k = 0; k < 4; ++k)
            e.p[k] = mk(pts[8*i+2*k], pts[8*i+2*k+1]);
        e.type = type[i];
        e.color = 7;
        EdgeRec rec;
        buildRecord(rec, e, e, e, 0);
        double param = 0;
        const SD sd = signedDistance(rec, mk(org[2*i], org[2*i+1]), param);
        out[3*i] = sd.d, out[3*i+1] = sd.dot, out[3*i+2] = param;
        flags[i] = rec.flags;
    }
}

__global__ void k_map_distance(const double *scale, const double *translate, const double *d, long n, float *out) {
    const long i = element();
    if (i < n) {
        Xform t;
        t.sx = t.sy = 1, t.tx = t.ty = 0;
        t.mapScale = scale[i], t.mapTranslate = translate[i];
        out[i] = mapDistance(t, d[i]);
    }
}

__global__ void k_float_above(const double *d, long n, float *out) {
    const long i = element();
    if (i < n)
        out[i] = floatAbove(d[i]);
}

// which: 0 waveMinNonNegative, 1 rowMinNonNegative
__global__ void k_wave_min(const float *v, long n, int which, float *out) {
    const long i = element();
    if (i < n)                                          // n is a multiple of 64: whole wavefronts only
        out[i] = which ? rowMinNonNegative(v[i], (int) (threadIdx.x&63)) : waveMinNonNegative(v[i]);
}

__global__ void k_row_rank(const uint32_t *key, long n, int32_t *out) {
    const long i = element();
    if (i < n)
        out[i] = rowRank(key[i]);
}

}

extern "C" {

int devmath_arch(char *name, int size) {
    hipDeviceProp_t p;
    const hipError_t e = hipGetDeviceProperties(&p, 0);
    if (e == hipSuccess)
        snprintf(name, (size_t) size, "%s", p.gcnArchName);
    return (int) e;
}

int devmath_sqrt(const double *x, long n, int which, double *y) {
    Dev d(n);
    const double *dx = d.in(x, n);
    double *dy = d.out(y, n);
    if (d.ok())
        k_sqrt<<<gridFor(n), BLOCK>>>(dx, n, which, dy);
    return d.finish();
}

int devmath_div(const double *a, const double *b, long n, int32_t *safe, double *viaRcp, double *ieee) {
    Dev d(n);
    const double *da = d.in(a, n), *db = d.in(b, n);
    int32_t *ds = d.out(safe, n);
    double *dq = d.out(viaRcp, n), *di = d.out(ieee, n);
    if (d.ok())
        k_div<<<gridFor(n), BLOCK>>>(da, db, n, ds, dq, di);
    return d.finish();
}

int devmath_cos_thirds(const double *t, long n, double *c) {
    Dev d(n);
    const double *dt = d.in(t, n);
    double *dc = d.out(c, 3*n);
    if (d.ok())
        k_cos_thirds<<<gridFor(n), BLOCK>>>(dt, n, dc);
    return d.finish();
}

int devmath_pow_third(const double *x, long n, double *y) {
    Dev d(n);
    const double *dx = d.in(x, n);
    double *dy = d.out(y, n);
    if (d.ok())
        k_pow_third<<<gridFor(n), BLOCK>>>(dx, n, dy);
    return d.finish();
}

int devmath_acos(const double *x, long n, double *y) {
    Dev d(n);
    const double *dx = d.in(x, n);
    double *dy = d.out(y, n);
    if (d.ok())
        k_acos<<<gridFor(n), BLOCK>>>(dx, n, dy);
    return d.finish();
}

int devmath_solve_quadratic(const double *abc, long n, int32_t *count, double *roots) {
    Dev d(n);
    const double *di = d.in(abc, 3*n);
    int32_t *dc = d.out(count, n);
    double *dr = d.out(roots, 2*n);
    if (d.ok())
        k_solve_quadratic<<<gridFor(n), BLOCK>>>(di, n, dc, dr);
    return d.finish();
}

int devmath_solve_cubic_normed_pre(const double *in, long n, int32_t *count, double *roots, int32_t *branch) {
    Dev d(n);
    const double *di = d.in(in, 5*n);
    int32_t *dc = d.out(count, n);
    double *dr = d.out(roots, 3*n);
    int32_t *db = d.out(branch, n);
    if (d.ok())
        k_solve_cubic_normed_pre<<<gridFor(n), BLOCK>>>(di, n, dc, dr, db);
    return d.finish();
}

int devmath_signed_distance(const double *pts, const int32_t *type, const double *org, long n, double *out, int32_t *flags) {
    Dev d(n);
    const double *dp = d.in(pts, 8*n);
    const int32_t *dt = d.in(type, n);
    const double *dg = d.in(org, 2*n);
    double *dout = d.out(out, 3*n);
    int32_t *df = d.out(flags, n);
    if (d.ok())
        k_signed_distance<<<gridFor(n), BLOCK>>>(dp, dt, dg, n, dout, df);
    return d.finish();
}

int devmath_map_distance(const double *scale, const double *translate, const double *dist, long n, float *out) {
    Dev d(n);
    const double *ds = d.in(scale, n), *dt = d.in(translate, n), *dd = d.in(dist, n);
    float *dout = d.out(out, n);
    if (d.ok())
        k_map_distance<<<gridFor(n), BLOCK>>>(ds, dt, dd, n, dout);
    return d.finish();
}

int devmath_float_above(const double *x, long n, float *out) {
    Dev d(n);
    const double *dx = d.in(x, n);
    float *dout = d.out(out, n);
    if (d.ok())
        k_float_above<<<gridFor(n), BLOCK>>>(dx, n, dout);
    return d.finish();
}

int devmath_wave_min(const float *v, long n, int which, float *out) {
    Dev d(n);
    const float *dv = d.in(v, n);
    float *dout = d.out(out, n);
    if (d.ok())
        k_wave_min<<<gridFor(n), BLOCK>>>(dv, n, which, dout);
    return d.finish();
}

int devmath_row_rank(const uint32_t *key, long n, int32_t *out) {
    Dev d(n);
    const uint32_t *dk = d.in(key, n);
    int32_t *dout = d.out(out, n);
    if (d.ok())
        k_row_rank<<<gridFor(n), BLOCK>>>(dk, n, dout);
    return d.finish();
}

}
