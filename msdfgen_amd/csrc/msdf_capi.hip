// msdf_capi.hip -- implementation of the C ABI declared in include/msdfgen_hip.h (libmsdfgen_hip.so).
// Host side of the MI355X MSDF hot path: device binding, batch upload + on-device digestion, kernel dispatch, and the
// single-shape host-pointer entry points that stand in for the reference's generate* / msdfErrorCorrection functions.
// There is deliberately no CPU compute path in this file: without a gfx950 device every compute call fails.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <sched.h>

#include "msdf_boxslots.hpp"
#include "msdf_classplan.hpp"
#include "msdf_gather.hpp"
#include "msdf_gatherplan.hpp"
#include "msdf_groupplan.hpp"
#include "msdf_hostplan.hpp"
#include "msdf_kernels.hpp"
#include "msdf_launchplan.hpp"
#include "msdf_prepplan.hpp"
#include "msdf_qualityplan.hpp"
#include "msdf_resources.hpp"
#include "msdf_single.hpp"
#include "msdf_sizedplan.hpp"

using namespace msdfhip;

namespace {

thread_local std::string tlsError;
std::atomic<int> gDevice(-1);
std::atomic<int> gLdsLimit(0);
std::atomic<int> gTiming(0);

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    tlsError = buf;
    return code;
}

// The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), in order WITHIN a queue: the host-output
// pipeline's three chunk streams (plus the caller's own streams) then alias, and a chunk's kernels wait for another chunk's 100 MB copy
// (measured with MSDFHIP_PIPELINE_TRACE: 12.0 -> 10.2 ms per 8 192 glyphs with 8 queues). The variable is read when the runtime initialises
// and belongs to the HOST PROCESS: the library does not touch the environment (round 3 called setenv from a load-time constructor --
// not thread-safe against the host's other threads, and a silent change for every other HIP user of the process). INTEGRATION.md,
// "environment", recommends GPU_MAX_HW_QUEUES=8; msdfgen_amd/lib.py (the Python host of the tests and the bench) sets it before HIP starts.

static long long nowNsEarly() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Measurement / experiment knobs from the environment, read ONCE (first use, or msdfhip_reload_tuning() -- tests and A/B scripts flip them
// between calls); the launch paths never touch getenv.
struct Tuning {
    PlanTuning plan;                 // what the launch plans read (msdf_launchplan.hpp)
    bool pipelineTrace;              // MSDFHIP_PIPELINE_TRACE      host-output pipeline prints per chunk when its kernels / its copy back finished (stderr)
    int microbatch;                  // MSDFHIP_MICROBATCH          0 / 1 disables the grouping of concurrent single-shape calls; N caps the group
    double microbatchMaxPad;         // MSDFHIP_MICROBATCH_MAX_PAD  calls of different bitmap sizes share a group while n*W*H <= this * sum of w*h (msdf_groupplan.hpp); below 1: equal sizes only
    bool noArgPayloadSingle;         // MSDFHIP_NO_ARG_PAYLOAD_SINGLE k_single_call reads small shapes from the staging area instead of its kernel arguments (A/B)
    bool noZeroCopySingle;           // MSDFHIP_NO_ZERO_COPY_SINGLE k_single_call on uploaded inputs / device outputs + one copy back (A/B)
    bool noFusedSingle;              // MSDFHIP_NO_FUSED_SINGLE     single-shape calls through the batched launch sequence instead of k_single_call (A/B)
    char devices[256];               // MSDFHIP_DEVICES             "all" | "0,1,..." devices the single-shape front door spreads over
    int pipelineDepth;               // MSDFHIP_PIPELINE_DEPTH      chunks of the host-output pipeline whose kernels may run at the same time (2; at most PIPE_SLOTS-1)
    bool prepLargeTier;              // MSDFHIP_PREP_LARGE_TIER     tests: the colouring kernel always with its 2 048-edge LDS tables (default: 256-edge tier when no contour is longer)
    int hostThreads;                 // MSDFHIP_HOST_THREADS        host threads of the streamed generator's flatten pool (0 = the usable cores, at most 32); read when the pool is created
    long singleSpinLimit;            // MSDFHIP_SINGLE_SPIN_LIMIT   tests: iterations k_single_call's grid barrier waits before it gives up (0 = scaled with the shape)
    bool singleVerbose;              // MSDFHIP_SINGLE_VERBOSE      report abandoned fused launches on stderr
    size_t errorWorkspaceBytes;      // MSDFHIP_ERROR_WORKSPACE_MB  list workspace of one launch of the error estimate, in MB (512; fractions allowed: tests put the chunk boundary at small sizes)
};
// Published through an atomic pointer: msdfhip_reload_tuning() builds a fresh table and swaps it in while launch paths on other threads keep
// reading the one they loaded. Superseded tables stay alive -- a thread may still hold a reference -- in gTuningTables (a few hundred bytes per
// reload; tests and A/B scripts only), which also keeps them reachable for leak checkers.
std::atomic<const Tuning *> gTuning(NULL);
std::mutex gTuningMutex;
std::vector<Tuning *> gTuningTables;                             // every table ever published (guarded by gTuningMutex)

void readTuning() {
    Tuning &t = *new Tuning;
    PlanTuning &p = t.plan;                                      // (at its defaults)
    const char *env;
    p.resLdsBudget = (env = getenv("MSDFHIP_RES_LDS_BUDGET")) ? (size_t) atol(env) : p.resLdsBudget;
    p.persistentRounds = (env = getenv("MSDFHIP_PERSISTENT_ROUNDS")) ? atol(env) : p.persistentRounds;
    p.serialClasses = getenv("MSDFHIP_SERIAL_CLASSES") != NULL;
    p.hasQueryLds = (env = getenv("MSDFHIP_QUERY_LDS")) != NULL;
    if (env)
        sscanf(env, "%d,%d", &p.querySlotCap, &p.queryLpcContours);
    p.hasQueryPolicy = (env = getenv("MSDFHIP_QUERY_POLICY")) != NULL;
    if (env)
        sscanf(env, "%d,%d,%d,%d,%f,%f", &p.qpEdgeCost, &p.qpMaxEdges, &p.qpMinCount, &p.qpWideMaxEdges, &p.qpWideLoad, &p.qpWideMeanCount);
    p.signCap = (env = getenv("MSDFHIP_SIGN_CAP")) ? (size_t) atol(env) : p.signCap;
    if (p.signCap < 3)                                           // one edge's intersections per row: below, the sign pass's chunks would hold no edge
        p.signCap = 3;
    t.pipelineTrace = getenv("MSDFHIP_PIPELINE_TRACE") != NULL;
    t.microbatch = (env = getenv("MSDFHIP_MICROBATCH")) ? atoi(env) : 256;
    if (t.microbatch < 1)
        t.microbatch = 1;
    // 5 is the padding of a real font's boxes, 1/0.202, not a fitted value: the one crossover sweep there is (profiles/microbatch_sizes.md (c):
    // one L x L call with 63 8 x 8 calls, driven from Python threads) has a group winning up to a padding of 51 and level from 58, half of which would be
    // 25-29. The sweep's baseline is too loose to raise the default on; at 5 a font's calls group already (97 % of them from 64 threads).
    t.microbatchMaxPad = (env = getenv("MSDFHIP_MICROBATCH_MAX_PAD")) ? atof(env) : 5.;
    t.devices[0] = 0;
    p.queryStatic = (env = getenv("MSDFHIP_QUERY_STATIC")) ? atoi(env) : p.queryStatic;
    p.queryGridSteps = (env = getenv("MSDFHIP_QUERY_GRID")) ? atoi(env) : p.queryGridSteps;
    p.queryBatch = (env = getenv("MSDFHIP_QUERY_BATCH")) && atoi(env) > 0 ? atoi(env) : p.queryBatch;
    t.noFusedSingle = getenv("MSDFHIP_NO_FUSED_SINGLE") != NULL;
    t.noZeroCopySingle = getenv("MSDFHIP_NO_ZERO_COPY_SINGLE") != NULL;
    t.noArgPayloadSingle = getenv("MSDFHIP_NO_ARG_PAYLOAD_SINGLE") != NULL;
    p.shortRounds = (env = getenv("MSDFHIP_SHORT_ROUNDS")) ? atol(env) : p.shortRounds;
    p.persistentGrid = (env = getenv("MSDFHIP_PERSISTENT_GRID")) ? atol(env) : p.persistentGrid;
    p.shareGridFactor = (env = getenv("MSDFHIP_SHARE_GRID")) ? atof(env) : p.shareGridFactor;
    p.smallLaunchTiles = (env = getenv("MSDFHIP_SMALL_LAUNCH_TILES")) ? atol(env) : p.smallLaunchTiles;
    if ((env = getenv("MSDFHIP_DEVICES")))
        snprintf(t.devices, sizeof(t.devices), "%s", env);
    p.smallMaxEdges = (env = getenv("MSDFHIP_SMALL_MAX_EDGES")) && atoi(env) > 0 ? atoi(env) : p.smallMaxEdges;
    p.ldsClassTpw = (env = getenv("MSDFHIP_LDS_CLASS_TPW")) && atoi(env) == 1 ? 1 : 4;
    t.pipelineDepth = (env = getenv("MSDFHIP_PIPELINE_DEPTH")) && atoi(env) >= 1 && atoi(env) <= 3 ? atoi(env) : 2;
    t.prepLargeTier = getenv("MSDFHIP_PREP_LARGE_TIER") != NULL;
    t.hostThreads = (env = getenv("MSDFHIP_HOST_THREADS")) && atoi(env) > 0 ? atoi(env) : 0;
    t.singleSpinLimit = (env = getenv("MSDFHIP_SINGLE_SPIN_LIMIT")) && atol(env) > 0 ? atol(env) : 0;
    t.singleVerbose = getenv("MSDFHIP_SINGLE_VERBOSE") != NULL;
    t.errorWorkspaceBytes = (env = getenv("MSDFHIP_ERROR_WORKSPACE_MB")) && atof(env) > 0 && atof(env) <= 65536 ? (size_t) (atof(env)*(double) (1u<<20)) : (size_t) 512u<<20;
    gTuningTables.push_back(&t);                                 // (callers hold gTuningMutex)
    gTuning.store(&t, std::memory_order_release);
}

const Tuning &tuning() {
    const Tuning *t = gTuning.load(std::memory_order_acquire);
    if (!t) {
        std::lock_guard<std::mutex> lock(gTuningMutex);
        if (!gTuning.load(std::memory_order_acquire))
            readTuning();
        t = gTuning.load(std::memory_order_acquire);
    }
    return *t;
}

// Which launch route the batched passes took (msdfhip_debug_route_counts; indices MSDFHIP_ROUTE_* of msdfgen_hip.h): bumped on the host at each launch site
// once the launch is issued, per launch site rather than per kernel instance (the small overlapping route and the direct global-scratch class share one).
std::atomic<unsigned long long> gRouteCounts[MSDFHIP_ROUTE_COUNT];

inline void countRoute(int route) { gRouteCounts[route].fetch_add(1, std::memory_order_relaxed); }

#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (void) hipGetLastError(); return fail(MSDFHIP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } } while (0)

// Binds the calling thread to `dev` (>= 0: the device a batch lives on) or to the process default (msdfhip_init; device 0 if never called).
int ensureDevice(int dev = -1) {
    if (gDevice.load() < 0) {
        int rc = msdfhip_init(0);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    if (dev < 0)
        dev = gDevice.load();
    else if (dev != gDevice.load()) {                            // another device of the node: it must be a gfx950 too (checked once per device)
        static std::atomic<unsigned long long> checked(0);
        if (dev >= 64 || !((checked.load()>>dev)&1ull)) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
                (void) hipGetLastError();
                return fail(MSDFHIP_ERR_NO_DEVICE, "hipGetDeviceProperties(%d) failed", dev);
            }
            if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
                return fail(MSDFHIP_ERR_NO_DEVICE, "device %d is %s; libmsdfgen_hip is built for gfx950 (MI355X) only", dev, prop.gcnArchName);
            if (dev < 64)
                checked.fetch_or(1ull<<dev);
        }
    }
    if (hipSetDevice(dev) != hipSuccess) {
        (void) hipGetLastError();                                // HIP's last error is sticky: do not leave it for an unrelated later check
        return fail(MSDFHIP_ERR_NO_DEVICE, "hipSetDevice(%d) failed", dev);
    }
    return MSDFHIP_OK;
}

// For the entry points that only receive device pointers: bind to the device that owns `p`.
int ensureDeviceOf(const void *p) {
    hipPointerAttribute_t attr;
    if (p && hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice)
        return ensureDevice(attr.device);
    (void) hipGetLastError();
    return ensureDevice();
}

int currentDevice() {
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess ? dev : 0;
}

int channelsOf(int mode) { return mode <= 2 ? 1 : mode; }

struct TimedLaunch { hipEvent_t a, b; int kind; };
std::mutex gTimingMutex;
std::vector<TimedLaunch> gTimed;

struct ScopedTimer {
    hipStream_t stream;
    TimedLaunch t;
    bool on;
    ScopedTimer(hipStream_t s, int kind, bool enabled = true) : stream(s), on(enabled && gTiming.load() != 0) {
        t.kind = kind;
        if (on) {
            if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess) { on = false; return; }
            hipEventRecord(t.a, stream);
        }
    }
    ~ScopedTimer() {
        if (on) {
            hipEventRecord(t.b, stream);
            std::lock_guard<std::mutex> lock(gTimingMutex);
            gTimed.push_back(t);
        }
    }
};

// What the launches on one batch (or on one glyph range after the other: pipeline slots, single-shape groups) work in. Launches on one batch are
// ordered by the caller; the mutex guards the buffers against concurrent callers that only size them.
struct Workspace {
    int device = 0;
    std::mutex mutex;
    WorkBuffer<float> scratch;        // intermediate fields of a generate call whose caller brought no scratch
    WorkBuffer<EcCandidate> deferred; // [0] = header (count), [1..] = distance checks deferred to k_ec_query, then its work list and k_ec_params' corner list
    WorkBuffer<EcGlyphParams> ecParams;   // per glyph: constants of the error-correction pass
    WorkBuffer<double> gres;          // global combiner scratch for glyphs whose contour count exceeds what LDS can hold
    WorkBuffer<unsigned> workQueue;   // item counters of the persistent distance launch: TWO sets of 8 per-XCD counters, 64 bytes apart; zeroed once by the host, then each launch zeroes the set the NEXT one uses
    unsigned queueParity = 0;         // which set the next persistent launch draws from
    WorkBuffer<int> bucket;           // per glyph: the class list (msdf_classplan.hpp) of the batch's ClassPlan
    WorkBuffer<int, true> hBucket;    // pinned host copy the list is uploaded from, ON THE LAUNCH STREAM (a synchronous copy of pageable memory may
                                      // still be in flight on the null stream when a kernel of a non-blocking stream starts)
    int bucketKey = -1;               // the contour limit and edge bound the list in `bucket` was built for (-1: none)
    bool bucketUploaded = false;      // an upload from hBucket may still be in flight
    WorkBuffer<int> ecOrder;          // glyph indices heaviest first (k_ec_scan / k_ec_query), built on first use; none: batch order
    WorkBuffer<int, true> hEcOrder;   // (pinned host copy it is uploaded from)
    Event ecOrderReady;               // (recorded behind that upload)
    bool ecOrderTried = false;
    WorkBuffer<int32_t> boxDims;      // msdfhip_batch_generate_sized: w_g, h_g per glyph, uploaded per call on the call's stream in front of its first launch
    WorkBuffer<int32_t, true> hBoxDims;   // (pinned host copy it is uploaded from)
    Event boxDimsRead;                // (recorded behind that upload: the next call waits for it before it rewrites hBoxDims)
    Stream sideStream[2];             // the three glyph classes of the distance pass run concurrently: two of them on these (fork / join by events)
    Event forkEvent, joinEvent[2];

    size_t reservedGlyphs = 0;        // the per-glyph buffers (bucket, hBucket, ecParams) are allocated for ranges of at least this many glyphs

    // A new glyph range follows (a pipeline slot is pointed at its next chunk): the class list is not its list. The caller has seen the range before it
    // finish -- the pipeline waits for the slot's `done` event, recorded behind everything of its previous chunk -- so no upload still reads hBucket.
    void newGlyphRange() { bucketKey = -1, bucketUploaded = false; }
    // Glyph ranges of up to n glyphs follow (a pipeline slot: a full chunk, whatever the length of its first one). Nothing of the workspace is in flight.
    void reserveGlyphs(size_t n) {
        bucket.release(), hBucket.release(), ecParams.release();   // (allocated again by the launches that need them)
        reservedGlyphs = n;
        newGlyphRange();
    }
    size_t glyphCapacity(int nGlyphs) const { return std::max(std::max((size_t) (nGlyphs > 0 ? nGlyphs : 0), reservedGlyphs), (size_t) 1); }
    // No destructor of its own: the members release what they own on the thread's current device -- whoever destroys a batch or a pooled pipe binds
    // `device` first -- and a view over an arena that never had to grow owns nothing: no device call at all.
};

// The shapes of a batch, fixed once it is digested: CSR arrays and edge records on the device, per-glyph counts on the host.
struct ShapeData {
    int nGlyphs = 0, nContours = 0, nEdges = 0, maxContours = 0, maxEdges = 0;
    // Each array is the batch's own (created from host arrays, prepared, digested) or borrowed: the caller's device arrays, the parent batch of a
    // glyph range, a range of an arena or of a pipeline slot.
    WorkBuffer<int32_t> dGlyphContourOffsets, dContourOffsets;
    WorkBuffer<double> dPoints;
    WorkBuffer<uint8_t> dTypes, dColors;
    WorkBuffer<EdgeRec> dRecs;
    WorkBuffer<int8_t> dWindings;
    mutable std::vector<int> hContours, hEdges;   // contours / edges per glyph (batches of device arrays: fetched on first need, fetchGlyphCounts)
    void countMaxima() {                          // maxContours / maxEdges of the per-glyph counts
        maxContours = maxEdges = 0;
        for (size_t g = 0; g < hContours.size(); ++g)
            maxContours = std::max(maxContours, hContours[g]), maxEdges = std::max(maxEdges, hEdges[g]);
    }
    void setCounts(const int *contours, const int *edges, int n) {
        hContours.assign(contours, contours+n), hEdges.assign(edges, edges+n);
        countMaxima();
    }
};

} // namespace

struct MsdfHipBatch : ShapeData {
    int device = 0;                   // the HIP device the batch lives on; every call on the batch binds the calling thread to it
    bool serialClasses = false;       // launch the glyph classes one after the other on the caller's stream (host-output pipeline: its chunks overlap instead)
    mutable WorkBuffer<double> dBounds;   // [nGlyphs][4] l, b, r, t of Shape::getBounds (msdfhip_batch_bounds / _frame; allocated on first need, the batch's own)
    bool boundsFixed = false;         // dBounds were taken at creation from the normalized edges (batches prepared from raw outlines: the arrays they keep are the coloured ones)
    mutable WorkBuffer<double> dBoxes;    // what k_box writes (msdfhip_batch_bounds_miters / _boxes): ext [n][4], xf [n][6], then wh [n][2] int32; allocated on first need
    mutable Workspace work;
    mutable ClassPlan plan;           // the classes of work.bucket
    WorkBuffer<int32_t> gatherTable;  // a batch gathered from others (msdfhip_batch_gather): the table its copy kernels read (msdf_gatherplan.hpp) ...
    WorkBuffer<int32_t, true> hGatherTable;   // ... and the pinned copy it is uploaded from on the call's stream; both go with the batch, so nobody waits for the upload
    void onDevice(int d) { device = work.device = d; }
};

namespace {

// What one generate call passes down its launch chain. Each caller builds it on its stack: nothing of a call, failed or not, stays on the batch.
struct GenerateCall {
    bool ecParamsQueued = false;      // k_ec_params of THIS request is already queued on the call's stream (prepareAhead, or next to the distance pass): launchEc skips it
    hipEvent_t afterDistance = NULL;  // host-output pipeline: recorded on the call's stream between the distance pass and what follows it (NULL: not wanted)
    unsigned *overflowOut = NULL;     // pipeline chunks, single-shape calls: where k_ec_query mirrors the candidate-overflow count (then no k_ec_slow launch)
    bool overflowMirrored = false;    // out: the correction pass did so
    bool ecShapeRows = false;         // the correction pairs protectEdges' texels along the shape's rows (EcParams::shapeRows): a legacy generator without the sign pass
    const int32_t *boxDims = NULL;    // msdfhip_batch_generate_sized: the device copy of the per-glyph box sizes (w, h below are then the slot's W, H); the sized kernels launch
};

BatchView viewOf(const MsdfHipBatch *b) {
    BatchView v;
    v.nGlyphs = b->nGlyphs;
    v.glyphContourOffsets = b->dGlyphContourOffsets.ptr;
    v.contourOffsets = b->dContourOffsets.ptr;
    v.recs = b->dRecs.ptr;
    v.windings = b->dWindings.ptr;
    return v;
}

int digest(MsdfHipBatch *b, hipStream_t stream) {
    HIPCHK(b->dRecs.ensure((size_t) (b->nEdges > 0 ? b->nEdges : 1)));          // (a view borrows room for them: nothing to do)
    HIPCHK(b->dWindings.ensure((size_t) (b->nContours > 0 ? b->nContours : 1)));
    const int edgeBlocks = (b->nEdges+255)/256, contourBlocks = (b->nContours+255)/256;
    if (edgeBlocks+contourBlocks > 0)                            // records and windings in one launch
        hipLaunchKernelGGL(k_prep_records, dim3(edgeBlocks+contourBlocks), dim3(256), 0, stream, b->dRecs.ptr, b->nEdges, b->nContours,
                           b->dContourOffsets.ptr, b->dPoints.ptr, b->dTypes.ptr, b->dColors.ptr, b->dWindings.ptr, edgeBlocks);
    HIPCHK(hipGetLastError());
    return MSDFHIP_OK;
}

// A batch's own copy of a host array: room for `alloc` elements (never none), the first `used` uploaded.
template <class T>
hipError_t uploadNew(WorkBuffer<T> &dst, const T *src, size_t alloc, size_t used) {
    const hipError_t e = dst.ensure(alloc);
    return e == hipSuccess && used ? hipMemcpy(dst.ptr, src, used*sizeof(T), hipMemcpyHostToDevice) : e;
}

int fetchGlyphCounts(const MsdfHipBatch *b) {             // device-array batches: the per-glyph counts are read back once
    if (!b->hContours.empty() || b->nGlyphs == 0)
        return MSDFHIP_OK;
    std::vector<int32_t> gco((size_t) b->nGlyphs+1), co((size_t) b->nContours+1);
    HIPCHK(hipMemcpy(gco.data(), b->dGlyphContourOffsets.ptr, sizeof(int32_t)*gco.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(co.data(), b->dContourOffsets.ptr, sizeof(int32_t)*co.size(), hipMemcpyDeviceToHost));
    b->hContours.resize((size_t) b->nGlyphs);
    b->hEdges.resize((size_t) b->nGlyphs);
    for (int g = 0; g < b->nGlyphs; ++g) {
        b->hContours[g] = gco[g+1]-gco[g];
        b->hEdges[g] = co[gco[g+1]]-co[gco[g]];
    }
    return MSDFHIP_OK;
}

static_assert(PLAN_TILE == TILE && PLAN_WAVE == WAVE && PLAN_QUAD == QUAD && PLAN_DISTANCE_WAVES_PER_SIMD == MSDF_DISTANCE_WAVES_PER_SIMD &&
              PLAN_SIMPLE_WAVES_PER_SIMD == MSDF_SIMPLE_WAVES_PER_SIMD && PLAN_SIGN_ROWS == SIGN_ROWS && PLAN_PB_SLOT_BYTES == sizeof(PBSlot),
              "msdf_launchplan.hpp plans for other kernels than those of msdf_kernels.hpp");

// Compute units of a device (4 SIMDs each): the number of wavefronts of a W-waves-per-SIMD kernel it holds at once is residentSlots()*4*W.
int residentSlots(int device) {
    static std::atomic<int> cus[64];
    if (device < 0 || device >= 64)
        return 256;
    int n = cus[device].load();
    if (!n) {
        hipDeviceProp_t prop;
        n = hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        cus[device].store(n);
    }
    return n;
}

// Workgroups of `kernel` (blockThreads threads, lds bytes of dynamic LDS) the device holds at once: occupancy per compute unit x compute units, looked
// up once per `slot` of the caller's cache (one gfx950 is like another: not keyed by device). 0: unknown.
int residentBlocks(std::atomic<int> &slot, int device, const void *kernel, int blockThreads, size_t lds) {
    int v = slot.load();
    if (!v) {
        int perCu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kernel, blockThreads, lds) != hipSuccess) {
            (void) hipGetLastError();
            perCu = 0;
        }
        v = perCu > 0 ? perCu*residentSlots(device) : -1;
        slot.store(v);
    }
    return v > 0 ? v : 0;
}

// What the launch plans (msdf_launchplan.hpp) read: built per call, on its stack.
PlanEnv planEnv(int device) {
    const PlanEnv env = { tuning().plan, (size_t) gLdsLimit.load(), residentSlots(device) };
    return env;
}
GlyphCounts countsOf(const MsdfHipBatch *b) {
    const GlyphCounts c = { b->nGlyphs, b->maxContours, b->maxEdges };
    return c;
}
int failTooComplex(const LdsPlan &plan, const PlanEnv &env) {
    return fail(MSDFHIP_ERR_TOO_COMPLEX, "a glyph has %d contours / %d edges: the survivor lists need %zu B of LDS per wavefront, device limit is %zu B",
                plan.maxContours, plan.listStride, plan.bytes, env.ldsLimit);
}

template <class K>
int setLds(K kernel, size_t bytes) {
    if (bytes > 64*1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes));
    return MSDFHIP_OK;
}

// The work queue of the persistent distance launch. Zeroing it with a memset in front of every launch put a tiny kernel at the head of the class's launch
// chain -- rocprofv3 shows `__amd_rocclr_fillBufferAligned` at 49 us on average (up to 83) per step: it waits for wavefront slots next to the other classes'
// launches like every small kernel between large ones. A batch now owns TWO sets of counters and its launches alternate between them: a launch draws from one
// and zeroes the other (distanceBody), so the host zeroes them once, when a batch (or pipeline view) first needs them. (Launches on one batch are ordered
// on the caller's stream, as they always had to be: they share the batch's workspaces.) Their one-time zeroing goes onto the stream of the first launch.
int ensureWorkQueue(const MsdfHipBatch *b, unsigned **out, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(b->work.mutex);
    WorkBuffer<unsigned> &q = b->work.workQueue;
    if (!q.ptr) {
        HIPCHK(q.ensure(64));
        // Zeroed ON THE STREAM of the launch that needs it first, i.e. ordered in front of that launch. (hipMemset would run on the legacy default stream, which
        // a non-blocking stream does not wait for, and may return before it has run: the counters could be zeroed UNDER the first launch -- the race the
        // sanitizer run of round 4 found in the single-call arenas, DESIGN.md 3.9. Later launches on this batch are ordered behind the first by the caller, as
        // they always had to be: they share the batch's workspaces.)
        const hipError_t e = hipMemsetAsync(q.ptr, 0, 256, stream);
        if (e != hipSuccess) {
            q.release();
            return fail(MSDFHIP_ERR_HIP, "work queue of the persistent launch: %s", hipGetErrorString(e));
        }
    }
    *out = q.ptr;
    return MSDFHIP_OK;
}

int ensureGres(const MsdfHipBatch *b, size_t bytes, double **out) {
    std::lock_guard<std::mutex> lock(b->work.mutex);
    HIPCHK(b->work.gres.ensure((bytes+sizeof(double)-1)/sizeof(double)));
    *out = b->work.gres.ptr;
    return MSDFHIP_OK;
}

// f(integral_constant<int, V>) for the V among VALUES that `value` equals; false if it equals none. f's instantiations are named in the order of VALUES
// (as with forDistanceVariant below, that order is the order of the kernels in the code object).
template <int... VALUES, class F>
bool forOneOf(int value, F &&f) {
    return (... || (value == VALUES ? (f(std::integral_constant<int, VALUES>()), true) : false));   // (a LEFT fold: the compiler expands a right fold from its last operand)
}

// The sized twins of the generate kernels (msdfhip_batch_generate_sized). A twin takes its uniform sibling's arguments and the boxes' sizes behind them: its
// pointer type is derived from the sibling's (sizedTwinOf, only ever declared), and the two are launched from ONE argument list (launchTwinned). The functions
// that look a twin up are defined at the END of this file: nothing in front of them names a twin, so the twins are instantiated behind every kernel the code
// object has always held (the order of the instantiations matters). All instantiations of one kernel template share a signature, hence one pointer type each.
template <class... A>
auto sizedTwinOf(void (*)(A...)) -> void (*)(A..., const int32_t *);
decltype(sizedTwinOf(k_distance<1, false, false, 1>)) distanceSizedKernel(int sel, bool overlap, bool gres, int tpw);
decltype(sizedTwinOf(k_distance_unculled<1, false>)) unculledSizedKernel(int sel, bool overlap);
decltype(sizedTwinOf(k_ec_slow<3, false, false>)) ecSlowSizedKernel(int n, bool overlap, bool gres);
decltype(sizedTwinOf(k_ec_fast<3, false>)) ecFastSizedKernel(int n, bool lazy);
decltype(sizedTwinOf(k_ec_query<3, false>)) ecQuerySizedKernel(int n, bool overlap);
decltype(sizedTwinOf(k_sign_correction<1>)) signSizedKernel(int n);
// (the quality calls: msdfhip_batch_estimate_sdf_error_sized, msdfhip_render_sdf_sized. Their twins take the call's device table in the place of the sizes.)
decltype(sizedTwinOf(k_sdf_error_lines<1>)) errorLinesSizedKernel(int n);
decltype(sizedTwinOf(k_sdf_error_sum)) errorSumSizedKernel();
decltype(sizedTwinOf(k_render_sdf<1, 1>)) renderSizedKernel(int no, int ns);

// One launch of a generate kernel (workgroups of one wavefront): of `uniform`, or in a sized call (dDims) of its twin, with dDims behind the same arguments.
// A... comes from the uniform kernel alone. The twin must be exactly void (*)(A..., const int32_t *): one that drifts from its sibling does not compile.
// The arguments are not deduced but taken as A..., so NULL, 0u and the like convert as they would in a direct call.
template <class... A>
void launchTwinned(void (*uniform)(A...), void (*twin)(A..., const int32_t *), const int32_t *dDims, dim3 grid, size_t lds, hipStream_t stream,
                   std::enable_if_t<true, A>... args) {
    if (dDims)
        hipLaunchKernelGGL(twin, grid, dim3(WAVE), lds, stream, args..., dDims);
    else
        hipLaunchKernelGGL(uniform, grid, dim3(WAVE), lds, stream, args...);
}
// (the same for a kernel of `block` threads per workgroup and no LDS: k_render_sdf)
template <class... A>
void launchTwinnedBlock(void (*uniform)(A...), void (*twin)(A..., const int32_t *), const int32_t *dDims, dim3 grid, dim3 block, hipStream_t stream,
                        std::enable_if_t<true, A>... args) {
    if (dDims)
        hipLaunchKernelGGL(twin, grid, block, 0, stream, args..., dDims);
    else
        hipLaunchKernelGGL(uniform, grid, block, 0, stream, args...);
}
template <class... A>
int setLdsTwinned(void (*uniform)(A...), void (*twin)(A..., const int32_t *), const int32_t *dDims, size_t bytes) {
    return dDims ? setLds(twin, bytes) : setLds(uniform, bytes);
}

// One planned launch of the distance pass (msdf_launchplan.hpp: planDistance); counts its route once it is issued.
template <int SEL, bool OVERLAP, bool GRES, int TPW_>
int launchDistance(const MsdfHipBatch *b, const MsdfHipGlyph *dGlyphs, int w, int h, float *dst, int toScratch, const DistanceLaunch &l, const PlanEnv &env,
                   hipStream_t stream, const int32_t *dDims = NULL) {
    const size_t blocks = distanceBlocks(l.count, w, h, TPW_);
    if (blocks == 0)
        return MSDFHIP_OK;
    if (blocks > 0x7fffffffull)
        return fail(MSDFHIP_ERR_INVALID, "launch of %zu tile quads exceeds the grid limit; split the batch", blocks);
    const auto twin = distanceSizedKernel(SEL, OVERLAP, GRES, TPW_);
    int rc = setLdsTwinned(k_distance<SEL, OVERLAP, GRES, TPW_>, twin, dDims, l.lds.bytes);
    if (rc != MSDFHIP_OK)
        return rc;
    const GridPlan grid = gridOf(l, w, h, env);
    DistanceArgs args;
    args.batch = viewOf(b), args.glyphs = dGlyphs, args.width = w, args.height = h, args.tilesX = (w+TILE-1)/TILE, args.tilesPerGlyph = tilesOf(w, h);
    args.maxEdges = l.lds.listStride, args.dst = dst, args.toScratch = toScratch, args.blockBase = 0, args.gres = NULL, args.gresStride = 0;
    args.glyphMap = l.mapped ? b->work.bucket.ptr+l.offset : NULL, args.nMapped = l.mapped ? l.count : 0, args.workQueue = NULL, args.workItems = 0;
    if (grid.gresBytes) {
        rc = ensureGres(b, grid.gresBytes, &args.gres);
        if (rc != MSDFHIP_OK)
            return rc;
        args.gresStride = l.lds.resBytes/sizeof(double);
    }
    const auto launch = [&](size_t groups) {                     // (args as they stand when it is called)
        const DistanceArgs &a = args;
        launchTwinned(k_distance<SEL, OVERLAP, GRES, TPW_>, twin, dDims, dim3((unsigned) groups), l.lds.bytes, stream, a.batch.nGlyphs, a.batch.glyphContourOffsets,
                      a.batch.contourOffsets, a.batch.recs, a.batch.windings, a.glyphs, a.width, a.height, a.tilesX, a.tilesPerGlyph, a.maxEdges, a.dst, a.toScratch,
                      a.blockBase, a.gres, a.gresStride, a.glyphMap, a.nMapped, a.workQueue, a.workItems);
    };
    if (grid.persistent) {
        unsigned *queue = NULL;
        rc = ensureWorkQueue(b, &queue, stream);
        if (rc != MSDFHIP_OK)
            return rc;
        // The parity is read and flipped under the batch's scratch mutex, and flipped only once the launch has been ISSUED: a launch that fails to
        // be issued has neither dirtied its own set nor zeroed the other, so the next launch must draw from the same (still zero) set again --
        // flipped up front, it would draw from the set the last successful launch left dirty and render no tile of the class.
        // Launches on one batch are ordered by the caller (they share the batch's workspaces).
        std::lock_guard<std::mutex> lock(b->work.mutex);
        args.workQueue = queue+(b->work.queueParity ? 16 : 0);    // (the kernel finds the other set at `queue ^ 64 bytes`)
        args.workItems = (unsigned) blocks;
        launch(grid.chunk);
        HIPCHK(hipGetLastError());
        b->work.queueParity ^= 1u;
    } else {
        for (size_t base = 0; base < blocks; base += grid.chunk) {
            args.blockBase = (unsigned) base;
            launch(blocks-base < grid.chunk ? blocks-base : grid.chunk);
        }
        HIPCHK(hipGetLastError());
    }
    countRoute(routeOf(l, grid));
    return MSDFHIP_OK;
}

// f(OVERLAP, GRES, TPW) with a planned launch's kernel variant as integral constants: the five instantiations of k_distance a selector has
// (named in the order the code object has always held them: a reordering moves every kernel behind them in the device assembly).
template <class F>
int forDistanceVariant(const DistanceLaunch &l, F &&f) {
    typedef std::integral_constant<int, 1> One;
    typedef std::integral_constant<int, (int) QUAD> Quad;
    if (!l.overlap)
        return l.gres ? f(std::false_type(), std::true_type(), One()) : f(std::false_type(), std::false_type(), Quad());
    if (l.gres)
        return f(std::true_type(), std::true_type(), One());
    return l.tpw != 1 ? f(std::true_type(), std::false_type(), Quad()) : f(std::true_type(), std::false_type(), One());
}

// Upload of a few KB from pinned host memory by a kernel instead of an SDMA copy (see k_upload_words; StreamFeeder::prepareChunk uses it the other way,
// device words into pinned memory). bytes must be a multiple of 4.
int uploadSmall(void *dst, const void *srcPinned, size_t bytes, hipStream_t stream) {
    if (bytes == 0)
        return MSDFHIP_OK;
    const size_t words = bytes/4, quads = (words+3)/4;
    const unsigned blocks = (unsigned) ((quads+255)/256 < 256 ? (quads+255)/256 : 256);
    hipLaunchKernelGGL(k_upload_words, dim3(blocks ? blocks : 1), dim3(256), 0, stream, reinterpret_cast<uint32_t *>(dst), reinterpret_cast<const uint32_t *>(srcPinned), words);
    HIPCHK(hipGetLastError());
    return MSDFHIP_OK;
}

// The class list of the overlapping combiner (msdf_classplan.hpp) for this contour limit, cached with the batch: b->work.bucket + b->plan.
int ensureBuckets(const MsdfHipBatch *b, int limit, hipStream_t stream) {
    Workspace &ws = b->work;
    std::lock_guard<std::mutex> lock(ws.mutex);
    const int bucketKey = limit+(tuning().plan.smallMaxEdges<<12);    // what the class lists depend on
    if (ws.bucketKey == bucketKey && ws.bucket.ptr)
        return MSDFHIP_OK;
    const int rcCounts = fetchGlyphCounts(b);
    if (rcCounts != MSDFHIP_OK)
        return rcCounts;
    const size_t cap = ws.glyphCapacity(b->nGlyphs);
    HIPCHK(ws.bucket.ensure(cap));
    HIPCHK(ws.hBucket.ensure(cap));
    if (ws.bucketUploaded)                                       // an earlier upload from hBucket (same batch, other limit) must have left it
        HIPCHK(hipStreamSynchronize(stream));
    const ClassPlan plan = planClasses(b->hContours.data(), b->hEdges.data(), b->nGlyphs, limit, tuning().plan.smallMaxEdges, (size_t) gLdsLimit.load(), ws.hBucket.ptr);
    const int rcUp = uploadSmall(ws.bucket.ptr, ws.hBucket.ptr, sizeof(int)*(size_t) b->nGlyphs, stream);   // (hBucket is pinned)
    if (rcUp != MSDFHIP_OK)
        return rcUp;
    ws.bucketUploaded = true;
    b->plan = plan, ws.bucketKey = bucketKey;
    return MSDFHIP_OK;
}

// The work list of the distance checks in heaviest-first order (edges x contours, like the glyph classes above): whole batches of at least
// 256 glyphs whose per-glyph counts are on the host; views of the host-output pipeline and the single-shape groups keep batch order.
int ensureEcOrder(const MsdfHipBatch *b, const int **order, hipStream_t stream) {
    Workspace &ws = b->work;
    std::lock_guard<std::mutex> lock(ws.mutex);
    *order = ws.ecOrder.ptr;
    if (ws.ecOrderTried) {
        if (ws.ecOrder.ptr && ws.ecOrderReady)                   // uploaded on the first caller's stream: any other stream waits for that (a no-op once it has landed)
            HIPCHK(hipStreamWaitEvent(stream, ws.ecOrderReady, 0));
        return MSDFHIP_OK;
    }
    ws.ecOrderTried = true;
    // (a borrowed class list marks the view of a single-shape group, which lives for one call: a list built for it would be an allocation per call)
    if (b->serialClasses || (ws.bucket.ptr && !ws.bucket.owned) || b->nGlyphs < 256 || b->hEdges.size() != (size_t) b->nGlyphs ||
        b->hContours.size() != (size_t) b->nGlyphs)
        return MSDFHIP_OK;
    const size_t bytes = sizeof(int)*(size_t) b->nGlyphs;
    // The list is an optimisation: every failure below leaves *order = NULL (batch order) and the call succeeds.
    if (ws.hEcOrder.ensure((size_t) b->nGlyphs) != hipSuccess) {  // pinned and kept with the batch: the upload is ordered on the launch stream, nobody waits
        (void) hipGetLastError();
        return MSDFHIP_OK;
    }
    int *host = ws.hEcOrder.ptr;
    for (int g = 0; g < b->nGlyphs; ++g)
        host[g] = g;
    const int *hE = b->hEdges.data(), *hC = b->hContours.data();
    std::stable_sort(host, host+b->nGlyphs, [hE, hC](int x, int y) { return (long long) hE[x]*(hC[x] > 1 ? hC[x] : 1) > (long long) hE[y]*(hC[y] > 1 ? hC[y] : 1); });
    if (ws.ecOrder.ensure((size_t) b->nGlyphs) != hipSuccess) {
        (void) hipGetLastError();
        return MSDFHIP_OK;
    }
    if (uploadSmall(ws.ecOrder.ptr, host, bytes, stream) != MSDFHIP_OK) {
        ws.ecOrder.release();
        return MSDFHIP_OK;
    }
    if (ws.ecOrderReady.create(hipEventDisableTiming) != hipSuccess || hipEventRecord(ws.ecOrderReady, stream) != hipSuccess) {
        (void) hipGetLastError();
        ws.ecOrderReady.release();
        if (hipStreamSynchronize(stream) != hipSuccess) {        // no event for the other streams to wait on: the list must have landed before it is used
            (void) hipGetLastError();
            ws.ecOrder.release();
            return MSDFHIP_OK;
        }
    }
    *order = ws.ecOrder.ptr;                                     // handed out only once it is (or is ordered to be) complete
    return MSDFHIP_OK;
}

int ensureSideStreams(const MsdfHipBatch *b) {
    Workspace &ws = b->work;
    if (ws.forkEvent)
        return MSDFHIP_OK;
    int least = 0, greatest = 0;
    (void) hipDeviceGetStreamPriorityRange(&least, &greatest);
    for (int k = 0; k < 2; ++k) {
        // The two side classes run at LOW queue priority: the long LDS-class launch on the caller's stream gets the slots first and the side
        // classes fill what it leaves, its tail included (distance pass 3.93 -> 3.80-3.88 ms; high: 4.01).
        HIPCHK(ws.sideStream[k].create(hipStreamNonBlocking, least));
        HIPCHK(ws.joinEvent[k].create(hipEventDisableTiming));
    }
    HIPCHK(ws.forkEvent.create(hipEventDisableTiming));
    return MSDFHIP_OK;
}

// The glyphs whose survivor lists exceed a CU's LDS take the list-free kernel (see k_distance_unculled): all of the batch, or those of dGlyphMap.
template <int SEL, bool OVERLAP>
int launchUnculled(const MsdfHipBatch *b, const MsdfHipGlyph *dGlyphs, int w, int h, float *dst, int toScratch, hipStream_t stream, const int *dGlyphMap = NULL,
                   int nMapped = 0, const int32_t *dDims = NULL) {
    const int tilesX = (w+TILE-1)/TILE, tiles = tilesX*((h+TILE-1)/TILE);
    const size_t items = (size_t) (dGlyphMap ? nMapped : b->nGlyphs)*(size_t) tiles;
    if (items == 0)
        return MSDFHIP_OK;
    if (items > 0xfffffff0ull)
        return fail(MSDFHIP_ERR_INVALID, "launch of %zu tiles exceeds the work-queue range; split the batch", items);
    const size_t resBytes = OVERLAP ? (size_t) (b->maxContours > 0 ? b->maxContours : 1)*SelTraits<SEL>::NCH*WAVE*sizeof(double) : 0;
    // workgroups: two per SIMD, fewer if their workspace slices would exceed 2 GB
    size_t groups = (size_t) residentSlots(b->device)*4u*2u;
    if (resBytes && groups*resBytes > ((size_t) 2<<30))
        groups = ((size_t) 2<<30)/resBytes;
    groups = groups < 1 ? 1 : groups > items ? items : groups;
    double *gres = NULL;
    int rc = ensureGres(b, groups*resBytes+256, &gres);
    if (rc != MSDFHIP_OK)
        return rc;
    unsigned *counter = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(gres)+groups*resBytes);
    HIPCHK(hipMemsetAsync(counter, 0, sizeof(unsigned), stream));
    const BatchView v = viewOf(b);
    launchTwinned(k_distance_unculled<SEL, OVERLAP>, unculledSizedKernel(SEL, OVERLAP), dDims, dim3((unsigned) groups), 0, stream, v.nGlyphs, v.glyphContourOffsets,
                  v.contourOffsets, v.recs, v.windings, dGlyphs, w, h, tilesX, tiles, dst, toScratch, gres, resBytes/sizeof(double), counter, (unsigned) items, dGlyphMap);
    HIPCHK(hipGetLastError());
    countRoute(MSDFHIP_ROUTE_DIST_UNCULLED);
    return MSDFHIP_OK;
}

int runCorrection(const MsdfHipBatch *b, int channels, int w, int h, const MsdfHipGlyph *dGlyphs, const float *src, float *out, uint8_t *stencil,
                  const MsdfHipConfig &cfg, hipStream_t stream, GenerateCall &call, bool paramsOnly = false);   // (below)
// The distance pass: planned by planDistance (msdf_launchplan.hpp), executed here.
// ecAhead: the config of the coming correction pass, whose k_ec_params may run next to the distance pass (NULL: not wanted); call.ecParamsQueued says whether it did.
template <int SEL>
int dispatchDistance(const MsdfHipBatch *b, const MsdfHipGlyph *dGlyphs, int w, int h, float *dst, int toScratch, bool overlap, hipStream_t stream,
                     const MsdfHipConfig *ecAhead, GenerateCall &call) {
    const PlanEnv env = planEnv(b->device);
    int rc = MSDFHIP_OK;
    const int limit = classListLimit(env, countsOf(b), w, h, SelTraits<SEL>::NCH, overlap);
    if (limit) {
        rc = ensureBuckets(b, limit, stream);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    const DistancePlan plan = planDistance(env, countsOf(b), w, h, SelTraits<SEL>::NCH, overlap, b->serialClasses, ecAhead != NULL, b->plan);
    if (plan.tooComplex)
        return failTooComplex(plan.refused, env);
    const auto unculled = plan.unculledOverlap ? launchUnculled<SEL, true> : launchUnculled<SEL, false>;   // the list-free kernel's combiner, chosen once
    ScopedTimer timer(stream, 0);                                // the distance pass of one generate call (one or more launches)
    hipStream_t streams[3] = { stream, stream, stream };         // by PLAN_STREAM_*
    if (plan.concurrent) {
        rc = ensureSideStreams(b);
        if (rc != MSDFHIP_OK)
            return rc;
        HIPCHK(hipEventRecord(b->work.forkEvent, stream));
        for (int k = 0; k < plan.nLaunches; ++k) {
            const int role = plan.launches[k].stream;
            if (role != PLAN_STREAM_CALLER) {
                streams[role] = b->work.sideStream[role-PLAN_STREAM_SIDE0];
                HIPCHK(hipStreamWaitEvent(streams[role], b->work.forkEvent, 0));
            }
        }
    }
    // (an error between fork and join must not leave side-stream kernels unordered with the caller's stream: the launches only set rc,
    // the join below always runs)
    int aheadRc = MSDFHIP_OK;
    if (plan.ecAhead)
        aheadRc = runCorrection(b, SelTraits<SEL>::NCH, w, h, dGlyphs, NULL, NULL, NULL, *ecAhead, streams[PLAN_STREAM_SIDE1], call, true);
    for (int k = 0; k < plan.nLaunches && rc == MSDFHIP_OK; ++k) {
        const DistanceLaunch &l = plan.launches[k];
        rc = forDistanceVariant(l, [&](auto o, auto g, auto t) {
            return launchDistance<SEL, decltype(o)::value, decltype(g)::value, decltype(t)::value>(b, dGlyphs, w, h, dst, toScratch, l, env, streams[l.stream], call.boxDims);
        });
    }
    hipError_t joinError = hipSuccess;
    for (int k = 0; k < 2; ++k)
        if (streams[PLAN_STREAM_SIDE0+k] != stream) {
            hipError_t e = hipEventRecord(b->work.joinEvent[k], streams[PLAN_STREAM_SIDE0+k]);
            if (e == hipSuccess)
                e = hipStreamWaitEvent(stream, b->work.joinEvent[k], 0);
            joinError = e != hipSuccess ? e : joinError;
        }
    rc = aheadRc != MSDFHIP_OK ? aheadRc : rc;                   // (queued before the classes: its error is the call's first)
    if (joinError != hipSuccess) {                               // could not order the streams by events: fall back to waiting for them here
        (void) hipGetLastError();
        for (int k = 0; k < 2; ++k)
            if (streams[PLAN_STREAM_SIDE0+k] != stream)
                (void) hipStreamSynchronize(streams[PLAN_STREAM_SIDE0+k]);
        if (rc == MSDFHIP_OK)
            rc = fail(MSDFHIP_ERR_HIP, "joining the glyph-class streams failed: %s", hipGetErrorString(joinError));
    }
    if (rc == MSDFHIP_OK && plan.unculled)                       // after the join: the list-free kernel shares the batch's workspace with the global-scratch class
        rc = unculled(b, dGlyphs, w, h, dst, toScratch, stream, plan.unculledMapped ? b->work.bucket.ptr+plan.unculledOffset : NULL, plan.unculledCount, call.boxDims);
    return rc;
}

// Records of the per-glyph candidate segments incl. the header (msdf_kernels.hpp, EcCandidate), followed by the work list of
// k_ec_query: int offsets[ecOffsetInts(nGlyphs)] (k_ec_scan).
size_t candidateRecords(int nGlyphs, size_t texelsPerGlyph) { return ecHeaderRecords(nGlyphs)+(size_t) nGlyphs*ecSegment(texelsPerGlyph); }
size_t offsetRecords(int nGlyphs) { return (ecOffsetInts(nGlyphs)*sizeof(int)+sizeof(EcCandidate)-1)/sizeof(EcCandidate); }
// ... followed by the corner list of k_ec_params: two ints per edge of the batch.
size_t deferredRecords(int nGlyphs, size_t texelsPerGlyph, int nEdges) {
    return candidateRecords(nGlyphs, texelsPerGlyph)+offsetRecords(nGlyphs)+((size_t) (nEdges > 0 ? nEdges : 1)*2*sizeof(int)+sizeof(EcCandidate)-1)/sizeof(EcCandidate);
}

int ensureDeferred(const MsdfHipBatch *b, size_t cap, EcCandidate **out) {
    std::lock_guard<std::mutex> lock(b->work.mutex);
    HIPCHK(b->work.deferred.ensure(cap));
    HIPCHK(b->work.ecParams.ensure(b->work.glyphCapacity(b->nGlyphs)));
    *out = b->work.deferred.ptr;
    return MSDFHIP_OK;
}

// Workgroups of k_ec_query<N, OVERLAP> the device holds at once at this LDS size (its tickets are dealt out statically to that many); 0: unknown.
template <int N, bool OVERLAP>
unsigned queryResidentBlocks(int device, size_t lds) {
    enum { LDS_STEP = 2048, LDS_STEPS = 81 };
    static std::atomic<int> cache[LDS_STEPS];
    const size_t step = (lds+LDS_STEP-1)/LDS_STEP;
    return step < LDS_STEPS ? (unsigned) residentBlocks(cache[step], device, reinterpret_cast<const void *>(k_ec_query<N, OVERLAP>), WAVE, step*LDS_STEP) : 0u;
}

// The correction pass as planCorrection (msdf_launchplan.hpp) laid it out; GRES is p.gres.
template <int N, bool OVERLAP, bool GRES>
int launchEc(const MsdfHipBatch *b, const MsdfHipGlyph *dGlyphs, int w, int h, const float *src, float *out, uint8_t *stencil,
             const MsdfHipConfig &cfg, hipStream_t stream, GenerateCall &call, bool paramsOnly, const EcPlan &p) {
    // paramsOnly (prepareAhead, dispatchDistance): only what does not depend on the distance field -- the work buffers and k_ec_params (per-glyph constants,
    // corner texels, zeroed candidate header) -- so that it is off the launch chain that follows the distance pass; call.ecParamsQueued says whether it
    // launched k_ec_params, and the full pass then skips that launch.
    const int tilesX = (w+TILE-1)/TILE, tiles = tilesOf(w, h);
    const unsigned blocks = (unsigned) b->nGlyphs*(unsigned) tiles;
    if (p.tooManyTexels)
        return fail(MSDFHIP_ERR_INVALID, "batch of %zu texels exceeds the 32-bit texel index of the error-correction pass; split the batch", p.allTexels);
    double *gres = NULL;
    int rc;
    if (GRES) {
        rc = ensureGres(b, (size_t) p.slowGrid*p.resBytes, &gres);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    const size_t gresStride = p.resBytes/sizeof(double);
    const int32_t *dDims = call.boxDims;                         // (a sized call: the twins of the kernels below, same grids, same LDS)
    // The uniform kernels of this call: those of the modern entry points, or (call.ecShapeRows: a legacy generator, which corrects without overlap support
    // and without the distance check, hence in the eager order) their instantiations that pair protectEdges' texels along the shape's rows.
    auto slowKernel = k_ec_slow<N, OVERLAP, GRES>;
    auto fastKernel = p.lazyProtect ? k_ec_fast<N, true> : k_ec_fast<N, false>;
    if (call.ecShapeRows) {
        if constexpr (!OVERLAP && !GRES) {
            if (dDims || p.lazyProtect)
                return fail(MSDFHIP_ERR_INVALID, "a correction along the shape's rows takes neither boxes of their own sizes nor the distance check");
            slowKernel = k_ec_slow<N, false, false, true>;
            fastKernel = k_ec_fast<N, false, true>;
        } else
            return fail(MSDFHIP_ERR_INVALID, "a correction along the shape's rows runs without overlap support");
    }
    const auto slowTwin = ecSlowSizedKernel(N, OVERLAP, GRES);   // (the shape-rows instantiations have no twin: refused above)
    const auto fastTwin = ecFastSizedKernel(N, p.lazyProtect);
    const auto queryTwin = ecQuerySizedKernel(N, OVERLAP);
    const BatchView v = viewOf(b);
    rc = setLdsTwinned(slowKernel, slowTwin, dDims, p.slowLds);
    if (rc != MSDFHIP_OK)
        return rc;
    ScopedTimer timer(stream, 1, !paramsOnly);
    if (p.route == EC_ROUTE_STAGE_SNAPSHOT || p.route == EC_ROUTE_SLOW_ALL) {   // k_ec_slow takes every texel
        if (paramsOnly)
            return MSDFHIP_OK;
        launchTwinned(slowKernel, slowTwin, dDims, dim3(p.route == EC_ROUTE_SLOW_ALL ? p.slowGrid : p.snapshotBlocks), p.slowLds, stream, v, dGlyphs, w, h, src, out,
                      stencil, cfg, NULL, 0u, 0, gres, gresStride);
        HIPCHK(hipGetLastError());
        if (p.route == EC_ROUTE_SLOW_ALL)
            countRoute(MSDFHIP_ROUTE_EC_SLOW_ALL);
        return MSDFHIP_OK;
    }
    const unsigned seg = ecSegment((size_t) w*h);                // candidate records per glyph
    EcCandidate *deferred = NULL;
    rc = ensureDeferred(b, deferredRecords(b->nGlyphs, (size_t) w*h, b->nEdges), &deferred);
    if (rc != MSDFHIP_OK)
        return rc;
    if (p.route == EC_ROUTE_TOO_COMPLEX)
        return fail(MSDFHIP_ERR_TOO_COMPLEX, "a glyph has %d contours / %d edges: the error-correction pass needs %zu B of LDS per wavefront, device limit is %d B",
                    b->maxContours, b->maxEdges, p.fastLds > p.queryLds ? p.fastLds : p.queryLds, gLdsLimit.load());
    rc = setLdsTwinned(k_ec_query<N, OVERLAP>, queryTwin, dDims, p.queryLds);
    if (rc != MSDFHIP_OK)
        return rc;
    rc = setLdsTwinned(fastKernel, fastTwin, dDims, p.fastLds);
    if (rc != MSDFHIP_OK)
        return rc;
    int *offsets = reinterpret_cast<int *>(deferred+candidateRecords(b->nGlyphs, (size_t) w*h));
    int *corners = reinterpret_cast<int *>(deferred+candidateRecords(b->nGlyphs, (size_t) w*h)+offsetRecords(b->nGlyphs));
    const unsigned queryBlocks = p.residentQueryBlocks(p.staticDeal ? queryResidentBlocks<N, OVERLAP>(b->device, p.queryLds) : 0u);
    const EcQueryPolicy policy = { p.lpcMaxContours, p.lpcEdgeCost, p.lpcMaxEdges, p.lpcMinCount, p.wideMaxEdges, p.wideLoad, p.wideMeanCount, p.gridSteps };
    if (!call.ecParamsQueued)
        hipLaunchKernelGGL(k_ec_params, dim3((unsigned) b->nGlyphs), dim3(WAVE), 0, stream, b->work.ecParams.ptr, viewOf(b), dGlyphs, cfg,
                           reinterpret_cast<unsigned *>(deferred), corners, offsets+ecSizesAt(b->nGlyphs));   // also zeroes the candidate header
    const int *ecOrder = NULL;                                   // glyphs heaviest first for the distance checks' work list (NULL: batch order)
    rc = ensureEcOrder(b, &ecOrder, stream);
    if (rc != MSDFHIP_OK)
        return rc;
    if (paramsOnly) {
        HIPCHK(hipGetLastError());
        call.ecParamsQueued = true;
        return MSDFHIP_OK;
    }
    launchTwinned(fastKernel, fastTwin, dDims, dim3(blocks), p.fastLds, stream, v, dGlyphs, w, h, tilesX, tiles, src, out, stencil, cfg, b->work.ecParams.ptr, deferred,
                  seg, b->maxEdges, corners);
    hipLaunchKernelGGL(k_ec_scan, dim3(1), dim3(1024), 0, stream, b->nGlyphs, reinterpret_cast<const unsigned *>(deferred), seg, offsets, policy, ecOrder);
    launchTwinned(k_ec_query<N, OVERLAP>, queryTwin, dDims, dim3(queryBlocks), p.queryLds, stream, v.nGlyphs, v.glyphContourOffsets, v.contourOffsets, v.recs, v.windings,
                  dGlyphs, w, h, src, out, stencil, cfg, b->work.ecParams.ptr, deferred, seg, offsets, offsets+2*(size_t) b->nGlyphs+2, p.queryBatch, p.slotCap,
                  p.slotOffset, policy, call.overflowOut, ecOrder, p.queryFlags);
    if (call.overflowOut)
        call.overflowMirrored = true;                            // the caller looks at the count after its copy back and reruns with the pass below if needed
    else
        launchTwinned(slowKernel, slowTwin, dDims, dim3(p.slowGrid), p.slowLds, stream, v, dGlyphs, w, h, src, out, stencil, cfg, deferred, seg, 1, gres, gresStride);
    HIPCHK(hipGetLastError());
    countRoute(ecOrder ? MSDFHIP_ROUTE_EC_QUERY_HEAVIEST : MSDFHIP_ROUTE_EC_QUERY_BATCH);
    if (p.wideSlots)
        countRoute(MSDFHIP_ROUTE_EC_WIDE_SLOTS);
    return MSDFHIP_OK;
}

template <int N>
int dispatchEc(const MsdfHipBatch *b, const MsdfHipGlyph *dGlyphs, int w, int h, const float *src, float *out, uint8_t *stencil,
               const MsdfHipConfig &cfg, hipStream_t stream, GenerateCall &call, bool paramsOnly) {
    const EcPlan p = planCorrection(planEnv(b->device), countsOf(b), w, h, N, cfg.overlap_support != 0, cfg.ec_mode, cfg.ec_distance_check, cfg.ec_stage_limit,
                                    ecFastLdsBytes(b->maxEdges, N));
    if (!cfg.overlap_support)
        return launchEc<N, false, false>(b, dGlyphs, w, h, src, out, stencil, cfg, stream, call, paramsOnly, p);
    return p.gres ? launchEc<N, true, true>(b, dGlyphs, w, h, src, out, stencil, cfg, stream, call, paramsOnly, p)
                  : launchEc<N, true, false>(b, dGlyphs, w, h, src, out, stencil, cfg, stream, call, paramsOnly, p);
}

int checkConfig(const MsdfHipConfig *cfg) {
    if (!cfg)
        return fail(MSDFHIP_ERR_INVALID, "cfg is NULL");
    if (cfg->ec_mode < 0 || cfg->ec_mode > 3 || cfg->ec_distance_check < 0 || cfg->ec_distance_check > 2 || cfg->ec_stage_limit < 0 || cfg->ec_stage_limit > 4)
        return fail(MSDFHIP_ERR_INVALID, "bad error-correction config (mode %d, distance check %d, stage limit %d)", cfg->ec_mode, cfg->ec_distance_check, cfg->ec_stage_limit);
    return MSDFHIP_OK;
}

int ensureScratch(const MsdfHipBatch *b, size_t floats, float **out) {
    std::lock_guard<std::mutex> lock(b->work.mutex);
    HIPCHK(b->work.scratch.ensure(floats));
    *out = b->work.scratch.ptr;
    return MSDFHIP_OK;
}

// Error correction only: src (packed pre-correction tiles) -> out.
int runCorrection(const MsdfHipBatch *b, int channels, int w, int h, const MsdfHipGlyph *dGlyphs, const float *src, float *out, uint8_t *stencil,
                  const MsdfHipConfig &cfg, hipStream_t stream, GenerateCall &call, bool paramsOnly) {
    int rc = MSDFHIP_OK;                                         // (channels is 3 or 4: the callers correct in modes 3 and 4 only)
    forOneOf<3, 4>(channels, [&](auto n) { rc = dispatchEc<decltype(n)::value>(b, dGlyphs, w, h, src, out, stencil, cfg, stream, call, paramsOnly); });
    return rc;
}

// What a generate call on `b` will need that does NOT depend on other work of the device: the class lists of the overlapping combiner and the correction
// pass's per-glyph constants. The host-output pipeline queues these on a chunk's stream BEFORE the chunk waits for its turn on the device -- a small
// kernel launched between two chunks' large ones waits 0.1-0.4 ms for wavefront slots, and every such launch in a chunk's chain delays the whole chunk
// (rocprofv3 timeline of the pipeline, profiles/r05_ab_notes.md).
int prepareAhead(const MsdfHipBatch *b, int mode, int w, int h, const MsdfHipGlyph *dGlyphs, const MsdfHipConfig *cfg, hipStream_t stream, GenerateCall &call) {
    if (b->nGlyphs == 0 || w == 0 || h == 0)
        return MSDFHIP_OK;
    const int nch = channelsOf(mode);
    int rc = MSDFHIP_OK;
    if (const int limit = classListLimitAhead(planEnv(b->device), countsOf(b), w, h, nch, cfg->overlap_support != 0))
        rc = ensureBuckets(b, limit, stream);
    if (rc == MSDFHIP_OK && mode >= 3 && cfg->ec_mode != MSDFHIP_EC_DISABLED)
        rc = runCorrection(b, nch, w, h, dGlyphs, NULL, NULL, NULL, *cfg, stream, call, true);
    return rc;
}

// distanceSignCorrection: src (packed tiles) -> out (packed if dstPacked, else the caller's bitmaps).
template <int N>
int launchSign(const MsdfHipBatch *b, int w, int h, const MsdfHipGlyph *dGlyphs, const float *src, float *out, int dstPacked, float zero, int fillRule,
               int rasterizeOnly, hipStream_t stream, const int32_t *dDims = NULL) {
    const SignPlan p = planSign(planEnv(b->device), b->nGlyphs, b->maxEdges, w, h);
    if (p.blocks > 0x7fffffffull)
        return fail(MSDFHIP_ERR_INVALID, "launch of %zu tile rows exceeds the grid limit; split the batch", p.blocks);
    const auto twin = signSizedKernel(N);
    int rc = setLdsTwinned(k_sign_correction<N>, twin, dDims, p.lds);
    if (rc != MSDFHIP_OK)
        return rc;
    ScopedTimer timer(stream, 2);
    launchTwinned(k_sign_correction<N>, twin, dDims, dim3((unsigned) p.blocks), p.lds, stream, viewOf(b), dGlyphs, w, h, p.spansX, p.span, p.spans, (int) p.cap, src, out,
                  dstPacked, zero, fillRule, rasterizeOnly);
    HIPCHK(hipGetLastError());
    countRoute(p.wholeRows ? MSDFHIP_ROUTE_SIGN_WHOLE_ROWS : MSDFHIP_ROUTE_SIGN_SPLIT);
    if (p.chunked)
        countRoute(MSDFHIP_ROUTE_SIGN_CHUNKED);
    return MSDFHIP_OK;
}

int runSignCorrection(const MsdfHipBatch *b, int channels, int w, int h, const MsdfHipGlyph *dGlyphs, const float *src, float *out, int dstPacked,
                      float zero, int fillRule, hipStream_t stream, const int32_t *dDims = NULL) {
    if (fillRule < 0 || fillRule > 3)
        return fail(MSDFHIP_ERR_INVALID, "fill rule %d (must be 0..3)", fillRule);
    int rc = MSDFHIP_OK;
    if (!forOneOf<1, 3, 4>(channels, [&](auto n) {
            const int rasterizeOnly = decltype(n)::value == 1 && src == NULL;   // one channel and no source field: rasterize()
            rc = launchSign<decltype(n)::value>(b, w, h, dGlyphs, src, out, dstPacked, zero, fillRule, rasterizeOnly, stream, dDims);
        }))
        return fail(MSDFHIP_ERR_INVALID, "channels %d (must be 1, 3 or 4)", channels);
    return rc;
}

// ---- the legacy generators and the legacy correction (msdf_legacy.hpp) ----------------------------------------------------------

// What a legacy generator makes of the caller's config: generateMSDF_legacy / generateMTSDF_legacy take an ErrorCorrectionConfig only, switch its
// distance check off and correct without overlap support (msdfgen.cpp:272-273, 331-332). Read from the caller: the correction mode, the two ratios,
// the sign-pass fields and the row order of the optional stencil; everything else is fixed here.
MsdfHipConfig legacyConfig(const MsdfHipConfig &in) {
    MsdfHipConfig cfg;
    msdfhip_default_config(&cfg);
    cfg.overlap_support = 0;
    cfg.ec_distance_check = MSDFHIP_DO_NOT_CHECK_DISTANCE;
    cfg.ec_mode = in.ec_mode, cfg.min_deviation_ratio = in.min_deviation_ratio, cfg.min_improve_ratio = in.min_improve_ratio;
    cfg.sign_correction = in.sign_correction, cfg.fill_rule = in.fill_rule, cfg.sdf_zero_value = in.sdf_zero_value;
    cfg.stencil_y_down = in.stencil_y_down;
    return cfg;
}

template <int MODE>
int launchLegacyDistanceKernel(const MsdfHipBatch *b, const MsdfHipGlyph *dGlyphs, int w, int h, float *dst, int toScratch, hipStream_t stream) {
    const LegacyDistancePlan p = planLegacyDistance(b->nGlyphs, w, h);
    if (p.blocks == 0)
        return MSDFHIP_OK;
    if (p.tooManyBlocks)
        return fail(MSDFHIP_ERR_INVALID, "launch of %zu tiles exceeds the grid limit; split the batch", p.blocks);
    ScopedTimer timer(stream, 0);
    hipLaunchKernelGGL(k_distance_legacy<MODE>, dim3((unsigned) p.blocks), dim3(WAVE), 0, stream, b->nGlyphs, (const int32_t *) b->dGlyphContourOffsets.ptr,
                       (const int32_t *) b->dContourOffsets.ptr, (const EdgeRec *) b->dRecs.ptr, dGlyphs, w, h, (w+TILE-1)/TILE, tilesOf(w, h), dst, toScratch);
    HIPCHK(hipGetLastError());
    return MSDFHIP_OK;
}

int launchLegacyDistance(int mode, const MsdfHipBatch *b, const MsdfHipGlyph *dGlyphs, int w, int h, float *dst, int toScratch, hipStream_t stream) {
    int rc = MSDFHIP_OK;                                         // (mode is 1..4: checked by the entry points)
    forOneOf<1, 2, 3, 4>(mode, [&](auto m) { rc = launchLegacyDistanceKernel<decltype(m)::value>(b, dGlyphs, w, h, dst, toScratch, stream); });
    return rc;
}

// msdfErrorCorrection_legacy of nGlyphs packed tiles, in place: pass 0 tiles -> scratch, pass 1 scratch -> tiles (planLegacyCorrection).
int launchLegacyCorrection(float *dTiles, float *dScratch, int nGlyphs, int w, int h, int channels, double thresholdX, double thresholdY, hipStream_t stream) {
    const LegacyEcPlan p = planLegacyCorrection(nGlyphs, w, h, channels);
    if (p.blocks == 0)
        return MSDFHIP_OK;
    for (int pass = 0; pass < 2; ++pass) {
        const float *src = pass == 0 ? dTiles : dScratch;
        float *dst = pass == 0 ? dScratch : dTiles;
        forOneOf<3, 4>(channels, [&](auto n) {
            hipLaunchKernelGGL(k_ec_legacy<decltype(n)::value>, dim3(p.blocks), dim3(PLAN_LEGACY_EC_THREADS), 0, stream, src, dst, nGlyphs, w, h, pass, thresholdX, thresholdY);
        });
        HIPCHK(hipGetLastError());                                   // (a pass that was not queued must not be followed by one that reads its output)
    }
    return MSDFHIP_OK;
}

// One legacy generate call on b (arguments checked, device bound, cfg = legacyConfig): legacy distance pass -> sign correction -> error correction
// without the distance check. With the sign pass this is the reference CLI's -legacy flow (main.cpp:1223-1298), which corrects the bitmap as it lies.
// Without it, it is generateMSDF_legacy / generateMTSDF_legacy, which re-orient their bitmap to the shape first (msdfgen.cpp:223, 278) and so pair
// protectEdges' texels along the shape's rows: call.ecShapeRows. The stencil's rows are the same either way (stencilIndex). Nothing of the call stays on the batch:
// like runGenerate it carries its state in `call`, and the legacy pass takes no class list, work queue or side stream of the batch.
int runGenerateLegacy(const MsdfHipBatch *b, int mode, int w, int h, const MsdfHipGlyph *dGlyphs, float *dOut, uint8_t *dStencil, float *dScratch,
                      const MsdfHipConfig &cfg, hipStream_t stream, GenerateCall &call) {
    if (b->nGlyphs == 0 || w == 0 || h == 0)
        return MSDFHIP_OK;
    const int nch = channelsOf(mode);
    const bool correct = mode >= 3 && cfg.ec_mode != MSDFHIP_EC_DISABLED;
    const bool signPass = cfg.sign_correction != 0;
    const int stages = (correct ? 1 : 0)+(signPass ? 1 : 0);
    const size_t tileFloats = (size_t) b->nGlyphs*w*h*nch;
    int rc = MSDFHIP_OK;
    if (stages && !dScratch) {
        rc = ensureScratch(b, tileFloats*stages, &dScratch);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    float *stageA = stages ? dScratch : NULL, *stageB = stages == 2 ? dScratch+tileFloats : NULL;
    float *dst = stages ? stageA : dOut;
    rc = launchLegacyDistance(mode, b, dGlyphs, w, h, dst, stages != 0, stream);
    if (rc != MSDFHIP_OK || !stages)
        return rc;
    const float *ecSrc = stageA;
    if (signPass) {
        rc = runSignCorrection(b, nch, w, h, dGlyphs, stageA, correct ? stageB : dOut, correct ? 1 : 0, cfg.sdf_zero_value, cfg.fill_rule, stream);
        if (rc != MSDFHIP_OK || !correct)
            return rc;
        ecSrc = stageB;
    }
    call.ecShapeRows = !signPass;
    return runCorrection(b, nch, w, h, dGlyphs, ecSrc, dOut, dStencil, cfg, stream, call);
}

} // namespace

extern "C" {

void msdfhip_default_config(MsdfHipConfig *cfg) {
    if (!cfg)
        return;
    cfg->overlap_support = 1;
    cfg->ec_mode = MSDFHIP_EC_EDGE_PRIORITY;
    cfg->ec_distance_check = MSDFHIP_CHECK_DISTANCE_AT_EDGE;
    cfg->ec_stage_limit = 0;
    cfg->min_deviation_ratio = 1.11111111111111111;
    cfg->min_improve_ratio = 1.11111111111111111;
    cfg->sign_correction = 0;
    cfg->fill_rule = 0;                                          // FILL_NONZERO (core/rasterization.h:17)
    cfg->sdf_zero_value = .5f;
    cfg->stencil_y_down = 0;
}

int msdfhip_abi_version(void) { return MSDFHIP_ABI_VERSION; }

const char *msdfhip_last_error(void) { return tlsError.c_str(); }

int msdfhip_init(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(MSDFHIP_ERR_NO_DEVICE, "no HIP device visible (hipGetDeviceCount -> %d); this library has no CPU fallback", count);
    if (device < 0 || device >= count)
        return fail(MSDFHIP_ERR_INVALID, "device %d out of range (0..%d)", device, count-1);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(MSDFHIP_ERR_NO_DEVICE, "hipGetDeviceProperties(%d) failed", device);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MSDFHIP_ERR_NO_DEVICE, "device %d is %s; libmsdfgen_hip is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    if (hipSetDevice(device) != hipSuccess)
        return fail(MSDFHIP_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
    gLdsLimit.store((int) (prop.maxSharedMemoryPerMultiProcessor > 0 ? prop.maxSharedMemoryPerMultiProcessor : prop.sharedMemPerBlock));
    gDevice.store(device);
    return MSDFHIP_OK;
}

int msdfhip_device_info(char *name, size_t name_len, int *cus, int *lds_bytes) {
    int rc = ensureDevice();
    if (rc != MSDFHIP_OK)
        return rc;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, gDevice.load()));
    if (name && name_len) {
        strncpy(name, prop.gcnArchName, name_len-1);
        name[name_len-1] = 0;
    }
    if (cus)
        *cus = prop.multiProcessorCount;
    if (lds_bytes)
        *lds_bytes = gLdsLimit.load();
    return MSDFHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------- batches

int msdfhip_batch_create_device(MsdfHipBatch **batch, int n_glyphs, int n_contours, int n_edges, int max_contours_per_glyph, int max_edges_per_glyph,
                                const int32_t *d_glyph_contour_offsets, const int32_t *d_contour_offsets,
                                const double *d_points, const uint8_t *d_types, const uint8_t *d_colors, void *stream) {
    if (!batch || n_glyphs < 0 || n_contours < 0 || n_edges < 0)
        return fail(MSDFHIP_ERR_INVALID, "bad batch dimensions");
    int rc = ensureDeviceOf(d_points ? (const void *) d_points : (const void *) d_glyph_contour_offsets);   // the device that OWNS the caller's arrays (a torch tensor on cuda:1 ...)
    if (rc != MSDFHIP_OK)
        return rc;
    MsdfHipBatch *b = new MsdfHipBatch();
    b->onDevice(currentDevice());                                // ... not the process default
    b->nGlyphs = n_glyphs, b->nContours = n_contours, b->nEdges = n_edges;
    b->maxContours = max_contours_per_glyph, b->maxEdges = max_edges_per_glyph;
    b->dGlyphContourOffsets.borrow(const_cast<int32_t *>(d_glyph_contour_offsets), (size_t) n_glyphs+1);   // the caller's arrays: never freed here
    b->dContourOffsets.borrow(const_cast<int32_t *>(d_contour_offsets), (size_t) n_contours+1);
    b->dPoints.borrow(const_cast<double *>(d_points), 8*(size_t) n_edges);
    b->dTypes.borrow(const_cast<uint8_t *>(d_types), (size_t) n_edges);
    b->dColors.borrow(const_cast<uint8_t *>(d_colors), (size_t) n_edges);
    rc = digest(b, (hipStream_t) stream);
    if (rc != MSDFHIP_OK) {
        msdfhip_batch_destroy(b);
        return rc;
    }
    *batch = b;
    return MSDFHIP_OK;
}

// Validates a CSR shape list given as HOST arrays before anything is dereferenced beyond its stated size; fills the per-glyph counts.
static int checkShapeArrays(int n_glyphs, const int32_t *gco, const int32_t *co, const double *points, const uint8_t *types, const uint8_t *colors,
                            bool colorsRequired, std::vector<int> &hContours, std::vector<int> &hEdges, int &maxC, int &maxE) {
    if (n_glyphs < 0 || !gco || !co)
        return fail(MSDFHIP_ERR_INVALID, "bad batch arguments");
    if (gco[0] != 0 || co[0] != 0)
        return fail(MSDFHIP_ERR_INVALID, "offset arrays must start at 0");
    for (int g = 0; g < n_glyphs; ++g)
        if (gco[g+1] < gco[g])
            return fail(MSDFHIP_ERR_INVALID, "glyph_contour_offsets not monotonic at %d", g);
    const int nC = gco[n_glyphs];
    for (int c = 0; c < nC; ++c)
        if (co[c+1] < co[c])
            return fail(MSDFHIP_ERR_INVALID, "contour_offsets not monotonic at %d", c);
    const int nE = co[nC];
    if (nE > 0 && (!points || !types || (colorsRequired && !colors)))
        return fail(MSDFHIP_ERR_INVALID, "NULL edge arrays");
    for (int e = 0; e < nE; ++e)
        if (types[e] < 1 || types[e] > 3)
            return fail(MSDFHIP_ERR_INVALID, "edge %d has type %d (must be 1, 2 or 3)", e, (int) types[e]);
    hContours.resize((size_t) n_glyphs);
    hEdges.resize((size_t) n_glyphs);
    maxC = maxE = 0;
    for (int g = 0; g < n_glyphs; ++g) {
        const int c = gco[g+1]-gco[g], e = co[gco[g+1]]-co[gco[g]];
        hContours[g] = c, hEdges[g] = e;
        maxC = c > maxC ? c : maxC;
        maxE = e > maxE ? e : maxE;
    }
    return MSDFHIP_OK;
}

int msdfhip_batch_create_on(MsdfHipBatch **batch, int device, int n_glyphs, const int32_t *gco, const int32_t *co, const double *points, const uint8_t *types,
                            const uint8_t *colors) {
    if (!batch)
        return fail(MSDFHIP_ERR_INVALID, "bad batch arguments");
    std::vector<int> hContours, hEdges;
    int maxC = 0, maxE = 0;
    int rc = checkShapeArrays(n_glyphs, gco, co, points, types, colors, true, hContours, hEdges, maxC, maxE);
    if (rc != MSDFHIP_OK)
        return rc;
    if (device >= 0) {
        int count = 0;
        rc = msdfhip_device_count(&count);
        if (rc != MSDFHIP_OK)
            return rc;
        if (device >= count)
            return fail(MSDFHIP_ERR_INVALID, "device %d out of range (0..%d)", device, count-1);
    }
    rc = ensureDevice(device);
    if (rc != MSDFHIP_OK)
        return rc;
    const int nC = gco[n_glyphs], nE = co[nC];
    MsdfHipBatch *b = new MsdfHipBatch();
    b->onDevice(currentDevice());
    b->nGlyphs = n_glyphs, b->nContours = nC, b->nEdges = nE, b->maxContours = maxC, b->maxEdges = maxE;
    b->hContours.swap(hContours);
    b->hEdges.swap(hEdges);
    const size_t eAlloc = nE > 0 ? nE : 1;
    hipError_t e = uploadNew(b->dGlyphContourOffsets, gco, (size_t) n_glyphs+1, (size_t) n_glyphs+1);
    if (e == hipSuccess) e = uploadNew(b->dContourOffsets, co, (size_t) nC+1, (size_t) nC+1);
    if (e == hipSuccess) e = uploadNew(b->dPoints, points, 8*eAlloc, 8*(size_t) nE);
    if (e == hipSuccess) e = uploadNew(b->dTypes, types, eAlloc, (size_t) nE);
    if (e == hipSuccess) e = uploadNew(b->dColors, colors, eAlloc, (size_t) nE);
    if (e != hipSuccess) {
        msdfhip_batch_destroy(b);
        return fail(MSDFHIP_ERR_HIP, "batch upload failed: %s", hipGetErrorString(e));
    }
    rc = digest(b, NULL);
    if (rc == MSDFHIP_OK && hipStreamSynchronize(NULL) != hipSuccess)
        rc = fail(MSDFHIP_ERR_HIP, "edge digestion failed: %s", hipGetErrorString(hipGetLastError()));
    if (rc != MSDFHIP_OK) {
        msdfhip_batch_destroy(b);
        return rc;
    }
    *batch = b;
    return MSDFHIP_OK;
}

int msdfhip_batch_create(MsdfHipBatch **batch, int n_glyphs, const int32_t *gco, const int32_t *co, const double *points, const uint8_t *types, const uint8_t *colors) {
    return msdfhip_batch_create_on(batch, -1, n_glyphs, gco, co, points, types, colors);
}

int msdfhip_batch_device(const MsdfHipBatch *b, int *device) {
    if (!b || !device)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    *device = b->device;
    return MSDFHIP_OK;
}

int msdfhip_device_count(int *count) {
    if (!count)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void) hipGetLastError();
        return fail(MSDFHIP_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    }
    *count = n;
    return MSDFHIP_OK;
}

} // extern "C"

namespace {

static_assert(PREP_FIN_TYPES == PREP_FIN_POINTS+1 && PREP_FIN_COLORS == PREP_FIN_POINTS+2 && PREP_NORM_TYPES == PREP_NORM_POINTS+1 && PREP_NORM_COLORS == PREP_NORM_POINTS+2,
              "msdfhip_batch_create_prepared_oriented adopts an edge set's regions as points, types, colors");
static_assert(PREP_PLAN_WAVE_MAX_EDGES == PREP_WAVE_MAX_EDGES, "msdf_prepplan.hpp sizes the colouring's global tables from the kernels' LDS tier");

// Shape preparation (row f3) as ONE queued sequence on `stream`, in the reference CLI's order: orientContours on the raw edges (orient.orient_contours),
// normalize (k_prep_normalize_flat + the cusp repair), the winding step on the normalized edges (orient.winding), then with coloring the coloured
// counts, their prefix and the colouring wave. Orientation changes no count, so the offsets and bounds below do not depend on it. Never allocates, never waits: msdfhip_batch_create_prepared runs it on the null stream, the streamed
// generator on each chunk's stream under the kernels of the chunks before it. With coloring the result is fin + co2, else norm + co1.
int queuePreparation(const MsdfHipPrepConfig *cfg, const MsdfHipOrientConfig &orient, int nGlyphs, int nC, int nE1, int longest, double crossThreshold,
                      const PrepBuffers &pb, hipStream_t stream) {
    if (nE1 && orient.orient_contours)                              // Shape::orientContours on the raw edges, in place (main.cpp:1105-1111)
        hipLaunchKernelGGL(k_prep_orient, dim3((unsigned) nGlyphs), dim3(WAVE), 0, stream, pb.raw, pb.gco, pb.co, nGlyphs, pb.votes, pb.hitX, pb.hitTag);
    if (nE1) {
        HIPCHK(hipMemsetAsync(pb.cusp, 0, sizeof(int32_t)*(size_t) (nC+1), stream));
        hipLaunchKernelGGL(k_prep_normalize_flat, dim3((nE1+255)/256), dim3(256), 0, stream, pb.raw, pb.co, pb.co1, nC, nE1, cfg->normalize ? 1 : 0, pb.norm, pb.cusp);
        if (cfg->normalize)
            hipLaunchKernelGGL(k_prep_normalize_cusps, dim3((nC+127)/128), dim3(128), 0, stream, pb.raw, pb.co, pb.co1, nC, pb.norm, (const int32_t *) pb.cusp);
        if (orient.winding)                                         // -reversewinding / -guesswinding on the normalized edges, in place (main.cpp:1131-1143)
            hipLaunchKernelGGL(k_prep_winding, dim3((unsigned) nGlyphs), dim3(WAVE), 0, stream, pb.norm, pb.gco, pb.co1, nGlyphs, (int) orient.winding);
    }
    if (cfg->coloring) {
        if (nC)
            hipLaunchKernelGGL(k_prep_count, dim3((nC+127)/128), dim3(128), 0, stream, pb.norm, pb.co1, nC, crossThreshold, pb.count);
        hipLaunchKernelGGL(k_prep_offsets, dim3(1), dim3(256), 0, stream, (const int32_t *) pb.count, nC, pb.co2);
        // one wavefront per glyph, lanes = edges / corners; the LDS tier of the launch from the longest contour (a contour beyond the tier uses `big`,
        // which exists only past the large tier: the small tier is chosen only when no contour exceeds it)
        const bool smallTier = longest <= PREP_WAVE_SMALL_EDGES && !tuning().prepLargeTier;
        #define PREP_COLOUR(INK, TIER) hipLaunchKernelGGL((k_prep_colour_wave<INK, TIER>), dim3((unsigned) nGlyphs), dim3(WAVE), 0, stream, pb.norm, pb.gco, \
                                                          pb.co1, (const int32_t *) pb.co2, nGlyphs, crossThreshold, pb.seeds, (unsigned long long) cfg->seed, pb.fin, pb.big)
        if (nGlyphs && cfg->coloring == 1) {
            if (smallTier) PREP_COLOUR(false, PREP_WAVE_SMALL_EDGES); else PREP_COLOUR(false, PREP_WAVE_MAX_EDGES);
        } else if (nGlyphs) {
            if (smallTier) PREP_COLOUR(true, PREP_WAVE_SMALL_EDGES); else PREP_COLOUR(true, PREP_WAVE_MAX_EDGES);
        }
        #undef PREP_COLOUR
    }
    HIPCHK(hipGetLastError());
    return MSDFHIP_OK;
}

int checkPrepConfig(const MsdfHipPrepConfig *cfg, const char *who) {
    if (!cfg)
        return fail(MSDFHIP_ERR_INVALID, "%s: NULL preparation config", who);
    if (cfg->coloring < 0 || cfg->coloring > 2)
        return fail(MSDFHIP_ERR_INVALID, "%s: coloring %d (0 keep, 1 edgeColoringSimple, 2 edgeColoringInkTrap)", who, cfg->coloring);
    return MSDFHIP_OK;
}

// NULL orient: keep (the v5 entry points). The checked value is returned in *out.
int checkOrientConfig(const MsdfHipOrientConfig *orient, const char *who, MsdfHipOrientConfig *out) {
    out->orient_contours = 0, out->winding = 0;
    if (!orient)
        return MSDFHIP_OK;
    if (orient->orient_contours < 0 || orient->orient_contours > 1)
        return fail(MSDFHIP_ERR_INVALID, "%s: orient_contours %d (0 or 1)", who, orient->orient_contours);
    if (orient->winding < 0 || orient->winding > 2)
        return fail(MSDFHIP_ERR_INVALID, "%s: winding %d (0 keep, 1 reverse, 2 guess)", who, orient->winding);
    *out = *orient;
    return MSDFHIP_OK;
}

// NULL frame: no framing (*out untouched, *framed = false). What the CLI answers with "Cannot fit the specified pixel range." (main.cpp:1164-1165) depends on
// the call's size and range alone, so it is refused here, like every other bad field, before anything is read or the device is touched.
int checkFrameConfig(const MsdfHipFrameConfig *frame, int w, int h, const char *who, FrameParams *out, bool *framed) {
    *framed = false;
    if (!frame)
        return MSDFHIP_OK;
    if (frame->range_mode < 0 || frame->range_mode > 1)
        return fail(MSDFHIP_ERR_INVALID, "%s: range_mode %d (0 unit range, 1 pixel range)", who, frame->range_mode);
    if (!(frame->range_lower != frame->range_upper))
        return fail(MSDFHIP_ERR_INVALID, "%s: range_lower == range_upper (%g): the distance mapping divides by their difference", who, frame->range_lower);
    if (frame->scale_specified < 0 || frame->scale_specified > 1)
        return fail(MSDFHIP_ERR_INVALID, "%s: scale_specified %d (0 or 1)", who, frame->scale_specified);
    if (frame->scale_specified && !(frame->scale_x != 0 && frame->scale_y != 0))
        return fail(MSDFHIP_ERR_INVALID, "%s: scale_specified with scale (%g, %g)", who, frame->scale_x, frame->scale_y);
    if (w < 0 || h < 0)
        return fail(MSDFHIP_ERR_INVALID, "%s: a %d x %d frame", who, w, h);
    FrameParams f;
    f.rangeMode = frame->range_mode, f.scaleSpecified = frame->scale_specified;
    f.lower = frame->range_lower, f.upper = frame->range_upper;
    f.sx = frame->scale_specified ? frame->scale_x : 1., f.sy = frame->scale_specified ? frame->scale_y : 1.;
    const V2 extent = frameExtent(f, w, h);
    if ((w > 0 && h > 0) && (extent.x <= 0 || extent.y <= 0))
        return fail(MSDFHIP_ERR_INVALID, "%s: cannot fit the specified pixel range (%g to %g) into %d x %d", who, frame->range_lower, frame->range_upper, w, h);
    *out = f, *framed = true;
    return MSDFHIP_OK;
}

// The fields of a box configuration (msdf_frame.hpp: planBox), refused like a bad frame: before anything is read or the device is touched.
int checkBoxConfig(const MsdfHipBoxConfig *cfg, const char *who, BoxParams *out, double *border) {
    if (!cfg)
        return fail(MSDFHIP_ERR_INVALID, "%s: NULL config", who);
    switch (planBox(cfg->scale, cfg->range_mode, cfg->range_lower, cfg->range_upper, cfg->align_x, cfg->align_y, out, border)) {
        case BOX_CONFIG_SCALE: return fail(MSDFHIP_ERR_INVALID, "%s: scale %g (positive and finite)", who, cfg->scale);
        case BOX_CONFIG_RANGE_MODE: return fail(MSDFHIP_ERR_INVALID, "%s: range_mode %d (0 unit range, 1 pixel range)", who, cfg->range_mode);
        case BOX_CONFIG_RANGE: return fail(MSDFHIP_ERR_INVALID, "%s: range %g to %g (finite, range_lower < range_upper, range_lower <= 0)", who, cfg->range_lower, cfg->range_upper);
        case BOX_CONFIG_ALIGN: return fail(MSDFHIP_ERR_INVALID, "%s: align (%d, %d) (0 or 1 each)", who, cfg->align_x, cfg->align_y);
    }
    return MSDFHIP_OK;
}

// k_frame on `stream`: bounds[g][4] of the glyphs of (gco, co) over the NORMALIZED edges (haveBounds: they are there already), and with dGlyphs their xf.
int queueFrame(const EdgeArrays &norm, const int32_t *gco, const int32_t *co, int nGlyphs, double *dBounds, bool haveBounds, const FrameParams *frame, int w, int h,
               MsdfHipGlyph *dGlyphs, hipStream_t stream) {
    if (!nGlyphs)
        return MSDFHIP_OK;
    const FrameParams none = { 0, 0, 0., 1., 1., 1. };
    hipLaunchKernelGGL(k_frame, dim3((unsigned) nGlyphs), dim3(WAVE), 0, stream, norm, gco, co, nGlyphs, dBounds, haveBounds ? 1 : 0, frame ? *frame : none, w, h,
                       frame ? dGlyphs : (MsdfHipGlyph *) NULL);
    HIPCHK(hipGetLastError());
    return MSDFHIP_OK;
}

} // namespace

extern "C" {

int msdfhip_batch_create_prepared(MsdfHipBatch **batch, int n_glyphs, const int32_t *gco, const int32_t *co, const double *points, const uint8_t *types,
                                  const uint8_t *colors, const uint64_t *seeds, const MsdfHipPrepConfig *cfg) {
    return msdfhip_batch_create_prepared_oriented(batch, n_glyphs, gco, co, points, types, colors, seeds, cfg, NULL);
}

int msdfhip_batch_create_prepared_oriented(MsdfHipBatch **batch, int n_glyphs, const int32_t *gco, const int32_t *co, const double *points, const uint8_t *types,
                                           const uint8_t *colors, const uint64_t *seeds, const MsdfHipPrepConfig *cfg, const MsdfHipOrientConfig *orientCfg) {
    if (!batch || n_glyphs < 0 || !gco || !co || !cfg)
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_batch_create_prepared");
    if (cfg->coloring < 0 || cfg->coloring > 2)
        return fail(MSDFHIP_ERR_INVALID, "coloring %d (0 keep, 1 edgeColoringSimple, 2 edgeColoringInkTrap)", cfg->coloring);
    MsdfHipOrientConfig orient;
    int rco = checkOrientConfig(orientCfg, "msdfhip_batch_create_prepared_oriented", &orient);
    if (rco != MSDFHIP_OK)
        return rco;
    int maxRawEdges = 0;
    {
        std::vector<int> hc, he;
        int mc = 0;
        int rcv = checkShapeArrays(n_glyphs, gco, co, points, types, colors, false, hc, he, mc, maxRawEdges);
        if (rcv != MSDFHIP_OK)
            return rcv;
    }
    int rc = ensureDevice();
    if (rc != MSDFHIP_OK)
        return rc;
    const int nC = gco[n_glyphs], nE = co[nC];

    // offsets after normalize are a host-side prefix over the raw contour sizes; the upper bound of the coloured size as well
    std::vector<int32_t> co1(nC+1, 0), co2(nC+1, 0);
    size_t bound2 = 0;
    int longest = 0;
    prepOffsets(co, nC, cfg->normalize != 0, co1.data(), &bound2, &longest);
    if (bound2 > 0x7fffffffull)
        return fail(MSDFHIP_ERR_INVALID, "too many edges");
    const int nE1 = co1[nC];
    #define PREP_CHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(MSDFHIP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
    // one allocation per region the configuration needs (msdf_prepplan.hpp), with the exact normalized count and the bound of the coloured one; the records
    // and windings come with digest(), which sizes them from the final count
    const PrepPlanConfig plan = { true, cfg->coloring, seeds != NULL, colors != NULL && nE > 0, orient.orient_contours != 0, orientHitsBig(maxRawEdges),
                                  longest > PREP_WAVE_MAX_EDGES, true, false };
    const PrepCounts counts = { (size_t) n_glyphs, (size_t) nC, (size_t) nE, (size_t) nE1, bound2 };
    const PrepSizes sizes = prepRegionSizes(plan, counts);
    WorkBuffer<char> owner[PREP_REGIONS];                        // scoped to this call, but for the six the batch adopts below
    void *region[PREP_REGIONS];
    for (int r = 0; r < PREP_REGIONS; ++r) {
        PREP_CHK(owner[r].ensure(sizes.bytes[r]));
        region[r] = owner[r].ptr;
    }
    const size_t offsetBytes = sizeof(int32_t)*(size_t) (nC+1);
    const struct { int region; const void *host; size_t bytes; } uploads[] = {
        { PREP_GCO, gco, sizeof(int32_t)*(size_t) (n_glyphs+1) }, { PREP_CO, co, offsetBytes }, { PREP_CO1, co1.data(), offsetBytes },
        { PREP_RAW_POINTS, points, sizeof(double)*8*(size_t) nE }, { PREP_RAW_TYPES, types, (size_t) nE }, { PREP_RAW_COLORS, colors, (size_t) nE },
        { PREP_SEEDS, seeds, sizeof(unsigned long long)*(size_t) n_glyphs } };
    for (size_t u = 0; u < sizeof(uploads)/sizeof(uploads[0]); ++u)
        if (region[uploads[u].region] && uploads[u].bytes)
            PREP_CHK(hipMemcpy(region[uploads[u].region], uploads[u].host, uploads[u].bytes, hipMemcpyHostToDevice));
    const double crossThreshold = cfg->coloring ? sin(cfg->angle_threshold) : 0.;   // edge-coloring.cpp:69, taken by the host's libm like the reference's
    // Every pass is queued without a host round trip; the coloured offsets come back once, at the end.
    const PrepBuffers pb = bindPrep(region);
    rc = queuePreparation(cfg, orient, n_glyphs, nC, nE1, longest, crossThreshold, pb, 0);
    if (rc != MSDFHIP_OK)
        return rc;
    // Shape::getBounds where the CLI takes it (main.cpp:1125-1132): of the normalized edges, which do not outlive this call when a colouring follows
    rc = queueFrame(pb.norm, pb.gco, pb.co1, n_glyphs, (double *) region[PREP_BOUNDS], false, NULL, 0, 0, NULL, 0);
    if (rc != MSDFHIP_OK)
        return rc;
    const int32_t *finalCo = co1.data();
    if (cfg->coloring) {
        PREP_CHK(hipMemcpy(co2.data(), pb.co2, sizeof(int32_t)*(size_t) (nC+1), hipMemcpyDeviceToHost));   // in stream order after the kernels above
        finalCo = co2.data();
    }
    PREP_CHK(hipGetLastError());
    PREP_CHK(hipDeviceSynchronize());
    #undef PREP_CHK

    int maxC = 0, maxE = 0;
    for (int g = 0; g < n_glyphs; ++g) {
        const int c = gco[g+1]-gco[g], e = finalCo[gco[g+1]]-finalCo[gco[g]];
        maxC = c > maxC ? c : maxC;
        maxE = e > maxE ? e : maxE;
    }
    MsdfHipBatch *b = new MsdfHipBatch();
    b->onDevice(currentDevice());
    b->nGlyphs = n_glyphs, b->nContours = nC, b->nEdges = finalCo[nC], b->maxContours = maxC, b->maxEdges = maxE;
    const int fin = cfg->coloring ? PREP_FIN_POINTS : PREP_NORM_POINTS;   // the batch takes over the final arrays (bindPrep's pb.fin)
    b->dGlyphContourOffsets.adopt(std::move(owner[PREP_GCO])), b->dContourOffsets.adopt(std::move(owner[cfg->coloring ? PREP_CO2 : PREP_CO1]));
    b->dPoints.adopt(std::move(owner[fin])), b->dTypes.adopt(std::move(owner[fin+1])), b->dColors.adopt(std::move(owner[fin+2]));
    b->dBounds.adopt(std::move(owner[PREP_BOUNDS])), b->boundsFixed = true;
    rc = digest(b, NULL);
    if (rc == MSDFHIP_OK && hipStreamSynchronize(NULL) != hipSuccess)
        rc = fail(MSDFHIP_ERR_HIP, "edge digestion failed: %s", hipGetErrorString(hipGetLastError()));
    if (rc != MSDFHIP_OK) {
        msdfhip_batch_destroy(b);
        return rc;
    }
    *batch = b;
    return MSDFHIP_OK;
}

int msdfhip_batch_candidate_counts(const MsdfHipBatch *b, uint32_t *counts) {
    if (!b || !counts)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    if (!b->work.deferred.ptr)
        return fail(MSDFHIP_ERR_INVALID, "no error-correction pass has run on this batch");
    int rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(counts, b->work.deferred.ptr, sizeof(uint32_t)*(size_t) (b->nGlyphs+1), hipMemcpyDeviceToHost));
    return MSDFHIP_OK;
}

int msdfhip_batch_info(const MsdfHipBatch *b, int *nGlyphs, int *nContours, int *nEdges, int *maxContours, int *maxEdges) {
    if (!b)
        return fail(MSDFHIP_ERR_INVALID, "NULL batch");
    if (nGlyphs) *nGlyphs = b->nGlyphs;
    if (nContours) *nContours = b->nContours;
    if (nEdges) *nEdges = b->nEdges;
    if (maxContours) *maxContours = b->maxContours;
    if (maxEdges) *maxEdges = b->maxEdges;
    return MSDFHIP_OK;
}

int msdfhip_batch_download(const MsdfHipBatch *b, int32_t *co, double *points, uint8_t *types, uint8_t *colors) {
    if (!b)
        return fail(MSDFHIP_ERR_INVALID, "NULL batch");
    int rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    HIPCHK(hipDeviceSynchronize());
    if (co)
        HIPCHK(hipMemcpy(co, b->dContourOffsets.ptr, sizeof(int32_t)*(size_t) (b->nContours+1), hipMemcpyDeviceToHost));
    if (points && b->nEdges)
        HIPCHK(hipMemcpy(points, b->dPoints.ptr, sizeof(double)*8*(size_t) b->nEdges, hipMemcpyDeviceToHost));
    if (types && b->nEdges)
        HIPCHK(hipMemcpy(types, b->dTypes.ptr, (size_t) b->nEdges, hipMemcpyDeviceToHost));
    if (colors && b->nEdges)
        HIPCHK(hipMemcpy(colors, b->dColors.ptr, (size_t) b->nEdges, hipMemcpyDeviceToHost));
    return MSDFHIP_OK;
}

int msdfhip_batch_digest(MsdfHipBatch *b, void *stream) {
    if (!b)
        return fail(MSDFHIP_ERR_INVALID, "NULL batch");
    int rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    return digest(b, (hipStream_t) stream);
}

void msdfhip_batch_destroy(MsdfHipBatch *b) {
    if (!b)
        return;
    (void) hipSetDevice(b->device);
    delete b;                                                    // (what it owns of its arrays and its workspace goes with it, on that device)
}

int msdfhip_batch_windings(const MsdfHipBatch *b, int32_t *windings) {
    if (!b || !windings)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    int rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    std::vector<int8_t> tmp((size_t) b->nContours+1);
    HIPCHK(hipDeviceSynchronize());
    if (b->nContours)
        HIPCHK(hipMemcpy(tmp.data(), b->dWindings.ptr, (size_t) b->nContours, hipMemcpyDeviceToHost));
    for (int c = 0; c < b->nContours; ++c)
        windings[c] = tmp[c];
    return MSDFHIP_OK;
}

// Shape::getBounds of the batch's glyphs into b->dBounds.ptr on `stream` (and, with `frame`, the framed xf into dGlyphs): one k_frame launch.
static int frameBatch(const MsdfHipBatch *b, const FrameParams *frame, int w, int h, MsdfHipGlyph *dGlyphs, hipStream_t stream) {
    HIPCHK(b->dBounds.ensure(4*(size_t) (b->nGlyphs > 0 ? b->nGlyphs : 1)));
    const EdgeArrays edges = { b->dPoints.ptr, b->dTypes.ptr, b->dColors.ptr };
    return queueFrame(edges, b->dGlyphContourOffsets.ptr, b->dContourOffsets.ptr, b->nGlyphs, b->dBounds.ptr, b->boundsFixed, frame, w, h, dGlyphs, stream);
}

int msdfhip_batch_bounds(const MsdfHipBatch *b, double *bounds) {
    if (!b || !bounds)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    int rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    HIPCHK(hipDeviceSynchronize());                              // (the edge arrays may still be written by work the caller queued)
    if (!b->boundsFixed) {
        rc = frameBatch(b, NULL, 0, 0, NULL, NULL);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    HIPCHK(hipStreamSynchronize(NULL));
    if (b->nGlyphs)
        HIPCHK(hipMemcpy(bounds, b->dBounds.ptr, sizeof(double)*4*(size_t) b->nGlyphs, hipMemcpyDeviceToHost));
    return MSDFHIP_OK;
}

int msdfhip_batch_frame(const MsdfHipBatch *b, const MsdfHipFrameConfig *frame, int w, int h, MsdfHipGlyph *dGlyphs, void *stream) {
    FrameParams f;
    bool framed = false;
    int rc = checkFrameConfig(frame, w, h, "msdfhip_batch_frame", &f, &framed);
    if (rc != MSDFHIP_OK)
        return rc;
    if (!b || !framed || !dGlyphs)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_frame: NULL argument");
    rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    return frameBatch(b, &f, w, h, dGlyphs, (hipStream_t) stream);
}

// One generate call on b (arguments checked, device bound): distance pass -> sign correction -> error correction.
static int runGenerate(const MsdfHipBatch *b, int mode, int w, int h, const MsdfHipGlyph *dGlyphs, float *dOut, uint8_t *dStencil, float *dScratch,
                       const MsdfHipConfig *cfg, hipStream_t stream, GenerateCall &call) {
    if (b->nGlyphs == 0 || w == 0 || h == 0)
        return MSDFHIP_OK;                                       // zero-size bitmap: no-op, like the reference loops
    int rc = MSDFHIP_OK;
    const bool overlap = cfg->overlap_support != 0;
    const bool correct = mode >= 3 && cfg->ec_mode != MSDFHIP_EC_DISABLED; // msdf-error-correction.cpp:13-14
    const bool signPass = cfg->sign_correction != 0;                       // main.cpp:1281-1298: generate -> sign correction -> error correction
    // Intermediate fields (packed [g][h][w][N], native rows): stage A = distance field, stage B = sign-corrected field.
    const int stages = (correct ? 1 : 0)+(signPass ? 1 : 0);
    const size_t tileFloats = (size_t) b->nGlyphs*w*h*channelsOf(mode);
    if (stages && !dScratch) {
        rc = ensureScratch(b, tileFloats*stages, &dScratch);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    float *stageA = stages ? dScratch : NULL, *stageB = stages == 2 ? dScratch+tileFloats : NULL;
    float *dst = stages ? stageA : dOut;
    const MsdfHipConfig *ecAhead = correct && !call.ecParamsQueued ? cfg : NULL;   // (taken only where the distance pass forks its classes onto side streams)
    forOneOf<1, 2, 3, 4>(mode, [&](auto sel) { rc = dispatchDistance<decltype(sel)::value>(b, dGlyphs, w, h, dst, stages != 0, overlap, stream, ecAhead, call); });
    if (rc == MSDFHIP_OK && call.afterDistance)
        HIPCHK(hipEventRecord(call.afterDistance, stream));
    if (rc != MSDFHIP_OK || !stages)
        return rc;
    const float *ecSrc = stageA;
    if (signPass) {
        rc = runSignCorrection(b, channelsOf(mode), w, h, dGlyphs, stageA, correct ? stageB : dOut, correct ? 1 : 0, cfg->sdf_zero_value, cfg->fill_rule, stream, call.boxDims);
        if (rc != MSDFHIP_OK || !correct)
            return rc;
        ecSrc = stageB;
    }
    return runCorrection(b, channelsOf(mode), w, h, dGlyphs, ecSrc, dOut, dStencil, *cfg, stream, call);
}

int msdfhip_batch_generate(const MsdfHipBatch *b, int mode, int w, int h, const MsdfHipGlyph *dGlyphs, float *dOut, uint8_t *dStencil,
                           float *dScratch, const MsdfHipConfig *cfg, void *streamPtr) {
    if (!b || mode < 1 || mode > 4 || w < 0 || h < 0 || !dGlyphs || !dOut)
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_batch_generate");
    int rc = checkConfig(cfg);
    if (rc != MSDFHIP_OK)
        return rc;
    rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    GenerateCall call;
    return runGenerate(b, mode, w, h, dGlyphs, dOut, dStencil, dScratch, cfg, (hipStream_t) streamPtr, call);
}

int msdfhip_batch_generate_legacy(const MsdfHipBatch *b, int mode, int w, int h, const MsdfHipGlyph *dGlyphs, float *dOut, uint8_t *dStencil,
                                  float *dScratch, const MsdfHipConfig *cfg, void *streamPtr) {
    if (!b || mode < 1 || mode > 4 || w < 0 || h < 0 || !dGlyphs || !dOut || !cfg)
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_batch_generate_legacy");
    const MsdfHipConfig legacy = legacyConfig(*cfg);
    int rc = checkConfig(&legacy);
    if (rc != MSDFHIP_OK)
        return rc;
    rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    GenerateCall call;
    return runGenerateLegacy(b, mode, w, h, dGlyphs, dOut, dStencil, dScratch, legacy, (hipStream_t) streamPtr, call);
}

int msdfhip_batch_error_correction_legacy(float *dTiles, int nGlyphs, int w, int h, int channels, float *dScratch, double thresholdX, double thresholdY,
                                          void *streamPtr) {
    if (nGlyphs < 0 || w < 0 || h < 0 || (channels != 3 && channels != 4))
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_batch_error_correction_legacy (channels must be 3 or 4)");
    if (nGlyphs == 0 || w == 0 || h == 0)
        return MSDFHIP_OK;
    if (!dTiles || !dScratch)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_error_correction_legacy: NULL argument");
    int rc = ensureDeviceOf(dTiles);
    if (rc != MSDFHIP_OK)
        return rc;
    return launchLegacyCorrection(dTiles, dScratch, nGlyphs, w, h, channels, thresholdX, thresholdY, (hipStream_t) streamPtr);
}

int msdfhip_tiles_to_bytes(const float *dTiles, int nGlyphs, int w, int h, int channels, const MsdfHipGlyph *dGlyphs, uint8_t *dAtlas, void *streamPtr) {
    if (nGlyphs < 0 || w < 0 || h < 0 || (channels != 1 && channels != 3 && channels != 4))
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_tiles_to_bytes");
    const size_t total = (size_t) nGlyphs*w*h;
    if (!total)
        return MSDFHIP_OK;
    if (!dTiles || !dGlyphs || !dAtlas)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    int rc = ensureDeviceOf(dTiles);
    if (rc != MSDFHIP_OK)
        return rc;
    hipStream_t stream = (hipStream_t) streamPtr;
    const unsigned blocks = (unsigned) ((total+255)/256 < 65536 ? (total+255)/256 : 65536);
    forOneOf<1, 3, 4>(channels, [&](auto n) { hipLaunchKernelGGL(k_tiles_to_bytes<decltype(n)::value>, dim3(blocks), dim3(256), 0, stream, dTiles, dGlyphs, nGlyphs, w, h, dAtlas); });
    HIPCHK(hipGetLastError());
    return MSDFHIP_OK;
}

namespace {

// The launches of an error estimate over `items` scanlines (> 0), planned by msdf_qualityplan.hpp: k_sdf_error_lines over chunks of lanes whose lists fit the
// workspace cap (MSDFHIP_ERROR_WORKSPACE_MB), then k_sdf_error_sum. w x h: the fields of a uniform call; in a sized call (`table`: the host copy of the device
// table of k_sdf_error_lines_sized) the largest width and height, and the twins run from the same argument lists with the table, which is uploaded on `stream`
// into the workspace, behind them. The workspace (ensureGres): lines[items] | the table | the lists of one chunk.
int runEstimate(const MsdfHipBatch *b, int channels, int w, int h, const MsdfHipGlyph *dGlyphs, const float *dTiles, int scanlinesPerRow, int fillRule, double *dErrors,
                hipStream_t stream, size_t items, const std::vector<int64_t> *table) {
    const size_t refCap = errorRefCap(b->maxEdges), sdfCap = errorSdfCap(w);
    const size_t perLane = errorLaneBytes(refCap, sdfCap);
    const size_t chunk = errorChunkLanes((int64_t) items, perLane, tuning().errorWorkspaceBytes);   // lanes per launch
    const size_t tableWords = table ? table->size() : 0;
    double *work = NULL;
    int rc = ensureGres(b, chunk*perLane+(items+tableWords)*sizeof(double), &work);
    if (rc != MSDFHIP_OK)
        return rc;
    double *lines = work;                                            // [items]
    double *listX = work+items+tableWords;                           // [refCap+sdfCap][chunk]
    int *listDir = reinterpret_cast<int *>(listX+(refCap+sdfCap)*chunk);
    const int32_t *dDims = NULL;
    if (table) {
        HIPCHK(hipMemcpyAsync(work+items, table->data(), sizeof(int64_t)*tableWords, hipMemcpyHostToDevice, stream));
        dDims = reinterpret_cast<const int32_t *>(work+items);
    }
    for (size_t base = 0; base < items; base += chunk) {
        const size_t n = items-base < chunk ? items-base : chunk;
        const dim3 grid((unsigned) ((n+63)/64));
        forOneOf<1, 3, 4>(channels, [&](auto c) {
            launchTwinned(k_sdf_error_lines<decltype(c)::value>, errorLinesSizedKernel(decltype(c)::value), dDims, grid, 0, stream, viewOf(b), dGlyphs, dTiles, w, h,
                          scanlinesPerRow, fillRule, base, n, listX, listDir, (int) refCap, lines);
        });
    }
    launchTwinned(k_sdf_error_sum, errorSumSizedKernel(), dDims, dim3((b->nGlyphs+63)/64), 0, stream, (const double *) lines, b->nGlyphs, h, scanlinesPerRow, dErrors);
    HIPCHK(hipGetLastError());
    return MSDFHIP_OK;
}

// The launch of a rendering of `total` output texels (> 0) with the range mapping `m` (msdf_qualityplan.hpp): k_render_sdf, or with dDims (the device table
// of a sized call) its twin from the same argument list.
int launchRender(int no, int ns, const int32_t *dDims, size_t total, hipStream_t stream, const float *dSdf, int nGlyphs, int sw, int sh, float *dOut, int ow, int oh,
                 const RenderMapping &m, int threshold, float sdThreshold) {
    const float sdBias = threshold ? 0.f : .5f-sdThreshold;
    const unsigned blocks = (unsigned) ((total+255)/256 < 65536 ? (total+255)/256 : 65536);
    #define RENDER(NO, NS) launchTwinnedBlock(k_render_sdf<NO, NS>, renderSizedKernel(NO, NS), dDims, dim3(blocks), dim3(256), stream, dSdf, nGlyphs, sw, sh, dOut, ow, oh, \
                                              m.scaleX, m.scaleY, threshold, m.mapScale, m.mapTranslate, sdThreshold, sdBias)
    if (no == 1 && ns == 1) RENDER(1, 1);
    else if (no == 3 && ns == 1) RENDER(3, 1);
    else if (no == 1 && ns == 3) RENDER(1, 3);
    else if (no == 3 && ns == 3) RENDER(3, 3);
    else if (no == 1 && ns == 4) RENDER(1, 4);
    else RENDER(4, 4);
    #undef RENDER
    HIPCHK(hipGetLastError());
    return MSDFHIP_OK;
}

bool renderChannelsOk(int no, int ns) { return (no == 1 && (ns == 1 || ns == 3 || ns == 4)) || (no == 3 && (ns == 1 || ns == 3)) || (no == 4 && ns == 4); }

} // namespace

int msdfhip_batch_estimate_sdf_error(const MsdfHipBatch *b, int channels, int w, int h, const MsdfHipGlyph *dGlyphs, const float *dTiles,
                                     int scanlinesPerRow, int fillRule, double *dErrors, void *streamPtr) {
    if (!b || !dGlyphs || !dTiles || !dErrors || w < 0 || h < 0 || (channels != 1 && channels != 3 && channels != 4))
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_batch_estimate_sdf_error");
    if (fillRule < 0 || fillRule > 3)
        return fail(MSDFHIP_ERR_INVALID, "fill rule %d (must be 0..3)", fillRule);
    int rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    hipStream_t stream = (hipStream_t) streamPtr;
    if (b->nGlyphs == 0)
        return MSDFHIP_OK;
    if (w <= 1 || h <= 1 || scanlinesPerRow < 1) {                   // sdf-error-estimation.cpp:136-137: the estimate is 0
        HIPCHK(hipMemsetAsync(dErrors, 0, sizeof(double)*(size_t) b->nGlyphs, stream));
        return MSDFHIP_OK;
    }
    const size_t perGlyph = (size_t) (h-1)*scanlinesPerRow, items = perGlyph*b->nGlyphs;
    return runEstimate(b, channels, w, h, dGlyphs, dTiles, scanlinesPerRow, fillRule, dErrors, stream, items, NULL);
}

int msdfhip_render_sdf(const float *dSdf, int nGlyphs, int sw, int sh, int ns, float *dOut, int ow, int oh, int no, double rangeLower, double rangeUpper,
                       float sdThreshold, void *streamPtr) {
    if (nGlyphs < 0 || sw < 0 || sh < 0 || ow < 0 || oh < 0)
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_render_sdf");
    if (!renderChannelsOk(no, ns))
        return fail(MSDFHIP_ERR_INVALID, "renderSDF has no overload for %d <- %d channels (core/render-sdf.h:12-17)", no, ns);
    const size_t total = (size_t) nGlyphs*ow*oh;
    if (!total)
        return MSDFHIP_OK;
    if (!dSdf || !dOut || sw == 0 || sh == 0)
        return fail(MSDFHIP_ERR_INVALID, "NULL or empty distance field");
    int rc = ensureDeviceOf(dSdf);
    if (rc != MSDFHIP_OK)
        return rc;
    return launchRender(no, ns, NULL, total, (hipStream_t) streamPtr, dSdf, nGlyphs, sw, sh, dOut, ow, oh, renderMapping(sw, sh, ow, oh, rangeLower, rangeUpper),
                        rangeLower == rangeUpper, sdThreshold);
}

int msdfhip_simulate_8bit(float *dPixels, size_t n, void *streamPtr) {
    if (!n)
        return MSDFHIP_OK;
    if (!dPixels)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    int rc = ensureDeviceOf(dPixels);
    if (rc != MSDFHIP_OK)
        return rc;
    const unsigned blocks = (unsigned) ((n+255)/256 < 65536 ? (n+255)/256 : 65536);
    hipLaunchKernelGGL(k_simulate_8bit, dim3(blocks), dim3(256), 0, (hipStream_t) streamPtr, dPixels, n);
    HIPCHK(hipGetLastError());
    return MSDFHIP_OK;
}

// ------------------------------------------------------------------------------------------- host-output pipeline
//
// msdfhip_batch_generate_host / _bytes_host: the end-to-end form an atlas generator wants -- the batch's glyphs rendered into HOST
// memory. The glyph list is cut into chunks; two slots (stream + device tile buffer + work buffers each) alternate, so the kernels
// of chunk k+1 overlap the device-to-host copy of chunk k. A chunk is a non-owning view of the batch (the CSR arrays are global:
// a glyph range is the same arrays with shifted glyph offsets).

enum { PIPE_SLOTS = 4 };
struct PipeSlot {
    Stream stream;                    // kernels and copy back of the slot's chunk (declared first: it goes last, after everything queued on it)
    Event done;                       // the slot's last device-to-host copy has finished
    Event kernelsDone;                // the kernels (and the small uploads before them) of the slot's last chunk have finished
    Event distanceDone;               // the distance pass of the slot's last chunk has finished (its correction pass may still run)
    WorkBuffer<unsigned, true> pinnedOverflow;   // pinned, device-visible word: k_ec_query mirrors the chunk's candidate-overflow count here (no k_ec_slow launch per chunk)
    bool busy = false;
    WorkBuffer<char> dev;             // [descriptors | float tiles | stencil | byte tiles] (slotLayout)
    WorkBuffer<MsdfHipGlyph, true> pinnedGlyphs;   // pinned staging of the chunk's descriptors: the generators' in the first half, the byte conversion's in the second
    WorkBuffer<char, true> pinnedTiles;   // pinned staging of the chunk's output when the caller's layout is not packed (scattered on the host)
    int pendingFirst = 0, pendingCount = 0;   // the chunk waiting in pinnedTiles for its scatter
    MsdfHipBatch view;                // glyph range of the parent batch + this slot's own workspace (its per-glyph buffers hold a full chunk)
    // streamed calls (msdfhip_generate_stream): the chunk's own inputs
    WorkBuffer<char, true> pinnedIn;  // pinned staging the host threads flatten the chunk's shapes into: [gco | co | points | types | colors]
    WorkBuffer<char> devIn;           // the same on the device, followed by the chunk's records and windings
    Event inputsUploaded;             // the chunk's upload has left pinnedIn
    bool inputsInFlight = false;
    Event prepCounted;                // streamed calls of raw outlines: the chunk's coloured contour offsets have reached pinnedIn (StreamFeeder::prepare)
    MsdfHipGlyph *frameGlyphs = NULL; // framed streamed calls: the chunk's descriptors on the device, uploaded BEFORE its shapes so that k_frame can write their xf

    hipError_t create() {
        hipError_t e = stream.create(hipStreamNonBlocking);
        Event *const events[] = { &done, &kernelsDone, &distanceDone, &inputsUploaded, &prepCounted };
        for (size_t k = 0; e == hipSuccess && k < sizeof(events)/sizeof(events[0]); ++k)
            e = events[k]->create(hipEventDisableTiming);
        if (e == hipSuccess && (e = pinnedOverflow.ensure(64)) == hipSuccess)
            pinnedOverflow.ptr[0] = 0;
        return e;
    }
};

// The slots of a pipeline in flight. Pipelines live in a process-wide pool per device (like the arenas of the single-shape calls):
// a host-output call takes one and returns it, so that a caller that builds a fresh batch per atlas does not pay for 100+ MB of
// device / pinned allocations every time; the pool is bounded by the peak number of concurrent host-output calls.
struct Pipe {
    int device = 0;
    PipeSlot slot[PIPE_SLOTS];
    hipError_t create(int d) {
        device = d;
        hipError_t e = hipSuccess;
        for (int k = 0; e == hipSuccess && k < PIPE_SLOTS; ++k) {
            slot[k].view.onDevice(d);
            e = slot[k].create();
        }
        return e;
    }
    void quiesce() {                  // idle streams answer at once
        for (int k = 0; k < PIPE_SLOTS; ++k)
            if (slot[k].stream)
                (void) hipStreamSynchronize(slot[k].stream);
    }
};

static DevicePool<Pipe> gPipePool;

// Points slot.view at glyphs [g0, g0+n) of b (shared, read-only inputs; the slot keeps its own work buffers across chunks and calls).
static void sliceBatch(const MsdfHipBatch *b, MsdfHipBatch &v, int g0, int n) {
    v.onDevice(b->device);
    v.nGlyphs = n, v.nContours = b->nContours, v.nEdges = b->nEdges;
    v.dGlyphContourOffsets.borrow(b->dGlyphContourOffsets.ptr+g0, (size_t) n+1);   // entries are absolute contour indices: valid from any starting glyph
    v.dContourOffsets.borrow(b->dContourOffsets.ptr, b->dContourOffsets.cap), v.dPoints.borrow(b->dPoints.ptr, b->dPoints.cap);
    v.dTypes.borrow(b->dTypes.ptr, b->dTypes.cap), v.dColors.borrow(b->dColors.ptr, b->dColors.cap);
    v.dRecs.borrow(b->dRecs.ptr, b->dRecs.cap), v.dWindings.borrow(b->dWindings.ptr, b->dWindings.cap);
    v.setCounts(b->hContours.data()+g0, b->hEdges.data()+g0, n);
    v.work.newGlyphRange();                                      // the class lists are per glyph range
    v.serialClasses = true;                                      // pipeline chunks overlap each other; side streams per chunk only alias the few hardware queues
}

static std::atomic<int> gPipeChunkGlyphs(0);                     // 0 = automatic (about 96 MB of float tiles per chunk)

// ---- host threads of the streamed generator (msdfhip_generate_stream): a small persistent pool that flattens the NEXT chunk's shapes into pinned staging
// while the device works on the chunks before it. Jobs are index ranges; whoever waits for a job helps to finish it. Created on first use, lives as long
// as the process (reachable through gHostPool; its idle threads sleep on a condition variable).
static int usableCores() {
    int n = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0)
        n = CPU_COUNT(&set);
    if (n <= 0)
        n = (int) std::thread::hardware_concurrency();
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {       // cgroup v2 quota: "max 100000" or "<quota> <period>"
        long long quota = 0, period = 0;
        if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) {
            const int q = (int) ((quota+period-1)/period);
            n = q < n ? q : n;
        }
        fclose(f);
    }
    return n < 1 ? 1 : n;
}

struct HostJob {
    std::function<void(int)> fn;
    int count;
    std::atomic<int> next, done;
    std::atomic<bool> cancelled;                                 // items not yet started are taken but not run (HostPool::cancelAndWait)
    std::mutex m;
    std::condition_variable cv;
    HostJob() : count(0), next(0), done(0), cancelled(false) { }
};

class HostPool {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::shared_ptr<HostJob> > queue;
    std::vector<std::thread> workers;
    static void runItems(HostJob &job) {
        for (int i; (i = job.next.fetch_add(1)) < job.count; ) {
            if (!job.cancelled.load())
                job.fn(i);
            if (job.done.fetch_add(1)+1 == job.count) {
                std::lock_guard<std::mutex> lock(job.m);
                job.cv.notify_all();
            }
        }
    }
    void loop() {
        for (;;) {
            std::shared_ptr<HostJob> job;
            {
                std::unique_lock<std::mutex> lock(mu);
                for (;;) {
                    while (!queue.empty() && queue.front()->next.load() >= queue.front()->count)
                        queue.pop_front();                       // all its items are taken: nothing left to start
                    if (!queue.empty())
                        break;
                    cv.wait(lock);
                }
                job = queue.front();
            }
            runItems(*job);
        }
    }
public:
    explicit HostPool(int threads) {
        for (int t = 0; t < threads; ++t) {
            workers.push_back(std::thread([this]() { loop(); }));
            workers.back().detach();
        }
    }
    int threads() const { return (int) workers.size(); }
    std::shared_ptr<HostJob> submit(int count, std::function<void(int)> fn) {
        std::shared_ptr<HostJob> job = std::make_shared<HostJob>();
        job->fn = fn, job->count = count;
        if (count > 0) {
            std::lock_guard<std::mutex> lock(mu);
            queue.push_back(job);
            cv.notify_all();
        }
        return job;
    }
    static void wait(HostJob &job) {                             // the waiting thread takes items too
        runItems(job);
        std::unique_lock<std::mutex> lock(job.m);
        while (job.done.load() < job.count)
            job.cv.wait(lock);
    }
    // A call that ends early: no further item of the job starts, and the items already running on pool threads have returned when this does --
    // nothing of the job touches the caller's objects or the call's buffers afterwards.
    static void cancelAndWait(HostJob &job) {
        job.cancelled.store(true);
        wait(job);
    }
};
static std::mutex gHostPoolMutex;
static HostPool *gHostPool = NULL;
static std::atomic<int> gHostThreads(0);                         // msdfhip_set_host_threads / MSDFHIP_HOST_THREADS; 0 = the usable cores (at most 32)
static HostPool &hostPool() {
    std::lock_guard<std::mutex> lock(gHostPoolMutex);
    if (!gHostPool) {
        int n = gHostThreads.load();
        if (n <= 0)
            n = tuning().hostThreads > 0 ? tuning().hostThreads : usableCores();
        n = n > 32 ? 32 : n;
        gHostPool = new HostPool(n > 1 ? n-1 : 0);               // the caller's thread works too
    }
    return *gHostPool;
}

// Where the chunks of a host-output call come from. A resident batch (msdfhip_batch_generate_host): a chunk is a view of the batch's arrays. A shape
// source (msdfhip_generate_stream): a chunk is flattened by the host threads into the slot's pinned staging, uploaded and digested on the slot's stream
// -- while the device works on the chunks before it.
struct ChunkFeeder {
    virtual ~ChunkFeeder() { }
    virtual void drain() { }                                     // no host work of the feeder is running or will start after this (every exit of runPipelineOnce)
    virtual bool frames() const { return false; }                // prepare() writes the xf of the chunk's descriptors (PipeSlot::frameGlyphs) on the device
    virtual int begin(PipeSlot *slots, const std::vector<int> &lengths) = 0;
    virtual int prepare(PipeSlot &p, int slot, size_t chunkIndex, int g0, int n, hipStream_t stream) = 0;
};

struct ResidentFeeder : ChunkFeeder {
    const MsdfHipBatch *b;
    explicit ResidentFeeder(const MsdfHipBatch *batch) : b(batch) { }
    int begin(PipeSlot *, const std::vector<int> &) { return MSDFHIP_OK; }
    int prepare(PipeSlot &p, int, size_t, int g0, int n, hipStream_t) {
        sliceBatch(b, p.view, g0, n);
        return MSDFHIP_OK;
    }
};

// The shapes of a streamed call, as counted up front (one cheap pass over the caller's objects: contours per glyph, edges per glyph).
struct StreamFeeder : ChunkFeeder {
    const MsdfHipShapeSource *src;
    int nG;
    std::vector<int> hContours, hEdges;                          // per glyph
    std::vector<long long> contourBase, edgeBase;                // prefix sums over the whole list (nG+1)
    PrepPlanConfig planCfg;                                      // which regions a chunk's input area holds (msdf_prepplan.hpp); hitsBig / longContour per chunk
    StreamPrepPlan plan;                                         // the chunks and what every slot must hold (begin)
    std::vector<std::shared_ptr<HostJob> > jobs;                 // flatten job of chunk k
    std::unique_ptr<std::atomic<int>[]> badType;                 // per chunk: a glyph whose fill produced an edge type outside 1..3 (-1: none); written by pool threads
    PipeSlot *slots;
    // Raw outlines (msdfhip_generate_stream_prepared): every chunk is prepared on its own stream between its upload and its digest (queuePreparation),
    // from the same staging the prepared form uses plus the host's normalized contour offsets (and the chunk's seeds) behind it.
    const MsdfHipPrepConfig *prep;                               // NULL: the shapes are prepared already
    const uint64_t *seeds;                                       // one per glyph of the whole list, or NULL (prep->seed)
    MsdfHipOrientConfig orient;                                  // orientation around the preparation (checked; all 0: keep)
    double crossThreshold;                                       // sin(angle_threshold), by the host's libm (edge-coloring.cpp:69)
    const FrameParams *frame;                                    // raw outlines only: every chunk is framed between its preparation and its digest (k_frame); NULL: the caller's xf
    int frameW, frameH;
    enum { GRAIN = 32 };                                         // glyphs per flatten item

    StreamFeeder(const MsdfHipShapeSource *source, int n, const MsdfHipPrepConfig *prepCfg = NULL, const uint64_t *glyphSeeds = NULL,
                 const MsdfHipOrientConfig *orientCfg = NULL, const FrameParams *frameCfg = NULL, int w = 0, int h = 0)
        : src(source), nG(n), slots(NULL), prep(prepCfg), seeds(glyphSeeds), crossThreshold(prepCfg && prepCfg->coloring ? sin(prepCfg->angle_threshold) : 0.),
          frame(prepCfg ? frameCfg : NULL), frameW(w), frameH(h) {
        orient.orient_contours = orientCfg ? orientCfg->orient_contours : 0, orient.winding = orientCfg ? orientCfg->winding : 0;
        const PrepPlanConfig c = { prep != NULL, prep ? prep->coloring : 0, seeds != NULL, true, orient.orient_contours != 0, false, false, frame != NULL, true };
        planCfg = c;
    }
    ~StreamFeeder() { drain(); }
    bool frames() const { return frame != NULL; }

    // The flatten jobs run on the detached pool threads, capture `this`, call the caller's fill callbacks and write into the leased pipe's pinned staging:
    // when the pipeline leaves early (a bad glyph, a HIP error inside the chunk loop) the jobs of the chunks ahead must not outlive the call.
    void drain() {
        for (size_t ci = 0; ci < jobs.size(); ++ci)
            if (jobs[ci])
                HostPool::cancelAndWait(*jobs[ci]);
        jobs.clear();
    }

    int count() {                                                // parallel over the glyphs; then the prefix sums
        hContours.assign((size_t) nG, 0), hEdges.assign((size_t) nG, 0);
        const int items = (nG+255)/256;
        std::atomic<int> bad(-1);
        std::shared_ptr<HostJob> job = hostPool().submit(items, [this, &bad](int it) {
            const int g1 = (it+1)*256 < nG ? (it+1)*256 : nG;
            for (int g = it*256; g < g1; ++g) {
                int32_t c = 0, e = 0;
                src->count(src->user, g, &c, &e);
                if (c < 0 || e < 0 || (c == 0 && e != 0))
                    bad.store(g);
                hContours[(size_t) g] = c, hEdges[(size_t) g] = e;
            }
        });
        HostPool::wait(*job);
        if (bad.load() >= 0)
            return fail(MSDFHIP_ERR_INVALID, "shape source: glyph %d reports %d contours / %d edges", bad.load(), hContours[(size_t) bad.load()], hEdges[(size_t) bad.load()]);
        contourBase.assign((size_t) nG+1, 0), edgeBase.assign((size_t) nG+1, 0);
        for (int g = 0; g < nG; ++g) {
            contourBase[(size_t) g+1] = contourBase[(size_t) g]+hContours[(size_t) g];
            edgeBase[(size_t) g+1] = edgeBase[(size_t) g]+hEdges[(size_t) g];
        }
        return MSDFHIP_OK;
    }

    // A chunk's inputs inside a slot's pinned staging / device input area (msdf_prepplan.hpp): the uploaded regions, then on the device the preparation's
    // buffers and the records + windings of the PREPARED edges. begin() sizes the slots from the plan's bounds; a chunk carves its exact counts.
    PrepCarve carve(const StreamChunk &ch, size_t nE1 = 0, size_t nE2 = 0, bool longContour = false, bool hitsBig = false) const {
        PrepPlanConfig c = planCfg;
        c.longContour = longContour, c.hitsBig = hitsBig;
        const PrepCounts counts = { (size_t) ch.length, ch.nC, ch.nE, nE1, nE2 };
        return prepCarve(c, counts);
    }

    void flattenItem(size_t ci, int item) {
        const int g0 = plan.chunks[ci].start, n = plan.chunks[ci].length;
        const long long c0 = contourBase[(size_t) g0], e0 = edgeBase[(size_t) g0];
        const PrepBuffers staged = bindPrep(slots[ci%PIPE_SLOTS].pinnedIn.ptr, carve(plan.chunks[ci]));   // (the uploaded regions alone)
        int32_t *gco = const_cast<int32_t *>(staged.gco), *co = const_cast<int32_t *>(staged.co);
        double *points = staged.raw.points;
        uint8_t *types = staged.raw.types, *colors = staged.raw.colors;
        const int first = item*GRAIN, last = first+GRAIN < n ? first+GRAIN : n;
        if (item == 0)
            gco[0] = 0, co[0] = 0;
        for (int k = first; k < last; ++k) {
            const int g = g0+k;
            const int32_t cRel = (int32_t) (contourBase[(size_t) g]-c0), eRel = (int32_t) (edgeBase[(size_t) g]-e0);
            const int nC = hContours[(size_t) g], nE = hEdges[(size_t) g];
            gco[k+1] = cRel+nC;
            if (nC > 0) {
                src->fill(src->user, g, eRel, co+cRel+1, points+(size_t) eRel*8, types+eRel, colors+eRel);
                bool ok = co[cRel+nC] == eRel+nE;                // the source must deliver what it counted
                for (int c = 0; c < nC && ok; ++c)
                    ok = co[cRel+1+c] >= (c ? co[cRel+c] : eRel);
                for (int e = 0; e < nE && ok; ++e)
                    ok = types[eRel+e] >= 1 && types[eRel+e] <= 3;
                if (!ok)
                    badType[ci].store(g);                        // (any thread may write it: the value only says which glyph to name)
            }
        }
    }

    void startFlatten(size_t ci) {
        if (ci >= plan.chunks.size() || jobs[ci])
            return;
        const int items = (plan.chunks[ci].length+GRAIN-1)/GRAIN;
        jobs[ci] = hostPool().submit(items, [this, ci](int item) { flattenItem(ci, item); });
    }

    int begin(PipeSlot *pipeSlots, const std::vector<int> &lengths) {
        slots = pipeSlots;
        plan = planStreamPrep(hContours.data(), hEdges.data(), lengths, planCfg);
        if (plan.refused >= 0) {
            const StreamChunk &ch = plan.chunks[(size_t) plan.refused];
            return fail(MSDFHIP_ERR_INVALID, "a pipeline chunk of %d glyphs holds %zu edges / %zu contours: beyond the 32-bit offsets of a batch", ch.length, ch.nE, ch.nC);
        }
        jobs.assign(lengths.size(), std::shared_ptr<HostJob>());
        badType.reset(new std::atomic<int>[lengths.size() ? lengths.size() : 1]);
        for (size_t ci = 0; ci < lengths.size(); ++ci)
            badType[ci].store(-1);
        const size_t needIn = plan.pinnedBytes, devNeed = plan.devBytes+256;
        for (int k = 0; k < PIPE_SLOTS; ++k) {                   // every slot can take the largest chunk (grown once, kept with the pooled pipe)
            PipeSlot &p = slots[k];
            if (p.pinnedIn.cap < needIn)
                HIPCHK(p.pinnedIn.ensure(needIn+needIn/4+4096));
            if (p.devIn.cap < devNeed) {
                HIPCHK(hipStreamSynchronize(p.stream));
                HIPCHK(p.devIn.ensure(devNeed+devNeed/4+4096));
            }
            p.inputsInFlight = false;
        }
        for (size_t ci = 0; ci < lengths.size() && ci < 2; ++ci)     // two chunks ahead of the device from the start
            startFlatten(ci);
        return MSDFHIP_OK;
    }

    int prepare(PipeSlot &p, int slot, size_t ci, int g0, int n, hipStream_t stream) {
        HostPool::wait(*jobs[ci]);
        if (badType[ci].load() >= 0)
            return fail(MSDFHIP_ERR_INVALID, "shape source: glyph %d did not deliver the contours / edges it counted, or an edge type outside 1..3", badType[ci].load());
        // keep the host threads two chunks ahead of the device: chunk ci+2 goes into the staging of the slot chunk ci+2-PIPE_SLOTS used -- that chunk's
        // upload (queued long ago) must have left it
        const size_t ahead = ci+2;
        if (ahead < plan.chunks.size()) {
            PipeSlot &q = slots[ahead%PIPE_SLOTS];
            if (&q != &p && q.inputsInFlight) {
                HIPCHK(hipEventSynchronize(q.inputsUploaded));
                q.inputsInFlight = false;
            }
            if (&q != &p)
                startFlatten(ahead);
        }
        const StreamChunk &ch = plan.chunks[ci];
        const int nC = (int) ch.nC;
        const PrepBuffers staged = bindPrep(p.pinnedIn.ptr, carve(ch));
        size_t bound2 = 0;
        int longest = 0;
        if (prep) {                                              // the normalized offsets and the seeds travel with the chunk's upload
            prepOffsets(staged.co, nC, prep->normalize != 0, const_cast<int32_t *>(staged.co1), &bound2, &longest);
            if (staged.seeds)
                memcpy(const_cast<unsigned long long *>(staged.seeds), seeds+g0, sizeof(uint64_t)*(size_t) n);
        }
        // the chunk's exact carve: inside the slot, which begin() sized from the bounds of these counts
        const PrepCarve cv = carve(ch, prep ? (size_t) staged.co1[nC] : 0, bound2, longest > PREP_WAVE_MAX_EDGES, ch.hitsBig);
        char *d = p.devIn.ptr;
        const PrepBuffers pb = bindPrep(d, cv);
        // (a kernel reading the pinned staging: never queues behind another chunk's copy back)
        const int rcUp = uploadSmall(d, p.pinnedIn.ptr, cv.uploadBytes, stream);
        if (rcUp != MSDFHIP_OK)
            return rcUp;
        HIPCHK(hipEventRecord(p.inputsUploaded, stream));
        p.inputsInFlight = true;
        MsdfHipBatch &v = p.view;
        v.onDevice(currentDevice());
        v.nGlyphs = n, v.nContours = nC, v.nEdges = (int) ch.nE;
        v.dGlyphContourOffsets.borrow(const_cast<int32_t *>(pb.gco), (size_t) n+1), v.dContourOffsets.borrow(const_cast<int32_t *>(pb.co), (size_t) nC+1);
        v.dPoints.borrow(pb.raw.points, cv.bytes[PREP_RAW_POINTS]/sizeof(double)), v.dTypes.borrow(pb.raw.types, cv.bytes[PREP_RAW_TYPES]);
        v.dColors.borrow(pb.raw.colors, cv.bytes[PREP_RAW_COLORS]);
        v.dRecs.borrow(reinterpret_cast<EdgeRec *>(prepRegionAt(d, cv, PREP_RECS)), cv.bytes[PREP_RECS]/sizeof(EdgeRec));   // (room for the final edges: digest has nothing to allocate)
        v.dWindings.borrow(reinterpret_cast<int8_t *>(prepRegionAt(d, cv, PREP_WINDINGS)), cv.bytes[PREP_WINDINGS]);
        v.setCounts(hContours.data()+g0, hEdges.data()+g0, n);
        if (prep) {
            const int rcPrep = prepareChunk(p, cv, pb, staged.gco, staged.co1, n, nC, longest, stream);
            if (rcPrep != MSDFHIP_OK)
                return rcPrep;
        }
        v.work.newGlyphRange();
        v.serialClasses = true;
        return digest(&v, stream);
    }

    // (raw outlines) the chunk's preparation on its stream, behind its upload; then p.view is pointed at the prepared arrays. The per-glyph edge counts the
    // launches are planned from are the PREPARED ones, and the colouring may split a contour in a way only the device knows: its contour offsets come back
    // (one small copy + an event). runPipelineOnce calls this after the previous chunk's kernels are queued, so the device has work while the host waits.
    // cv, pb: the chunk's carve and its buffers on the device; hGco, hCo1: the offsets in the pinned staging.
    int prepareChunk(PipeSlot &p, const PrepCarve &cv, const PrepBuffers &pb, const int32_t *hGco, const int32_t *hCo1, int n, int nC, int longest, hipStream_t stream) {
        int rc = queuePreparation(prep, orient, n, nC, hCo1[nC], longest, crossThreshold, pb, stream);
        if (rc != MSDFHIP_OK)
            return rc;
        if (frame) {                                             // bounds of the normalized edges -> xf of the chunk's descriptors, which are on the device already
            rc = queueFrame(pb.norm, pb.gco, pb.co1, n, reinterpret_cast<double *>(prepRegionAt(p.devIn.ptr, cv, PREP_BOUNDS)), false, frame, frameW, frameH, p.frameGlyphs, stream);
            if (rc != MSDFHIP_OK)
                return rc;
        }
        const int32_t *hFinal = hCo1;                            // without colouring the host knows the final offsets already
        if (prep->coloring) {
            // the offsets come back by the word-copy kernel writing into the pinned staging rather than by a copy, which would share the copy engine with
            // the earlier chunks' tiles (measured the same either way on 8 192 glyphs, tools/stream_raw_bench.py: the wait is the preparation itself)
            int32_t *hCo2 = reinterpret_cast<int32_t *>(p.pinnedIn.ptr+cv.uploadBytes);
            rc = uploadSmall(hCo2, pb.co2, sizeof(int32_t)*(size_t) (nC+1), stream);
            if (rc != MSDFHIP_OK)
                return rc;
            HIPCHK(hipEventRecord(p.prepCounted, stream));
            HIPCHK(hipEventSynchronize(p.prepCounted));
            hFinal = hCo2;
        }
        MsdfHipBatch &v = p.view;
        v.nEdges = hFinal[nC];
        const int fin = prep->coloring ? PREP_FIN_POINTS : PREP_NORM_POINTS;
        v.dContourOffsets.borrow(prep->coloring ? pb.co2 : const_cast<int32_t *>(pb.co1), (size_t) nC+1);
        v.dPoints.borrow(pb.fin.points, cv.bytes[fin]/sizeof(double)), v.dTypes.borrow(pb.fin.types, cv.bytes[fin+1]), v.dColors.borrow(pb.fin.colors, cv.bytes[fin+2]);
        for (int g = 0; g < n; ++g)
            v.hEdges[(size_t) g] = hFinal[hGco[g+1]]-hFinal[hGco[g]];
        v.countMaxima();
        return MSDFHIP_OK;
    }

    static_assert(PIPE_SLOTS >= 3, "StreamFeeder flattens two chunks ahead of the one being queued: it needs three staging areas");
};

// Rows of the chunk waiting in the slot's pinned staging -> the caller's rectangles (any offsets / strides; nothing else is touched).
static void scatterPending(PipeSlot &p, const MsdfHipGlyph *glyphs, char *dst, size_t elem, int w, int h, int N) {
    const size_t rowBytes = (size_t) w*N*elem, tileBytes = rowBytes*h;
    for (int g = 0; g < p.pendingCount; ++g) {
        const MsdfHipGlyph &gd = glyphs[p.pendingFirst+g];
        const char *src = p.pinnedTiles.ptr+(size_t) g*tileBytes;
        for (int y = 0; y < h; ++y)
            memcpy(dst+((long long) gd.out_offset+(long long) gd.row_stride*y)*(long long) elem, src+(size_t) y*rowBytes, rowBytes);
    }
    p.pendingCount = 0;
}

// out != NULL: float tiles into the caller's bitmaps (glyphs[g].out_offset / row_stride in floats). atlas != NULL: pixelFloatToByte
// + blit into the caller's 8-bit atlas (out_offset / row_stride in bytes). Exactly one of the two.
// b: a resident batch (its chunks are views of it), or NULL with `feeder` = a shape source whose chunks are flattened, uploaded and digested as they come.
// GPU_MAX_HW_QUEUES as the host process set it (0: unset -- the runtime's default of 4). The library never changes the environment (see the top of this
// file); a multi-chunk pipeline call of a host that left the default says so ONCE on stderr when MSDFHIP_VERBOSE is set: its chunk streams alias on the
// 4 queues and a chunk's kernels wait behind another chunk's copy back (measured 12.0 instead of 10.2 ms per 8 192 glyphs, INTEGRATION.md "environment").
static int hwQueuesEnv() {
    const char *env = getenv("GPU_MAX_HW_QUEUES");
    return env && atoi(env) > 0 ? atoi(env) : 0;
}
static void hintHwQueuesOnce() {
    static std::atomic<bool> said(false);
    const int q = hwQueuesEnv();
    if ((q == 0 || q < 8) && getenv("MSDFHIP_VERBOSE") && !said.exchange(true))    // opt-in: a drop-in library does not write to its host's stderr; msdfhip_hw_queues_env() reports the same
        fprintf(stderr, "msdfgen_hip: note: GPU_MAX_HW_QUEUES is %s; the host-output pipeline overlaps its chunks on distinct hardware queues -- export "
                        "GPU_MAX_HW_QUEUES=8 before the process starts (INTEGRATION.md, \"environment\")\n", q ? "below 8" : "not set (HIP uses 4)");
}

// MSDFHIP_PIPELINE_TRACE: timed events per chunk (kernels enqueued / finished, copy finished) relative to the first enqueue; tools/pipeline_timeline.py reads the line
struct PipeTrace {
    struct Events { Event start, kernels, copied; long long hostEnqueued; };   // (they go with the trace, on every exit of the call)
    std::vector<Events> chunks;
    const bool on;
    const long long t0;
    PipeTrace() : on(tuning().pipelineTrace), t0(nowNsEarly()) { }
    void chunkStarts(hipStream_t stream) {
        if (!on)
            return;
        chunks.emplace_back();
        Events &te = chunks.back();
        te.start.create(hipEventDefault), te.kernels.create(hipEventDefault), te.copied.create(hipEventDefault);
        te.hostEnqueued = nowNsEarly()-t0;
        hipEventRecord(te.start, stream);
    }
    void kernelsQueued(hipStream_t stream) {
        if (on)
            hipEventRecord(chunks.back().kernels, stream);
    }
    void copyQueued(hipStream_t stream) {
        if (on)
            hipEventRecord(chunks.back().copied, stream);
    }
    void print(bool floatOutput, int nG, const std::vector<int> &lengths) {   // (every stream of the pipe has been synchronised)
        if (!on || chunks.empty())
            return;
        fprintf(stderr, "{\"pipeline_trace\": \"%s\", \"glyphs\": %d, \"host_total_ms\": %.3f, \"chunks\": [", floatOutput ? "float" : "uint8", nG, (nowNsEarly()-t0)/1e6);
        for (size_t i = 0; i < chunks.size(); ++i) {
            float a = 0, k = 0, c = 0;
            hipEventElapsedTime(&a, chunks[0].start, chunks[i].start);
            hipEventElapsedTime(&k, chunks[0].start, chunks[i].kernels);
            hipEventElapsedTime(&c, chunks[0].start, chunks[i].copied);
            fprintf(stderr, "%s{\"glyphs\": %d, \"host_enqueue_ms\": %.3f, \"stream_start_ms\": %.3f, \"kernels_done_ms\": %.3f, \"copy_done_ms\": %.3f}", i ? ", " : "",
                    lengths[i], chunks[i].hostEnqueued/1e6, a, k, c);
        }
        fprintf(stderr, "]}\n");
    }
};

// What the chunks of one host-output call share.
struct PipeCall {
    int mode, w, h, N;
    const MsdfHipGlyph *glyphs;
    const MsdfHipConfig *cfg;
    float *out;                       // float tiles into the caller's bitmaps, or
    uint8_t *atlas;                   // bytes into the caller's atlas
    uint8_t *stencil;                 // NULL: not wanted (or no correction pass runs)
    char *dstBytes;                   // `out` or `atlas`
    size_t texels, tile, elem;        // texels / values per tile (also bytes per 8-bit tile); bytes per value of the caller's buffer
    int chunk, depth;                 // glyphs a slot holds; chunks whose kernels may run at a time
    SlotLayout at;                    // of every slot's device buffer
    bool mirrorOverflow;
};

// The chunk's descriptors on the slot's stream: the generators' (the caller's layout relative to the chunk's range, or packed tiles) and, for 8-bit output,
// the conversion's behind them.
static int queueChunkDescriptors(const PipeCall &pc, PipeSlot &p, int g0, int n, MsdfHipGlyph *dGlyphs, ChunkSpan &span) {
    const int w = pc.w, h = pc.h, N = pc.N;
    hipStream_t compute = p.stream;
    int rc;
    // dense (chunkSpan): the chunk goes back as ONE copy. Otherwise the chunk is rendered as packed tiles, copied into pinned staging and scattered
    // row by row on the host (pendingCount).
    span = chunkSpan(pc.glyphs+g0, n, w, h, N);
    const bool floatsInCallerLayout = pc.out != NULL && span.dense;
    for (int g = 0; g < n; ++g) {                                // descriptors of the generators: the caller's layout (relative to the range) or packed tiles
        p.pinnedGlyphs.ptr[g] = pc.glyphs[g0+g];
        if (floatsInCallerLayout)
            p.pinnedGlyphs.ptr[g].out_offset -= span.spanLo;
        else
            p.pinnedGlyphs.ptr[g].out_offset = (int64_t) ((size_t) g*pc.tile), p.pinnedGlyphs.ptr[g].row_stride = w*N;
    }
    rc = uploadSmall(dGlyphs, p.pinnedGlyphs.ptr, sizeof(MsdfHipGlyph)*(size_t) n, compute);
    if (rc != MSDFHIP_OK)
        return rc;
    if (pc.atlas) {                                              // descriptors of the conversion: it reads the packed float tiles and blits into the byte layout
        MsdfHipGlyph *hBlit = p.pinnedGlyphs.ptr+p.pinnedGlyphs.cap/2;
        for (int g = 0; g < n; ++g) {
            hBlit[g] = pc.glyphs[g0+g];
            if (span.dense)
                hBlit[g].out_offset -= span.spanLo;
            else
                hBlit[g].out_offset = (int64_t) ((size_t) g*pc.tile), hBlit[g].row_stride = w*N;
        }
        rc = uploadSmall(dGlyphs+pc.chunk, hBlit, sizeof(MsdfHipGlyph)*(size_t) n, compute);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    return MSDFHIP_OK;
}

// A chunk's inputs: everything here -- the chunk's shapes (streamed calls: upload + digest), its descriptors and the two preparations of prepareAhead --
// does not depend on the chunks before it: it is queued AHEAD of the chunk's turn on the device and runs under the earlier chunks' kernels.
static int queueChunkInputs(const PipeCall &pc, ChunkFeeder *feeder, PipeSlot &p, int slot, size_t ci, int g0, int n, ChunkSpan &span, GenerateCall &call) {
    const int w = pc.w, h = pc.h;
    hipStream_t compute = p.stream;
    MsdfHipGlyph *dGlyphs = reinterpret_cast<MsdfHipGlyph *>(p.dev.ptr+pc.at.offGlyphs);
    int rc;
    const bool framed = feeder->frames();                        // the feeder's k_frame writes xf into the descriptors: they go up first (same stream: in order)
    p.frameGlyphs = framed ? dGlyphs : NULL;
    if (framed) {
        rc = queueChunkDescriptors(pc, p, g0, n, dGlyphs, span);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    rc = feeder->prepare(p, slot, ci, g0, n, compute);           // a view of the resident batch, or: flattened shapes -> upload -> digest on the chunk's stream
    if (rc != MSDFHIP_OK)
        return rc;
    if (!framed) {
        rc = queueChunkDescriptors(pc, p, g0, n, dGlyphs, span);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    call.afterDistance = p.distanceDone;
    call.overflowOut = pc.mirrorOverflow ? p.pinnedOverflow.ptr : NULL;
    return prepareAhead(&p.view, pc.mode, w, h, dGlyphs, pc.cfg, compute, call);
}

// The chunk's turn: its kernels once the chunk `depth` back has finished its own, then its way back to the caller -- one copy where its rectangles
// tile a range of the caller's buffer, else pinned staging (scattered when the slot is taken next) -- on the slot's stream.
static int queueChunkWork(const PipeCall &pc, PipeSlot *pipe, int slot, size_t ci, int g0, int n, const ChunkSpan &span, GenerateCall &call, PipeTrace &trace) {
    const int w = pc.w, h = pc.h, N = pc.N;
    PipeSlot &p = pipe[slot];
    hipStream_t compute = p.stream;
    MsdfHipGlyph *dGlyphs = reinterpret_cast<MsdfHipGlyph *>(p.dev.ptr+pc.at.offGlyphs);
    float *dTiles = reinterpret_cast<float *>(p.dev.ptr+pc.at.offTiles);
    uint8_t *dStencil = pc.stencil ? reinterpret_cast<uint8_t *>(p.dev.ptr+pc.at.offStencil) : NULL;
    uint8_t *dBytes = reinterpret_cast<uint8_t *>(p.dev.ptr+pc.at.offBytes);
    if (ci >= (size_t) pc.depth)                                 // at most `depth` (two) chunks' kernels at a time, in order: chunk k starts when chunk k-depth's KERNELS are done
        HIPCHK(hipStreamWaitEvent(compute, pipe[(slot+PIPE_SLOTS-pc.depth)%PIPE_SLOTS].kernelsDone, 0));
    p.pinnedOverflow.ptr[0] = 0;                                     // (the slot's previous chunk is done: nothing on the device writes it any more)
    int rc = runGenerate(&p.view, pc.mode, w, h, dGlyphs, dTiles, dStencil, NULL, pc.cfg, compute, call);
    if (rc != MSDFHIP_OK)
        return rc;
    const char *dResult = reinterpret_cast<const char *>(dTiles);
    if (pc.atlas) {
        rc = msdfhip_tiles_to_bytes(dTiles, n, w, h, N, dGlyphs+pc.chunk, dBytes, compute);
        if (rc != MSDFHIP_OK)
            return rc;
        dResult = reinterpret_cast<const char *>(dBytes);
    }
    trace.kernelsQueued(compute);
    HIPCHK(hipEventRecord(p.kernelsDone, compute));
    if (span.dense)
        HIPCHK(hipMemcpyAsync(pc.dstBytes+(size_t) span.spanLo*pc.elem, dResult, (size_t) n*pc.tile*pc.elem, hipMemcpyDeviceToHost, p.stream));
    else {
        HIPCHK(p.pinnedTiles.ensure((size_t) pc.chunk*pc.tile*pc.elem));
        HIPCHK(hipMemcpyAsync(p.pinnedTiles.ptr, dResult, (size_t) n*pc.tile*pc.elem, hipMemcpyDeviceToHost, p.stream));
        p.pendingFirst = g0, p.pendingCount = n;
    }
    if (pc.stencil)
        HIPCHK(hipMemcpyAsync(pc.stencil+(size_t) g0*pc.texels, dStencil, (size_t) n*pc.texels, hipMemcpyDeviceToHost, p.stream));
    HIPCHK(hipEventRecord(p.done, p.stream));
    trace.copyQueued(p.stream);
    p.busy = true;
    return MSDFHIP_OK;
}

// mirrorOverflow: the chunks' correction passes do not launch the per-texel overflow pass (k_ec_slow: a launch at the END of every chunk's chain that almost
// never has anything to do, but waits 0.07-0.24 ms for wavefront slots between the other chunks' kernels, rocprofv3 timeline of the pipeline); k_ec_query
// mirrors the chunk's candidate-overflow count into the slot's pinned word instead, the host looks at it when the chunk's copy is done, and *overflowed says
// whether any chunk of the call had one -- the caller then runs the call once more WITH the overflow pass (pathological inputs only; same results either way).
static int runPipelineOnce(const MsdfHipBatch *b, ChunkFeeder *feeder, int device, int nGlyphs, int mode, int w, int h, const MsdfHipGlyph *glyphs, float *out, size_t outFloats,
                           uint8_t *atlas, size_t atlasBytes, uint8_t *stencil, const MsdfHipConfig *cfg, bool mirrorOverflow, bool *overflowed) {
    *overflowed = false;
    if ((!b && !feeder) || !glyphs || (!out && !atlas) || mode < 1 || mode > 4 || w < 0 || h < 0)
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to the host-output generator");
    int rc = checkConfig(cfg);
    if (rc != MSDFHIP_OK)
        return rc;
    rc = ensureDevice(b ? b->device : device);
    if (rc != MSDFHIP_OK)
        return rc;
    const int nG = b ? b->nGlyphs : nGlyphs, N = channelsOf(mode);
    if (nG == 0 || w == 0 || h == 0)
        return MSDFHIP_OK;
    DevicePool<Pipe>::Lease lease;
    const hipError_t taken = gPipePool.take(currentDevice(), lease);
    if (taken != hipSuccess)
        return fail(MSDFHIP_ERR_HIP, "host-output pipeline: creating a stream / event failed: %s", hipGetErrorString(taken));
    if (b)
        rc = fetchGlyphCounts(b);
    if (rc != MSDFHIP_OK)
        return rc;
    ResidentFeeder resident(b);
    if (!feeder)
        feeder = &resident;
    struct FeederDrain {                                         // declared after the lease: runs BEFORE the pipe goes back to the pool, on every exit (HIPCHK returns included)
        ChunkFeeder *f;
        ~FeederDrain() { f->drain(); }
    } drainGuard = { feeder };
    PipeSlot *pipe = lease->slot;
    PipeCall pc;
    pc.mode = mode, pc.w = w, pc.h = h, pc.N = N, pc.glyphs = glyphs, pc.cfg = cfg, pc.out = out, pc.atlas = atlas, pc.mirrorOverflow = mirrorOverflow;
    pc.texels = (size_t) w*h, pc.tile = pc.texels*N, pc.elem = out ? sizeof(float) : 1;
    pc.dstBytes = out ? reinterpret_cast<char *>(out) : reinterpret_cast<char *>(atlas);
    // every rectangle must lie inside the caller's buffer (how a chunk travels back is decided per chunk, chunkSpan: one contiguous copy when
    // its rectangles exactly tile a contiguous range, else pinned staging + a row scatter on the host; either way texels outside the
    // rectangles are never touched, and devices sharing one atlas cannot disturb each other)
    const size_t total = out ? outFloats : atlasBytes;
    for (int g = 0; g < nG; ++g) {
        const RectSpan r = rectSpan(glyphs[g], w, h, N);
        if (r.lo < 0 || (unsigned long long) r.hi > total)
            return fail(MSDFHIP_ERR_INVALID, "glyph %d's rectangle [%lld, %lld) lies outside the output buffer of %zu elements", g, r.lo, r.hi, total);
    }
    const int set = gPipeChunkGlyphs.load(), wanted = set > 0 ? set : defaultChunk(pc.tile);
    const int chunk = pc.chunk = wanted > nG ? nG : wanted;
    const bool correct = mode >= 3 && cfg->ec_mode != MSDFHIP_EC_DISABLED;
    pc.stencil = correct ? stencil : NULL;                       // the reference leaves the caller's buffer alone when no correction runs
    pc.at = slotLayout(chunk, pc.tile, pc.texels, pc.stencil != NULL, atlas != NULL);
    for (int k = 0; k < PIPE_SLOTS; ++k) {                       // every slot holds a full chunk (grown once, kept with the pooled pipe)
        PipeSlot &p = pipe[k];
        if (p.dev.cap < pc.at.devBytes) {
            HIPCHK(hipStreamSynchronize(p.stream));
            HIPCHK(p.dev.ensure(pc.at.devBytes));
        }
        HIPCHK(p.pinnedGlyphs.ensure(2*(size_t) chunk));
        if (p.view.work.reservedGlyphs < (size_t) chunk) {       // per-glyph work buffers of the view: reallocated on demand by the launches
            HIPCHK(hipStreamSynchronize(p.stream));
            p.view.work.reserveGlyphs((size_t) chunk);
        }
        p.pendingCount = 0;
    }
    const std::vector<int> lengths = chunkSchedule(nG, chunk, out != NULL);
    if (lengths.size() > 1)
        hintHwQueuesOnce();
    PipeTrace trace;
    // Schedule: chunk k runs -- kernels, then its copy back -- on the stream of slot k % PIPE_SLOTS, so the copy of one chunk overlaps the
    // kernels of the next ones, and the kernels of two consecutive chunks overlap each other (a 2 048-glyph step alone leaves the device
    // half empty in its tails: serialising the chunks' kernels on one stream was measured, 17 instead of 12 ms). THREE slots: with two, the
    // device idled 0.8 ms per chunk while a copy held the slot the next chunk needed (MSDFHIP_PIPELINE_TRACE, profiles/r03_ab_notes.md).
    pc.depth = tuning().pipelineDepth;
    rc = feeder->begin(pipe, lengths);
    if (rc != MSDFHIP_OK)
        return rc;
    int slot = 0, g0 = 0;
    for (size_t ci = 0; ci < lengths.size() && rc == MSDFHIP_OK; g0 += lengths[ci], ++ci, slot = (slot+1)%PIPE_SLOTS) {
        PipeSlot &p = pipe[slot];
        if (p.busy) {                                            // the slot's previous copy must have left its buffers
            HIPCHK(hipEventSynchronize(p.done));
            p.busy = false;
            if (mirrorOverflow && p.pinnedOverflow.ptr[0] != 0)
                *overflowed = true;
            if (p.pendingCount)
                scatterPending(p, glyphs, pc.dstBytes, pc.elem, w, h, N);
            p.pendingCount = 0;
        }
        trace.chunkStarts(p.stream);
        ChunkSpan span;
        GenerateCall call;
        rc = queueChunkInputs(pc, feeder, p, slot, ci, g0, lengths[ci], span, call);
        if (rc == MSDFHIP_OK)
            rc = queueChunkWork(pc, pipe, slot, ci, g0, lengths[ci], span, call, trace);
    }
    for (int k = 0; k < PIPE_SLOTS; ++k) {
        PipeSlot &p = pipe[k];
        hipError_t e = hipStreamSynchronize(p.stream);
        p.busy = false;
        if (e != hipSuccess && rc == MSDFHIP_OK)
            rc = fail(MSDFHIP_ERR_HIP, "host-output pipeline: %s", hipGetErrorString(e));
        if (mirrorOverflow && e == hipSuccess && p.pinnedOverflow.ptr[0] != 0)
            *overflowed = true;
        if (rc == MSDFHIP_OK && p.pendingCount)
            scatterPending(p, glyphs, pc.dstBytes, pc.elem, w, h, N);
        p.pendingCount = 0;
    }
    trace.print(out != NULL, nG, lengths);
    return rc;
}

static std::atomic<unsigned long long> gPipelineOverflowReruns(0);

static int runPipeline(const MsdfHipBatch *b, ChunkFeeder *feeder, int device, int nGlyphs, int mode, int w, int h, const MsdfHipGlyph *glyphs, float *out, size_t outFloats,
                       uint8_t *atlas, size_t atlasBytes, uint8_t *stencil, const MsdfHipConfig *cfg) {
    bool overflowed = false;
    int rc = runPipelineOnce(b, feeder, device, nGlyphs, mode, w, h, glyphs, out, outFloats, atlas, atlasBytes, stencil, cfg, true, &overflowed);
    if (rc == MSDFHIP_OK && overflowed) {                        // some glyph's candidate segment overflowed: the whole call again, every chunk with the overflow pass
        ++gPipelineOverflowReruns;
        rc = runPipelineOnce(b, feeder, device, nGlyphs, mode, w, h, glyphs, out, outFloats, atlas, atlasBytes, stencil, cfg, false, &overflowed);
    }
    return rc;
}

unsigned long long msdfhip_pipeline_overflow_reruns(int reset) {
    return reset ? gPipelineOverflowReruns.exchange(0) : gPipelineOverflowReruns.load();
}

int msdfhip_batch_generate_host(const MsdfHipBatch *b, int mode, int w, int h, const MsdfHipGlyph *glyphs, float *out, size_t outFloats,
                                uint8_t *stencil, const MsdfHipConfig *cfg) {
    if (!out)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    if (!b)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    return runPipeline(b, NULL, -1, 0, mode, w, h, glyphs, out, outFloats, NULL, 0, stencil, cfg);
}

int msdfhip_batch_generate_bytes_host(const MsdfHipBatch *b, int mode, int w, int h, const MsdfHipGlyph *glyphs, uint8_t *atlas, size_t atlasBytes,
                                      const MsdfHipConfig *cfg) {
    if (!atlas)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    if (!b)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    return runPipeline(b, NULL, -1, 0, mode, w, h, glyphs, NULL, 0, atlas, atlasBytes, NULL, cfg);
}

// ---- streamed generation: shapes in, host bitmaps out, everything in between overlapped (SURVEY.md 8d's end-to-end metric) ----------------------
//
// msdfhip_batch_create + msdfhip_batch_generate_host run one after the other: flatten all shapes (the caller), upload + digest all, then the chunk
// pipeline. Here the glyph list is cut into the pipeline's chunks FIRST and every stage works chunk-wise: the host threads flatten chunk k+1 / k+2 from the
// caller's shape objects straight into pinned staging while chunk k's upload, digest and kernels run and chunk k-1's tiles are copied back.
// prep != NULL (msdfhip_generate_stream_prepared): the source delivers RAW outlines, each chunk is prepared on the device on its own stream.
static int generateStream(const char *who, int device, int mode, int w, int h, int n_glyphs, const MsdfHipShapeSource *source, const MsdfHipGlyph *glyphs,
                          float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes, uint8_t *stencil, const MsdfHipConfig *cfg,
                          const MsdfHipPrepConfig *prep, const uint64_t *seeds, const MsdfHipOrientConfig *orient = NULL, const FrameParams *frame = NULL) {
    if (!source || !source->count || !source->fill || n_glyphs < 0 || (!out) == (!atlas) || (n_glyphs > 0 && !glyphs))
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to %s (a shape source with count and fill, exactly one of out / atlas)", who);
    if (atlas && stencil)
        return fail(MSDFHIP_ERR_INVALID, "%s: a stencil buffer only goes with float output", who);
    if (n_glyphs == 0)
        return MSDFHIP_OK;
    if (device >= 0) {
        int count = 0;
        int rc = msdfhip_device_count(&count);
        if (rc != MSDFHIP_OK)
            return rc;
        if (device >= count)
            return fail(MSDFHIP_ERR_INVALID, "device %d out of range (0..%d)", device, count-1);
    }
    int rc = ensureDevice(device);
    if (rc != MSDFHIP_OK)
        return rc;
    StreamFeeder feeder(source, n_glyphs, prep, seeds, orient, frame, w, h);
    rc = feeder.count();
    if (rc != MSDFHIP_OK)
        return rc;
    return runPipeline(NULL, &feeder, currentDevice(), n_glyphs, mode, w, h, glyphs, out, out_floats, atlas, atlas_bytes, stencil, cfg);
}

int msdfhip_generate_stream(int device, int mode, int w, int h, int n_glyphs, const MsdfHipShapeSource *source, const MsdfHipGlyph *glyphs, float *out,
                            size_t out_floats, uint8_t *atlas, size_t atlas_bytes, uint8_t *stencil, const MsdfHipConfig *cfg) {
    return generateStream("msdfhip_generate_stream", device, mode, w, h, n_glyphs, source, glyphs, out, out_floats, atlas, atlas_bytes, stencil, cfg, NULL, NULL);
}

// Raw outlines in: the chunk pipeline above with the device's shape preparation (msdfhip_batch_create_prepared's sequence) between each chunk's upload and
// its digest, on the chunk's stream.
int msdfhip_generate_stream_prepared(int device, int mode, int w, int h, int n_glyphs, const MsdfHipShapeSource *source, const MsdfHipGlyph *glyphs, float *out,
                                     size_t out_floats, uint8_t *atlas, size_t atlas_bytes, uint8_t *stencil, const MsdfHipConfig *cfg,
                                     const MsdfHipPrepConfig *prep, const uint64_t *seeds) {
    return msdfhip_generate_stream_prepared_oriented(device, mode, w, h, n_glyphs, source, glyphs, out, out_floats, atlas, atlas_bytes, stencil, cfg, prep, seeds, NULL);
}

// + orientation around the preparation (orient NULL: keep); checked before the source is read.
int msdfhip_generate_stream_prepared_oriented(int device, int mode, int w, int h, int n_glyphs, const MsdfHipShapeSource *source, const MsdfHipGlyph *glyphs,
                                              float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes, uint8_t *stencil, const MsdfHipConfig *cfg,
                                              const MsdfHipPrepConfig *prep, const uint64_t *seeds, const MsdfHipOrientConfig *orient) {
    return msdfhip_generate_stream_prepared_oriented_framed(device, mode, w, h, n_glyphs, source, glyphs, out, out_floats, atlas, atlas_bytes, stencil, cfg, prep, seeds,
                                                            orient, NULL);
}

// + framing on the device (frame NULL: the caller's xf); every config is checked before the source is read.
int msdfhip_generate_stream_prepared_oriented_framed(int device, int mode, int w, int h, int n_glyphs, const MsdfHipShapeSource *source, const MsdfHipGlyph *glyphs,
                                                     float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes, uint8_t *stencil, const MsdfHipConfig *cfg,
                                                     const MsdfHipPrepConfig *prep, const uint64_t *seeds, const MsdfHipOrientConfig *orient,
                                                     const MsdfHipFrameConfig *frame) {
    int rc = checkPrepConfig(prep, "msdfhip_generate_stream_prepared");
    if (rc != MSDFHIP_OK)
        return rc;
    MsdfHipOrientConfig o;
    rc = checkOrientConfig(orient, "msdfhip_generate_stream_prepared_oriented", &o);
    if (rc != MSDFHIP_OK)
        return rc;
    FrameParams f;
    bool framed = false;
    rc = checkFrameConfig(frame, w, h, "msdfhip_generate_stream_prepared_oriented_framed", &f, &framed);
    if (rc != MSDFHIP_OK)
        return rc;
    return generateStream("msdfhip_generate_stream_prepared", device, mode, w, h, n_glyphs, source, glyphs, out, out_floats, atlas, atlas_bytes, stencil, cfg, prep, seeds,
                          &o, framed ? &f : NULL);
}

namespace {
struct CsrSource {                                               // a shape source over HOST CSR arrays (what msdfhip_batch_create takes)
    const int32_t *gco, *co;
    const double *points;
    const uint8_t *types, *colors;
    static void count(void *user, int g, int32_t *nC, int32_t *nE) {
        const CsrSource &s = *static_cast<const CsrSource *>(user);
        *nC = s.gco[g+1]-s.gco[g], *nE = s.co[s.gco[g+1]]-s.co[s.gco[g]];
    }
    static void fill(void *user, int g, int32_t edgeBase, int32_t *contourEnd, double *points, uint8_t *types, uint8_t *colors) {
        const CsrSource &s = *static_cast<const CsrSource *>(user);
        const int c0 = s.gco[g], c1 = s.gco[g+1], e0 = s.co[c0], nE = s.co[c1]-e0;
        for (int c = c0; c < c1; ++c)
            contourEnd[c-c0] = edgeBase+(s.co[c+1]-e0);
        memcpy(points, s.points+(size_t) e0*8, (size_t) nE*8*sizeof(double));
        memcpy(types, s.types+e0, (size_t) nE);
        if (s.colors)
            memcpy(colors, s.colors+e0, (size_t) nE);
        else
            memset(colors, 7, (size_t) nE);                      // (raw outlines without colours: WHITE)
    }
};
}

int msdfhip_generate_stream_csr(int device, int mode, int w, int h, int n_glyphs, const int32_t *gco, const int32_t *co, const double *points, const uint8_t *types,
                                const uint8_t *colors, const MsdfHipGlyph *glyphs, float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes, uint8_t *stencil,
                                const MsdfHipConfig *cfg) {
    std::vector<int> hc, he;
    int maxC = 0, maxE = 0;
    int rc = checkShapeArrays(n_glyphs, gco, co, points, types, colors, true, hc, he, maxC, maxE);
    if (rc != MSDFHIP_OK)
        return rc;
    CsrSource csr = { gco, co, points, types, colors };
    MsdfHipShapeSource source = { &csr, CsrSource::count, CsrSource::fill };
    return msdfhip_generate_stream(device, mode, w, h, n_glyphs, &source, glyphs, out, out_floats, atlas, atlas_bytes, stencil, cfg);
}

int msdfhip_generate_stream_csr_prepared(int device, int mode, int w, int h, int n_glyphs, const int32_t *gco, const int32_t *co, const double *points,
                                         const uint8_t *types, const uint8_t *colors, const MsdfHipGlyph *glyphs, float *out, size_t out_floats, uint8_t *atlas,
                                         size_t atlas_bytes, uint8_t *stencil, const MsdfHipConfig *cfg, const MsdfHipPrepConfig *prep, const uint64_t *seeds) {
    return msdfhip_generate_stream_csr_prepared_oriented(device, mode, w, h, n_glyphs, gco, co, points, types, colors, glyphs, out, out_floats, atlas, atlas_bytes,
                                                         stencil, cfg, prep, seeds, NULL);
}

int msdfhip_generate_stream_csr_prepared_oriented(int device, int mode, int w, int h, int n_glyphs, const int32_t *gco, const int32_t *co, const double *points,
                                                  const uint8_t *types, const uint8_t *colors, const MsdfHipGlyph *glyphs, float *out, size_t out_floats,
                                                  uint8_t *atlas, size_t atlas_bytes, uint8_t *stencil, const MsdfHipConfig *cfg, const MsdfHipPrepConfig *prep,
                                                  const uint64_t *seeds, const MsdfHipOrientConfig *orient) {
    return msdfhip_generate_stream_csr_prepared_oriented_framed(device, mode, w, h, n_glyphs, gco, co, points, types, colors, glyphs, out, out_floats, atlas,
                                                                atlas_bytes, stencil, cfg, prep, seeds, orient, NULL);
}

int msdfhip_generate_stream_csr_prepared_oriented_framed(int device, int mode, int w, int h, int n_glyphs, const int32_t *gco, const int32_t *co,
                                                         const double *points, const uint8_t *types, const uint8_t *colors, const MsdfHipGlyph *glyphs, float *out,
                                                         size_t out_floats, uint8_t *atlas, size_t atlas_bytes, uint8_t *stencil, const MsdfHipConfig *cfg,
                                                         const MsdfHipPrepConfig *prep, const uint64_t *seeds, const MsdfHipOrientConfig *orient,
                                                         const MsdfHipFrameConfig *frame) {
    int rc = checkPrepConfig(prep, "msdfhip_generate_stream_csr_prepared");
    if (rc != MSDFHIP_OK)
        return rc;
    MsdfHipOrientConfig o;
    rc = checkOrientConfig(orient, "msdfhip_generate_stream_csr_prepared_oriented", &o);
    if (rc != MSDFHIP_OK)
        return rc;
    FrameParams f;
    bool framed = false;
    rc = checkFrameConfig(frame, w, h, "msdfhip_generate_stream_csr_prepared_oriented_framed", &f, &framed);
    if (rc != MSDFHIP_OK)
        return rc;
    std::vector<int> hc, he;
    int maxC = 0, maxE = 0;
    rc = checkShapeArrays(n_glyphs, gco, co, points, types, colors, false, hc, he, maxC, maxE);
    if (rc != MSDFHIP_OK)
        return rc;
    CsrSource csr = { gco, co, points, types, colors };
    MsdfHipShapeSource source = { &csr, CsrSource::count, CsrSource::fill };
    return generateStream("msdfhip_generate_stream_csr_prepared", device, mode, w, h, n_glyphs, &source, glyphs, out, out_floats, atlas, atlas_bytes, stencil, cfg,
                          prep, seeds, &o, framed ? &f : NULL);
}

int msdfhip_set_host_threads(int threads) {
    if (threads < 0)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_set_host_threads(%d)", threads);
    std::lock_guard<std::mutex> lock(gHostPoolMutex);
    if (gHostPool)                                               // (the pool is created once, on first use)
        return gHostPool->threads()+1;
    gHostThreads.store(threads);
    return 0;
}

int msdfhip_hw_queues_env(void) { return hwQueuesEnv(); }

int msdfhip_set_pipeline_chunk(int glyphs_per_chunk) {
    if (glyphs_per_chunk < 0)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_set_pipeline_chunk(%d)", glyphs_per_chunk);
    gPipeChunkGlyphs.store(glyphs_per_chunk);
    return MSDFHIP_OK;
}

int msdfhip_host_alloc(void **p, size_t bytes) {
    if (!p)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    int rc = ensureDevice();
    if (rc != MSDFHIP_OK)
        return rc;
    // portable: usable by every device of the process (the sharded generator writes one buffer from several GPUs)
    if (pinnedAlloc(p, bytes, hipHostMallocPortable) != hipSuccess)
        return fail(MSDFHIP_ERR_NOMEM, "hipHostMalloc(%zu) failed", bytes);
    return MSDFHIP_OK;
}

int msdfhip_host_free(void *p) {
    if (p && pinnedFree(p) != hipSuccess)
        return fail(MSDFHIP_ERR_HIP, "hipHostFree failed");
    return MSDFHIP_OK;
}

// ------------------------------------------------------------------------------------------- glyph-sharded, multi-device
//
// glyphs are independent, so a glyph list is cut into contiguous ranges of equal modelled cost (shardRanges, msdf_hostplan.hpp), one range
// per device, one host thread + its own streams per device, no exchange between devices; every device copies its tiles straight into the caller's
// buffer. The bytes do not depend on the split.

int msdfhip_generate_sharded(const int *devices, int n_devices, int mode, int w, int h, int n_glyphs, const int32_t *gco, const int32_t *co,
                             const double *points, const uint8_t *types, const uint8_t *colors, const MsdfHipGlyph *glyphs,
                             float *out, size_t outFloats, uint8_t *atlas, size_t atlasBytes, const MsdfHipConfig *cfg) {
    if (!devices || n_devices < 1 || !glyphs || (!out) == (!atlas))
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_generate_sharded (exactly one of out / atlas)");
    std::vector<int> hc, he;
    int maxC = 0, maxE = 0;
    int rc = checkShapeArrays(n_glyphs, gco, co, points, types, colors, true, hc, he, maxC, maxE);
    if (rc != MSDFHIP_OK)
        return rc;
    int count = 0;
    rc = msdfhip_device_count(&count);
    if (rc != MSDFHIP_OK)
        return rc;
    for (int k = 0; k < n_devices; ++k)
        if (devices[k] < 0 || devices[k] >= count)
            return fail(MSDFHIP_ERR_INVALID, "device %d out of range (0..%d)", devices[k], count-1);
    if (gDevice.load() < 0) {
        rc = msdfhip_init(devices[0]);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    std::vector<int> bounds;
    shardRanges(gco, co, n_glyphs, n_devices, bounds);
    std::vector<int> rcs((size_t) n_devices, MSDFHIP_OK);
    std::vector<std::string> errors((size_t) n_devices);
    std::vector<std::thread> workers;
    for (int k = 0; k < n_devices; ++k)
        workers.push_back(std::thread([&, k]() {
            const int g0 = bounds[k], g1 = bounds[k+1];
            if (g1 <= g0)
                return;
            // the range's own CSR arrays: offsets rebased, edge arrays are slices of the caller's
            const int c0 = gco[g0], c1 = gco[g1], e0 = co[c0];
            std::vector<int32_t> lgco((size_t) (g1-g0)+1), lco((size_t) (c1-c0)+1);
            for (int g = g0; g <= g1; ++g)
                lgco[g-g0] = gco[g]-c0;
            for (int c = c0; c <= c1; ++c)
                lco[c-c0] = co[c]-e0;
            MsdfHipBatch *b = NULL;
            int r = msdfhip_batch_create_on(&b, devices[k], g1-g0, lgco.data(), lco.data(), points+(size_t) e0*8, types+e0, colors+e0);
            if (r == MSDFHIP_OK) {
                r = out ? runPipeline(b, NULL, -1, 0, mode, w, h, glyphs+g0, out, outFloats, NULL, 0, NULL, cfg)
                        : runPipeline(b, NULL, -1, 0, mode, w, h, glyphs+g0, NULL, 0, atlas, atlasBytes, NULL, cfg);
                msdfhip_batch_destroy(b);
            }
            rcs[k] = r;
            if (r != MSDFHIP_OK)
                errors[k] = tlsError;
        }));
    for (size_t k = 0; k < workers.size(); ++k)
        workers[k].join();
    for (int k = 0; k < n_devices; ++k)
        if (rcs[k] != MSDFHIP_OK) {
            tlsError = errors[k];
            return rcs[k];
        }
    return MSDFHIP_OK;
}

// ------------------------------------------------------------------------------------------- single-shape host calls

// Resources of one host-pointer call in flight: a stream, a device arena, a pinned staging buffer. They grow on demand and are
// reused, so a steady stream of generate*() calls (the way msdf-atlas-gen's workers call the reference) performs no allocation:
// stage -> async H2D -> kernels -> async D2H -> one stream sync. Arenas live in a process-wide pool per device: a call takes one and
// returns it, so short-lived worker threads (msdf-atlas-gen spawns a fresh team per Workload::finish()) reuse them instead of
// leaking one per thread; the pool is bounded by the peak number of concurrent calls.
struct ThreadArena {
    int device = 0;
    Stream stream;
    WorkBuffer<char> dev;
    WorkBuffer<char, true> pinned;
    WorkBuffer<unsigned> barrier;     // counters of k_single_call ([0] grid barrier, [16] finished workgroups): zeroed once, only ever counted up --
    unsigned barrierEpoch = 0, doneCount = 0, doneEpoch = 0;   // their values between calls, and the completion-flag value of the last call
    char *pinnedDev = NULL;           // the device's address of `pinned` (hipHostGetDevicePointer): k_single_call reads its inputs / writes its tile there

    hipError_t create(int d) {
        device = d;
        hipError_t e = stream.create(hipStreamNonBlocking);
        if (e == hipSuccess)
            e = barrier.ensure(64);
        // (zeroed ON THE ARENA'S STREAM: hipMemset runs on the legacy default stream, which a non-blocking stream does not wait for -- the first
        // k_single_call of a fresh arena could start before it and have its counters zeroed under it; found by the TSan run of tests/sanitize)
        return e == hipSuccess ? hipMemsetAsync(barrier.ptr, 0, 256, stream) : e;
    }
    void quiesce() {
        if (stream)
            (void) hipStreamSynchronize(stream);
    }
};

static DevicePool<ThreadArena> gArenaPool;
typedef DevicePool<ThreadArena>::Lease ArenaHold;               // (quiescent: the call saw its own completion -- stream sync or k_single_call's flag)

static int takeArena(ArenaHold &lease) {
    const hipError_t e = gArenaPool.take(currentDevice(), lease);
    return e == hipSuccess ? MSDFHIP_OK : fail(MSDFHIP_ERR_HIP, "single-shape call: creating its stream / barrier failed: %s", hipGetErrorString(e));
}

static int arenaReserve(ThreadArena &a, size_t devBytes, size_t pinnedBytes) {
    if (a.dev.cap < devBytes)
        HIPCHK(a.dev.ensure(devBytes+devBytes/2+4096));
    if (a.pinned.cap < pinnedBytes) {
        a.pinnedDev = NULL;
        HIPCHK(a.pinned.ensure(pinnedBytes+pinnedBytes/2+4096));
        if (hipHostGetDevicePointer((void **) &a.pinnedDev, a.pinned.ptr, 0) != hipSuccess) {   // not mapped: k_single_call then works on device copies
            (void) hipGetLastError();
            a.pinnedDev = NULL;
        }
    }
    return MSDFHIP_OK;
}

// (SingleOp, what the single-shape call does to `pixels`: msdf_groupplan.hpp)

// One host-pointer call (generate* / msdfErrorCorrection / distanceSignCorrection / rasterize on one shape and one bitmap).
struct ShapeCall {
    int mode, channels, op, w, h, rowStride, flip, nC;
    float *pixels;
    const int32_t *co;
    const double *points;
    const uint8_t *types, *colors;
    double xf[6];
    MsdfHipConfig cfg;
    uint8_t *stencil;
    // micro-batcher state (guarded by gQueueMutex)
    bool claimed, done;
    int rc;
    std::string error;
    std::condition_variable cv;
};

// Calls can share one launch sequence when everything that is a launch parameter agrees; the sizes of their bitmaps may differ where the operation has
// sized kernels (groupCompatible, msdf_groupplan.hpp: the rule is written there).
static GroupKey keyOf(const ShapeCall &c) {
    const GroupKey k = { c.mode, c.channels, c.op, c.w, c.h, &c.cfg, sizeof(MsdfHipConfig) };
    return k;
}
static bool sameLaunch(const ShapeCall &a, const ShapeCall &b) {
    return groupCompatible(keyOf(a), keyOf(b));
}

static std::atomic<long long> gNsStage(0), gNsDevice(0), gNsScatter(0);
static std::atomic<unsigned long long> gSingleTimeouts(0), gSingleLost(0), gSingleRefused(0);   // fused launches that gave up at their grid barrier / ended without their flag (both rerun through the batched sequence)
static std::atomic<unsigned long long> gSinglePhase[8], gSingleCalls(0), gSingleCycles(0);   // sums of k_single_call's phase stamps (msdfhip_debug_single_call_phases)
static long long nowNs() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Runs n compatible calls as ONE device batch on the calling thread's arena: stage all inputs -> one H2D copy -> digest + kernels ->
// one D2H copy -> scatter the tiles into the callers' bitmaps. n == 1 is the plain single-shape call.
// Leader slots = groups in flight at once. Two was right while a lone call was seven launches (more leaders only interleaved their launch chains);
// with one fused launch per lone call (k_single_call) four measured better at every thread count: 4 threads 21.5 -> 42.8 k glyphs/s, 16 threads
// 45 -> 49 k, 64 threads 96 -> 122 k (8 leaders: 43 / 53 / 103 k; 16: 27 / 62 / 75 k; profiles/r04_host_calls.jsonl).
enum { DEFAULT_LEADERS = 4 };
static std::atomic<int> gMaxGroup(-1), gMaxLeaders(DEFAULT_LEADERS);

// End of a latency-bound call: poll the stream for a bounded time before handing the thread to the blocking wait (whose wake-up alone
// costs 10-20 us, a sixth of a single-shape call).
static hipError_t waitStream(hipStream_t stream) {
    const long long deadline = nowNs()+400000;                   // 0.4 ms of polling at most
    for (;;) {
        const hipError_t e = hipStreamQuery(stream);
        if (e != hipErrorNotReady)
            return e;
        if (nowNs() > deadline)
            return hipStreamSynchronize(stream);
    }
}

// MSDFHIP_DEVICES = "all" | "0,1,...": the devices the front door (single-shape host-pointer calls, i.e. every unmodified caller of the C++
// shim) spreads its groups over, round robin -- an 8-GPU node serves msdf-atlas-gen's worker pool without a line changed in the caller
// (VERDICT r2 missing #3). Unset: the process default device only. A device may be listed more than once.
static std::mutex gFrontMutex;
static std::vector<int> gFrontDevices;
static bool gFrontParsed = false;
static std::atomic<unsigned> gFrontNext(0);

static int frontDoorDevice() {
    std::lock_guard<std::mutex> lock(gFrontMutex);
    if (!gFrontParsed) {
        gFrontParsed = true;
        gFrontDevices.clear();
        const char *spec = tuning().devices;
        int count = 0;
        if (spec[0] && hipGetDeviceCount(&count) == hipSuccess) {
            if (!strcmp(spec, "all"))
                for (int d = 0; d < count; ++d)
                    gFrontDevices.push_back(d);
            else
                for (const char *p = spec; *p; ) {
                    char *end = NULL;
                    const long d = strtol(p, &end, 10);
                    if (end == p)
                        break;
                    if (d >= 0 && d < count)
                        gFrontDevices.push_back((int) d);
                    p = *end == ',' ? end+1 : end;
                }
        }
        (void) hipGetLastError();
        if (gFrontDevices.size() > 1 && gMaxLeaders.load() == DEFAULT_LEADERS)   // as many groups in flight per device as on one device
            gMaxLeaders.store(DEFAULT_LEADERS*(int) gFrontDevices.size());
    }
    if (gFrontDevices.empty())
        return -1;
    return gFrontDevices[gFrontNext.fetch_add(1u)%gFrontDevices.size()];
}

// k_single_call's grid barrier needs all workgroups of a launch resident at the same time, and the launch is not cooperative. Two things make
// that hold: (1) the fused launches in flight on a device are counted against what the device can hold of this kernel at this LDS size
// (hipOccupancyMaxActiveBlocksPerMultiprocessor x compute units) -- a call that would not fit takes the batched sequence; (2) what this process cannot
// count (persistent k_distance launches of other threads, other processes) is covered by the bounded spin + rerun (msdf_single.hpp: gridBarrier).
static std::atomic<int> gFusedInFlight[64];                     // workgroups of fused launches in flight, per device
static int fusedCapacity(int device, int variant, size_t lds) {  // variant = mode*2 + overlap (2..9)
    enum { LDS_STEP = 4096, LDS_STEPS = 17 };
    static std::atomic<int> cache[10][LDS_STEPS];                // (one gfx950 is like another: not keyed by device)
    const size_t step = (lds+LDS_STEP-1)/LDS_STEP;
    if (variant < 2 || variant > 9 || step >= LDS_STEPS)
        return 0;
    const void *kernel = NULL;
    forSingleCallVariant(variant, [&](auto sel, auto overlap) { kernel = reinterpret_cast<const void *>(k_single_call<decltype(sel)::value, decltype(overlap)::value>); });
    return residentBlocks(cache[variant][step], device, kernel, WAVE*SINGLE_TEAM, step*LDS_STEP);
}
struct FusedReservation {                                        // the workgroups a fused launch holds of its device, released when the call is over
    std::atomic<int> *counter;
    int groups;
    FusedReservation() : counter(NULL), groups(0) { }
    ~FusedReservation() { release(); }
    bool take(int device, int variant, size_t lds, int want) {
        if (device < 0 || device >= 64)
            return false;
        const int capacity = fusedCapacity(device, variant, lds);
        std::atomic<int> &c = gFusedInFlight[device];
        if (c.fetch_add(want)+want > capacity) {
            c.fetch_sub(want);
            return false;
        }
        counter = &c, groups = want;
        return true;
    }
    void release() {
        if (counter)
            counter->fetch_sub(groups);
        counter = NULL;
    }
};

// Everything about a group of n compatible calls that is known before its arena is leased and never changes afterwards.
struct GroupPlan {
    int n, maxC, maxE, stages;        // calls; the largest contour / edge count of one; intermediate fields of a generate call (correction, sign correction)
    bool bitmapIsInput, correct, anyStencil;
    bool fusedShape;                  // ONE generate*() call on a bitmap of at most 256 tiles: k_single_call's private areas are reserved
    size_t sumC, sumE, eAlloc, cAlloc, texels, tileBytes, tilesAll, candCap;
    // pinned staging, mirrored at the start of the device arena. Inputs first: one H2D copy of inputBytes; hStatus onwards: one D2H copy (copyBackAndWait)
    size_t hGco, hCo, hPts, hTypes, hColors, hGlyph, hSrc, inputBytes, hBucket, hStatus, hOut, hStencil, resultBytes, pinnedBytes;
    // device-only work buffers behind the mirror
    size_t dRecs, dWind, dScratch, dCands, dParams, gresNeed, dGres, dPriv, devBytes;
    size_t pvWind, pvOff, pvGco, pvGlyph, pvStride;   // k_single_call: offsets inside one workgroup's private digest area, and the areas' stride (msdf_single.hpp)
    // A group of bitmaps of different sizes (msdf_groupplan.hpp): one sized call at w x h = the largest width x the largest height. texels / tileBytes are then
    // those of a SLOT, hSrc / hOut hold the boxes packed at `offsets`, hDims (in the input region: it travels with the one upload) the n*2 box sizes, and
    // dSlots is the device-only source region of the in-place operations, which k_boxes_to_slots fills from the packed upload.
    bool mixed;
    int w, h;
    size_t hDims, dSlots, outBytes;   // outBytes: the results without the stencils
    std::vector<int64_t> offsets;     // mixed: n+1 float offsets (groupPackedOffsets)
};

static GroupPlan planGroup(ShapeCall *const *calls, int n, const GroupSelection *sel = NULL) {
    const ShapeCall &c0 = *calls[0];
    const int channels = c0.channels, op = c0.op;
    const MsdfHipConfig *cfg = &c0.cfg;
    GroupPlan p;
    p.n = n;
    p.mixed = sel && !sel->uniform && n > 1;
    const int w = p.w = p.mixed ? sel->W : c0.w, h = p.h = p.mixed ? sel->H : c0.h;
    size_t packedBytes = 0;
    if (p.mixed) {
        std::vector<int32_t> sizes(2*(size_t) n);
        for (int g = 0; g < n; ++g)
            sizes[2*(size_t) g] = calls[g]->w, sizes[2*(size_t) g+1] = calls[g]->h;
        p.offsets.resize((size_t) n+1);
        groupPackedOffsets(n, sizes.data(), channels, p.offsets.data());
        packedBytes = (size_t) p.offsets[(size_t) n]*sizeof(float);
    }
    p.bitmapIsInput = op == OP_ERROR_CORRECTION || op == OP_SIGN_CORRECTION;
    const bool generates = op == OP_GENERATE || op == OP_GENERATE_LEGACY;
    p.correct = (generates || op == OP_ERROR_CORRECTION) && channels >= 3 && cfg->ec_mode != MSDFHIP_EC_DISABLED;
    p.stages = generates ? (p.correct ? 1 : 0)+(cfg->sign_correction ? 1 : 0) : 0;
    p.anyStencil = false;
    p.sumC = p.sumE = 0, p.maxC = p.maxE = 0;
    for (int g = 0; g < n; ++g) {
        const ShapeCall &c = *calls[g];
        const int nE = c.co[c.nC];
        p.sumC += c.nC, p.sumE += nE;
        p.maxC = c.nC > p.maxC ? c.nC : p.maxC, p.maxE = nE > p.maxE ? nE : p.maxE;
        p.anyStencil = p.anyStencil || (c.stencil != NULL && p.correct);   // no correction pass: the reference leaves the caller's buffer untouched
    }
    const size_t texels = p.texels = (size_t) w*h, tileBytes = p.tileBytes = texels*channels*sizeof(float);
    const size_t eAlloc = p.eAlloc = p.sumE > 0 ? p.sumE : 1, cAlloc = p.cAlloc = p.sumC > 0 ? p.sumC : 1;
    const size_t tilesAll = p.tilesAll = (size_t) ((w+TILE-1)/TILE)*((h+TILE-1)/TILE);
    const size_t singleCand = n == 1 && tilesAll <= 256 ? ecHeaderRecords((int) tilesAll)+tilesAll*SINGLE_TILE_SEGMENT+(eAlloc*2*sizeof(int)+sizeof(EcCandidate)-1)/sizeof(EcCandidate) : 0;
    p.candCap = deferredRecords(n, texels, (int) p.sumE) > singleCand ? deferredRecords(n, texels, (int) p.sumE) : singleCand;   // (k_single_call lays the buffer out per tile)

    // host staging layout (inputs first: one H2D copy; then the results: one D2H copy)
    Carver hc;
    p.hGco = hc.take((n+1)*sizeof(int32_t)), p.hCo = hc.take((p.sumC+1)*sizeof(int32_t)), p.hPts = hc.take(eAlloc*8*sizeof(double));
    p.hTypes = hc.take(eAlloc), p.hColors = hc.take(eAlloc), p.hGlyph = hc.take(n*sizeof(MsdfHipGlyph));
    p.hSrc = p.bitmapIsInput ? hc.take(p.mixed ? packedBytes : n*tileBytes) : hc.off;
    p.hDims = p.mixed ? hc.take(n*2*sizeof(int32_t)) : hc.off;
    p.inputBytes = hc.off;
    p.hBucket = hc.take(n*sizeof(int));                          // class lists of the overlapping combiner (uploaded on the stream by the launch code)
    p.hStatus = hc.take(256);                                    // [0]: candidate-overflow count of the correction pass, copied back with the results
    p.outBytes = p.mixed ? packedBytes : n*tileBytes;
    p.hOut = hc.take(p.outBytes), p.hStencil = hc.take(n*texels);
    p.resultBytes = hc.off-p.hOut;
    p.pinnedBytes = hc.off;
    // device layout: mirror of the staging area, then device-only work buffers
    Carver dc;
    dc.off = hc.off;
    p.dRecs = dc.take(eAlloc*sizeof(EdgeRec)), p.dWind = dc.take(cAlloc), p.dScratch = dc.take(n*tileBytes*p.stages);
    p.dCands = dc.take(p.correct ? p.candCap*sizeof(EcCandidate) : 0), p.dParams = dc.take(n*sizeof(EcGlyphParams));
    p.dSlots = dc.take(p.mixed && p.bitmapIsInput ? n*tileBytes : 0);
    // combiner scratch of the small-launch distance kernels (one tile per wavefront), see dispatchDistance
    p.gresNeed = op == OP_GENERATE && cfg->overlap_support && p.maxC > 1 && (size_t) n*tilesAll <= 8192 ? (size_t) n*tilesAll*p.maxC*channels*WAVE*sizeof(double) : 0;
    if (p.gresNeed > ((size_t) 64<<20))
        p.gresNeed = 0;
    p.dGres = dc.take(p.gresNeed);
    // k_single_call: one private digest area per workgroup (msdf_single.hpp) -- only reserved for calls that can take that path
    p.pvWind = (eAlloc*sizeof(EdgeRec)+63)/64*64, p.pvOff = (p.pvWind+cAlloc+63)/64*64, p.pvGco = (p.pvOff+(cAlloc+1)*sizeof(int32_t)+63)/64*64;
    p.pvGlyph = p.pvGco+64, p.pvStride = (p.pvGlyph+sizeof(MsdfHipGlyph)+255)/256*256;
    p.fusedShape = n == 1 && op == OP_GENERATE && tilesAll <= 256 && (tilesAll+1)*p.pvStride <= ((size_t) 32<<20);
    p.dPriv = dc.take(p.fusedShape ? (tilesAll+1)*p.pvStride : 0);
    p.devBytes = dc.off;
    return p;
}

// Flattens the calls' shapes (and, for the in-place operations, their bitmaps) into the arena's pinned staging as one CSR batch.
static void stageGroup(const GroupPlan &p, ThreadArena &a, ShapeCall *const *calls, int n) {
    const int channels = calls[0]->channels;
    int32_t *gco = reinterpret_cast<int32_t *>(a.pinned.ptr+p.hGco), *co = reinterpret_cast<int32_t *>(a.pinned.ptr+p.hCo);
    int32_t *dims = reinterpret_cast<int32_t *>(a.pinned.ptr+p.hDims);
    MsdfHipGlyph *gd = reinterpret_cast<MsdfHipGlyph *>(a.pinned.ptr+p.hGlyph);
    size_t cAt = 0, eAt = 0;
    co[0] = 0;
    for (int g = 0; g < n; ++g) {
        const ShapeCall &c = *calls[g];
        const int nE = c.co[c.nC];
        gco[g] = (int32_t) cAt;
        for (int k = 1; k <= c.nC; ++k)
            co[cAt+k] = (int32_t) (eAt+c.co[k]);
        if (nE) {
            memcpy(a.pinned.ptr+p.hPts+eAt*8*sizeof(double), c.points, (size_t) nE*8*sizeof(double));
            memcpy(a.pinned.ptr+p.hTypes+eAt, c.types, nE);
            memcpy(a.pinned.ptr+p.hColors+eAt, c.colors, nE);
        }
        cAt += c.nC, eAt += nE;
        memcpy(gd[g].xf, c.xf, sizeof(gd[g].xf));
        const int w = c.w, h = c.h;                              // (of every call of a group that is not mixed: p.w, p.h)
        // the device tiles are tightly packed in memory-row order: one after the other, or (mixed) each box at its packed offset; an in-place operation's
        // bitmaps are staged the same way
        const size_t at = p.mixed ? (size_t) p.offsets[(size_t) g] : (size_t) g*p.texels*channels;
        gd[g].out_offset = (int64_t) at;
        gd[g].row_stride = w*channels;
        gd[g].flip = c.flip ? 1 : 0;
        if (p.mixed)
            dims[2*(size_t) g] = w, dims[2*(size_t) g+1] = h;
        if (p.bitmapIsInput)
            for (int y = 0; y < h; ++y)
                memcpy(a.pinned.ptr+p.hSrc+(at+(size_t) y*w*channels)*sizeof(float), c.pixels+(ptrdiff_t) c.rowStride*y, sizeof(float)*(size_t) w*channels);
    }
    gco[n] = (int32_t) cAt;
}

// b becomes a view into the arena: its workspace borrows the arena's regions and owns only what has to grow beyond them.
static void buildView(const GroupPlan &p, ThreadArena &a, ShapeCall *const *calls, int n, MsdfHipBatch &b) {
    b.onDevice(a.device);
    b.nGlyphs = n, b.nContours = (int) p.sumC, b.nEdges = (int) p.sumE;
    b.dGlyphContourOffsets.borrow(reinterpret_cast<int32_t *>(a.dev.ptr+p.hGco), (size_t) n+1);
    b.dContourOffsets.borrow(reinterpret_cast<int32_t *>(a.dev.ptr+p.hCo), p.sumC+1);
    b.dPoints.borrow(reinterpret_cast<double *>(a.dev.ptr+p.hPts), 8*p.eAlloc);
    b.dTypes.borrow(reinterpret_cast<uint8_t *>(a.dev.ptr+p.hTypes), p.eAlloc);
    b.dColors.borrow(reinterpret_cast<uint8_t *>(a.dev.ptr+p.hColors), p.eAlloc);
    b.dRecs.borrow(reinterpret_cast<EdgeRec *>(a.dev.ptr+p.dRecs), p.eAlloc);
    b.dWindings.borrow(reinterpret_cast<int8_t *>(a.dev.ptr+p.dWind), p.cAlloc);
    if (p.correct)
        b.work.deferred.borrow(reinterpret_cast<EcCandidate *>(a.dev.ptr+p.dCands), p.candCap);
    b.work.ecParams.borrow(reinterpret_cast<EcGlyphParams *>(a.dev.ptr+p.dParams), (size_t) n);
    b.work.bucket.borrow(reinterpret_cast<int *>(a.dev.ptr+p.hBucket), (size_t) n), b.work.hBucket.borrow(reinterpret_cast<int *>(a.pinned.ptr+p.hBucket), (size_t) n);
    if (p.gresNeed)
        b.work.gres.borrow(reinterpret_cast<double *>(a.dev.ptr+p.dGres), p.gresNeed/sizeof(double));
    b.hContours.resize((size_t) n);
    b.hEdges.resize((size_t) n);
    for (int g = 0; g < n; ++g) {
        b.hContours[g] = calls[g]->nC;
        b.hEdges[g] = calls[g]->co[calls[g]->nC];
    }
    b.countMaxima();
}

// The status words and the results (with the stencils only where one is wanted) -> pinned staging, and the end of everything queued on the arena's stream.
static int copyBackAndWait(const GroupPlan &p, ThreadArena &a) {
    HIPCHK(hipMemcpyAsync(a.pinned.ptr+p.hStatus, a.dev.ptr+p.hStatus, 256+(p.anyStencil ? p.resultBytes : p.outBytes), hipMemcpyDeviceToHost, a.stream));
    HIPCHK(waitStream(a.stream));
    return MSDFHIP_OK;
}

// k_single_call's arguments. Zero copy: the kernel reads the staged CSR arrays straight from pinned host memory (phase 0) and writes the result tile and
// its status words there; else a.dev.ptr holds the inputs already.
static void fillSingleArgs(SingleArgs &sa, const GroupPlan &p, const SinglePlan &single, ThreadArena &a, const MsdfHipBatch &b, const ShapeCall &c, bool overlapEff, bool zeroCopy) {
    const size_t sumC = p.sumC, sumE = p.sumE;
    char *in = zeroCopy ? a.pinnedDev : a.dev.ptr;
    sa.srcContourOffsets = reinterpret_cast<const int32_t *>(in+p.hCo), sa.points = reinterpret_cast<const double *>(in+p.hPts);
    sa.types = reinterpret_cast<const uint8_t *>(in+p.hTypes), sa.colors = reinterpret_cast<const uint8_t *>(in+p.hColors);
    sa.srcGlyph = reinterpret_cast<const MsdfHipGlyph *>(in+p.hGlyph);
    sa.priv = a.dev.ptr+p.dPriv, sa.privStride = p.pvStride, sa.privWindings = p.pvWind, sa.privOffsets = p.pvOff, sa.privGlyphOffsets = p.pvGco, sa.privGlyph = p.pvGlyph;
    sa.nContours = (int) sumC, sa.nEdges = (int) sumE;
    {   // small shapes inside the kernel arguments (msdf_single.hpp)
        Carver pc;
        const size_t pCo = pc.take((sumC+1)*sizeof(int32_t)), pPts = pc.take(sumE*8*sizeof(double)), pTypes = pc.take(sumE), pColors = pc.take(sumE);
        const size_t pGlyph = pc.take(sizeof(MsdfHipGlyph));
        sa.payloadBytes = 0;
        if (pc.off <= sizeof(sa.payload) && !tuning().noArgPayloadSingle) {
            sa.payloadBytes = (unsigned) pc.off, sa.payOffsets = (unsigned) pCo, sa.payPoints = (unsigned) pPts, sa.payTypes = (unsigned) pTypes;
            sa.payColors = (unsigned) pColors, sa.payGlyph = (unsigned) pGlyph;
            memcpy(sa.payload+pCo, a.pinned.ptr+p.hCo, (sumC+1)*sizeof(int32_t));
            memcpy(sa.payload+pPts, a.pinned.ptr+p.hPts, sumE*8*sizeof(double));
            memcpy(sa.payload+pTypes, a.pinned.ptr+p.hTypes, sumE);
            memcpy(sa.payload+pColors, a.pinned.ptr+p.hColors, sumE);
            memcpy(sa.payload+pGlyph, a.pinned.ptr+p.hGlyph, sizeof(MsdfHipGlyph));
        }
    }
    sa.width = c.w, sa.height = c.h, sa.tilesX = (c.w+TILE-1)/TILE, sa.tiles = (int) p.tilesAll, sa.listStride = p.maxE;
    sa.scratch = p.correct ? reinterpret_cast<float *>(a.dev.ptr+p.dScratch) : NULL;
    sa.out = reinterpret_cast<float *>((zeroCopy ? a.pinnedDev : a.dev.ptr)+p.hOut);
    sa.stencil = p.anyStencil ? reinterpret_cast<uint8_t *>(a.dev.ptr+p.hStencil) : NULL;
    sa.gres = overlapEff && !single.resInLds ? reinterpret_cast<double *>(a.dev.ptr+p.dGres) : NULL, sa.gresStride = single.resBytes/sizeof(double);
    // candidates: a counter and a segment of SINGLE_TILE_SEGMENT records per TILE (the tile's workgroup judges them itself), then the corner list
    sa.cfg = c.cfg, sa.correct = p.correct ? 1 : 0, sa.ecParams = b.work.ecParams.ptr, sa.cands = b.work.deferred.ptr, sa.seg = SINGLE_TILE_SEGMENT;
    sa.corners = p.correct ? reinterpret_cast<int *>(b.work.deferred.ptr+ecHeaderRecords((int) p.tilesAll)+p.tilesAll*SINGLE_TILE_SEGMENT) : NULL;
    sa.sizes = NULL;
    sa.slotCap = single.slotCap, sa.slotOffset = single.slotOffset;
    sa.teamXchgOffset = (unsigned) single.teamXchgOffset;
    sa.barrier = a.barrier.ptr, sa.barrierBase = a.barrierEpoch, sa.doneBase = a.doneCount;
    sa.doneValue = a.doneEpoch+1u ? a.doneEpoch+1u : 1u;
    {   // ~70 ns per iteration: 2-3 ms for a font glyph, growing with the edges a tile may have to walk, at most the old 0.3 s
        const unsigned long long limit = (1ull<<15)+((unsigned long long) sumE<<8);
        sa.spinLimit = tuning().singleSpinLimit ? (unsigned) tuning().singleSpinLimit : (unsigned) (limit < (1ull<<22) ? limit : (1ull<<22));
    }
    sa.status = reinterpret_cast<unsigned *>((zeroCopy ? a.pinnedDev : a.dev.ptr)+p.hStatus);
}

// ---- one launch for the whole call (msdf_single.hpp) where it applies: ONE shape, a generate*() call without the scanline pass, a bitmap of
// at most 256 tiles, lists / correction scratch within 64 KB of LDS. FUSED_RERUN: the launch did not do its job -- it gave up at its grid barrier, ended
// without its flag, or a tile's candidates overflowed their segment (pathological inputs) -- and the caller runs the batched sequence; the inputs are on
// the device for it, and the arena's counters are as a fresh arena has them.
// Zero copy where the staging area is mapped into the device: no upload launch in front, no copy behind, and the host learns of the end by polling a
// word the last workgroup writes instead of a stream synchronisation. With a stencil (rare) the results take the device buffers and one copy, as the
// batched path does.
enum FusedOutcome { FUSED_DONE, FUSED_RERUN };
static int runFused(const GroupPlan &p, const SinglePlan &single, ThreadArena &a, ArenaHold &lease, const MsdfHipBatch &b, FusedReservation &fusedSlots, const ShapeCall &c,
                    bool overlapEff, bool zeroCopy, FusedOutcome &outcome) {
    outcome = FUSED_RERUN;
    SingleArgs sa;
    fillSingleArgs(sa, p, single, a, b, c, overlapEff, zeroCopy);
    const unsigned groups = (unsigned) p.tilesAll+(p.correct ? 1u : 0u);
    volatile unsigned *hostStatus = reinterpret_cast<volatile unsigned *>(a.pinned.ptr+p.hStatus);
    if (zeroCopy)
        hostStatus[0] = hostStatus[1] = hostStatus[2] = 0;       // overflow / barrier flags are only ever RAISED by the kernel; [2]: the staging area is recycled, whatever sits there is not this call's flag
    else
        HIPCHK(hipMemsetAsync(a.dev.ptr+p.hStatus, 0, 64, a.stream));
    forSingleCallVariant(c.mode*2+(overlapEff ? 1 : 0), [&](auto sel, auto overlap) {
        hipLaunchKernelGGL((k_single_call<decltype(sel)::value, decltype(overlap)::value>), dim3(groups), dim3(WAVE*SINGLE_TEAM), single.lds, a.stream, sa);
    });
    {
        const hipError_t launched = hipGetLastError();
        if (launched != hipSuccess)                              // nothing ran: the counters and the epochs kept here still agree
            return fail(MSDFHIP_ERR_HIP, "k_single_call launch failed: %s", hipGetErrorString(launched));
    }
    a.barrierEpoch += (p.correct ? 1u : 0u)*groups, a.doneCount += groups;   // what this launch adds to the two counters
    a.doneEpoch = sa.doneValue;
    bool abandoned = false;                                      // the launch did not do its job: rerun through the batched sequence, from fresh counters
    if (zeroCopy) {
        // Polls the completion word: pause between looks (the sibling hyperthread keeps its core), and once a call has outlasted the common
        // case give the core away between looks -- 64 waiting leaders must not starve the threads that stage the next calls.
        const long long deadline = nowNs()+2000000;              // 2 ms of polling, then the runtime's own wait (a failed launch never raises the flag)
        for (unsigned looks = 0; hostStatus[2] != sa.doneValue && nowNs() < deadline; ++looks) {
            if (looks < 4096)
                __builtin_ia32_pause();
            else
                sched_yield();
        }
        if (hostStatus[2] != sa.doneValue) {
            HIPCHK(hipStreamSynchronize(a.stream));
            if (hostStatus[2] != sa.doneValue) {
                unsigned counters[32] = { 0 };
                (void) hipMemcpy(counters, a.barrier.ptr, sizeof(counters), hipMemcpyDeviceToHost);
                gSingleLost += 1;
                if (tuning().singleVerbose)
                    fprintf(stderr, "msdfgen_hip: k_single_call ended without raising its completion flag (flag %u, expected %u; status %u %u; finished-workgroup "
                            "counter %u, expected %u + %u; barrier counter %u, base %u): rerunning the call through the batched sequence\n", (unsigned) hostStatus[2],
                            sa.doneValue, (unsigned) hostStatus[0], (unsigned) hostStatus[1], counters[16], sa.doneBase, groups, counters[0], sa.barrierBase);
                abandoned = true;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        lease.quiescent = !abandoned;
    } else {
        const int rc = copyBackAndWait(p, a);
        if (rc != MSDFHIP_OK)
            return rc;
    }
    if (hostStatus[1] != 0) {                                    // workgroups gave up at the grid barrier (the launch was not resident as a whole)
        gSingleTimeouts += 1;
        abandoned = true;
    }
    fusedSlots.release();
    if (abandoned) {                                             // the values on the device no longer match the epochs kept here: leave the counters as a fresh arena has them
        lease.quiescent = false;
        HIPCHK(hipStreamSynchronize(a.stream));
        HIPCHK(hipMemsetAsync(a.barrier.ptr, 0, 256, a.stream));
        a.barrierEpoch = a.doneCount = 0;
    }
    if (!abandoned && hostStatus[0] == 0)
        outcome = FUSED_DONE;
    if (outcome == FUSED_DONE && p.correct && zeroCopy) {        // (all phases ran and the stamps are at hand: the diagnostics count these calls)
        for (int k = 0; k < 7; ++k)
            gSinglePhase[k] += (unsigned long long) hostStatus[8+k];
        gSinglePhase[7] += (unsigned long long) hostStatus[7];
        gSingleCycles += (unsigned long long) hostStatus[15];
        ++gSingleCalls;
    }
    if (outcome == FUSED_RERUN && zeroCopy)                      // rerun through the batched sequence: it expects the inputs on the device
        HIPCHK(hipMemcpyAsync(a.dev.ptr, a.pinned.ptr, p.inputBytes, hipMemcpyHostToDevice, a.stream));
    return MSDFHIP_OK;
}

// The batched launch sequence of the group's operation, results and status words back in the pinned staging. k_ec_query mirrors the candidate-overflow count
// next to the results instead of a launch of the overflow pass per call; where a glyph's candidate segment did overflow (more than 1/16 of its texels needed
// a distance check: pathological inputs only) the operation runs once more, with the per-texel overflow pass in its launch sequence -- an in-place correction
// too: the input copy on the device is intact.
static int launchBoxesToSlots(float *dSlots, const float *dPacked, const MsdfHipGlyph *dGlyphs, const int32_t *dDims, int n, int channels, size_t slot, hipStream_t stream);   // (at the end of this file: it names k_boxes_to_slots)

static int runBatched(const GroupPlan &p, ThreadArena &a, MsdfHipBatch &b, const ShapeCall &c) {
    const MsdfHipGlyph *dGlyph = reinterpret_cast<const MsdfHipGlyph *>(a.dev.ptr+p.hGlyph);
    const float *dSrc = reinterpret_cast<const float *>(a.dev.ptr+p.hSrc);
    float *dOut = reinterpret_cast<float *>(a.dev.ptr+p.hOut);
    uint8_t *dStencil = p.anyStencil ? reinterpret_cast<uint8_t *>(a.dev.ptr+p.hStencil) : NULL;
    // A mixed group: the sized twins at the launches of a p.w x p.h call. Their sizes came with the inputs; the sized passes read a source field at the start
    // of its slot, so an in-place operation's packed bitmaps are spread into slots on the device first (what crossed PCIe is the packed region only).
    const int32_t *dDims = p.mixed ? reinterpret_cast<const int32_t *>(a.dev.ptr+p.hDims) : NULL;
    int rc = digest(&b, a.stream);
    if (rc == MSDFHIP_OK && p.mixed && p.bitmapIsInput) {
        rc = launchBoxesToSlots(reinterpret_cast<float *>(a.dev.ptr+p.dSlots), dSrc, dGlyph, dDims, p.n, c.channels, p.texels, a.stream);
        dSrc = reinterpret_cast<const float *>(a.dev.ptr+p.dSlots);
    }
    for (int attempt = 0; rc == MSDFHIP_OK && attempt < 2; ++attempt) {   // mirrored, then with the overflow pass
        GenerateCall call;
        call.overflowOut = attempt == 0 ? reinterpret_cast<unsigned *>(a.dev.ptr+p.hStatus) : NULL;
        call.boxDims = dDims;
        if (c.op == OP_ERROR_CORRECTION)
            rc = runCorrection(&b, c.channels, p.w, p.h, dGlyph, dSrc, dOut, dStencil, c.cfg, a.stream, call);
        else if (c.op == OP_SIGN_CORRECTION)
            rc = runSignCorrection(&b, c.channels, p.w, p.h, dGlyph, dSrc, dOut, 0, c.cfg.sdf_zero_value, c.cfg.fill_rule, a.stream, dDims);
        else if (c.op == OP_RASTERIZE)
            rc = runSignCorrection(&b, 1, p.w, p.h, dGlyph, NULL, dOut, 0, 0.f, c.cfg.fill_rule, a.stream, dDims);
        else if (c.op == OP_GENERATE_LEGACY)                     // (c.cfg is a legacyConfig: msdfhip_generate_legacy; never mixed: groupOpTakesSizes)
            rc = runGenerateLegacy(&b, c.mode, p.w, p.h, dGlyph, dOut, dStencil, p.stages ? reinterpret_cast<float *>(a.dev.ptr+p.dScratch) : NULL, c.cfg, a.stream, call);
        else
            rc = runGenerate(&b, c.mode, p.w, p.h, dGlyph, dOut, dStencil, p.stages ? reinterpret_cast<float *>(a.dev.ptr+p.dScratch) : NULL, &c.cfg, a.stream, call);
        if (rc == MSDFHIP_OK)
            rc = copyBackAndWait(p, a);
        if (!(call.overflowMirrored && *reinterpret_cast<const unsigned *>(a.pinned.ptr+p.hStatus) != 0))
            break;
    }
    return rc;
}

// The tiles in the pinned staging -> the callers' bitmaps (any row stride) and stencils.
static void scatterGroup(const GroupPlan &p, ThreadArena &a, ShapeCall *const *calls, int n) {
    const int channels = calls[0]->channels;
    for (int g = 0; g < n; ++g) {
        const ShapeCall &c = *calls[g];
        const int w = c.w, h = c.h;                              // (mixed: the call's own box at its packed offset, its stencil packed at the start of slot g)
        const float *tile = reinterpret_cast<const float *>(a.pinned.ptr+p.hOut)+(p.mixed ? (size_t) p.offsets[(size_t) g] : (size_t) g*p.texels*channels);
        for (int y = 0; y < h; ++y)
            memcpy(c.pixels+(ptrdiff_t) c.rowStride*y, tile+(size_t) y*w*channels, sizeof(float)*(size_t) w*channels);
        if (c.stencil && p.anyStencil)
            memcpy(c.stencil, a.pinned.ptr+p.hStencil+(size_t) g*p.texels, (size_t) w*h);
    }
}

// sel: what the leader's selection found (NULL: one call, or calls of one size). A group of different sizes takes the batched sequence with sizes; every other
// group runs exactly as it did before sizes could differ.
static int runGroup(ShapeCall *const *calls, int n, const GroupSelection *sel = NULL) {
    const ShapeCall &c0 = *calls[0];
    const MsdfHipConfig *cfg = &c0.cfg;
    int rc = ensureDevice(frontDoorDevice());
    if (rc != MSDFHIP_OK)
        return rc;
    const GroupPlan plan = planGroup(calls, n, sel);
    ArenaHold lease;
    rc = takeArena(lease);
    if (rc != MSDFHIP_OK)
        return rc;
    ThreadArena &a = *lease;
    rc = arenaReserve(a, plan.devBytes, plan.pinnedBytes);
    if (rc != MSDFHIP_OK)
        return rc;

    const long long t0 = nowNs();
    stageGroup(plan, a, calls, n);
    const long long t1 = nowNs();
    // Does the call take ONE launch (k_single_call, msdf_single.hpp)? ONE shape, a generate*() call without the scanline pass, a bitmap of at most
    // 256 tiles, lists / correction scratch within 64 KB of LDS. Decided before the upload: with the staging area mapped into the device the
    // kernel reads its inputs from there and nothing is uploaded at all.
    const bool overlapEff = cfg->overlap_support && plan.maxC > 1;
    const SinglePlan single = planSingleLaunch(plan.maxC, plan.maxE, c0.channels, overlapEff, plan.correct);
    bool fused = plan.fusedShape && !tuning().noFusedSingle && !cfg->sign_correction && cfg->ec_stage_limit == 0 &&
                 single.lds <= (size_t) 64*1024 && (!overlapEff || single.resInLds || plan.gresNeed >= plan.tilesAll*single.resBytes);
    FusedReservation fusedSlots;                                 // (see fusedCapacity: all workgroups of the launch must be resident together)
    if (fused) {
        fused = fusedSlots.take(a.device, c0.mode*2+(overlapEff ? 1 : 0), single.lds, (int) plan.tilesAll+(plan.correct ? 1 : 0));
        if (!fused)
            gSingleRefused += 1;
    }
    const bool zeroCopy = fused && a.pinnedDev != NULL && !plan.anyStencil && !tuning().noZeroCopySingle;
    if (zeroCopy) {
        // (nothing to upload)
    } else if (plan.inputBytes <= ((size_t) 1<<20)) {            // a few KB: read from the pinned staging by a kernel -- no SDMA submission on the latency path
        rc = uploadSmall(a.dev.ptr, a.pinned.ptr, plan.inputBytes, a.stream);
        if (rc != MSDFHIP_OK)
            return rc;
    } else
        HIPCHK(hipMemcpyAsync(a.dev.ptr, a.pinned.ptr, plan.inputBytes, hipMemcpyHostToDevice, a.stream));

    MsdfHipBatch b;
    buildView(plan, a, calls, n, b);
    FusedOutcome outcome = FUSED_RERUN;
    if (fused)
        rc = runFused(plan, single, a, lease, b, fusedSlots, c0, overlapEff, zeroCopy, outcome);
    if (rc == MSDFHIP_OK && outcome == FUSED_RERUN)
        rc = runBatched(plan, a, b, c0);
    if (rc != MSDFHIP_OK) {
        hipStreamSynchronize(a.stream);
        return rc;
    }
    const long long t2 = nowNs();
    scatterGroup(plan, a, calls, n);
    gNsStage += t1-t0, gNsDevice += t2-t1, gNsScatter += nowNs()-t2;
    return MSDFHIP_OK;
}

// ---- transparent micro-batching ---------------------------------------------------------------------------
// Callers such as msdf-atlas-gen's worker threads each call generateMSDF for one glyph at a time. A single call is bound by launch
// and PCIe latency (~150 us), not by the GPU. Concurrent calls are therefore combined, group-commit style: a call that finds a
// free leader slot runs at once (no waiting, no timer: a lone caller never pays for the mechanism); calls that arrive while the
// leaders are busy queue up, and the next leader takes every queued call with the same launch parameters along as one device
// batch. Results do not depend on the grouping (glyphs are independent).
static std::mutex gQueueMutex;
static std::vector<ShapeCall *> gQueue;                          // arrival order; claimed entries belong to a running leader
static int gActiveLeaders = 0;
static std::atomic<long long> gStatCalls(0), gStatBatches(0), gStatLargest(0);
static std::atomic<long long> gStatMixedBatches(0), gStatMixedCalls(0), gStatPaddedTexels(0), gStatBoxTexels(0);   // groups run with sizes (msdfhip_microbatch_mixed_stats)
static long long gHoldUntilNs = 0;                               // msdfhip_microbatch_hold: no new leader starts before this time (guarded by gQueueMutex; 0: no hold)
static const size_t GROUP_BYTES_LIMIT = 256u<<20;                // tiles of one group (bounds the per-thread arena)

static int maxGroup() {
    int v = gMaxGroup.load();
    if (v < 0) {
        v = tuning().microbatch;                                 // MSDFHIP_MICROBATCH: 0 disables; N > 1 caps the group size (256)
        gMaxGroup.store(v);
    }
    return v;
}

static ShapeCall *firstUnclaimed() {
    for (size_t i = 0; i < gQueue.size(); ++i)
        if (!gQueue[i]->claimed)
            return gQueue[i];
    return NULL;
}

static int submitCall(ShapeCall &c) {
    const int cap = maxGroup();
    if (cap <= 1) {
        ShapeCall *one = &c;
        ++gStatCalls, ++gStatBatches;
        return runGroup(&one, 1);
    }
    std::vector<ShapeCall *> group;
    GroupSelection selection;
    {
        std::unique_lock<std::mutex> lock(gQueueMutex);
        c.claimed = c.done = false;
        gQueue.push_back(&c);
        for (;;) {                                               // (under a hold the wait is bounded: the hold ends by itself, and nobody is there to notify then)
            const long long holdLeft = gHoldUntilNs-nowNs();
            if (c.done || (holdLeft <= 0 && gActiveLeaders < gMaxLeaders.load() && firstUnclaimed() == &c))
                break;
            if (holdLeft > 0)
                c.cv.wait_for(lock, std::chrono::nanoseconds(holdLeft));
            else
                c.cv.wait(lock);
        }
        if (c.done) {
            if (c.rc != MSDFHIP_OK)
                tlsError = c.error;
            return c.rc;
        }
        // The leader's own call, then every queued call that may share its launch sequence, in arrival order; the selection (msdf_groupplan.hpp) says which of
        // them it takes. What it passes over stays queued for the next leader, like the calls of another launch.
        std::vector<ShapeCall *> compatible(1, &c);
        for (size_t i = 0; i < gQueue.size(); ++i) {
            ShapeCall *q = gQueue[i];
            if (!q->claimed && q != &c && sameLaunch(*q, c))
                compatible.push_back(q);
        }
        std::vector<int32_t> sizes(2*compatible.size()), scratch(2*compatible.size());
        std::vector<uint8_t> taken(compatible.size());
        for (size_t i = 0; i < compatible.size(); ++i)
            sizes[2*i] = compatible[i]->w, sizes[2*i+1] = compatible[i]->h;
        groupSelect((int) compatible.size(), sizes.data(), c.channels, cap, GROUP_BYTES_LIMIT, tuning().microbatchMaxPad, taken.data(), scratch.data(), selection);
        for (size_t i = 0; i < compatible.size(); ++i)
            if (taken[i]) {
                compatible[i]->claimed = true;
                group.push_back(compatible[i]);
            }
        ++gActiveLeaders;
        if (gActiveLeaders < gMaxLeaders.load())
            if (ShapeCall *next = firstUnclaimed())
                next->cv.notify_one();                           // a second leader may start on what is left
    }
    int rc = runGroup(group.data(), (int) group.size(), &selection);
    gStatCalls += (long long) group.size();
    ++gStatBatches;
    if (!selection.uniform && group.size() > 1) {
        ++gStatMixedBatches;
        gStatMixedCalls += (long long) group.size();
        gStatPaddedTexels += (long long) (group.size()*selection.slot), gStatBoxTexels += (long long) selection.boxTexels;
    }
    for (long long seen = gStatLargest.load(); (long long) group.size() > seen && !gStatLargest.compare_exchange_weak(seen, (long long) group.size()); ) { }
    std::string error = rc != MSDFHIP_OK ? tlsError : std::string();
    std::vector<int> rcs(group.size(), rc);
    std::vector<std::string> errors(group.size(), error);
    if (rc != MSDFHIP_OK && group.size() > 1)                    // attribute the failure: rerun the members one by one
        for (size_t i = 0; i < group.size(); ++i) {
            rcs[i] = runGroup(&group[i], 1);
            errors[i] = rcs[i] != MSDFHIP_OK ? tlsError : std::string();
        }
    int mine = MSDFHIP_OK;
    {
        std::unique_lock<std::mutex> lock(gQueueMutex);
        for (size_t i = 0; i < group.size(); ++i) {
            ShapeCall *q = group[i];
            for (size_t k = 0; k < gQueue.size(); ++k)
                if (gQueue[k] == q) {
                    gQueue.erase(gQueue.begin()+k);
                    break;
                }
            if (q == &c) {
                mine = rcs[i];
                if (mine != MSDFHIP_OK)
                    tlsError = errors[i];
            } else {
                q->rc = rcs[i];
                q->error = errors[i];
                q->done = true;
                q->cv.notify_one();
            }
        }
        --gActiveLeaders;
        if (ShapeCall *next = firstUnclaimed())
            next->cv.notify_one();
    }
    return mine;
}

static int singleShape(int mode, int channels, int op, float *pixels, int w, int h, int rowStride, int flip,
                       const int32_t *co, int nC, const double *points, const uint8_t *types, const uint8_t *colors,
                       const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil) {
    if (w < 0 || h < 0 || nC < 0 || !co || !xf || (!pixels && w*h > 0))
        return fail(MSDFHIP_ERR_INVALID, "bad arguments");
    int rc = checkConfig(cfg);
    if (rc != MSDFHIP_OK)
        return rc;
    if (w == 0 || h == 0)
        return MSDFHIP_OK;
    if (op == OP_ERROR_CORRECTION && cfg->ec_mode == MSDFHIP_EC_DISABLED)
        return MSDFHIP_OK;
    rc = ensureDevice();
    if (rc != MSDFHIP_OK)
        return rc;
    if (co[0] != 0)
        return fail(MSDFHIP_ERR_INVALID, "contour_offsets must start at 0");
    for (int c = 0; c < nC; ++c)
        if (co[c+1] < co[c])
            return fail(MSDFHIP_ERR_INVALID, "contour_offsets not monotonic at %d", c);
    const int nE = co[nC];
    if (nE > 0 && (!points || !types || !colors))
        return fail(MSDFHIP_ERR_INVALID, "NULL edge arrays");
    for (int e = 0; e < nE; ++e)
        if (types[e] < 1 || types[e] > 3)
            return fail(MSDFHIP_ERR_INVALID, "edge %d has type %d (must be 1, 2 or 3)", e, (int) types[e]);
    ShapeCall c;
    c.mode = mode, c.channels = channels, c.op = op, c.w = w, c.h = h, c.rowStride = rowStride, c.flip = flip ? 1 : 0, c.nC = nC;
    c.pixels = pixels, c.co = co, c.points = points, c.types = types, c.colors = colors, c.stencil = stencil;
    memcpy(c.xf, xf, sizeof(c.xf));
    c.cfg = *cfg;
    c.claimed = c.done = false;
    c.rc = MSDFHIP_OK;
    return submitCall(c);
}

// Host-pointer forms of renderSDF / simulate8bit (the shim's overloads): rows gathered into the calling thread's arena, one H2D copy,
// the kernel, one D2H copy. Strides in floats, may be negative (BitmapSection).
int msdfhip_render_sdf_host(float *out, int ow, int oh, int outStride, int no, const float *sdf, int sw, int sh, int sdfStride, int ns,
                            double rangeLower, double rangeUpper, float sdThreshold) {
    if (ow < 0 || oh < 0 || sw < 0 || sh < 0)
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_render_sdf_host");
    if (!((no == 1 && (ns == 1 || ns == 3 || ns == 4)) || (no == 3 && (ns == 1 || ns == 3)) || (no == 4 && ns == 4)))
        return fail(MSDFHIP_ERR_INVALID, "renderSDF has no overload for %d <- %d channels (core/render-sdf.h:12-17)", no, ns);
    if (ow == 0 || oh == 0)
        return MSDFHIP_OK;
    if (!out || !sdf || sw == 0 || sh == 0)
        return fail(MSDFHIP_ERR_INVALID, "NULL or empty bitmap");
    int rc = ensureDevice();
    if (rc != MSDFHIP_OK)
        return rc;
    const size_t inBytes = sizeof(float)*(size_t) sw*sh*ns, outBytes = sizeof(float)*(size_t) ow*oh*no;
    Carver c;
    const size_t offIn = c.take(inBytes), offOut = c.take(outBytes);
    ArenaHold lease;
    rc = takeArena(lease);
    if (rc != MSDFHIP_OK)
        return rc;
    ThreadArena &a = *lease;
    rc = arenaReserve(a, c.off, c.off);
    if (rc != MSDFHIP_OK)
        return rc;
    for (int y = 0; y < sh; ++y)
        memcpy(a.pinned.ptr+offIn+sizeof(float)*(size_t) y*sw*ns, sdf+(ptrdiff_t) sdfStride*y, sizeof(float)*(size_t) sw*ns);
    HIPCHK(hipMemcpyAsync(a.dev.ptr+offIn, a.pinned.ptr+offIn, inBytes, hipMemcpyHostToDevice, a.stream));
    rc = msdfhip_render_sdf(reinterpret_cast<const float *>(a.dev.ptr+offIn), 1, sw, sh, ns, reinterpret_cast<float *>(a.dev.ptr+offOut), ow, oh, no,
                            rangeLower, rangeUpper, sdThreshold, a.stream);
    if (rc != MSDFHIP_OK)
        return rc;
    HIPCHK(hipMemcpyAsync(a.pinned.ptr+offOut, a.dev.ptr+offOut, outBytes, hipMemcpyDeviceToHost, a.stream));
    HIPCHK(hipStreamSynchronize(a.stream));
    for (int y = 0; y < oh; ++y)
        memcpy(out+(ptrdiff_t) outStride*y, a.pinned.ptr+offOut+sizeof(float)*(size_t) y*ow*no, sizeof(float)*(size_t) ow*no);
    return MSDFHIP_OK;
}

int msdfhip_simulate_8bit_host(float *pixels, int w, int h, int rowStride, int channels) {
    if (w < 0 || h < 0 || channels < 1 || channels > 4)
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_simulate_8bit_host");
    if (w == 0 || h == 0)
        return MSDFHIP_OK;
    if (!pixels)
        return fail(MSDFHIP_ERR_INVALID, "NULL bitmap");
    int rc = ensureDevice();
    if (rc != MSDFHIP_OK)
        return rc;
    const size_t bytes = sizeof(float)*(size_t) w*h*channels;
    ArenaHold lease;
    rc = takeArena(lease);
    if (rc != MSDFHIP_OK)
        return rc;
    ThreadArena &a = *lease;
    rc = arenaReserve(a, bytes, bytes);
    if (rc != MSDFHIP_OK)
        return rc;
    for (int y = 0; y < h; ++y)
        memcpy(a.pinned.ptr+sizeof(float)*(size_t) y*w*channels, pixels+(ptrdiff_t) rowStride*y, sizeof(float)*(size_t) w*channels);
    HIPCHK(hipMemcpyAsync(a.dev.ptr, a.pinned.ptr, bytes, hipMemcpyHostToDevice, a.stream));
    rc = msdfhip_simulate_8bit(reinterpret_cast<float *>(a.dev.ptr), (size_t) w*h*channels, a.stream);
    if (rc != MSDFHIP_OK)
        return rc;
    HIPCHK(hipMemcpyAsync(a.pinned.ptr, a.dev.ptr, bytes, hipMemcpyDeviceToHost, a.stream));
    HIPCHK(hipStreamSynchronize(a.stream));
    for (int y = 0; y < h; ++y)
        memcpy(pixels+(ptrdiff_t) rowStride*y, a.pinned.ptr+sizeof(float)*(size_t) y*w*channels, sizeof(float)*(size_t) w*channels);
    return MSDFHIP_OK;
}

int msdfhip_generate(int mode, float *pixels, int w, int h, int rowStride, int flip, const int32_t *co, int nC, const double *points,
                     const uint8_t *types, const uint8_t *colors, const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil) {
    if (mode < 1 || mode > 4)
        return fail(MSDFHIP_ERR_INVALID, "mode %d (must be 1..4)", mode);
    return singleShape(mode, channelsOf(mode), OP_GENERATE, pixels, w, h, rowStride, flip, co, nC, points, types, colors, xf, cfg, stencil);
}

// The legacy generators on one shape. A group of them takes the batched launch sequence (runBatched: planGroup reserves k_single_call's areas for
// OP_GENERATE only), and sameLaunch never puts a legacy call and a modern one into one group: their ops differ.
int msdfhip_generate_legacy(int mode, float *pixels, int w, int h, int rowStride, int flip, const int32_t *co, int nC, const double *points,
                            const uint8_t *types, const uint8_t *colors, const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil) {
    if (mode < 1 || mode > 4)
        return fail(MSDFHIP_ERR_INVALID, "mode %d (must be 1..4)", mode);
    if (!cfg)
        return fail(MSDFHIP_ERR_INVALID, "cfg is NULL");
    const MsdfHipConfig legacy = legacyConfig(*cfg);
    return singleShape(mode, channelsOf(mode), OP_GENERATE_LEGACY, pixels, w, h, rowStride, flip, co, nC, points, types, colors, xf, &legacy, stencil);
}

// msdfErrorCorrection_legacy on a host bitmap: rows gathered into the calling thread's arena, one H2D copy, the two passes, one D2H copy.
int msdfhip_error_correction_legacy(int channels, float *pixels, int w, int h, int rowStride, double thresholdX, double thresholdY) {
    if (w < 0 || h < 0 || (channels != 3 && channels != 4))
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_error_correction_legacy (channels must be 3 or 4)");
    if (w == 0 || h == 0)
        return MSDFHIP_OK;
    if (!pixels)
        return fail(MSDFHIP_ERR_INVALID, "NULL bitmap");
    int rc = ensureDevice();
    if (rc != MSDFHIP_OK)
        return rc;
    const size_t rowBytes = sizeof(float)*(size_t) w*channels, bytes = rowBytes*h;
    Carver c;
    const size_t offTiles = c.take(bytes), offScratch = c.take(bytes);
    ArenaHold lease;
    rc = takeArena(lease);
    if (rc != MSDFHIP_OK)
        return rc;
    ThreadArena &a = *lease;
    rc = arenaReserve(a, c.off, bytes);
    if (rc != MSDFHIP_OK)
        return rc;
    for (int y = 0; y < h; ++y)
        memcpy(a.pinned.ptr+rowBytes*y, pixels+(ptrdiff_t) rowStride*y, rowBytes);
    HIPCHK(hipMemcpyAsync(a.dev.ptr+offTiles, a.pinned.ptr, bytes, hipMemcpyHostToDevice, a.stream));
    rc = launchLegacyCorrection(reinterpret_cast<float *>(a.dev.ptr+offTiles), reinterpret_cast<float *>(a.dev.ptr+offScratch), 1, w, h, channels, thresholdX, thresholdY,
                                a.stream);
    if (rc != MSDFHIP_OK)
        return rc;
    HIPCHK(hipMemcpyAsync(a.pinned.ptr, a.dev.ptr+offTiles, bytes, hipMemcpyDeviceToHost, a.stream));
    HIPCHK(hipStreamSynchronize(a.stream));
    for (int y = 0; y < h; ++y)
        memcpy(pixels+(ptrdiff_t) rowStride*y, a.pinned.ptr+rowBytes*y, rowBytes);
    return MSDFHIP_OK;
}

int msdfhip_generate_sdf(float *pixels, int w, int h, int rowStride, int flip, const int32_t *co, int nC, const double *points,
                         const uint8_t *types, const uint8_t *colors, const double *xf, const MsdfHipConfig *cfg) {
    return msdfhip_generate(MSDFHIP_MODE_SDF, pixels, w, h, rowStride, flip, co, nC, points, types, colors, xf, cfg, NULL);
}

int msdfhip_generate_psdf(float *pixels, int w, int h, int rowStride, int flip, const int32_t *co, int nC, const double *points,
                          const uint8_t *types, const uint8_t *colors, const double *xf, const MsdfHipConfig *cfg) {
    return msdfhip_generate(MSDFHIP_MODE_PSDF, pixels, w, h, rowStride, flip, co, nC, points, types, colors, xf, cfg, NULL);
}

int msdfhip_generate_msdf(float *pixels, int w, int h, int rowStride, int flip, const int32_t *co, int nC, const double *points,
                          const uint8_t *types, const uint8_t *colors, const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil) {
    return msdfhip_generate(MSDFHIP_MODE_MSDF, pixels, w, h, rowStride, flip, co, nC, points, types, colors, xf, cfg, stencil);
}

int msdfhip_generate_mtsdf(float *pixels, int w, int h, int rowStride, int flip, const int32_t *co, int nC, const double *points,
                           const uint8_t *types, const uint8_t *colors, const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil) {
    return msdfhip_generate(MSDFHIP_MODE_MTSDF, pixels, w, h, rowStride, flip, co, nC, points, types, colors, xf, cfg, stencil);
}

int msdfhip_error_correction(int channels, float *pixels, int w, int h, int rowStride, int flip, const int32_t *co, int nC, const double *points,
                             const uint8_t *types, const uint8_t *colors, const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil) {
    if (channels != 3 && channels != 4)
        return fail(MSDFHIP_ERR_INVALID, "channels %d (must be 3 or 4)", channels);
    return singleShape(channels, channels, OP_ERROR_CORRECTION, pixels, w, h, rowStride, flip, co, nC, points, types, colors, xf, cfg, stencil);
}

// msdfFastDistanceErrorCorrection / msdfFastEdgeErrorCorrection (core/msdf-error-correction.cpp:50-59, 87-113): findErrors(sdf) + apply with
// no shape -- no corner / edge protection, optionally protectAll() first. That is msdfErrorCorrectionInner on an empty shape with
// mode INDISCRIMINATE (nothing protected) or EDGE_ONLY (protectAll) and DO_NOT_CHECK_DISTANCE, so the same kernels run it.
int msdfhip_error_correction_shapeless(int channels, float *pixels, int w, int h, int rowStride, const double *xf, double minDeviationRatio, int protectAll) {
    if (channels != 3 && channels != 4)
        return fail(MSDFHIP_ERR_INVALID, "channels %d (must be 3 or 4)", channels);
    static const int32_t noContours[1] = { 0 };
    MsdfHipConfig cfg;
    msdfhip_default_config(&cfg);
    cfg.overlap_support = 0;
    cfg.ec_mode = protectAll ? MSDFHIP_EC_EDGE_ONLY : MSDFHIP_EC_INDISCRIMINATE;
    cfg.ec_distance_check = MSDFHIP_DO_NOT_CHECK_DISTANCE;
    cfg.min_deviation_ratio = minDeviationRatio;
    return singleShape(channels, channels, OP_ERROR_CORRECTION, pixels, w, h, rowStride, 0, noContours, 0, NULL, NULL, NULL, xf, &cfg, NULL);
}

int msdfhip_distance_sign_correction(int channels, float *pixels, int w, int h, int rowStride, int flip, const int32_t *co, int nC, const double *points,
                                     const uint8_t *types, const uint8_t *colors, const double *xf, float zero, int fillRule) {
    if (channels != 1 && channels != 3 && channels != 4)
        return fail(MSDFHIP_ERR_INVALID, "channels %d (must be 1, 3 or 4)", channels);
    if (fillRule < 0 || fillRule > 3)
        return fail(MSDFHIP_ERR_INVALID, "fill rule %d (must be 0..3)", fillRule);
    if (!xf)
        return fail(MSDFHIP_ERR_INVALID, "xf is NULL");
    MsdfHipConfig cfg;
    msdfhip_default_config(&cfg);
    cfg.sign_correction = 1, cfg.fill_rule = fillRule, cfg.sdf_zero_value = zero;
    const double xf6[6] = { xf[0], xf[1], xf[2], xf[3], 1., 0. };  // the distance mapping plays no role here
    return singleShape(channels, channels, OP_SIGN_CORRECTION, pixels, w, h, rowStride, flip, co, nC, points, types, colors, xf6, &cfg, NULL);
}

int msdfhip_set_microbatch(int maxGroup_, int maxLeaders) {
    if (maxGroup_ < 0 || maxLeaders < 1)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_set_microbatch(%d, %d)", maxGroup_, maxLeaders);
    gMaxGroup.store(maxGroup_ < 1 ? 1 : maxGroup_);
    gMaxLeaders.store(maxLeaders);
    return MSDFHIP_OK;
}

int msdfhip_microbatch_stats(long long *calls, long long *batches, long long *largest, int reset) {
    if (calls) *calls = gStatCalls.load();
    if (batches) *batches = gStatBatches.load();
    if (largest) *largest = gStatLargest.load();
    if (reset)
        gStatCalls = 0, gStatBatches = 0, gStatLargest = 0;
    return MSDFHIP_OK;
}

int msdfhip_microbatch_mixed_stats(long long *mixedBatches, long long *mixedCalls, long long *paddedTexels, long long *boxTexels, int reset) {
    if (mixedBatches) *mixedBatches = gStatMixedBatches.load();
    if (mixedCalls) *mixedCalls = gStatMixedCalls.load();
    if (paddedTexels) *paddedTexels = gStatPaddedTexels.load();
    if (boxTexels) *boxTexels = gStatBoxTexels.load();
    if (reset)
        gStatMixedBatches = 0, gStatMixedCalls = 0, gStatPaddedTexels = 0, gStatBoxTexels = 0;
    return MSDFHIP_OK;
}

// Host state only: no device is touched. hold_ms > 0: calls that arrive queue up and no new leader starts until the hold is released or hold_ms have passed
// (every waiting call bounds its own wait by the hold's end, so a hold nobody releases cannot park callers); running leaders finish. 0: release.
int msdfhip_microbatch_hold(int holdMs) {
    if (holdMs < 0)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_microbatch_hold(%d)", holdMs);
    std::unique_lock<std::mutex> lock(gQueueMutex);
    int unclaimed = 0;
    for (size_t i = 0; i < gQueue.size(); ++i)
        unclaimed += gQueue[i]->claimed ? 0 : 1;
    gHoldUntilNs = holdMs > 0 ? nowNs()+(long long) holdMs*1000000 : 0;
    if (holdMs == 0)
        if (ShapeCall *next = firstUnclaimed())
            next->cv.notify_one();
    return unclaimed;
}

int msdfhip_microbatch_times(double *stageMs, double *deviceMs, double *scatterMs, int reset) {
    if (stageMs) *stageMs = gNsStage.load()*1e-6;
    if (deviceMs) *deviceMs = gNsDevice.load()*1e-6;
    if (scatterMs) *scatterMs = gNsScatter.load()*1e-6;
    if (reset)
        gNsStage = 0, gNsDevice = 0, gNsScatter = 0;
    return MSDFHIP_OK;
}

int msdfhip_rasterize(float *pixels, int w, int h, int rowStride, int flip, const int32_t *co, int nC, const double *points,
                      const uint8_t *types, const uint8_t *colors, const double *xf, int fillRule) {
    if (fillRule < 0 || fillRule > 3)
        return fail(MSDFHIP_ERR_INVALID, "fill rule %d (must be 0..3)", fillRule);
    if (!xf)
        return fail(MSDFHIP_ERR_INVALID, "xf is NULL");
    MsdfHipConfig cfg;
    msdfhip_default_config(&cfg);
    cfg.fill_rule = fillRule;
    const double xf6[6] = { xf[0], xf[1], xf[2], xf[3], 1., 0. };
    return singleShape(1, 1, OP_RASTERIZE, pixels, w, h, rowStride, flip, co, nC, points, types, colors, xf6, &cfg, NULL);
}

int msdfhip_shape_distance(int selector, int overlap, const int32_t *co, int nC, const double *points, const uint8_t *types, const uint8_t *colors,
                           int nPoints, const double *pts, double *out) {
    if (selector < 1 || selector > 4 || nPoints < 0 || !co || !pts || !out)
        return fail(MSDFHIP_ERR_INVALID, "bad arguments");
    if (nPoints == 0)
        return MSDFHIP_OK;
    const int32_t gco[2] = { 0, nC };
    MsdfHipBatch *b = NULL;
    int rc = msdfhip_batch_create(&b, 1, gco, co, points, types, colors);
    if (rc != MSDFHIP_OK)
        return rc;
    const std::unique_ptr<MsdfHipBatch, void (*)(MsdfHipBatch *)> batch(b, msdfhip_batch_destroy);
    const int nch = channelsOf(selector);
    size_t lds = overlap ? (size_t) b->maxContours*nch*WAVE*sizeof(double) : 0;
    double *gres = NULL;
    size_t gresStride = 0;
    int chunkPoints = nPoints;
    if (lds > (size_t) gLdsLimit.load()) {                       // more contours than a CU's LDS holds scratch for: a global workspace slice per workgroup
        gresStride = lds/sizeof(double);
        size_t groups = (size_t) (nPoints+WAVE-1)/WAVE;
        if (groups*lds > ((size_t) 2<<30))                       // bounded workspace: the points go through in several launches
            groups = ((size_t) 2<<30)/lds > 0 ? ((size_t) 2<<30)/lds : 1;
        chunkPoints = (int) (groups*WAVE < (size_t) nPoints ? groups*WAVE : (size_t) nPoints);
        rc = ensureGres(b, groups*lds, &gres);
        if (rc != MSDFHIP_OK)
            return rc;
        lds = 0;
    }
    WorkBuffer<double> dPts, dOut;                               // (freed before the batch, on its device)
    hipError_t e = dPts.ensure(2*(size_t) nPoints);
    if (e == hipSuccess) e = dOut.ensure(4*(size_t) nPoints);
    if (e == hipSuccess) e = hipMemcpy(dPts.ptr, pts, sizeof(double)*2*(size_t) nPoints, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const dim3 block(WAVE);
        const BatchView v = viewOf(b);
        #define LAUNCH_SD(S, O) do { rc = setLds(k_shape_distance<S, O>, lds); \
            for (int base = 0; rc == MSDFHIP_OK && base < nPoints; base += chunkPoints) { \
                const int n = nPoints-base < chunkPoints ? nPoints-base : chunkPoints; \
                hipLaunchKernelGGL((k_shape_distance<S, O>), dim3((n+WAVE-1)/WAVE), block, lds, 0, v, n, dPts.ptr+2*(size_t) base, dOut.ptr+4*(size_t) base, gres, gresStride); \
            } } while (0)
        switch (selector*2+(overlap ? 1 : 0)) {
            case 2: LAUNCH_SD(1, false); break;
            case 3: LAUNCH_SD(1, true); break;
            case 4: LAUNCH_SD(2, false); break;
            case 5: LAUNCH_SD(2, true); break;
            case 6: LAUNCH_SD(3, false); break;
            case 7: LAUNCH_SD(3, true); break;
            case 8: LAUNCH_SD(4, false); break;
            default: LAUNCH_SD(4, true); break;
        }
        #undef LAUNCH_SD
        if (rc != MSDFHIP_OK)
            return rc;
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(NULL);
        if (e == hipSuccess) e = hipMemcpy(out, dOut.ptr, sizeof(double)*4*(size_t) nPoints, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess)
        return fail(MSDFHIP_ERR_HIP, "msdfhip_shape_distance: %s", hipGetErrorString(e));
    return MSDFHIP_OK;
}

// -------------------------------------------------------------------------------------------------------- timing hook

// The pools of the host-pointer entry points (one arena per concurrent single-shape call, one two-slot pipeline per concurrent host-output
// call: ~100-200 MB of device + pinned memory each) only ever grow to the PEAK concurrency. A long-lived process that is done with a
// burst returns them here; resources of calls in flight are not in the pools and stay untouched.
int msdfhip_trim(void) {
    gArenaPool.drain();
    gPipePool.drain();
    return MSDFHIP_OK;
}

// The devices the front door spreads over (MSDFHIP_DEVICES, parsed on first use): fills out[0..min(cap, n)-1], returns n (0 = default device only).
int msdfhip_front_door_devices(int *out, int cap) {
    (void) frontDoorDevice();
    std::lock_guard<std::mutex> lock(gFrontMutex);
    for (int i = 0; out && i < cap && i < (int) gFrontDevices.size(); ++i)
        out[i] = gFrontDevices[i];
    return (int) gFrontDevices.size();
}

int msdfhip_reload_tuning(void) {
    {
        std::lock_guard<std::mutex> lock(gTuningMutex);
        readTuning();
    }
    gMaxGroup.store(-1);
    {
        std::lock_guard<std::mutex> lock(gFrontMutex);
        gFrontParsed = false;
    }
    return MSDFHIP_OK;
}

// Where the time of the fused single-shape launches went (k_single_call stamps workgroup 0's phase boundaries with the 100 MHz realtime counter):
// out[0] calls, out[1..6] microseconds per call of workgroup 0's digest | distance tile | wait for all tiles | correction sweep | wait for all sweeps |
// distance checks, out[7] start of workgroup 0 -> last workgroup finished.
int msdfhip_single_call_fallbacks(unsigned long long *barrier_timeouts, unsigned long long *lost_flags, unsigned long long *refused, int reset) {
    if (barrier_timeouts)
        *barrier_timeouts = gSingleTimeouts.load();
    if (lost_flags)
        *lost_flags = gSingleLost.load();
    if (refused)
        *refused = gSingleRefused.load();
    if (reset)
        gSingleTimeouts.store(0), gSingleLost.store(0), gSingleRefused.store(0);
    return MSDFHIP_OK;
}

int msdfhip_debug_route_counts(unsigned long long *out, int cap, int reset) {
    int n = 0;
    for (; out && n < cap && n < MSDFHIP_ROUTE_COUNT; ++n)
        out[n] = gRouteCounts[n].load(std::memory_order_relaxed);
    if (reset)
        for (int k = 0; k < MSDFHIP_ROUTE_COUNT; ++k)
            gRouteCounts[k].store(0, std::memory_order_relaxed);
    return n;
}

int msdfhip_debug_single_call_phases(double *out8, int reset) {
    if (!out8)
        return fail(MSDFHIP_ERR_INVALID, "NULL argument");
    const unsigned long long calls = gSingleCalls.load();
    unsigned long long v[8];
    for (int k = 0; k < 8; ++k)
        v[k] = gSinglePhase[k].load();
    // stamps are 32-bit counter values summed over the calls: differences of the sums are sums of the differences (mod 2^32 per call is harmless for
    // sub-second intervals as long as few calls straddle a wrap: 43 s apart)
    out8[0] = (double) calls;
    const double per = calls ? 0.01/(double) calls : 0.;         // 10 ns units -> us per call
    out8[1] = (double) (long long) (v[1]-v[0])*per, out8[2] = (double) (long long) (v[2]-v[1])*per, out8[3] = (double) (long long) (v[3]-v[2])*per;
    out8[4] = (double) (long long) (v[4]-v[3])*per, out8[5] = (double) (long long) (v[5]-v[4])*per, out8[6] = (double) (long long) (v[6]-v[5])*per;
    out8[7] = (double) (long long) (v[7]-v[0])*per;
    if ((long long) (v[6]-v[0]) > 0)                             // shader clock in MHz during the launches, encoded into the fraction of out8[0] would be obscure:
        out8[0] = (double) calls+1e-6*((double) gSingleCycles.load()/((double) (long long) (v[6]-v[0])*0.01));   // calls + MHz * 1e-6
    if (reset) {
        gSingleCycles.store(0);
        gSingleCalls.store(0);
        for (int k = 0; k < 8; ++k)
            gSinglePhase[k].store(0);
    }
    return MSDFHIP_OK;
}

int msdfhip_set_kernel_timing(int enable) {
    gTiming.store(enable ? 1 : 0);
    return MSDFHIP_OK;
}

int msdfhip_kernel_timing(double *avgDistance, double *avgCorrection, int *launches, int reset) {
    std::lock_guard<std::mutex> lock(gTimingMutex);
    double sum[3] = { 0, 0, 0 };                                 // 0 distance, 1 error correction, 2 sign correction
    int cnt[3] = { 0, 0, 0 };
    for (size_t i = 0; i < gTimed.size(); ++i) {
        float ms = 0;
        if (hipEventSynchronize(gTimed[i].b) == hipSuccess && hipEventElapsedTime(&ms, gTimed[i].a, gTimed[i].b) == hipSuccess) {
            sum[gTimed[i].kind] += ms;
            ++cnt[gTimed[i].kind];
        }
    }
    if (avgDistance) *avgDistance = cnt[0] ? sum[0]/cnt[0] : 0;
    if (avgCorrection) *avgCorrection = cnt[1] ? (sum[1]+sum[2])/cnt[1] : cnt[2] ? sum[2]/cnt[2] : 0;   // everything after the distance kernel
    if (launches) *launches = cnt[0];
    if (reset) {
        for (size_t i = 0; i < gTimed.size(); ++i) {
            hipEventDestroy(gTimed[i].a);
            hipEventDestroy(gTimed[i].b);
        }
        gTimed.clear();
    }
    return MSDFHIP_OK;
}

} // extern "C"

// The tables of the measurement builds (msdf_measure.hpp: their readers, which hand out zeros / 0 counters in a regular build).
extern "C" int msdfhip_debug_bbcount(unsigned *out, int cap, int reset) {
    int n = 0;
    HIPCHK(msdfhip::readBbcount(out, cap, reset, n));
    return n;
}

extern "C" int msdfhip_debug_wait_profile(unsigned long long *out24, int reset) {
    HIPCHK(msdfhip::readWaitProfile(out24, reset));
    return MSDFHIP_OK;
}

// ---- per-glyph box sizes: msdfhip_batch_generate_sized, msdfhip_tiles_to_bytes_sized ---------------------------------------------------------------
//
// The launch chain is that of a uniform call at W x H = the batch's largest box (msdf_sizedplan.hpp): runGenerate with GenerateCall::boxDims set plans with the
// same planners, takes the same routes and counts them in the same counters; where it would launch a kernel, launchTwinned launches the kernel's sized twin from the
// same argument list. It gets the twin from one of the functions below, by the sibling's template arguments as plain integers. They are the ONLY code that names the
// twins and they come last in this file, so that the twins are instantiated behind every kernel the code object has always held. Their return types are derived from
// the siblings' (sizedTwinOf), so a twin whose signature drifts does not compile here either.

namespace {

decltype(sizedTwinOf(k_distance<1, false, false, 1>)) distanceSizedKernel(int sel, bool overlap, bool gres, int tpw) {
    // (the five variants of forDistanceVariant per selector. Not written with it: the nested conditional instantiates the overlapping three in an order
    // of its own, which is the order the code object holds them in.)
#define MSDF_SIZED_VARIANTS(SEL) \
    case SEL: return !overlap ? (gres ? k_distance_sized<SEL, false, true, 1> : k_distance_sized<SEL, false, false, (int) QUAD>) \
                     : gres ? k_distance_sized<SEL, true, true, 1> : tpw != 1 ? k_distance_sized<SEL, true, false, (int) QUAD> : k_distance_sized<SEL, true, false, 1>;
    switch (sel) {
        MSDF_SIZED_VARIANTS(1)
        MSDF_SIZED_VARIANTS(2)
        MSDF_SIZED_VARIANTS(3)
        MSDF_SIZED_VARIANTS(4)
    }
#undef MSDF_SIZED_VARIANTS
    return NULL;
}
decltype(sizedTwinOf(k_distance_unculled<1, false>)) unculledSizedKernel(int sel, bool overlap) {
    decltype(unculledSizedKernel(sel, overlap)) twin = NULL;
    forOneOf<1, 2, 3, 4>(sel, [&](auto s) { twin = overlap ? k_distance_unculled_sized<decltype(s)::value, true> : k_distance_unculled_sized<decltype(s)::value, false>; });
    return twin;
}
decltype(sizedTwinOf(k_ec_slow<3, false, false>)) ecSlowSizedKernel(int n, bool overlap, bool gres) {      // (the three of dispatchEc per channel count)
    decltype(ecSlowSizedKernel(n, overlap, gres)) twin = NULL;
    forOneOf<3, 4>(n, [&](auto c) {
        enum { N = decltype(c)::value };
        twin = !overlap ? k_ec_slow_sized<N, false, false> : gres ? k_ec_slow_sized<N, true, true> : k_ec_slow_sized<N, true, false>;
    });
    return twin;
}
decltype(sizedTwinOf(k_ec_fast<3, false>)) ecFastSizedKernel(int n, bool lazy) {
    decltype(ecFastSizedKernel(n, lazy)) twin = NULL;
    forOneOf<3, 4>(n, [&](auto c) { twin = lazy ? k_ec_fast_sized<decltype(c)::value, true> : k_ec_fast_sized<decltype(c)::value, false>; });
    return twin;
}
decltype(sizedTwinOf(k_ec_query<3, false>)) ecQuerySizedKernel(int n, bool overlap) {
    decltype(ecQuerySizedKernel(n, overlap)) twin = NULL;
    forOneOf<3, 4>(n, [&](auto c) { twin = overlap ? k_ec_query_sized<decltype(c)::value, true> : k_ec_query_sized<decltype(c)::value, false>; });
    return twin;
}
decltype(sizedTwinOf(k_sign_correction<1>)) signSizedKernel(int n) {
    return n == 1 ? k_sign_correction_sized<1> : n == 3 ? k_sign_correction_sized<3> : k_sign_correction_sized<4>;   // (likewise: instantiated as 3, 4, 1)
}

// The sizes of a sized call, validated (msdf_sizedplan.hpp). No device call.
int checkSizes(const char *who, int nGlyphs, const int32_t *sizes, SizedLayout &layout) {
    switch (sizedLayout(nGlyphs, sizes, layout)) {
        case SIZED_NO_SIZES: return fail(MSDFHIP_ERR_INVALID, "%s: sizes is NULL", who);
        case SIZED_BAD_BOX: return fail(MSDFHIP_ERR_INVALID, "%s: glyph %d has a %d x %d box (each side must be at least 1)", who, layout.badGlyph, (int) sizes[2*(size_t) layout.badGlyph],
                                        (int) sizes[2*(size_t) layout.badGlyph+1]);
        case SIZED_TOO_MANY_TEXELS: return fail(MSDFHIP_ERR_INVALID, "%s: %d slots of %d x %d texels exceed the 32-bit texel index; split the batch", who, nGlyphs, layout.W, layout.H);
    }
    return MSDFHIP_OK;
}

// The device copy of n (w, h) pairs in the workspace of `ws`, uploaded from its pinned host copy on `stream`: ordered in front of whatever the caller
// launches on that stream next. (The device copy is shared by the calls on one batch like every other work buffer: they are ordered by the caller.)
int uploadBoxDims(Workspace &ws, int n, const int32_t *sizes, hipStream_t stream, const int32_t **out) {
    std::lock_guard<std::mutex> lock(ws.mutex);
    const size_t ints = 2*ws.glyphCapacity(n);
    if (ws.boxDimsRead && ws.hBoxDims.ptr)                       // the previous call's upload has read the pinned copy before it is rewritten
        HIPCHK(hipEventSynchronize(ws.boxDimsRead));
    HIPCHK(ws.boxDims.ensure(ints));
    HIPCHK(ws.hBoxDims.ensure(ints));
    memcpy(ws.hBoxDims.ptr, sizes, sizeof(int32_t)*2*(size_t) n);
    const int rc = uploadSmall(ws.boxDims.ptr, ws.hBoxDims.ptr, sizeof(int32_t)*2*(size_t) n, stream);
    if (rc != MSDFHIP_OK)
        return rc;
    if (!ws.boxDimsRead)
        HIPCHK(ws.boxDimsRead.create(hipEventDisableTiming));
    HIPCHK(hipEventRecord(ws.boxDimsRead, stream));
    *out = ws.boxDims.ptr;
    return MSDFHIP_OK;
}

} // namespace

extern "C" {

int msdfhip_batch_generate_sized(const MsdfHipBatch *b, int mode, const int32_t *sizes, const MsdfHipGlyph *dGlyphs, float *dOut, uint8_t *dStencil, float *dScratch,
                                 const MsdfHipConfig *cfg, void *streamPtr) {
    if (!b || mode < 1 || mode > 4 || !dGlyphs || !dOut)
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_batch_generate_sized");
    SizedLayout layout;
    int rc = checkSizes("msdfhip_batch_generate_sized", b->nGlyphs, sizes, layout);
    if (rc != MSDFHIP_OK)
        return rc;
    rc = checkConfig(cfg);
    if (rc != MSDFHIP_OK)
        return rc;
    if (b->nGlyphs == 0)
        return MSDFHIP_OK;
    rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    GenerateCall call;
    rc = uploadBoxDims(b->work, b->nGlyphs, sizes, (hipStream_t) streamPtr, &call.boxDims);
    if (rc != MSDFHIP_OK)
        return rc;
    return runGenerate(b, mode, layout.W, layout.H, dGlyphs, dOut, dStencil, dScratch, cfg, (hipStream_t) streamPtr, call);
}

int msdfhip_tiles_to_bytes_sized(const float *dTiles, int nGlyphs, const int32_t *sizes, const int64_t *tileOffsets, int channels, const MsdfHipGlyph *dGlyphs, uint8_t *dAtlas,
                                 void *streamPtr) {
    if (nGlyphs < 0 || (channels != 1 && channels != 3 && channels != 4))
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_tiles_to_bytes_sized");
    SizedLayout layout;
    int rc = checkSizes("msdfhip_tiles_to_bytes_sized", nGlyphs, sizes, layout);
    if (rc != MSDFHIP_OK)
        return rc;
    if (nGlyphs == 0)
        return MSDFHIP_OK;
    if (!dTiles || !tileOffsets || !dGlyphs || !dAtlas)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_tiles_to_bytes_sized: NULL argument");
    rc = ensureDeviceOf(dTiles);
    if (rc != MSDFHIP_OK)
        return rc;
    hipStream_t stream = (hipStream_t) streamPtr;
    // The two host arrays go to a device buffer of this call (sizes, then offsets), freed once the conversion has run: no batch whose workspace could hold them.
    WorkBuffer<long long> dMeta;
    HIPCHK(dMeta.ensure(2*(size_t) nGlyphs));
    std::vector<long long> meta(2*(size_t) nGlyphs);
    memcpy(meta.data(), sizes, sizeof(int32_t)*2*(size_t) nGlyphs);
    for (int g = 0; g < nGlyphs; ++g)
        meta[(size_t) nGlyphs+g] = (long long) tileOffsets[g];
    HIPCHK(hipMemcpyAsync(dMeta.ptr, meta.data(), sizeof(long long)*meta.size(), hipMemcpyHostToDevice, stream));
    const unsigned gx = (unsigned) ((layout.slot+255)/256 < 64 ? (layout.slot+255)/256 : 64), gy = (unsigned) (nGlyphs < 65535 ? nGlyphs : 65535);
    const int32_t *dDims = reinterpret_cast<const int32_t *>(dMeta.ptr);
    const long long *dOffsets = dMeta.ptr+nGlyphs;
    forOneOf<1, 3, 4>(channels, [&](auto n) {
        hipLaunchKernelGGL(k_tiles_to_bytes_sized<decltype(n)::value>, dim3(gx, gy), dim3(256), 0, stream, dTiles, dGlyphs, nGlyphs, dDims, dOffsets, dAtlas);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));                        // (the staging vector and the device buffer of this call go with it)
    return MSDFHIP_OK;
}

} // extern "C"

// ---- box sizes on the device: msdfhip_batch_bounds_miters, msdfhip_batch_boxes ----------------------------------------------------------------------
//
// One k_box launch (msdf_frame.hpp) and one copy back. The ONLY code that names k_box, behind the sized twins: it is instantiated last (forDistanceVariant).

namespace {

// k_box over the batch on the NULL stream into b->dBoxes, read back into `host` ([n][4] ext, [n][6] xf, [n][2] int32 wh; the last two only with `box`).
// Synchronous. The plain bounds land in b->dBounds on the way, as msdfhip_batch_bounds leaves them.
int runBoxes(const MsdfHipBatch *b, double border, double miterLimit, int polarity, const BoxParams *box, std::vector<double> &host) {
    const size_t n = (size_t) b->nGlyphs;
    HIPCHK(hipDeviceSynchronize());                              // (the edge arrays may still be written by work the caller queued)
    HIPCHK(b->dBounds.ensure(4*n));
    HIPCHK(b->dBoxes.ensure(11*n));
    const EdgeArrays edges = { b->dPoints.ptr, b->dTypes.ptr, b->dColors.ptr };
    double *ext = b->dBoxes.ptr, *xf = ext+4*n;
    int32_t *wh = reinterpret_cast<int32_t *>(xf+6*n);
    const BoxParams none = { 1., 0., 1., 0, 0 };
    if (box)
        hipLaunchKernelGGL(k_box<true>, dim3((unsigned) n), dim3(WAVE), 0, (hipStream_t) NULL, edges, b->dGlyphContourOffsets.ptr, b->dContourOffsets.ptr, b->nGlyphs, b->dBounds.ptr,
                           b->boundsFixed ? 1 : 0, border, miterLimit, polarity, *box, ext, wh, xf);
    else
        hipLaunchKernelGGL(k_box<false>, dim3((unsigned) n), dim3(WAVE), 0, (hipStream_t) NULL, edges, b->dGlyphContourOffsets.ptr, b->dContourOffsets.ptr, b->nGlyphs, b->dBounds.ptr,
                           b->boundsFixed ? 1 : 0, border, miterLimit, polarity, none, ext, (int32_t *) NULL, (double *) NULL);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(NULL));
    host.resize(11*n);
    HIPCHK(hipMemcpy(host.data(), b->dBoxes.ptr, sizeof(double)*(box ? 11 : 4)*n, hipMemcpyDeviceToHost));   // (in stream order behind the kernel)
    return MSDFHIP_OK;
}

} // namespace

extern "C" {

int msdfhip_batch_bounds_miters(const MsdfHipBatch *b, double border, double miterLimit, int polarity, double *bounds) {
    if (!b || !bounds)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_bounds_miters: NULL argument");
    if (b->nGlyphs == 0)
        return MSDFHIP_OK;
    int rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    std::vector<double> host;
    rc = runBoxes(b, border, miterLimit, polarity, NULL, host);
    if (rc != MSDFHIP_OK)
        return rc;
    memcpy(bounds, host.data(), sizeof(double)*4*(size_t) b->nGlyphs);
    return MSDFHIP_OK;
}

int msdfhip_batch_boxes(const MsdfHipBatch *b, const MsdfHipBoxConfig *cfg, int32_t *sizes, double *xf, double *bounds) {
    BoxParams box;
    double border = 0;
    int rc = checkBoxConfig(cfg, "msdfhip_batch_boxes", &box, &border);
    if (rc != MSDFHIP_OK)
        return rc;
    if (!b || !sizes || !xf)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_boxes: NULL argument");
    if (b->nGlyphs == 0)
        return MSDFHIP_OK;
    rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    std::vector<double> host;
    rc = runBoxes(b, border, cfg->miter_limit, cfg->polarity, &box, host);
    if (rc != MSDFHIP_OK)
        return rc;
    const size_t n = (size_t) b->nGlyphs;
    const int32_t *wh = reinterpret_cast<const int32_t *>(host.data()+10*n);
    for (size_t k = 0; k < 2*n; ++k)
        if (wh[k] < 0)
            return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_boxes: the box of glyph %zu is not a number or has a side beyond %d texels at scale %g", k/2, (int) BOX_MAX_SIDE, cfg->scale);
    memcpy(sizes, wh, sizeof(int32_t)*2*n);
    memcpy(xf, host.data()+4*n, sizeof(double)*6*n);
    if (bounds)
        memcpy(bounds, host.data(), sizeof(double)*4*n);
    return MSDFHIP_OK;
}

} // extern "C"

// ---- quality calls for boxes: msdfhip_batch_estimate_sdf_error_sized, msdfhip_render_sdf_sized -----------------------------------------------------
//
// The launches are those of the uniform calls (runEstimate, launchRender) with the twins in the kernels' places. The ONLY code that names the twins, behind k_box:
// they are instantiated last. What the launches depend on -- the item and texel prefixes, their refusals, the chunks, the range mapping per glyph -- is host code
// of msdf_qualityplan.hpp.

namespace {

decltype(sizedTwinOf(k_sdf_error_lines<1>)) errorLinesSizedKernel(int n) {
    return n == 1 ? k_sdf_error_lines_sized<1> : n == 3 ? k_sdf_error_lines_sized<3> : k_sdf_error_lines_sized<4>;
}
decltype(sizedTwinOf(k_sdf_error_sum)) errorSumSizedKernel() { return k_sdf_error_sum_sized<>; }
decltype(sizedTwinOf(k_render_sdf<1, 1>)) renderSizedKernel(int no, int ns) {
    return no == 1 ? (ns == 1 ? k_render_sdf_sized<1, 1> : ns == 3 ? k_render_sdf_sized<1, 3> : k_render_sdf_sized<1, 4>)
         : no == 3 ? (ns == 1 ? k_render_sdf_sized<3, 1> : k_render_sdf_sized<3, 3>) : k_render_sdf_sized<4, 4>;
}

} // namespace

extern "C" {

int msdfhip_batch_estimate_sdf_error_sized(const MsdfHipBatch *b, int channels, const int32_t *sizes, const int64_t *tileOffsets, const MsdfHipGlyph *dGlyphs,
                                           const float *dTiles, int scanlinesPerRow, int fillRule, double *dErrors, void *streamPtr) {
    if (!b || (channels != 1 && channels != 3 && channels != 4))
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_batch_estimate_sdf_error_sized");
    if (fillRule < 0 || fillRule > 3)
        return fail(MSDFHIP_ERR_INVALID, "fill rule %d (must be 0..3)", fillRule);
    SizedLayout layout;
    int rc = checkSizes("msdfhip_batch_estimate_sdf_error_sized", b->nGlyphs, sizes, layout);
    if (rc != MSDFHIP_OK)
        return rc;
    if (b->nGlyphs == 0)
        return MSDFHIP_OK;
    if (!tileOffsets || !dGlyphs || !dTiles || !dErrors)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_estimate_sdf_error_sized: NULL argument");
    // The device table of k_sdf_error_lines_sized, in 8-byte words: the sizes | the item prefix | the tile offsets.
    const size_t n = (size_t) b->nGlyphs;
    std::vector<int64_t> table(3*n+1);
    size_t items = 0;
    if (scanlinesPerRow >= 1) {
        if (errorItemPrefix(b->nGlyphs, sizes, scanlinesPerRow, table.data()+n) != QUALITY_OK)
            return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_estimate_sdf_error_sized: more than 2^48 scanlines; split the batch");
        items = (size_t) table[2*n];
    }
    rc = ensureDevice(b->device);
    if (rc != MSDFHIP_OK)
        return rc;
    hipStream_t stream = (hipStream_t) streamPtr;
    if (!items) {                                                    // sdf-error-estimation.cpp:136-137: every estimate is 0
        HIPCHK(hipMemsetAsync(dErrors, 0, sizeof(double)*n, stream));
        return MSDFHIP_OK;
    }
    memcpy(table.data(), sizes, sizeof(int32_t)*2*n);
    for (size_t g = 0; g < n; ++g)
        table[2*n+1+g] = tileOffsets[g];
    rc = runEstimate(b, channels, layout.W, layout.H, dGlyphs, dTiles, scanlinesPerRow, fillRule, dErrors, stream, items, &table);
    if (rc != MSDFHIP_OK)
        return rc;
    HIPCHK(hipStreamSynchronize(stream));                            // (the host table has been read, and the device copy in the batch's workspace is done with)
    return MSDFHIP_OK;
}

int msdfhip_render_sdf_sized(const float *dSdf, int nGlyphs, const int32_t *sdfSizes, const int64_t *sdfOffsets, int ns, float *dOut, const int32_t *outSizes,
                             const int64_t *outOffsets, int no, double rangeLower, double rangeUpper, float sdThreshold, void *streamPtr) {
    if (nGlyphs < 0)
        return fail(MSDFHIP_ERR_INVALID, "bad arguments to msdfhip_render_sdf_sized");
    if (!renderChannelsOk(no, ns))
        return fail(MSDFHIP_ERR_INVALID, "renderSDF has no overload for %d <- %d channels (core/render-sdf.h:12-17)", no, ns);
    SizedLayout layout;
    int rc = checkSizes("msdfhip_render_sdf_sized", nGlyphs, sdfSizes, layout);
    if (rc != MSDFHIP_OK)
        return rc;
    if (nGlyphs == 0)
        return MSDFHIP_OK;
    if (!outSizes)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_render_sdf_sized: out_sizes is NULL");
    // The device table of k_render_sdf_sized, in 8-byte words: field sizes | output sizes | the output texel prefix | field offsets | output offsets | the mappings.
    const size_t n = (size_t) nGlyphs;
    std::vector<int64_t> table(9*n+1);
    int bad = -1;
    switch (renderTexelPrefix(nGlyphs, outSizes, table.data()+2*n, &bad)) {
        case QUALITY_BAD_OUTPUT: return fail(MSDFHIP_ERR_INVALID, "msdfhip_render_sdf_sized: glyph %d has a %d x %d output (a side may be 0, not negative)", bad, (int) outSizes[2*(size_t) bad],
                                             (int) outSizes[2*(size_t) bad+1]);
        case QUALITY_TOO_MANY: return fail(MSDFHIP_ERR_INVALID, "msdfhip_render_sdf_sized: more than 2^48 output texels; split the batch");
    }
    const size_t total = (size_t) table[3*n];
    if (!total)
        return MSDFHIP_OK;
    if (!dSdf || !dOut || !sdfOffsets || !outOffsets)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_render_sdf_sized: NULL argument");
    rc = ensureDeviceOf(dSdf);
    if (rc != MSDFHIP_OK)
        return rc;
    memcpy(table.data(), sdfSizes, sizeof(int32_t)*2*n);
    memcpy(table.data()+n, outSizes, sizeof(int32_t)*2*n);
    double *params = reinterpret_cast<double *>(table.data()+5*n+1);
    for (size_t g = 0; g < n; ++g) {
        table[3*n+1+g] = sdfOffsets[g], table[4*n+1+g] = outOffsets[g];
        const int ow = outSizes[2*g], oh = outSizes[2*g+1];
        if (ow > 0 && oh > 0) {
            const RenderMapping m = renderMapping(sdfSizes[2*g], sdfSizes[2*g+1], ow, oh, rangeLower, rangeUpper);
            params[4*g] = m.scaleX, params[4*g+1] = m.scaleY, params[4*g+2] = m.mapScale, params[4*g+3] = m.mapTranslate;
        }
    }
    hipStream_t stream = (hipStream_t) streamPtr;
    // The table goes to a device buffer of this call, freed once the rendering has run: no batch whose workspace could hold it.
    WorkBuffer<long long> dTable;
    HIPCHK(dTable.ensure(table.size()));
    HIPCHK(hipMemcpyAsync(dTable.ptr, table.data(), sizeof(int64_t)*table.size(), hipMemcpyHostToDevice, stream));
    const RenderMapping none = { 0, 0, 0, 0 };
    rc = launchRender(no, ns, reinterpret_cast<const int32_t *>(dTable.ptr), total, stream, dSdf, nGlyphs, 0, 0, dOut, 0, 0, none, rangeLower == rangeUpper, sdThreshold);
    if (rc != MSDFHIP_OK)
        return rc;
    HIPCHK(hipStreamSynchronize(stream));                            // (the host table and the device buffer of this call go with it)
    return MSDFHIP_OK;
}

} // extern "C"

// ---- a new batch out of glyphs of resident ones: msdfhip_batch_gather ----------------------------------------------------------------------------------
//
// The plan is host code of msdf_gatherplan.hpp; the copies are the three kernels of msdf_gather.hpp, templates that ONLY this code names, behind the quality
// twins: they are instantiated last. Records and windings come from digest(), like every new batch's.

namespace {

int failGather(int code, const GatherRefusal &bad) {
    switch (code) {
        case GATHER_NO_SOURCES: return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: no sources (n_sources must be at least 1)");
        case GATHER_BAD_COUNT: return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: n_glyphs is negative");
        case GATHER_NO_INDICES: return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: indices is NULL");
        case GATHER_NO_SOURCE_OF: return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: source_of is NULL with more than one source");
        case GATHER_BAD_SOURCE: return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: source_of[%d] = %lld is outside 0..%d", bad.position, bad.value, bad.limit-1);
        case GATHER_BAD_INDEX: return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: indices[%d] = %lld is outside its source's %d glyphs", bad.position, bad.value, bad.limit);
        case GATHER_MIXED_DEVICES: return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: sources[%d] lives on device %lld, sources[0] on device %d", bad.position, bad.value, bad.limit);
        case GATHER_TOO_MANY_CONTOURS: return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: %lld contours up to indices[%d] exceed INT32_MAX; split the selection", bad.value, bad.position);
        case GATHER_TOO_MANY_EDGES: return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: %lld edges up to indices[%d] exceed INT32_MAX; split the selection", bad.value, bad.position);
    }
    return MSDFHIP_OK;
}

// Everything of the call behind its checks, on the new batch b (destroyed by the caller on failure).
int runGather(MsdfHipBatch *b, const MsdfHipBatch *const *sources, const std::vector<GatherSource> &src, int n, const int32_t *sourceOf, const int32_t *indices,
              const GatherTotals &totals, hipStream_t stream) {
    const int nSources = (int) src.size();
    b->nGlyphs = n, b->nContours = (int) totals.contours, b->nEdges = (int) totals.edges;
    b->maxContours = totals.maxContours, b->maxEdges = totals.maxEdges;
    b->hContours.resize((size_t) n), b->hEdges.resize((size_t) n);
    bool fixed = false;
    for (int s = 0; s < nSources; ++s)
        fixed = fixed || sources[s]->boundsFixed;
    // the table: the plan's int32 block, then one row of pointers per source
    const GatherColumns col = gatherColumns(n);
    const size_t tableInts = col.ints+sizeof(GatherSourceArrays)/sizeof(int32_t)*(size_t) nSources;
    const size_t eAlloc = b->nEdges > 0 ? (size_t) b->nEdges : 1;
    HIPCHK(b->hGatherTable.ensure(tableInts));
    HIPCHK(b->gatherTable.ensure(tableInts));
    HIPCHK(b->dGlyphContourOffsets.ensure((size_t) n+1));
    HIPCHK(b->dContourOffsets.ensure((size_t) b->nContours+1));
    HIPCHK(b->dPoints.ensure(8*eAlloc));
    HIPCHK(b->dTypes.ensure(eAlloc));
    HIPCHK(b->dColors.ensure(eAlloc));
    if (fixed)
        HIPCHK(b->dBounds.ensure(4*(size_t) (n > 0 ? n : 1)));
    gatherFill(src.data(), nSources, n, sourceOf, indices, b->hGatherTable.ptr, b->hContours.data(), b->hEdges.data());
    GatherSourceArrays *rows = reinterpret_cast<GatherSourceArrays *>(b->hGatherTable.ptr+col.ints);
    for (int s = 0; s < nSources; ++s) {
        const MsdfHipBatch *from = sources[s];
        if (fixed && !from->boundsFixed) {                       // its bounds as msdfhip_batch_bounds would compute them, on the call's stream
            const int rc = frameBatch(from, NULL, 0, 0, NULL, stream);
            if (rc != MSDFHIP_OK)
                return rc;
        }
        const GatherSourceArrays row = { from->dContourOffsets.ptr, from->dPoints.ptr, from->dTypes.ptr, from->dColors.ptr, fixed ? from->dBounds.ptr : NULL };
        rows[s] = row;
    }
    // glyph_contour_offsets IS the plan's first column; the rest of the block goes to the table
    int rc = uploadSmall(b->dGlyphContourOffsets.ptr, b->hGatherTable.ptr+col.dstContour0, sizeof(int32_t)*((size_t) n+1), stream);
    if (rc == MSDFHIP_OK)
        rc = uploadSmall(b->gatherTable.ptr+col.source, b->hGatherTable.ptr+col.source, sizeof(int32_t)*(tableInts-col.source), stream);
    if (rc != MSDFHIP_OK)
        return rc;
    const int32_t *t = b->gatherTable.ptr;
    const GatherSourceArrays *dRows = reinterpret_cast<const GatherSourceArrays *>(t+col.ints);
    hipLaunchKernelGGL(k_gather_contours<>, dim3((unsigned) (((size_t) b->nContours+1+255)/256)), dim3(256), 0, stream, b->dContourOffsets.ptr, n, b->nContours, b->nEdges,
                       t+col.source, t+col.srcContour0, t+col.srcEdge0, (const int32_t *) b->dGlyphContourOffsets.ptr, t+col.dstEdge0, dRows);
    if (b->nEdges > 0)
        hipLaunchKernelGGL(k_gather_edges<>, dim3((unsigned) ((4*(size_t) b->nEdges+255)/256)), dim3(256), 0, stream, b->dPoints.ptr, b->dTypes.ptr, b->dColors.ptr, n, b->nEdges,
                           t+col.source, t+col.srcEdge0, t+col.dstEdge0, dRows);
    if (fixed && n > 0)
        hipLaunchKernelGGL(k_gather_bounds<>, dim3((unsigned) ((2*(size_t) n+255)/256)), dim3(256), 0, stream, b->dBounds.ptr, n, t+col.source, t+col.srcGlyph, dRows);
    HIPCHK(hipGetLastError());
    b->boundsFixed = fixed;
    return digest(b, stream);
}

} // namespace

extern "C" int msdfhip_batch_gather(MsdfHipBatch **batch, const MsdfHipBatch *const *sources, int n_sources, int n_glyphs, const int32_t *source_of,
                                    const int32_t *indices, void *stream) {
    if (!batch)
        return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: batch is NULL");
    GatherRefusal bad = { -1, 0, 0 };
    int code = gatherCheckCounts(sources != NULL, n_sources, n_glyphs, source_of, indices);
    if (code != GATHER_OK)
        return failGather(code, bad);
    std::vector<GatherSource> src((size_t) n_sources);
    for (int s = 0; s < n_sources; ++s)
        if (!sources[s])
            return fail(MSDFHIP_ERR_INVALID, "msdfhip_batch_gather: sources[%d] is NULL", s);
    for (int s = 0; s < n_sources; ++s) {
        const GatherSource one = { sources[s]->nGlyphs, sources[s]->device, NULL, NULL };
        src[(size_t) s] = one;
    }
    code = gatherCheckArgs(src.data(), n_sources, n_glyphs, source_of, indices, bad);
    if (code != GATHER_OK)
        return failGather(code, bad);
    int rc = ensureDevice(sources[0]->device);
    if (rc != MSDFHIP_OK)
        return rc;
    for (int s = 0; s < n_sources; ++s) {
        rc = fetchGlyphCounts(sources[s]);                       // (batches of device arrays: read back once, the first time anybody needs them)
        if (rc != MSDFHIP_OK)
            return rc;
        src[(size_t) s].contours = sources[s]->hContours.data(), src[(size_t) s].edges = sources[s]->hEdges.data();
    }
    GatherTotals totals;
    code = gatherTotals(src.data(), n_glyphs, source_of, indices, totals, bad);
    if (code != GATHER_OK)
        return failGather(code, bad);
    MsdfHipBatch *b = new MsdfHipBatch();
    b->onDevice(currentDevice());
    rc = runGather(b, sources, src, n_glyphs, source_of, indices, totals, (hipStream_t) stream);
    if (rc != MSDFHIP_OK) {
        msdfhip_batch_destroy(b);
        return rc;
    }
    *batch = b;
    return MSDFHIP_OK;
}

// ---- groups of single-shape calls of different sizes: the packed bitmaps of an in-place operation into slots ------------------------------------------
//
// The ONLY code that names k_boxes_to_slots (msdf_boxslots.hpp), behind the gather kernels: it is instantiated last. runBatched calls it for a mixed group of
// msdfhip_error_correction / msdfhip_distance_sign_correction calls, whose sized passes read box g's source field at the start of slot g.

static int launchBoxesToSlots(float *dSlots, const float *dPacked, const MsdfHipGlyph *dGlyphs, const int32_t *dDims, int n, int channels, size_t slot, hipStream_t stream) {
    const size_t slotFloats = slot*(size_t) channels, chunks = (slotFloats+3)/4;
    hipLaunchKernelGGL(k_boxes_to_slots<>, dim3((unsigned) ((chunks+255)/256), (unsigned) n), dim3(256), 0, stream, dSlots, dPacked, dGlyphs, dDims, (long long) slotFloats, channels);
    HIPCHK(hipGetLastError());
    return MSDFHIP_OK;
}
