// msdf_measure.hpp -- the measurement builds of the kernels: their device tables, the hooks the kernels call, the host-side readers.
//   -DMSDF_PROFILE_WAITS       where a k_distance wavefront's cycles go: s_memtime stamps inside the hand-placed load batches, around the relevance tests,
//                              the evaluations and the combiner's walks                                  (tools/profile_waits.py, profile_single_waits.py)
//   -DMSDF_PROFILE_QUERY=1|2   the same for k_ec_query. =2: every stamp first waits for all outstanding memory operations (attributes the time to the
//                              segments, slows the kernel); =1: plain stamps -- per-item totals, the longest item and the histogram stay meaningful, the
//                              kernel runs at its own pace                                               (tools/profile_query.py)
//   -DMSDF_BBCOUNT=<counters>  a table of execution counts per basic block; the tool inserts the bumps into the kernels' assembly (tools/isa_bbcount.py)
// The kernels call the hooks unconditionally: real functions in a measurement build, empty inline ones on empty types in a regular build. The rule: a new
// stamp is a hook call in the kernel and a definition here, never an #if in a kernel body. (Included by msdf_device.hpp behind its macros; host-compilable.)
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
// A real hook is inlined before anything else and stays unoptimised until then (minsize: its loops stay rolled), so that the optimiser meets the stamps
// in the kernel's own body, where they used to be written: the measurement builds' code objects did not change by a byte when the hooks were introduced.
#define MSDF_HOOK __device__ __forceinline__ __attribute__((minsize))
#define MSDF_HD_HOOK MSDF_HD __attribute__((always_inline, minsize))
#else
#define MSDF_HD_HOOK MSDF_HD
#endif

namespace msdfhip {

// What an edge policy counts while it is walked: per tile (k_distance, EdgesCulledPacked) or per query (k_ec_query, EdgesCooperative).
enum ProfSlot : int {
    PROF_BATCH = 0, PROF_CURVE_BATCH = 2,   // WAITS: cycles in the R+E0 batch of the survivor walk (issue -> landed), in the E1+E2 batch of a curve; [+1] batches
    PROF_EVAL = 4, PROF_RELEVANCE = 6,      //        cycles evaluating edges (selAddEdge); [+1] evaluations | cycles in relevance tests + vote
    PROF_SLOW_BATCHES = 7,                  //        batches that took > 1000 cycles | (> 3000 cycles)<<32
    PROF_QUERY_EDGES = 0, PROF_QUERY_MERGES = 1,   // QUERY: all-edge evaluation into the slots, per-contour slot merges
    PROF_WALK = 8, PROF_BOOKKEEPING = 9,    // both (the combiners of msdf_device.hpp): contour walks of pass 0, per-contour bookkeeping after a walk,
    PROF_SECOND_WALK = 10, PROF_EPILOGUE = 11,   //  second walks, combiner epilogue
    PROF_TILE = 13,                         // WAITS: whole tile (prologue + distance + stores)
    PROF_HEADER = 14, PROF_PASS_A = 15      // WAITS, a wavefront's sums only: phase 1 up to the landed header loads, pass A
};
// The device tables as the tools read them, BY INDEX: msdfhip_debug_wait_profile copies a table out as it is.
enum WaitProfileSlot : int {                // gWaitProfile[24], summed over wavefronts by lane 0 when a wavefront ends
    WP_WAVES, WP_WAVE_CYCLES, WP_PHASE1, WP_BATCH_CYCLES, WP_BATCHES, WP_CURVE_BATCH_CYCLES, WP_CURVE_BATCHES, WP_EVAL_CYCLES, WP_EVALS, WP_RELEVANCE,   // 0 .. 9
    WP_PHASE2, WP_BATCHES_OVER_1000, WP_BATCHES_OVER_3000, WP_WALK, WP_BOOKKEEPING, WP_SECOND_WALK, WP_EPILOGUE, WP_TILE, WP_HEADER, WP_PASS_A            // 10 .. 19
};
enum QueryProfileSlot : int {               // gQueryProfile[24], written by lane 0 when a wavefront of k_ec_query ends
    QP_WAVES, QP_WAVE_CYCLES, QP_WAVES_WITH_WORK, QP_FIRST_START, QP_LAST_END,   // 0 .. 4; first start / last end: atomic min / max
    QP_CHUNK_ITEMS, QP_CHUNK_CYCLES, QP_COOP_ITEMS, QP_COOP_CYCLES,             // 5 .. 8: the two kinds of work item, count and cycles
    QP_TICKET, QP_LOOKUP, QP_GLYPH_STATE, QP_EVALUATION, QP_STORE,              // 9 .. 13 cycles: ticket wait, glyph lookup, per-glyph loads, evaluation (candidate load, interpolation, distance query, comparison), store + barrier
    QP_LONGEST_ITEM, QP_COOP_ROUNDS, QP_LAST_WORK_END, QP_LONGEST_WHO           // 14 .. 17: longest item (cycles), cooperative rounds (64 edges each), end of the last wavefront that still found work, longest item as cycles/256<<24 | glyph<<1 | chunk
};
enum QueryDetailSlot : int {                // gQueryDetail[16], the second page: inside the cooperative distance query; [10 .. 15] items by duration: < 16 k cycles, < 32 k, ... >= 512 k
    QD_QUERIES, QD_CYCLES, QD_EDGES, QD_MERGES, QD_WALK, QD_BOOKKEEPING, QD_SECOND_WALK, QD_EPILOGUE, QD_CONTOURS, QD_WITH_SLOTS, QD_HISTOGRAM
};

// ---- the counters of an edge policy: a base class of it, behind its own fields. Empty in a regular build (and in the other kernel's measurement build).
struct NoCounters {
    MSDF_HD unsigned long long now() const { return 0; }
    MSDF_HD unsigned long long reset() const { return 0; }
    MSDF_HD void add(int, unsigned long long) const { }
    MSDF_HD void batch(unsigned long long) const { }
    MSDF_HD void pin(double &) const { }
    MSDF_HD void queryDone(unsigned long long, int, const void *, int) const { }
    MSDF_HD static unsigned long long clock() { return 0; }
    MSDF_HD static void itemDone(unsigned long long) { }
    template <class... Sums> MSDF_HD static void waveDone(Sums...) { }
};
MSDF_HD NoCounters profOf(const void *) { return NoCounters(); }   // any policy without counters; one that derives from the counters below prefers their overload

#if defined(MSDF_PROFILE_WAITS)
struct WaitCounters {
    mutable unsigned long long prof[16];
    MSDF_HOOK unsigned long long now() const { return __builtin_readcyclecounter(); }
    MSDF_HOOK unsigned long long reset() const { for (int i = 0; i < 16; ++i) prof[i] = 0; return now(); }
    MSDF_HOOK void add(int slot, unsigned long long dt) const { prof[slot] += dt; }
    MSDF_HOOK void batch(unsigned long long dt) const {
        prof[PROF_BATCH] += dt, prof[PROF_BATCH+1] += 1;
        if (dt > 1000) prof[PROF_SLOW_BATCHES] += 1;
        if (dt > 3000) prof[PROF_SLOW_BATCHES] += 1ull<<32;
    }
    MSDF_HOOK void pin(double &v) const { asm volatile("" : "+v"(v)); }
};
MSDF_HOOK const WaitCounters &profOf(const WaitCounters *c) { return *c; }
#else
typedef NoCounters WaitCounters;
#endif

#if defined(MSDF_PROFILE_QUERY)
__device__ unsigned long long gQueryDetail[16];
__device__ unsigned long long gQueryProfile[24];
struct QueryCounters {
    mutable unsigned long long prof[16];
    MSDF_HOOK static unsigned long long clock() {                  // THE stamp of the query probe (ecQueryBody keeps its stamps and sums in plain locals, dead code in a regular build)
#if MSDF_PROFILE_QUERY >= 2
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
        return __builtin_readcyclecounter();
    }
    MSDF_HOOK unsigned long long now() const { return clock(); }
    MSDF_HOOK unsigned long long reset() const { for (int i = 0; i < 16; ++i) prof[i] = 0; return now(); }
    MSDF_HOOK void add(int slot, unsigned long long dt) const { prof[slot] += dt; }
    MSDF_HOOK void queryDone(unsigned long long t0, int C, const void *slots, int lane) const {
        if (lane == 0) {
            atomicAdd(&gQueryDetail[QD_QUERIES], 1ull), atomicAdd(&gQueryDetail[QD_CYCLES], now()-t0);
            atomicAdd(&gQueryDetail[QD_EDGES], prof[PROF_QUERY_EDGES]), atomicAdd(&gQueryDetail[QD_MERGES], prof[PROF_QUERY_MERGES]), atomicAdd(&gQueryDetail[QD_WALK], prof[PROF_WALK]);
            atomicAdd(&gQueryDetail[QD_BOOKKEEPING], prof[PROF_BOOKKEEPING]), atomicAdd(&gQueryDetail[QD_SECOND_WALK], prof[PROF_SECOND_WALK]), atomicAdd(&gQueryDetail[QD_EPILOGUE], prof[PROF_EPILOGUE]);
            atomicAdd(&gQueryDetail[QD_CONTOURS], (unsigned long long) C), atomicAdd(&gQueryDetail[QD_WITH_SLOTS], (unsigned long long) (slots ? 1 : 0));
        }
    }
    MSDF_HOOK static void itemDone(unsigned long long dt) {       // a work item of ecQueryBody took dt cycles: its histogram bucket
        if (threadIdx.x == 0) {
            int bucket = 0;
            for (unsigned long long d = dt>>14; d && bucket < 6; d >>= 1)
                ++bucket;
            atomicAdd(&gQueryDetail[QD_HISTOGRAM+(bucket > 5 ? 5 : bucket)], 1ull);
        }
    }
    typedef unsigned long long Sum;                                 // (the sums by value, one by one: the arrays they sit in stay the kernel's own locals)
    MSDF_HOOK static void waveDone(Sum start, Sum lastWork, Sum chunkItems, Sum chunkCycles, Sum coopItems, Sum coopCycles, Sum ticket, Sum lookup, Sum glyphState, Sum evaluation,
                                   Sum store, Sum coopRounds, Sum longest, Sum longestWho) {   // a wavefront of ecQueryBody ends
        const Sum end = clock();
        if (threadIdx.x == 0) {
            atomicAdd(&gQueryProfile[QP_WAVES], 1ull), atomicAdd(&gQueryProfile[QP_WAVE_CYCLES], end-start);
            if (lastWork)
                atomicAdd(&gQueryProfile[QP_WAVES_WITH_WORK], 1ull), atomicMax(&gQueryProfile[QP_LAST_WORK_END], lastWork);
            atomicMin(&gQueryProfile[QP_FIRST_START], start), atomicMax(&gQueryProfile[QP_LAST_END], end);
            atomicAdd(&gQueryProfile[QP_CHUNK_ITEMS], chunkItems), atomicAdd(&gQueryProfile[QP_CHUNK_CYCLES], chunkCycles), atomicAdd(&gQueryProfile[QP_COOP_ITEMS], coopItems), atomicAdd(&gQueryProfile[QP_COOP_CYCLES], coopCycles);
            atomicAdd(&gQueryProfile[QP_TICKET], ticket), atomicAdd(&gQueryProfile[QP_LOOKUP], lookup), atomicAdd(&gQueryProfile[QP_GLYPH_STATE], glyphState), atomicAdd(&gQueryProfile[QP_EVALUATION], evaluation);
            atomicAdd(&gQueryProfile[QP_STORE], store), atomicMax(&gQueryProfile[QP_LONGEST_ITEM], longest), atomicAdd(&gQueryProfile[QP_COOP_ROUNDS], coopRounds);
            atomicMax(&gQueryProfile[QP_LONGEST_WHO], (longest>>8)<<24|longestWho);   // cycles/256 | glyph<<1 | chunk
        }
    }
};
MSDF_HOOK const QueryCounters &profOf(const QueryCounters *c) { return *c; }
#else
typedef NoCounters QueryCounters;
#endif

// ---- the hooks on an edge policy (the walks and combiners of msdf_device.hpp and msdf_kernels.hpp)
template <class Edges> MSDF_HD_HOOK unsigned long long profNow(const Edges &edges) { return profOf(&edges).now(); }     // a clock read
template <class Edges> MSDF_HD_HOOK unsigned long long profReset(const Edges &edges) { return profOf(&edges).reset(); } // a new tile, a new query: zeroes the policy's counters, then a clock read
template <class Edges> MSDF_HD_HOOK void profAdd(const Edges &edges, int slot, unsigned long long dt) { profOf(&edges).add(slot, dt); }
template <class Edges> MSDF_HD_HOOK void profBatch(const Edges &edges, unsigned long long dt) { profOf(&edges).batch(dt); }   // one R+E0 batch of dt cycles
template <class Edges> MSDF_HD_HOOK void profPin(const Edges &edges, double &v) { profOf(&edges).pin(v); }                    // the next stamp must not move above the code that computes v
template <class Edges> MSDF_HD_HOOK void profQueryDone(const Edges &edges, unsigned long long t0, int C, const void *slots, int lane) { profOf(&edges).queryDone(t0, C, slots, lane); }   // one cooperative query, begun at t0, into gQueryDetail

// ---- a k_distance wavefront (distanceBody): its stamps; `sums`, its counters summed over its tiles, is an object of its own (an array that loops index
// stays out of registers for as long as it shares an object with anything else). Lane 0 flushes both into gWaitProfile when the wavefront ends.
#if defined(MSDF_PROFILE_WAITS)
__device__ unsigned long long gWaitProfile[24];
struct WaitProbe {
    unsigned long long start, header, phase2;
    MSDF_HOOK void begin(WaitCounters &sums) { start = __builtin_readcyclecounter(); __builtin_memset(sums.prof, 0, sizeof(sums.prof)); }
    MSDF_HOOK void headerLanded(int fromHeader) {                 // the header loads have landed when a value computed from them is usable
        int sink = MSDF_UNIFORM(fromHeader);
        asm volatile("" : "+s"(sink));
        header = __builtin_readcyclecounter()+(unsigned long long) (sink&0);
    }
    MSDF_HOOK void passADone(WaitCounters &sums) {
        const unsigned long long t = __builtin_readcyclecounter();
        sums.prof[PROF_HEADER] = header-start, sums.prof[PROF_PASS_A] = t-header;
    }
    MSDF_HOOK void phase1Done() { phase2 = __builtin_readcyclecounter(); }
    MSDF_HOOK void tileDone(WaitCounters &sums, const WaitCounters &edges, unsigned long long tile0) {
        edges.prof[PROF_TILE] += __builtin_readcyclecounter()-tile0;
        for (int i = 0; i < 16; ++i)
            sums.prof[i] += edges.prof[i];
    }
    MSDF_HOOK void flush(const WaitCounters &sums, int lane) const {
        const unsigned long long end = __builtin_readcyclecounter(), *acc = sums.prof;
        if (lane == 0) {
            atomicAdd(&gWaitProfile[WP_WAVES], 1ull), atomicAdd(&gWaitProfile[WP_WAVE_CYCLES], end-start), atomicAdd(&gWaitProfile[WP_PHASE1], phase2-start);
            atomicAdd(&gWaitProfile[WP_BATCH_CYCLES], acc[PROF_BATCH]), atomicAdd(&gWaitProfile[WP_BATCHES], acc[PROF_BATCH+1]);
            atomicAdd(&gWaitProfile[WP_CURVE_BATCH_CYCLES], acc[PROF_CURVE_BATCH]), atomicAdd(&gWaitProfile[WP_CURVE_BATCHES], acc[PROF_CURVE_BATCH+1]);
            atomicAdd(&gWaitProfile[WP_EVAL_CYCLES], acc[PROF_EVAL]), atomicAdd(&gWaitProfile[WP_EVALS], acc[PROF_EVAL+1]), atomicAdd(&gWaitProfile[WP_RELEVANCE], acc[PROF_RELEVANCE]);
            atomicAdd(&gWaitProfile[WP_PHASE2], end-phase2);
            atomicAdd(&gWaitProfile[WP_BATCHES_OVER_1000], acc[PROF_SLOW_BATCHES]&0xffffffffull), atomicAdd(&gWaitProfile[WP_BATCHES_OVER_3000], acc[PROF_SLOW_BATCHES]>>32);
            atomicAdd(&gWaitProfile[WP_WALK], acc[PROF_WALK]), atomicAdd(&gWaitProfile[WP_BOOKKEEPING], acc[PROF_BOOKKEEPING]), atomicAdd(&gWaitProfile[WP_SECOND_WALK], acc[PROF_SECOND_WALK]);
            atomicAdd(&gWaitProfile[WP_EPILOGUE], acc[PROF_EPILOGUE]), atomicAdd(&gWaitProfile[WP_TILE], acc[PROF_TILE]);
            atomicAdd(&gWaitProfile[WP_HEADER], acc[PROF_HEADER]), atomicAdd(&gWaitProfile[WP_PASS_A], acc[PROF_PASS_A]);
        }
    }
};
#else
struct WaitProbe {
    MSDF_HD void begin(WaitCounters &) { }
    MSDF_HD void headerLanded(int) { }
    MSDF_HD void passADone(WaitCounters &) { }
    MSDF_HD void phase1Done() { }
    MSDF_HD void tileDone(WaitCounters &, const WaitCounters &, unsigned long long) { }
    MSDF_HD void flush(const WaitCounters &, int) const { }
};
#endif

} // namespace msdfhip

// ---- the basic-block table. The tool compiles msdf_capi.hip to gfx950 assembly, inserts a counter bump at the top of every basic block of the chosen kernels
// (one lane of a few extra VGPRs per block; exec- and SCC-neutral), flushes the lanes into this table with atomics at s_endpgm and assembles the result back
// into a library: the kernels' own instruction stream is the production one. Its assembly names this C symbol. (A DEFINITION: the one-line extern "C" form only declares.)
#if defined(MSDF_BBCOUNT)
extern "C" { __device__ __attribute__((used)) unsigned msdfhip_bbcount[MSDF_BBCOUNT]; }
#endif

// ---- host side: what msdfhip_debug_wait_profile and msdfhip_debug_bbcount (msdf_capi.hip) hand out. A regular build has no tables: zeros, 0 counters.
#if defined(__HIPCC__)
namespace msdfhip {
#define MSDF_MEASURE_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

inline hipError_t readWaitProfile(unsigned long long *out24, int reset) {   // reads the build's table, then clears it if `reset`
#if defined(MSDF_PROFILE_WAITS)
    const unsigned long long zero[24] = { 0 };
    if (out24)
        MSDF_MEASURE_TRY(hipMemcpyFromSymbol(out24, HIP_SYMBOL(gWaitProfile), sizeof(zero)));
    if (reset)
        MSDF_MEASURE_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gWaitProfile), zero, sizeof(zero)));
#elif defined(MSDF_PROFILE_QUERY)                                    // the tables of k_ec_query instead: reset == 2 reads the second page, only reset == 1 clears
    unsigned long long zero[24] = { 0 };
    const unsigned long long zero16[16] = { 0 };
    zero[QP_FIRST_START] = ~0ull;                                   // an atomic minimum
    if (out24)
        MSDF_MEASURE_TRY(hipMemcpyFromSymbol(out24, HIP_SYMBOL(gQueryProfile), sizeof(zero)));
    if (out24 && reset == 2)                                        // (over the first 16 entries of the first page)
        MSDF_MEASURE_TRY(hipMemcpyFromSymbol(out24, HIP_SYMBOL(gQueryDetail), sizeof(zero16)));
    if (reset == 1) {
        MSDF_MEASURE_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gQueryProfile), zero, sizeof(zero)));
        MSDF_MEASURE_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gQueryDetail), zero16, sizeof(zero16)));
    }
#else
    if (out24)
        memset(out24, 0, 24*sizeof(unsigned long long));
    (void) reset;
#endif
    return hipSuccess;
}

inline hipError_t readBbcount(unsigned *out, int cap, int reset, int &n) {   // n: the counters copied (at most cap), then cleared if `reset`
#if defined(MSDF_BBCOUNT)
    n = cap < (int) MSDF_BBCOUNT ? cap : (int) MSDF_BBCOUNT;
    MSDF_MEASURE_TRY(hipDeviceSynchronize());
    if (out && n > 0)
        MSDF_MEASURE_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(msdfhip_bbcount), sizeof(unsigned)*(size_t) n));
    if (reset) {
        static const std::vector<unsigned> zero((size_t) MSDF_BBCOUNT, 0u);
        MSDF_MEASURE_TRY(hipMemcpyToSymbol(HIP_SYMBOL(msdfhip_bbcount), zero.data(), sizeof(unsigned)*zero.size()));
    }
#else
    (void) out, (void) cap, (void) reset;
    n = 0;
#endif
    return hipSuccess;
}

} // namespace msdfhip
#endif
