// A fake <hip/hip_runtime.h> for tests/resources_host: only the types and functions msdf_resources.hpp calls, over a ledger of what is live,
// on which device each handle was released, how many calls were made, and a switch that fails the k-th creating call.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <map>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
typedef struct FakeStream *hipStream_t;
typedef struct FakeEvent *hipEvent_t;
enum { hipHostMallocDefault = 0, hipStreamNonBlocking = 1, hipEventDefault = 0, hipEventDisableTiming = 2 };

namespace fakehip {

enum Kind { DEVICE_MEMORY, PINNED_MEMORY, STREAM, EVENT, KINDS };

struct Release { Kind kind; const void *handle; int device; };

struct Ledger {
    std::map<const void *, Kind> live;          // what exists
    std::vector<Release> releases;              // every release, with the device current then
    std::vector<const void *> doubleReleases;   // handles released while not live
    std::vector<const char *> log;              // creating and releasing calls by name, in order
    long calls = 0;                             // every fake HIP call
    long creations = 0, failAt = 0;             // creating calls so far; the creating call with this number fails (0: none)
    int device = 0;
    int streamPriority = 0, streamSyncs = 0;    // of the last stream created; hipStreamSynchronize calls
    unsigned lastFlags = 0;
    size_t lastBytes = 0;
    std::vector<void *> released;               // blocks of released handles, kept to the end: no two handles of a run share an address
    ~Ledger() {
        for (size_t i = 0; i < released.size(); ++i)
            free(released[i]);
    }
    int liveOf(Kind k) const {
        int n = 0;
        for (std::map<const void *, Kind>::const_iterator i = live.begin(); i != live.end(); ++i)
            n += i->second == k;
        return n;
    }
};

inline Ledger &ledger() {
    static Ledger l;
    return l;
}

inline hipError_t create(Kind kind, void **out, const char *name) {
    Ledger &l = ledger();
    ++l.calls;
    l.log.push_back(name);
    if (++l.creations == l.failAt)
        return hipErrorOutOfMemory;                                  // (*out untouched, as a failing HIP call leaves it)
    *out = malloc(64);                                               // a real block: one never released is a leak under AddressSanitizer too
    l.live[*out] = kind;
    return hipSuccess;
}

inline hipError_t release(Kind kind, void *handle, const char *name) {
    Ledger &l = ledger();
    ++l.calls;
    l.log.push_back(name);
    if (!handle)
        return hipSuccess;
    const Release r = { kind, handle, l.device };
    l.releases.push_back(r);
    std::map<const void *, Kind>::iterator at = l.live.find(handle);
    if (at == l.live.end() || at->second != kind) {
        l.doubleReleases.push_back(handle);
        return hipErrorInvalidValue;
    }
    l.live.erase(at);
    l.released.push_back(handle);
    return hipSuccess;
}

} // namespace fakehip

inline hipError_t hipMalloc(void **p, size_t bytes) { fakehip::ledger().lastBytes = bytes; return fakehip::create(fakehip::DEVICE_MEMORY, p, "hipMalloc"); }
inline hipError_t hipFree(void *p) { return fakehip::release(fakehip::DEVICE_MEMORY, p, "hipFree"); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags) {
    fakehip::ledger().lastBytes = bytes, fakehip::ledger().lastFlags = flags;
    return fakehip::create(fakehip::PINNED_MEMORY, p, "hipHostMalloc");
}
inline hipError_t hipHostFree(void *p) { return fakehip::release(fakehip::PINNED_MEMORY, p, "hipHostFree"); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) {
    fakehip::ledger().lastFlags = flags, fakehip::ledger().streamPriority = 0;
    return fakehip::create(fakehip::STREAM, (void **) s, "hipStreamCreateWithFlags");
}
inline hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int priority) {
    fakehip::ledger().lastFlags = flags, fakehip::ledger().streamPriority = priority;
    return fakehip::create(fakehip::STREAM, (void **) s, "hipStreamCreateWithPriority");
}
inline hipError_t hipStreamDestroy(hipStream_t s) { return fakehip::release(fakehip::STREAM, s, "hipStreamDestroy"); }
inline hipError_t hipStreamSynchronize(hipStream_t s) {
    fakehip::Ledger &l = fakehip::ledger();
    ++l.calls, ++l.streamSyncs;
    return l.live.count(s) ? hipSuccess : hipErrorInvalidValue;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) {
    fakehip::ledger().lastFlags = flags;
    return fakehip::create(fakehip::EVENT, (void **) e, "hipEventCreateWithFlags");
}
inline hipError_t hipEventDestroy(hipEvent_t e) { return fakehip::release(fakehip::EVENT, e, "hipEventDestroy"); }
inline hipError_t hipGetDevice(int *d) { ++fakehip::ledger().calls; *d = fakehip::ledger().device; return hipSuccess; }
inline hipError_t hipSetDevice(int d) { ++fakehip::ledger().calls; fakehip::ledger().device = d; return hipSuccess; }
inline hipError_t hipGetLastError() { ++fakehip::ledger().calls; return hipSuccess; }
