// msdf_resources.hpp against a fake HIP runtime that keeps a ledger (fake/hip/hip_runtime.h, first on the include path): who releases what, how
// often, on which device, on which exit. Stand-alone; tests/test_resources_host.py builds it plain and under the address / undefined-behaviour
// sanitizers. Exit status 0 and a last line "resources_host: N checks" mean every check held.
#include "../../msdfgen_amd/csrc/msdf_resources.hpp"

#include <cstdio>
#include <cstring>
#include <utility>

using namespace msdfhip;
using fakehip::ledger;

static long gChecks = 0;
#define CHECK(cond) do { ++gChecks; if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static bool nothingLive() { return ledger().live.empty() && ledger().doubleReleases.empty(); }
static long releasesOf(const void *handle) {
    long n = 0;
    for (size_t i = 0; i < ledger().releases.size(); ++i)
        n += ledger().releases[i].handle == handle;
    return n;
}

// Shaped like a slot of the host-output pipeline: 1 stream, 5 events, 1 pinned block, 2 buffers.
struct Slot {
    Stream stream;
    Event events[5];
    WorkBuffer<unsigned, true> word;
    WorkBuffer<char> dev;
    WorkBuffer<char, true> staging;
    hipError_t create() {
        hipError_t e = stream.create(hipStreamNonBlocking);
        for (int k = 0; e == hipSuccess && k < 5; ++k)
            e = events[k].create(hipEventDisableTiming);
        if (e == hipSuccess) e = word.ensure(64);
        if (e == hipSuccess) e = dev.ensure(1000);
        if (e == hipSuccess) e = staging.ensure(1000);
        return e;
    }
};
enum { SLOT_CREATIONS = 9 };

// A pooled object: two slots, as DevicePool wants them.
struct Pooled {
    int device = -1;
    Slot slot[2];
    int quiesced = 0;
    hipError_t create(int d) {
        device = d;
        hipError_t e = slot[0].create();
        return e == hipSuccess ? slot[1].create() : e;
    }
    void quiesce() {
        ++quiesced;
        for (int k = 0; k < 2; ++k)
            if (slot[k].stream)
                (void) hipStreamSynchronize(slot[k].stream);
    }
};

static void ownedAndBorrowed() {
    char mine[32];
    {
        WorkBuffer<int> owned, borrowed;
        WorkBuffer<int, true> pinned;
        CHECK(owned.ensure(10) == hipSuccess && owned.owned && owned.cap == 10 && ledger().lastBytes == 10*sizeof(int));
        CHECK(pinned.ensure(3) == hipSuccess && ledger().lastBytes == 3*sizeof(int) && ledger().lastFlags == hipHostMallocDefault);
        borrowed.borrow(reinterpret_cast<int *>(mine), 8);
        CHECK(!borrowed.owned && borrowed.cap == 8 && borrowed.ensure(8) == hipSuccess && borrowed.ptr == reinterpret_cast<int *>(mine));
        CHECK(ledger().liveOf(fakehip::DEVICE_MEMORY) == 1 && ledger().liveOf(fakehip::PINNED_MEMORY) == 1);
        const void *a = owned.ptr, *b = pinned.ptr;
        const long before = ledger().calls;
        CHECK(owned.ensure(10) == hipSuccess && owned.ensure(0) == hipSuccess && owned.ptr == a && ledger().calls == before);   // enough already: no call
        // a borrowed buffer that has to grow drops what it borrowed and owns the new block
        CHECK(borrowed.ensure(9) == hipSuccess && borrowed.owned && borrowed.ptr != reinterpret_cast<int *>(mine) && releasesOf(mine) == 0);
        const void *c = borrowed.ptr;
        borrowed.borrow(reinterpret_cast<int *>(mine), 8);                                  // ... and borrowing again frees it
        CHECK(releasesOf(c) == 1 && !borrowed.owned);
        Stream s;
        Event e, timed;
        CHECK(s.create(hipStreamNonBlocking) == hipSuccess && ledger().lastFlags == hipStreamNonBlocking && ledger().streamPriority == 0);
        CHECK(strcmp(ledger().log.back(), "hipStreamCreateWithFlags") == 0);
        CHECK(s.create(hipStreamNonBlocking, -1) == hipSuccess && ledger().streamPriority == -1 && ledger().liveOf(fakehip::STREAM) == 1);   // the first one went
        CHECK(e.create(hipEventDisableTiming) == hipSuccess && ledger().lastFlags == hipEventDisableTiming);
        CHECK(timed.create(hipEventDefault) == hipSuccess && ledger().lastFlags == hipEventDefault);
        const void *hs = (hipStream_t) s, *he = (hipEvent_t) e;
        e.release();
        CHECK(!e && releasesOf(he) == 1);
        e.release();
        CHECK(releasesOf(he) == 1);
        (void) hs, (void) a, (void) b;
    }
    CHECK(nothingLive() && releasesOf(mine) == 0);
    for (size_t i = 0; i < ledger().releases.size(); ++i)                                    // exactly once each
        CHECK(releasesOf(ledger().releases[i].handle) == 1 || ledger().live.count(ledger().releases[i].handle) == 0);
}

static void moves() {
    WorkBuffer<double> a;
    CHECK(a.ensure(4) == hipSuccess);
    double *p = a.ptr;
    WorkBuffer<double> b(std::move(a));
    CHECK(!a.ptr && !a.cap && !a.owned && b.ptr == p && b.cap == 4 && b.owned);
    WorkBuffer<double> c;
    CHECK(c.ensure(2) == hipSuccess);
    const void *old = c.ptr;
    c = std::move(b);
    CHECK(releasesOf(old) == 1 && !b.ptr && !b.owned && c.ptr == p);
    WorkBuffer<char> bytes;                                                                  // a byte region taken over as a typed array
    CHECK(bytes.ensure(40) == hipSuccess);
    char *raw = bytes.ptr;
    WorkBuffer<double> typed;
    typed.adopt(std::move(bytes));
    CHECK(!bytes.ptr && !bytes.owned && typed.ptr == reinterpret_cast<double *>(raw) && typed.cap == 5 && typed.owned && releasesOf(raw) == 0);
    char mine[16];
    WorkBuffer<char> view;
    view.borrow(mine, 16);
    typed.adopt(std::move(view));                                                            // adopting a borrowed one frees the old block and stays borrowed
    CHECK(releasesOf(raw) == 1 && !typed.owned && typed.cap == 2);
    Stream s, t;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess);
    hipStream_t h = s;
    t = std::move(s);
    CHECK(!s && (hipStream_t) t == h);
    Event e;
    CHECK(e.create(hipEventDisableTiming) == hipSuccess);
    hipEvent_t he = e;
    Event f(std::move(e));
    CHECK(!e && (hipEvent_t) f == he && ledger().liveOf(fakehip::EVENT) == 1);
    c.release(), t.release(), f.release();
    CHECK(nothingLive() && releasesOf(p) == 1 && releasesOf(h) == 1 && releasesOf(he) == 1);
}

static void ensureOrder() {
    WorkBuffer<int> b;
    CHECK(b.ensure(4) == hipSuccess);
    const size_t at = ledger().log.size();
    CHECK(b.ensure(5) == hipSuccess && ledger().log.size() == at+2);
    CHECK(strcmp(ledger().log[at], "hipFree") == 0 && strcmp(ledger().log[at+1], "hipMalloc") == 0);      // the old block goes first
    ledger().failAt = ledger().creations+1;
    CHECK(b.ensure(6) != hipSuccess && !b.ptr && !b.cap && !b.owned && nothingLive());
    Stream s;
    ledger().failAt = ledger().creations+1;
    CHECK(s.create(hipStreamNonBlocking) != hipSuccess && !s);
    Event e;
    ledger().failAt = ledger().creations+1;
    CHECK(e.create(hipEventDisableTiming) != hipSuccess && !e);
    ledger().failAt = 0;
    CHECK(nothingLive());
}

static void failureAtEveryStep() {
    for (long k = 1; k <= SLOT_CREATIONS+1; ++k) {
        const size_t releasesBefore = ledger().releases.size();
        {
            Slot slot;
            ledger().failAt = ledger().creations+k;
            const hipError_t e = slot.create();
            ledger().failAt = 0;
            CHECK((e == hipSuccess) == (k > SLOT_CREATIONS));
            CHECK((long) ledger().live.size() == (k > SLOT_CREATIONS ? SLOT_CREATIONS : k-1));
        }
        CHECK(nothingLive());
        CHECK((long) (ledger().releases.size()-releasesBefore) == (k > SLOT_CREATIONS ? SLOT_CREATIONS : k-1));
    }
}

static void ownsNothing() {
    char arena[64];
    const long before = ledger().calls;
    {
        Slot view;                                                                           // a view: everything empty or borrowed
        view.dev.borrow(arena, 32), view.staging.borrow(arena+32, 32);
    }
    CHECK(ledger().calls == before);
}

static void pool() {
    DevicePool<Pooled> pool;
    Pooled *first = NULL, *second = NULL, *other = NULL;
    {
        DevicePool<Pooled>::Lease a, b, c;
        (void) hipSetDevice(0);
        CHECK(pool.take(0, a) == hipSuccess && pool.take(0, b) == hipSuccess);
        (void) hipSetDevice(1);
        CHECK(pool.take(1, c) == hipSuccess);
        first = &*a, second = &*b, other = &*c;
        CHECK(first != second && a->device == 0 && c->device == 1 && (long) ledger().live.size() == 3*2*SLOT_CREATIONS);
    }                                                                                        // returned in the order c, b, a
    CHECK(first->quiesced == 1 && second->quiesced == 1 && other->quiesced == 1);
    {
        DevicePool<Pooled>::Lease a, b, c, d;
        CHECK(pool.take(0, a) == hipSuccess && &*a == first);                                // the most recently returned one of device 0, never device 1's
        CHECK(pool.take(0, b) == hipSuccess && &*b == second);
        CHECK(pool.take(1, c) == hipSuccess && &*c == other);
        const size_t live = ledger().live.size();
        ledger().failAt = ledger().creations+SLOT_CREATIONS+3;                               // a fresh one that fails in its second slot
        CHECK(pool.take(1, d) != hipSuccess && ledger().live.size() == live && ledger().doubleReleases.empty());
        ledger().failAt = 0;
        a.quiescent = true;                                                                  // the call saw its own completion: no wait on return
    }
    CHECK(first->quiesced == 1 && second->quiesced == 2 && other->quiesced == 2);
    auto early = [&](int way) -> int {                                                      // a lease returns its object on every exit
        DevicePool<Pooled>::Lease l;
        if (pool.take(0, l) != hipSuccess)
            return -1;
        if (way == 0)
            return 0;
        if (way == 1)
            return 1;
        return 2;
    };
    for (int way = 0; way < 3; ++way) {
        CHECK(early(way) == way);
        DevicePool<Pooled>::Lease l;
        CHECK(pool.take(0, l) == hipSuccess && (&*l == first || &*l == second) && (long) ledger().live.size() == 3*2*SLOT_CREATIONS);
    }
    // drain: every pooled object goes with its own device current; the one out on lease is untouched and comes back afterwards
    (void) hipSetDevice(1);
    {
        DevicePool<Pooled>::Lease out;
        CHECK(pool.take(0, out) == hipSuccess);
        Pooled *held = &*out;
        const int quiescedBefore = held->quiesced;
        std::map<const void *, int> deviceOf;                                                // handle -> the device of the object that owns it
        Pooled *pooled[2] = { held == first ? second : first, other };
        for (int i = 0; i < 2; ++i)
            for (int k = 0; k < 2; ++k) {
                Slot &s = pooled[i]->slot[k];
                const void *handles[] = { (hipStream_t) s.stream, (hipEvent_t) s.events[0], (hipEvent_t) s.events[4], s.word.ptr, s.dev.ptr, s.staging.ptr };
                for (size_t h = 0; h < sizeof(handles)/sizeof(handles[0]); ++h)
                    deviceOf[handles[h]] = pooled[i]->device;
            }
        const size_t releasesBefore = ledger().releases.size();
        const int syncsBefore = ledger().streamSyncs;
        pool.drain();
        CHECK(ledger().device == 1);                                                         // the caller's device is back
        CHECK(ledger().streamSyncs == syncsBefore+4);                                        // the streams of the two pooled objects, before they went
        CHECK((long) (ledger().releases.size()-releasesBefore) == 2*2*SLOT_CREATIONS && (long) ledger().live.size() == 2*SLOT_CREATIONS);
        size_t seen = 0;
        for (size_t i = releasesBefore; i < ledger().releases.size(); ++i) {
            const fakehip::Release &r = ledger().releases[i];
            if (deviceOf.count(r.handle)) {
                CHECK(r.device == deviceOf[r.handle]);
                ++seen;
            }
            CHECK(r.device == 0 || r.device == 1);
        }
        CHECK(seen == deviceOf.size());
        CHECK(held->quiesced == quiescedBefore && held->slot[0].stream && ledger().live.count((hipStream_t) held->slot[0].stream));
        pool.drain();                                                                        // nothing pooled: nothing released
        CHECK((long) ledger().live.size() == 2*SLOT_CREATIONS);
    }
    {
        DevicePool<Pooled>::Lease again;
        (void) hipSetDevice(0);
        const long created = ledger().creations;
        CHECK(pool.take(0, again) == hipSuccess && ledger().creations == created);           // the object that was out is in the pool again
    }
    pool.drain();
    CHECK(nothingLive());
}

int main() {
    ownedAndBorrowed();
    moves();
    ensureOrder();
    failureAtEveryStep();
    ownsNothing();
    pool();
    CHECK(nothingLive());                                                                    // process end: the ledger is empty
    for (size_t i = 0; i < ledger().releases.size(); ++i)
        CHECK(ledger().releases[i].handle != NULL);
    CHECK(ledger().doubleReleases.empty());
    printf("resources_host: %ld checks\n", gChecks);
    return 0;
}
