// msdf_resources.hpp -- who frees what: the holders of every device resource of the host runtime (msdf_capi.hip). Device and pinned memory,
// streams, events, and the per-device pools of the objects built from them. Nothing here knows a kernel, a plan or an ABI type.
//
// The one rule the holders do NOT enforce: a resource is released on the thread's CURRENT device. Whoever destroys an object that owns some
// binds the object's device first (msdfhip_batch_destroy, DevicePool::drain); a holder that owns nothing makes no HIP call at all.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <mutex>
#include <vector>

namespace msdfhip {

// hipHostMalloc for the library's own staging buffers. The HIP runtime recycles pinned address ranges without ThreadSanitizer seeing
// the free / allocation pair (it is not instrumented), so under TSan the allocator's own synchronisation is stated explicitly (release at
// the free, acquire at the allocation) -- otherwise writes of two threads to buffers that merely reuse an address are reported as races.
// The pairing goes through ONE tag for all pinned memory, not through the block's base address: a recycled range may come back inside a
// block with another base (seen once in four runs: staging writes of one call reported against the scatter reads of an earlier call of
// another thread, same addresses, different owners) -- every allocation then acquires every earlier free, as a heap allocator would.
#if defined(__has_feature)
#if __has_feature(thread_sanitizer)
#define MSDFHIP_TSAN 1
extern "C" void __tsan_acquire(void *addr);
extern "C" void __tsan_release(void *addr);
#endif
#endif
#if defined(MSDFHIP_TSAN)
static char gPinnedHeapTag;
#endif
inline hipError_t pinnedAlloc(void **p, size_t bytes, unsigned flags = hipHostMallocDefault) {
    const hipError_t e = hipHostMalloc(p, bytes ? bytes : 1, flags);
#if defined(MSDFHIP_TSAN)
    if (e == hipSuccess)
        __tsan_acquire(&gPinnedHeapTag);                         // pairs with the pinnedFree of whoever owned (any part of) the range before
#endif
    return e;
}
inline hipError_t pinnedFree(void *p) {
#if defined(MSDFHIP_TSAN)
    if (p)
        __tsan_release(&gPinnedHeapTag);
#endif
    return hipHostFree(p);
}

// A grow-on-demand allocation: device memory, or (PINNED) host staging through pinnedAlloc / pinnedFree. It is OWNED -- freed when it has to grow and
// when it goes -- or BORROWED (a caller's array, a range of an arena, another batch's buffer), and then only dropped.
template <class T, bool PINNED = false>
struct WorkBuffer {
    T *ptr = NULL;
    size_t cap = 0;                   // elements
    bool owned = false;
    WorkBuffer() { }
    WorkBuffer(WorkBuffer &&o) noexcept : ptr(o.ptr), cap(o.cap), owned(o.owned) { o.forget(); }
    WorkBuffer &operator=(WorkBuffer &&o) noexcept {
        if (this != &o) {
            release();
            ptr = o.ptr, cap = o.cap, owned = o.owned;
            o.forget();
        }
        return *this;
    }
    ~WorkBuffer() { release(); }
    void release() {
        if (owned && ptr)
            (void) (PINNED ? pinnedFree(ptr) : hipFree(ptr));
        forget();
    }
    void borrow(T *p, size_t n) { release(); ptr = p, cap = n; }
    // Takes over what `o` holds, owned or borrowed, under this element type (the prepared batch: byte regions become its typed arrays).
    template <class U>
    void adopt(WorkBuffer<U, PINNED> &&o) {
        release();
        ptr = reinterpret_cast<T *>(o.ptr), cap = o.cap*sizeof(U)/sizeof(T), owned = o.owned;
        o.ptr = NULL, o.cap = 0, o.owned = false;
    }
    // At least n elements; the contents do not survive growth. Frees before it allocates; on failure the buffer is empty. n == 0 allocates nothing.
    hipError_t ensure(size_t n) {
        if (cap >= n)
            return hipSuccess;
        release();
        const hipError_t e = PINNED ? pinnedAlloc((void **) &ptr, n*sizeof(T)) : hipMalloc((void **) &ptr, n*sizeof(T));
        if (e != hipSuccess) {
            ptr = NULL;
            return e;
        }
        cap = n, owned = true;
        return hipSuccess;
    }
private:
    void forget() { ptr = NULL, cap = 0, owned = false; }
};

// Move-only owner of one HIP handle; reads as the handle. An empty owner's destructor makes no HIP call.
template <class H, hipError_t (*DESTROY)(H)>
struct HandleOwner {
    H handle = NULL;
    HandleOwner() { }
    HandleOwner(HandleOwner &&o) noexcept : handle(o.handle) { o.handle = NULL; }
    HandleOwner &operator=(HandleOwner &&o) noexcept {
        if (this != &o) {
            release();
            handle = o.handle, o.handle = NULL;
        }
        return *this;
    }
    ~HandleOwner() { release(); }
    void release() {
        if (handle)
            (void) DESTROY(handle);
        handle = NULL;
    }
    operator H() const { return handle; }
protected:
    hipError_t created(hipError_t e) {                           // (a failed creation leaves the owner empty)
        if (e != hipSuccess)
            handle = NULL;
        return e;
    }
};

struct Stream : HandleOwner<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags, int priority = 0) {        // priority 0: the default one
        release();
        return created(priority ? hipStreamCreateWithPriority(&handle, flags, priority) : hipStreamCreateWithFlags(&handle, flags));
    }
};

struct Event : HandleOwner<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags) {
        release();
        return created(hipEventCreateWithFlags(&handle, flags));
    }
};

// Process-wide pool of reusable objects, per device: a call takes one and its lease returns it on every exit, so the pool is bounded by the peak
// number of concurrent calls. T has: int device; hipError_t create(int device) (on the current device); void quiesce() (waits for its streams, also
// on a half-built object); a destructor that releases everything. Objects still pooled when the process ends are left to it.
template <class T>
class DevicePool {
    std::mutex mutex;
    std::vector<T *> idle;
public:
    class Lease {
        friend class DevicePool;
        DevicePool *pool = NULL;
        T *obj = NULL;
    public:
        bool quiescent = false;       // the call saw its own completion: nothing of it is in flight, the object goes back without a wait
        Lease() { }
        Lease(const Lease &) = delete;
        Lease &operator=(const Lease &) = delete;
        // Whatever exit the call took (an error return may leave copies / kernels in flight): nothing of it is pending when the next caller takes the object.
        ~Lease() {
            if (!obj)
                return;
            if (!quiescent) {
                obj->quiesce();
                (void) hipGetLastError();
            }
            std::lock_guard<std::mutex> lock(pool->mutex);
            pool->idle.push_back(obj);
        }
        T *operator->() const { return obj; }
        T &operator*() const { return *obj; }
    };
    // The most recently returned object of `device` (the thread's current one), else a fresh one. A half-built object never reaches the pool.
    hipError_t take(int device, Lease &lease) {
        lease.pool = this;
        {
            std::lock_guard<std::mutex> lock(mutex);
            for (size_t i = idle.size(); i-- > 0; )
                if (idle[i]->device == device) {
                    lease.obj = idle[i];
                    idle.erase(idle.begin()+i);
                    return hipSuccess;
                }
        }
        T *fresh = new T();
        const hipError_t e = fresh->create(device);
        if (e != hipSuccess) {
            fresh->quiesce();
            delete fresh;
            (void) hipGetLastError();
            return e;
        }
        lease.obj = fresh;
        return hipSuccess;
    }
    // Releases every pooled object on its own device; objects out on lease are not in the pool and come back to it later.
    void drain() {
        std::vector<T *> all;
        {
            std::lock_guard<std::mutex> lock(mutex);
            all.swap(idle);
        }
        int prev = 0;
        (void) hipGetDevice(&prev);
        for (size_t i = 0; i < all.size(); ++i) {
            (void) hipSetDevice(all[i]->device);
            all[i]->quiesce();
            delete all[i];
        }
        (void) hipSetDevice(prev);
        (void) hipGetLastError();
    }
};

} // namespace msdfhip
