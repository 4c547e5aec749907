// gsr_common.h -- plumbing shared by the translation units of libgsr_hip.so: errors, owning handles, the host's waits, launch sizes.
#pragma once
#include <hip/hip_runtime.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>

#include "../../include/gsr_hip.h"

namespace gsr {

// thread-local message behind gsr_last_error()
std::string& last_error();
int32_t fail(int32_t code, const char* fmt, ...);

#define GSR_HIP(expr)                                                                            \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return ::gsr::fail(GSR_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                               __FILE__, __LINE__);                                              \
    } while (0)

#define GSR_TRY(expr)                  \
    do {                               \
        int32_t _r = (expr);           \
        if (_r != GSR_OK) return _r;   \
    } while (0)

// Grow-only device buffer: the library owns its workspace and performs no allocation in steady
// state (a second level or ICP call of the same size reuses everything).  It frees its memory when it goes out of scope, so a
// context or a function that holds one keeps no release list.  borrow() makes it stand for memory of the CALLER instead: reserve()
// is then a no-op and nothing here ever frees that pointer.  Only this struct writes `p` and `cap`; everything else reads them.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { swap(o); return *this; }      // (what this one held goes with `o`)
    ~DevBuf() { release(); }
    void borrow(void* caller_ptr) { release(); p = caller_ptr; cap = BORROWED; }
    int32_t reserve(size_t bytes) {
        if (bytes <= cap) return GSR_OK;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return fail(GSR_E_HIP, "hipFree: %s", hipGetErrorString(e)); }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return fail(GSR_E_HIP, "hipMalloc(%zu bytes): %s", want, hipGetErrorString(e)); }
        cap = want;
        return GSR_OK;
    }
    void release() { if (p && cap != BORROWED) (void)hipFree(p); p = nullptr; cap = 0; }      // an early free; a borrowed pointer is only let go
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
    void swap(DevBuf& o) { void* tp = p; p = o.p; o.p = tp; size_t tc = cap; cap = o.cap; o.cap = tc; }

private:
    static constexpr size_t BORROWED = (size_t)-1;      // as a capacity: larger than any request
};

// The other things the library creates on a device, each destroyed by its holder.  A stream the CALLER passed in (gsr_hem_ctx::stream,
// gsr_icp_ctx::stream) is not one of them and stays a raw hipStream_t.  All three are empty until created and convert to the raw handle.
struct Event {
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { hipEvent_t t = e; e = o.e; o.e = t; return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create() { return hipEventCreate(&e); }                                               // timed
    hipError_t create_untimed() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }      // ordering only
    operator hipEvent_t() const { return e; }

private:
    hipEvent_t e = nullptr;
};

struct Stream {     // non-blocking
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept { hipStream_t t = s; s = o.s; o.s = t; return *this; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }

private:
    hipStream_t s = nullptr;
};

// pinned host memory, device-mapped and COHERENT (the device's system-scope stores reach the host while the stream is still running:
// the read-backs the host polls for), zeroed
struct PinnedBlock {
    PinnedBlock() = default;
    PinnedBlock(PinnedBlock&& o) noexcept : p(o.p) { o.p = nullptr; }
    PinnedBlock& operator=(PinnedBlock&& o) noexcept { void* t = p; p = o.p; o.p = t; return *this; }
    ~PinnedBlock() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes) {
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) memset(p, 0, bytes); else p = nullptr;
        return e;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }

private:
    void* p = nullptr;
};

// one step of a host spin loop on device-written pinned memory: a pause instruction on x86, a yield elsewhere; after ~20 us of
// spinning (the read-backs normally arrive in ~5 us) the core is handed back between looks
inline void cpu_relax(unsigned spins) {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    asm volatile("" ::: "memory");
#endif
    if (spins > 4096u && (spins & 63u) == 0u) sched_yield();
}

// The host's wait for the sequence number `seq` that a kernel already enqueued on `st` publishes in pinned memory behind its payload
// (k_collect, k_level_collect, k_icp_publish).  poll: the host does not call hipStreamSynchronize (20-75 us until the thread is awake
// again) but looks at that word in its own memory (~5 us); after 200 ms, or without polling, the synchronisation waits and reports.
inline int32_t wait_host_flag(hipStream_t st, const volatile unsigned long long* flag, unsigned long long seq, bool poll) {
    bool seen = false;
    if (poll) {
        (void)hipStreamQuery(st);                               // makes sure the queue is submitted
        (void)hipGetLastError();                                // (hipErrorNotReady is not an error here)
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 1; !(seen = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq); ++spins) {
            if ((spins & 0x3ffu) == 0u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;   // a fault upstream: let the
            cpu_relax(spins);                                                                                             // synchronisation report it
        }
    }
    if (!seen) GSR_HIP(hipStreamSynchronize(st));
    return GSR_OK;
}

// one integer atomic per wave: the first lane with `flag` adds how many lanes have it (call it with the whole wave present)
template <class T>
__device__ __forceinline__ void wave_count(bool flag, T* ctr) {
    const unsigned long long m = __ballot(flag);
    if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(ctr, (T)__popcll(m));
}

inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// grid for a grid-stride elementwise kernel: enough blocks to fill 256 CUs x 8, no more
inline int stride_grid(int64_t n, int block = 256) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;
    return (int)g;
}

// glibc TYPE_3 rand() model (the reference draws parent flags from the never-seeded libc rand(),
// src/cpp_ext/include/base.hpp:44-56).  Product-side implementation; the oracle has its own.
struct GlibcRng {
    uint32_t st[31];
    int f = 3, r = 0;
    void seed(uint32_t s);
    inline uint32_t next() {
        uint32_t v = (st[f] += st[r]);
        if (++f == 31) f = 0;
        if (++r == 31) r = 0;
        return v >> 1;
    }
    inline uint32_t hem_rand() {
        uint32_t x = 0;
        for (int i = 0; i < 8; ++i) x |= (next() & 15u) << (4 * i);
        return x;
    }
};

}  // namespace gsr
