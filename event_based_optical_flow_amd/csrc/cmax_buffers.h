// Owning buffers of the library's host code: device memory (DevBuf) and pinned host staging (PinnedBuf), grown on demand, and the wait
// on a run counter that a kernel writes into such staging (wait_run_counter).
// Needs the HIP runtime and cmax_common.h only (tests/buffers_check.hip compiles it without the handle).
//
// The synchronisation rule, for every buffer: the stream is synchronised before memory that may be in use by work queued on it is
// freed, and only then -- a buffer that holds nothing grows without a wait.  (hipFree synchronises the device anyway; the wait in front
// of it orders nothing anew, it names the stream whose work the memory belongs to.)
#pragma once

#include <atomic>
#include <cstring>
#include <utility>

#include "cmax_common.h"

namespace cmax {

// `count` elements of device memory.  reserve() keeps what is there while it is large enough and otherwise allocates EXACTLY what was
// asked for (no geometric growth: the event arrays of a 20M-event batch are not to be held twice); the contents do not survive a
// growth.  `counter` (may be null) is the owner's tally of live bytes: reserve adds to it, release takes off again.
template <typename T>
class __attribute__((visibility("hidden"))) DevBuf {
   public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    int64_t capacity() const { return cap_; }  // elements

    void release() {
        if (p_) (void)hipFree(p_);
        if (counter_) *counter_ -= cap_ * (int64_t)sizeof(T);
        p_ = nullptr;
        cap_ = 0;
        counter_ = nullptr;
    }

    // *grew (optional) = new memory was obtained: its contents are the allocator's, callers that rely on zeros clear it
    int reserve(int64_t *counter, int64_t count, hipStream_t stream, bool *grew = nullptr) {
        if (grew) *grew = false;
        if (count <= cap_) return 0;
        if (p_) {
            CMAX_CHECK_HIP(hipStreamSynchronize(stream));
            release();
        }
        if (count <= 0) count = 1;
        const hipError_t e = hipMalloc((void **)&p_, (size_t)count * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            set_error("hipMalloc(%lld bytes) failed: %s", (long long)(count * sizeof(T)), hipGetErrorString(e));
            return CMAX_ENOMEM;
        }
        cap_ = count;
        counter_ = counter;
        if (counter_) *counter_ += cap_ * (int64_t)sizeof(T);
        if (grew) *grew = true;
        return 0;
    }

    friend void swap(DevBuf &a, DevBuf &b) {
        std::swap(a.p_, b.p_);
        std::swap(a.cap_, b.cap_);
        std::swap(a.counter_, b.counter_);
    }

   private:
    T *p_ = nullptr;
    int64_t cap_ = 0;
    int64_t *counter_ = nullptr;
};

// Buffers that grow together: all of them are freed before the first one is allocated again (the allocator sees the frees first),
// behind ONE wait for the stream.
template <typename... B>
static int release_all(hipStream_t stream, B &...b) {
    if ((... || (b.get() != nullptr))) CMAX_CHECK_HIP(hipStreamSynchronize(stream));
    (b.release(), ...);
    return 0;
}

// Pinned host staging.  Grows by half as much again (+64): the work list and the read-back follow the batch, and a pinned allocation is slow.
// Coherent + mapped: kernels write results and run counters straight into these buffers and the host polls them (cmax_objective_host,
// the patch plan's tail) -- visibility must not hang on HIP_HOST_COHERENT; zeroed: a flag word is polled before anything ever wrote it.
// Nothing waits before the old memory is freed: its users wait for the last copy out of it themselves (an event, or the stream).
// dev(): the address a kernel writes the block through, taken where the memory is obtained -- null whenever get() is.
template <typename T>
class __attribute__((visibility("hidden"))) PinnedBuf {
   public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *dev() const { return dev_; }
    int64_t capacity() const { return cap_; }

    void release() {
        if (p_) (void)hipHostFree(p_);
        p_ = dev_ = nullptr;
        cap_ = 0;
    }

    int reserve(int64_t count) {
        if (count <= cap_) return 0;
        release();
        const int64_t want = count + count / 2 + 64;
        if (hipHostMalloc((void **)&p_, (size_t)want * sizeof(T), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
            p_ = nullptr;
            set_error("hipHostMalloc(%lld bytes) failed", (long long)(want * sizeof(T)));
            return CMAX_ENOMEM;
        }
        std::memset((void *)p_, 0, (size_t)want * sizeof(T));
        cap_ = want;
        if (hipHostGetDevicePointer((void **)&dev_, p_, 0) != hipSuccess) {
            (void)hipGetLastError();
            dev_ = p_;  // unified addressing: pinned host memory is addressable from the device as it is
        }
        return 0;
    }

   private:
    T *p_ = nullptr, *dev_ = nullptr;
    int64_t cap_ = 0;
};

// The one wait on a run counter: a kernel stores `expected` into *flag (pinned memory) behind a system-wide fence once its results are
// visible.  Polling that word returns as soon as the last kernel has written, without the sleep / wake-up of hipStreamSynchronize (~10 us
// late, profiles/r02_solver_objective.txt); when `spins` polls have not seen it -- none are made with spins == 0 -- the stream is waited
// for like everybody else does.  *seen = the counter's value at return: what a value other than `expected` means is the caller's to say.
static inline int wait_run_counter(volatile unsigned long long *flag, unsigned long long expected, long spins, hipStream_t stream,
                                   unsigned long long *seen) {
    for (long spin = 0; spin < spins && *flag != expected; ++spin) {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#elif defined(__aarch64__)
        asm volatile("yield" ::: "memory");
#endif
    }
    if (*flag != expected) CMAX_CHECK_HIP(hipStreamSynchronize(stream));
    *seen = *flag;
    std::atomic_thread_fence(std::memory_order_acquire);
    return 0;
}

}  // namespace cmax
