// Stand-alone host check of csrc/cmax_buffers.h (tests/test_buffers.py compiles and runs it): the header alone, with this file's own
// cmax::set_error.  Without a device every allocation fails, and the buffers must say so every time; with one, a few KB are reserved,
// regrown, swapped and released.  Prints "no-device ok" / "device ok" and returns 0, or names the failed check and returns 1.
#include <cstdarg>
#include <cstdio>

#include "../event_based_optical_flow_amd/csrc/cmax_buffers.h"

namespace cmax {
static char g_error[512];
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
}  // namespace cmax

using cmax::DevBuf;
using cmax::PinnedBuf;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, cmax::g_error); \
            g_failed = 1;                                                 \
        }                                                                 \
    } while (0)

static void check_without_device() {
    int64_t bytes = 0;
    {
        DevBuf<float> a, b;
        bool grew = true;
        CHECK(a.reserve(&bytes, 1000, nullptr, &grew) == CMAX_ENOMEM);
        CHECK(!grew && a.get() == nullptr && a.capacity() == 0 && bytes == 0);
        CHECK(cmax::g_error[0] != 0);
        a.release();
        CHECK(a.get() == nullptr && a.capacity() == 0 && bytes == 0);
        swap(a, b);
        CHECK(a.get() == nullptr && b.get() == nullptr && a.capacity() == 0 && b.capacity() == 0);
        // a second request, smaller than the failed one: the buffer must not believe it holds anything
        CHECK(a.reserve(&bytes, 10, nullptr) == CMAX_ENOMEM);
        CHECK(a.get() == nullptr && a.capacity() == 0 && bytes == 0);
        CHECK(cmax::release_all(nullptr, a, b) == 0);
        PinnedBuf<int> p;
        CHECK(p.reserve(100) == CMAX_ENOMEM);
        CHECK(p.get() == nullptr && p.dev() == nullptr && p.capacity() == 0);  // the device view fails with the pointer
        CHECK(p.reserve(10) == CMAX_ENOMEM);
        CHECK(p.get() == nullptr && p.dev() == nullptr);
        p.release();
        CHECK(p.dev() == nullptr);
    }  // (the destructors of empty buffers)
    CHECK(bytes == 0);
}

static void check_with_device() {
    int64_t bytes = 0;
    hipStream_t s = nullptr;
    {
        DevBuf<float> a, b;
        bool grew = false;
        CHECK(a.reserve(&bytes, 0, s) == 0 && a.get() == nullptr && bytes == 0);  // nothing asked for, nothing held
        CHECK(a.reserve(&bytes, 1000, s, &grew) == 0);
        CHECK(grew && a.get() != nullptr && a.capacity() == 1000 && bytes == 4000);
        float *first = a.get();
        CHECK(hipMemsetAsync(a, 0, 4000, s) == hipSuccess);  // (work on the stream the regrowth below has to wait for)
        CHECK(a.reserve(&bytes, 500, s, &grew) == 0);
        CHECK(!grew && a.get() == first && a.capacity() == 1000 && bytes == 4000);
        // held until the regrowth is over: the allocator cannot hand the freed address out again
        DevBuf<float> hold;
        CHECK(hold.reserve(nullptr, 1000, s) == 0);
        CHECK(a.reserve(&bytes, 1500, s, &grew) == 0);
        CHECK(grew && a.get() != nullptr && a.get() != first && a.capacity() == 1500 && bytes == 6000);  // the one live allocation
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        CHECK(hipMemGetAddressRange(&base, &size, a.get()) == hipSuccess && base == (hipDeviceptr_t)a.get() && size == 6000);  // exactly what was asked for
        hold.release();
        CHECK(b.reserve(&bytes, 300, s) == 0 && bytes == 6000 + 1200);
        float *pa = a.get(), *pb = b.get();
        swap(a, b);
        CHECK(a.get() == pb && b.get() == pa && a.capacity() == 300 && b.capacity() == 1500 && bytes == 7200);
        a.release();
        CHECK(a.get() == nullptr && a.capacity() == 0 && bytes == 6000);
        CHECK(cmax::release_all(s, a, b) == 0);
        CHECK(b.get() == nullptr && b.capacity() == 0 && bytes == 0);
        CHECK(b.reserve(&bytes, 64, s) == 0 && bytes == 256);
        PinnedBuf<int> p;
        CHECK(p.reserve(100) == 0 && p.capacity() == 100 + 50 + 64);
        int sum = 0;
        for (int64_t i = 0; i < p.capacity(); ++i) sum |= p[i];
        CHECK(sum == 0);  // zero-filled
        // the device view: there with the memory, kept by a reserve that fits, the new block's after one that grows, gone with release
        auto views_block = [](const PinnedBuf<int> &buf) {
            hipPointerAttribute_t at;
            return buf.dev() != nullptr && hipPointerGetAttributes(&at, buf.dev()) == hipSuccess && at.hostPointer == (void *)buf.get() &&
                   at.devicePointer == (void *)buf.dev();
        };
        CHECK(views_block(p));
        int *pp = p.get(), *pd = p.dev();
        CHECK(p.reserve(200) == 0 && p.get() == pp && p.dev() == pd);
        CHECK(p.reserve(1000) == 0 && p.capacity() == 1000 + 500 + 64);
        CHECK(views_block(p));
        p.release();
        CHECK(p.get() == nullptr && p.dev() == nullptr && p.capacity() == 0);
    }  // b's destructor takes its bytes off
    CHECK(bytes == 0);
    CHECK(hipDeviceSynchronize() == hipSuccess);
}

int main() {
    int ndev = 0;
    const bool device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    if (device) check_with_device();
    else check_without_device();
    if (g_failed) return 1;
    printf("%s ok\n", device ? "device" : "no-device");
    return 0;
}
