// device_buffer_main.cpp -- DeviceBuffer (ndt_amd/csrc/ndt_buffer.hpp) on its own: built and run by test_device_buffer.py.
//
//   device_buffer_main nodevice   no HIP device: a failed hipMalloc leaves an empty buffer and NDT_E_NOMEM, again and again
//   device_buffer_main device     a device: reserve / reuse / grow / head room / release on a stream of its own (a few KB)
//
// Exit 0: every check held; 1: one did not (named on stderr); 77: the machine is not the one the mode is for.
#include "ndt_buffer.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

static int g_code = 0;
static char g_text[256] = "";
int ndt_impl::fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_text, sizeof(g_text), fmt, ap);
    va_end(ap);
    return g_code = code;
}
using ndt_impl::DeviceBuffer;

#define CHECK(cond)                                                                                        \
    do {                                                                                                   \
        if (!(cond)) {                                                                                     \
            fprintf(stderr, "device_buffer_main: line %d: %s does not hold (last error: %s)\n", __LINE__, #cond, g_text);  \
            return 1;                                                                                      \
        }                                                                                                  \
    } while (0)

static int without_device()
{
    DeviceBuffer b;
    b.p = (void *)(size_t)0x1000;       // garbage, as a hipMalloc that fails leaves its out-pointer alone
    CHECK(b.reserve(1024, nullptr, "first") == NDT_E_NOMEM);
    CHECK(g_code == NDT_E_NOMEM && strstr(g_text, "first") != nullptr);
    CHECK(b.p == nullptr && b.bytes == 0);
    CHECK(b.reserve(16, nullptr, "smaller") == NDT_E_NOMEM);       // (a size left standing by the failure would answer NDT_OK)
    CHECK(b.p == nullptr && b.bytes == 0);
    b.release();
    CHECK(b.p == nullptr && b.bytes == 0);
    return 0;
}

static int with_device()
{
    CHECK(hipSetDevice(0) == hipSuccess);
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    DeviceBuffer b;
    b.release();                                                    // harmless on an empty buffer
    CHECK(b.reserve(1000, s, "first") == NDT_OK);
    CHECK(b.p != nullptr && b.bytes >= 1000);
    void *const p0 = b.p;
    const size_t n0 = b.bytes;
    CHECK(b.reserve(500, s, "smaller") == NDT_OK);
    CHECK(b.p == p0 && b.bytes == n0);
    CHECK(b.reserve(0, s, "nothing") == NDT_OK && b.p == p0 && b.bytes == n0);
    CHECK(hipMemsetAsync(b.p, 0x5a, b.bytes, s) == hipSuccess);     // work on the stream that the growth below has to drain
    CHECK(b.reserve(4000, s, "larger") == NDT_OK);
    CHECK(b.p != nullptr && b.bytes >= 4000);
    CHECK(b.as<char>() == (char *)b.p);
    CHECK(hipMemsetAsync(b.p, 0, b.bytes, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess);
    DeviceBuffer roomy;
    CHECK(roomy.reserve(1000, s, "head room", true) == NDT_OK);
    CHECK(roomy.p != nullptr && roomy.bytes == 1000 + 1000 / 4);
    CHECK(roomy.reserve(1250, s, "inside the head room", true) == NDT_OK && roomy.bytes == 1250);
    CHECK(roomy.reserve(1251, s, "past the head room", true) == NDT_OK && roomy.bytes == 1251 + 1251 / 4);
    CHECK(hipMemsetAsync(roomy.p, 0, roomy.bytes, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess);
    b.release();
    CHECK(b.p == nullptr && b.bytes == 0);
    CHECK(b.reserve(0, s, "one byte") == NDT_OK && b.p != nullptr && b.bytes >= 1);
    CHECK(hipMemsetAsync(b.p, 0, b.bytes, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess);
    b.release();
    roomy.release();
    CHECK(roomy.p == nullptr && roomy.bytes == 0);
    CHECK(hipGetLastError() == hipSuccess);
    CHECK(hipStreamDestroy(s) == hipSuccess);
    return 0;
}

int main(int argc, char **argv)
{
    const bool want_device = argc > 1 && !strcmp(argv[1], "device");
    if (!want_device && !(argc > 1 && !strcmp(argv[1], "nodevice"))) {
        fprintf(stderr, "usage: device_buffer_main nodevice | device\n");
        return 2;
    }
    int count = 0;
    const bool have_device = hipGetDeviceCount(&count) == hipSuccess && count > 0;
    printf("device_buffer_main: %d HIP device(s)\n", have_device ? count : 0);
    if (have_device != want_device) return 77;
    const int rc = want_device ? with_device() : without_device();
    if (rc == 0) printf("device_buffer_main: every check held (%s)\n", argv[1]);
    return rc;
}
