/* Walks the scaffold of the stand-alone handles, rgbd_odometry_amd/csrc/dvo_handle.h, over counting fakes of the HIP calls it makes
 * (plain malloc underneath; the n-th allocation, the device query and the device count can be told to fail).  Stand-alone: built with
 * the address and undefined-behaviour sanitizers by tests/test_handle_cpu.py, linked without the HIP runtime. */
#include "../../include/dvo_amd.h"
#include "dvo_handle.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

namespace {
std::set<void *> g_live_dev, g_live_host;
int g_allocs = 0, g_fail_at = 0;                  /* g_fail_at: the n-th allocation from now fails (0: none) */
int g_device = 0, g_sets = 0, g_n_devices = 4, g_streams = 0, g_stream_syncs = 0;
bool g_get_fails = false;
hipError_t g_count_error = hipSuccess;

int live() { return (int)(g_live_dev.size() + g_live_host.size()); }
hipError_t fake_alloc(std::set<void *> &pool, void **p, size_t bytes) {
    *p = nullptr;
    if (g_fail_at > 0 && --g_fail_at == 0) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    pool.insert(*p);
    g_allocs++;
    return hipSuccess;
}
hipError_t fake_free(std::set<void *> &pool, void *p) {
    if (!p) return hipSuccess;
    if (!pool.erase(p)) { std::fprintf(stderr, "free of a block that is not live (double free, or the wrong kind)\n"); std::abort(); }
    std::free(p);
    return hipSuccess;
}

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(g_live_dev, p, bytes); }
hipError_t hipFree(void *p) { return fake_free(g_live_dev, p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return fake_alloc(g_live_host, p, bytes); }
hipError_t hipHostFree(void *p) { return fake_free(g_live_host, p); }
hipError_t hipGetDevice(int *d) {
    if (g_get_fails) return hipErrorInvalidDevice;
    *d = g_device;
    return hipSuccess;
}
hipError_t hipSetDevice(int d) { g_device = d; g_sets++; return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) { *n = g_n_devices; return g_count_error; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : e == hipErrorNoDevice ? "no device" : "other"; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = reinterpret_cast<hipStream_t>(&g_streams); g_streams++; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { g_stream_syncs++; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { g_streams--; return hipSuccess; }
}

using namespace dvo_host;

void walk_staging() {
    {
        Staging s;
        CHECK(s.dev.size() == 0 && s.reserve(0) == hipSuccess && g_allocs == 0);                 /* nothing asked, nothing done */
        CHECK(s.reserve(100) == hipSuccess && s.host.size() == 100 && s.dev.size() == 100);
        CHECK(g_live_host.size() == 1 && g_live_dev.size() == 1 && g_allocs == 2);
        void *h0 = s.host.get(), *d0 = s.dev.get();
        CHECK(s.reserve(100) == hipSuccess && s.reserve(7) == hipSuccess && g_allocs == 2);  /* a request that fits never grows */
        CHECK(s.host.get() == h0 && s.dev.get() == d0);
        CHECK(s.reserve(101) == hipSuccess && s.dev.size() == 101 && s.host.size() == 101 && g_allocs == 4 && live() == 2);
        g_fail_at = 2;                                                                       /* the pinned block grows, the device block fails */
        CHECK(s.reserve(500) == hipErrorOutOfMemory);
        CHECK(live() == 0 && !s.host && !s.dev && s.host.size() == 0 && s.dev.size() == 0);
        g_fail_at = 1;                                                                       /* the pinned block fails: the device block is not tried */
        const int before = g_allocs;
        CHECK(s.reserve(500) == hipErrorOutOfMemory && g_allocs == before && live() == 0 && s.dev.size() == 0);
        CHECK(s.reserve(500) == hipSuccess && s.dev.size() == 500 && s.host.size() == 500 && live() == 2);               /* and a later call works */
    }
    CHECK(live() == 0);                                                                      /* no block is live after destruction */
}

void walk_guard() {
    g_device = 2; g_sets = 0; g_get_fails = false;
    {
        OnDevice g(1);
        CHECK(g_device == 1 && g_sets == 1);
        { OnDevice inner(1); CHECK(g_device == 1 && g_sets == 1); }                          /* already current: nothing */
        CHECK(g_device == 1 && g_sets == 1);
    }
    CHECK(g_device == 2 && g_sets == 2);                                                     /* the caller's device is back */
    { OnDevice g(2); }
    CHECK(g_device == 2 && g_sets == 2);
    { OnDevice g(-1); CHECK(g_device == 2); }                                                /* no handle: nothing, no query either */
    CHECK(g_sets == 2);
    g_get_fails = true;                                                                      /* the caller's device cannot be read */
    { OnDevice g(3); CHECK(g_device == 3 && g_sets == 3); }
    CHECK(g_device == 3 && g_sets == 3);                                                     /* nothing to restore */
    { OnDevice g(1, false); CHECK(g_device == 3 && g_sets == 3); }                           /* a context's guard leaves the device alone then */
    CHECK(g_device == 3 && g_sets == 3);
    g_get_fails = false;
    { OnDevice g(1, false); CHECK(g_device == 1 && g_sets == 4); }                           /* ... and is the same guard otherwise */
    CHECK(g_device == 3 && g_sets == 5);
    g_get_fails = false;
}

int fail_into(std::string *where, int code, const std::string &msg) { *where = msg; return code; }
int checked(std::string *where, hipError_t result) {
    DVO_HIP_CHECK(fail_into, where, result, "result");
    return DVO_OK;
}

void walk_errors() {
    CHECK(hip_status(hipErrorOutOfMemory) == DVO_ERR_NOMEM && hip_status(hipErrorInvalidValue) == DVO_ERR_HIP);
    CHECK(hip_status(hipErrorNoDevice) == DVO_ERR_HIP && hip_status(hipErrorLaunchFailure) == DVO_ERR_HIP);
    std::string msg = "untouched";
    CHECK(checked(&msg, hipSuccess) == DVO_OK && msg == "untouched");
    CHECK(checked(&msg, hipErrorOutOfMemory) == DVO_ERR_NOMEM && msg == "result: out of memory");
    CHECK(checked(&msg, hipErrorInvalidValue) == DVO_ERR_HIP && msg == "result: other");
    std::string why = "untouched";
    g_n_devices = 4; g_count_error = hipSuccess;
    CHECK(device_check(&why) == DVO_OK && why == "untouched");
    g_n_devices = 0;
    CHECK(device_check(&why) == DVO_ERR_NO_DEVICE && why == "no HIP device available: device count is 0 (this engine has no CPU fallback)");
    g_n_devices = 4; g_count_error = hipErrorNoDevice;
    CHECK(device_check(&why) == DVO_ERR_NO_DEVICE && why == "no HIP device available: no device (this engine has no CPU fallback)");
    g_count_error = hipSuccess;
}

struct Thing : Handle { Staging block; };
int call(Thing &t, unsigned long long &launches, int stop_after) {                           /* a call of a handle, cut short on request */
    CallStats stats(t, launches);
    if (stop_after == 0) return DVO_ERR_HIP;
    launches += 3;
    stats.launched();
    if (stop_after == 1) return DVO_ERR_HIP;
    stats.synced();
    return DVO_OK;
}

void walk_handle() {
    g_device = 1;
    Thing *t = new Thing();
    CHECK(t->open() == hipSuccess && t->device == 1 && t->stream && g_streams == 1);
    CHECK(t->block.reserve(64) == hipSuccess && live() == 2);
    unsigned long long launches = 40;                                                        /* the thread's counter: only differences count */
    t->last_launches = 9; t->last_syncs = 9;
    CHECK(call(*t, launches, 2) == DVO_OK && t->last_launches == 3 && t->last_syncs == 1 && launches == 43);
    CHECK(call(*t, launches, 0) == DVO_ERR_HIP && t->last_launches == 0 && t->last_syncs == 0);       /* an early return: both zero */
    CHECK(call(*t, launches, 1) == DVO_ERR_HIP && t->last_launches == 3 && t->last_syncs == 0);       /* launched, never synchronised */
    CHECK(call(*t, launches, 2) == DVO_OK && t->last_launches == 3 && t->last_syncs == 1);
    int l = -1, s = -1;
    CHECK(t->stats(&l, nullptr) == DVO_OK && t->stats(nullptr, &s) == DVO_OK && l == 3 && s == 1);
    g_device = 0; g_stream_syncs = 0;
    {                                                                                        /* destroy: guard, close, delete */
        OnDevice guard(t->device);
        t->close();
        CHECK(g_stream_syncs == 1 && g_streams == 0 && !t->stream);
        t->close();                                                                          /* a second close does nothing */
        CHECK(g_stream_syncs == 1 && g_streams == 0);
        delete t;
        CHECK(live() == 0 && g_device == 1);                                                 /* the buffers went on the handle's device */
    }
    CHECK(g_device == 0);
}

int main() {
    walk_staging();
    walk_guard();
    walk_errors();
    walk_handle();
    CHECK(live() == 0);
    std::puts("ok");
    return 0;
}
