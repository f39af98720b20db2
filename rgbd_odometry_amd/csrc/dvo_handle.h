/*
 * dvo_handle.h -- what every handle of the host layer does the same way: make its device current, turn a hipError_t into a status
 * code, refuse creation without a device, grow a pinned block with its device twin, and count the launches and synchronisations of a
 * call.  Host only; internal, not installed.  It needs the HIP runtime's API header and dvo_buffers.h alone, so a plain C++ compiler
 * builds it against fakes (tests/host/handle_main.cpp); the status codes are include/dvo_amd.h's, which comes before this header.
 */
#ifndef DVO_HANDLE_H_
#define DVO_HANDLE_H_

#include <hip/hip_runtime_api.h>
#include <string>
#include "dvo_buffers.h"

namespace dvo_host {
/* A handle lives on the device that was current when it was created.  Every C entry point makes that device current for its duration
 * and restores the caller's afterwards, so a handle can be driven from a thread whose current device differs (one host thread per GPU,
 * INTEGRATION.md section 3).  A negative ordinal does nothing.  If the caller's device cannot be read nothing is restored, and
 * the handle's is made current all the same only with `blind` (the stand-alone handles; a context leaves the device alone). */
struct OnDevice {
    int prev = -1, dev;
    explicit OnDevice(int d, bool blind = true) : dev(d) {
        if (dev < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) { prev = -1; if (!blind) return; }
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~OnDevice() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
    OnDevice(const OnDevice &) = delete;
    OnDevice &operator=(const OnDevice &) = delete;
};
/* the status code of a failed HIP call */
inline int hip_status(hipError_t e) { return e == hipErrorOutOfMemory ? DVO_ERR_NOMEM : DVO_ERR_HIP; }
/* on an error of `expr`: return fail(h, its status code, "<text>: <the runtime's words>").  A file's own short form passes #expr as
 * `text`, so that the message spells the expression as the source does, macros unexpanded */
#define DVO_HIP_CHECK(fail, h, expr, text)                                                                         \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess) return fail(h, dvo_host::hip_status(e_), std::string(text) + ": " + hipGetErrorString(e_)); \
    } while (0)
/* creation: DVO_OK with a device to run on, else DVO_ERR_NO_DEVICE and why */
inline int device_check(std::string *why) {
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e == hipSuccess && ndev >= 1) return DVO_OK;
    *why = std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") + " (this engine has no CPU fallback)";
    return DVO_ERR_NO_DEVICE;
}
/* A pinned block and a device block of one size: what a call stages on its way up, or its results on their way down.  reserve() comes
 * before anything of the call is enqueued, so a call it fails has changed nothing; nothing is in flight between two calls, and an
 * allocation is a device-wide wait beyond the one synchronisation a call counts. */
struct Staging {
    PinnedBuf<unsigned char> host;
    DevBuf<unsigned char> dev;
    /* room for `bytes` in both (contents undefined when they grow); on a failure both are empty */
    hipError_t reserve(size_t bytes) {
        if (bytes <= host.size() && bytes <= dev.size()) return hipSuccess;
        hipError_t e = host.alloc(bytes);
        if (e == hipSuccess) e = dev.alloc(bytes);
        if (e != hipSuccess) { host.reset(); dev.reset(); }
        return e;
    }
};
/* What the stand-alone handles share.  Their buffers are members of the handle proper: `delete` under an OnDevice frees them there. */
struct Handle {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int last_launches = 0, last_syncs = 0;         /* of the last call that reached the device (CallStats) */
    hipError_t open() {                            /* at creation: the current device and a stream of its own */
        if (hipGetDevice(&device) != hipSuccess) device = 0;
        return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    }
    void close() {                                 /* before `delete`, under an OnDevice: nothing is in flight when the buffers go */
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); stream = nullptr; }
    }
    int stats(int *l, int *s) const { if (l) *l = last_launches; if (s) *s = last_syncs; return DVO_OK; }      /* either may be NULL */
};
/* The bracket of a call for the handle's stats: both are zero from the start, the launches are taken after the last launch and the
 * synchronisation after it returned; a failure in between leaves what was reached.  `counter`: dvo::g_kernel_launches of the thread */
struct CallStats {
    Handle &h;
    const unsigned long long &counter, before;
    CallStats(Handle &h_, const unsigned long long &c) : h(h_), counter(c), before(c) { h.last_launches = 0; h.last_syncs = 0; }
    void launched() { h.last_launches = (int)(counter - before); }
    void synced() { h.last_syncs = 1; }
};
}  // namespace dvo_host
#endif
