/* Walks the landing pipeline of the frame uploads, rgbd_odometry_amd/csrc/dvo_upload_ring.h, over counting fakes of the HIP calls it
 * makes (plain malloc underneath, the n-th allocation can be told to fail; streams and events are counted; every stream and event
 * call goes into a log).  A driver takes the ring through chunks the way the upload paths do, and the ordering rules are then read
 * off the log.  Stand-alone: built with the address and undefined-behaviour sanitizers by tests/test_upload_ring_cpu.py, linked
 * without the HIP runtime. */
#include "dvo_upload_ring.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

namespace {
std::set<void *> g_live_dev, g_live_host;
int g_allocs = 0, g_fail_at = 0;                  /* g_fail_at: the n-th allocation from now fails (0: none) */
int g_streams = 0, g_events = 0, g_prio_asked = 0;
unsigned g_event_flags = 0, g_stream_flags = 0;

enum Op { RECORD, STREAM_WAIT, EVENT_SYNC, STREAM_SYNC, COPY, HOST_WRITE, KERNEL, CONSUMER_IDLE, ALLOC };
struct Call { Op op; const void *stream; const void *event; const void *dst; int buf; };      /* buf: of the driver's own entries */
std::vector<Call> g_log;

int live() { return (int)(g_live_dev.size() + g_live_host.size()); }
hipError_t fake_alloc(std::set<void *> &pool, void **p, size_t bytes) {
    *p = nullptr;
    g_log.push_back({ALLOC, nullptr, nullptr, nullptr, -1});
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
hipError_t hipDeviceGetStreamPriorityRange(int *lo, int *hi) { *lo = 0; *hi = -3; return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int prio) {
    *s = reinterpret_cast<hipStream_t>(new char);
    g_streams++; g_stream_flags = flags; g_prio_asked = prio;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { g_log.push_back({STREAM_SYNC, s, nullptr, nullptr, -1}); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { delete reinterpret_cast<char *>(s); g_streams--; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) {
    *e = reinterpret_cast<hipEvent_t>(new char);
    g_events++; g_event_flags = flags;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { delete reinterpret_cast<char *>(e); g_events--; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { g_log.push_back({RECORD, s, e, nullptr, -1}); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { g_log.push_back({STREAM_WAIT, s, e, nullptr, -1}); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { g_log.push_back({EVENT_SYNC, nullptr, e, nullptr, -1}); return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t s) {
    std::memcpy(dst, src, bytes);                       /* the sanitizer sees a copy beyond either block */
    g_log.push_back({COPY, s, nullptr, dst, -1});
    return hipSuccess;
}
}

using namespace dvo_host;

namespace {
char g_consumer_tag;
hipStream_t consumer() { return reinterpret_cast<hipStream_t>(&g_consumer_tag); }
hipError_t consumer_idle() { g_log.push_back({CONSUMER_IDLE, consumer(), nullptr, nullptr, -1}); return hipSuccess; }

/* one chunk, as the upload paths take it; stop_after_copied: an error between "copied" and "consumed" */
int drive_chunk(UploadRing &R, size_t bytes, bool through_mirror, bool stop_after_copied = false) {
    int b = -1;
    CHECK(R.acquire(&b) == hipSuccess && (b == 0 || b == 1));
    if (through_mirror) {
        CHECK(R.mirror_free(b) == hipSuccess);
        std::memset(R.mirror(b), 0x5a, bytes);
        g_log.push_back({HOST_WRITE, nullptr, nullptr, nullptr, b});
        CHECK(hipMemcpyAsync(R.landing(b), R.mirror(b), bytes / 2, hipMemcpyHostToDevice, R.copy_stream(0)) == hipSuccess);
        CHECK(hipMemcpyAsync(R.landing(b) + bytes / 2, R.mirror(b) + bytes / 2, bytes - bytes / 2, hipMemcpyHostToDevice, R.copy_stream(1)) == hipSuccess);
    } else {
        std::vector<unsigned char> src(bytes, 1);
        CHECK(hipMemcpyAsync(R.landing(b), src.data(), bytes, hipMemcpyHostToDevice, R.copy_stream(b)) == hipSuccess);
    }
    CHECK(R.copied(b) == hipSuccess);
    if (stop_after_copied) return b;
    CHECK(R.consumer_waits(b, consumer()) == hipSuccess);
    g_log.push_back({KERNEL, consumer(), nullptr, nullptr, b});
    CHECK(R.consumed(b, consumer()) == hipSuccess);
    return b;
}

/* reads the ordering rules off the log of a run of `chunks` whole chunks on a ring that was idle before */
void check_log(const UploadRing &R, int chunks, bool through_mirror) {
    const void *cs[2] = {R.copy_stream(0), R.copy_stream(1)};
    const unsigned char *land[2] = {R.landing(0), R.landing(1)};
    const size_t size = R.landing_bytes();
    std::map<const void *, int> done_of, copied_of;      /* event -> buffer, learnt where the driver's own entries name the buffer */
    bool used[2] = {false, false};                        /* the buffer has been read by a kernel: a copy into it must wait */
    bool mirror_sent[2] = {false, false};                 /* the mirror has a copy in flight: a host write must wait */
    std::set<const void *> copy_waited[2], consumer_waited, host_synced;
    const void *pending_copied[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}, *pending_done[2] = {nullptr, nullptr};
    int done_records = 0, copied_records = 0, kernels = 0;
    int last_buf = -1;
    for (const Call &k : g_log) {
        switch (k.op) {
        case COPY: {
            const unsigned char *d = static_cast<const unsigned char *>(k.dst);
            const int b = (d >= land[0] && d < land[0] + size) ? 0 : 1;
            CHECK(d >= land[b] && d < land[b] + size && (k.stream == cs[0] || k.stream == cs[1]));
            if (used[b]) CHECK(pending_done[b] && copy_waited[0].count(pending_done[b]) && copy_waited[1].count(pending_done[b]));
            if (through_mirror) mirror_sent[b] = true;
            last_buf = b;
            break;
        }
        case HOST_WRITE:
            if (mirror_sent[k.buf]) CHECK(host_synced.count(pending_copied[k.buf][0]) && host_synced.count(pending_copied[k.buf][1]));
            break;
        case RECORD:
            if (k.stream == consumer()) {                 /* done: after the kernel of the chunk */
                CHECK(last_buf >= 0);
                pending_done[last_buf] = k.event; done_records++;
                copy_waited[0].erase(k.event); copy_waited[1].erase(k.event);
                CHECK(!done_of.count(k.event) || done_of[k.event] == last_buf);
                done_of[k.event] = last_buf;
            } else {
                const int q = k.stream == cs[0] ? 0 : 1;
                CHECK(k.stream == cs[q] && last_buf >= 0);
                pending_copied[last_buf][q] = k.event; copied_records++;
                consumer_waited.erase(k.event); host_synced.erase(k.event);
                CHECK(!copied_of.count(k.event) || copied_of[k.event] == 2 * last_buf + q);
                copied_of[k.event] = 2 * last_buf + q;
            }
            break;
        case STREAM_WAIT:
            if (k.stream == consumer()) consumer_waited.insert(k.event);
            else copy_waited[k.stream == cs[0] ? 0 : 1].insert(k.event);
            break;
        case EVENT_SYNC: host_synced.insert(k.event); break;
        case KERNEL:
            CHECK(k.buf == last_buf && pending_copied[k.buf][0] && pending_copied[k.buf][1]);
            CHECK(consumer_waited.count(pending_copied[k.buf][0]) && consumer_waited.count(pending_copied[k.buf][1]));
            used[k.buf] = true; kernels++;
            break;
        default: break;
        }
    }
    CHECK(kernels == chunks && done_records == chunks && copied_records == 2 * chunks);      /* `done` once per chunk */
    CHECK((int)done_of.size() == std::min(chunks, 2) && (int)copied_of.size() == 2 * std::min(chunks, 2));
}

void walk_pipeline() {
    for (int through_mirror = 0; through_mirror < 2; through_mirror++)
        for (int chunks = 1; chunks <= 5; chunks++) {
            {
                UploadRing R;
                CHECK(R.create() == hipSuccess && g_streams == 2 && g_events == 6);
                CHECK(g_prio_asked == -3 && g_stream_flags == hipStreamNonBlocking);          /* the highest priority the device has */
                CHECK(g_event_flags == (hipEventDisableTiming | hipEventDisableSystemFence));
                CHECK(R.create() == hipSuccess && g_streams == 2 && g_events == 6);            /* at first use only */
                CHECK(R.grow(256, through_mirror != 0, consumer_idle) == hipSuccess);
                CHECK(live() == (through_mirror ? 4 : 2) && R.landing_bytes() == 256 && R.mirror_bytes() == (through_mirror ? 256u : 0u));
                g_log.clear();
                for (int k = 0; k < chunks; k++) CHECK(drive_chunk(R, 256, through_mirror != 0) == (k & 1));      /* the buffers alternate */
                check_log(R, chunks, through_mirror != 0);
                CHECK(R.next() == (chunks & 1));
            }
            CHECK(live() == 0 && g_streams == 0 && g_events == 0);                             /* destruction leaves nothing live */
        }
}

void walk_error_between_copied_and_consumed() {
    UploadRing R;
    CHECK(R.create() == hipSuccess && R.grow(64, true, consumer_idle) == hipSuccess);
    CHECK(drive_chunk(R, 64, true) == 0);
    CHECK(drive_chunk(R, 64, true, true) == 1 && R.used(1) && R.next() == 0);      /* the call ends in an error: the turn has passed on */
    g_log.clear();
    CHECK(drive_chunk(R, 64, true) == 0 && drive_chunk(R, 64, true) == 1 && drive_chunk(R, 64, true) == 0);
    /* buffer 1's copies of the broken call are waited for like any other: its mirror by the host, and the copy streams on its `done` */
    int syncs = 0, waits = 0;
    for (const Call &k : g_log) { syncs += k.op == EVENT_SYNC; waits += k.op == STREAM_WAIT && k.stream != consumer(); }
    CHECK(syncs == 6 && waits == 6);
}

void walk_growth() {
    for (int mirrors = 0; mirrors < 2; mirrors++)
        for (int n = 1; n <= (mirrors ? 4 : 2); n++) {
            UploadRing R;
            CHECK(R.create() == hipSuccess && R.grow(100, mirrors != 0, consumer_idle) == hipSuccess);
            drive_chunk(R, 100, mirrors != 0);
            drive_chunk(R, 100, mirrors != 0);
            CHECK(R.used(0) && R.used(1));
            g_log.clear();
            CHECK(R.grow(100, mirrors != 0, consumer_idle) == hipSuccess && R.grow(7, mirrors != 0, consumer_idle) == hipSuccess && g_log.empty());   /* fits: nothing happens */
            CHECK(R.used(0) && R.used(1));
            g_fail_at = n;
            CHECK(R.grow(200, mirrors != 0, consumer_idle) == hipErrorOutOfMemory);
            CHECK(live() == 0 && R.landing_bytes() == 0 && R.mirror_bytes() == 0);             /* all four, or none */
            for (int b = 0; b < 2; b++) CHECK(!R.landing(b) && !R.mirror(b) && !R.used(b));
            /* both copy streams and the consumer were drained before the first block went */
            CHECK(g_log.size() >= 4 && g_log[0].op == STREAM_SYNC && g_log[0].stream == R.copy_stream(0) && g_log[1].op == STREAM_SYNC &&
                  g_log[1].stream == R.copy_stream(1) && g_log[2].op == CONSUMER_IDLE && g_log[3].op == ALLOC);
            CHECK(R.grow(200, mirrors != 0, consumer_idle) == hipSuccess && live() == (mirrors ? 4 : 2) && R.landing_bytes() == 200);   /* a later grow works */
            CHECK(drive_chunk(R, 200, mirrors != 0) >= 0);
        }
    CHECK(live() == 0 && g_streams == 0 && g_events == 0);
    {   /* mirrors join landing buffers that are large enough already: only the two pinned blocks are made */
        UploadRing R;
        CHECK(R.create() == hipSuccess && R.grow(100, false, consumer_idle) == hipSuccess && live() == 2);
        unsigned char *l0 = R.landing(0);
        drive_chunk(R, 100, false);
        CHECK(R.grow(50, true, consumer_idle) == hipSuccess && live() == 4 && R.landing(0) == l0 && R.mirror_bytes() == 50 && !R.used(0));
        g_fail_at = 2;                                      /* ... and a failure there empties the landing buffers too */
        CHECK(R.grow(100, true, consumer_idle) == hipErrorOutOfMemory && live() == 0 && R.landing_bytes() == 0);
    }
    CHECK(live() == 0 && g_streams == 0 && g_events == 0);
}

void walk_source_table() {
    {
        SourceTable T;
        g_log.clear();
        CHECK(T.reserve(8, consumer_idle) == hipSuccess && T.size() == 8 && live() == 2 && g_events == 1);
        CHECK(g_event_flags == hipEventDisableTiming);
        CHECK(g_log.size() == 3 && g_log[0].op == CONSUMER_IDLE);                              /* the first use has no copy to wait for */
        for (int i = 0; i < 8; i++) T.staging()[i] = &g_log;
        CHECK(T.send(8, consumer()) == hipSuccess && T.device()[7] == &g_log);
        g_log.clear();
        CHECK(T.reserve(6, consumer_idle) == hipSuccess && g_log.size() == 1 && g_log[0].op == EVENT_SYNC);      /* fits: only the staging copy's wait */
        g_fail_at = 2;                                      /* the pinned half fails: it is allocated last, its size speaks for both */
        CHECK(T.reserve(16, consumer_idle) == hipErrorOutOfMemory && T.size() == 0);
        CHECK(T.reserve(4, consumer_idle) == hipSuccess && T.size() == 4 && live() == 2);
        g_fail_at = 1;
        CHECK(T.reserve(16, consumer_idle) == hipErrorOutOfMemory && T.size() == 0);
        CHECK(T.reserve(16, consumer_idle) == hipSuccess && T.size() == 16 && live() == 2 && g_events == 1);
    }
    CHECK(live() == 0 && g_events == 0);
}
}  // namespace

int main() {
    walk_pipeline();
    walk_error_between_copied_and_consumed();
    walk_growth();
    walk_source_table();
    CHECK(live() == 0 && g_streams == 0 && g_events == 0);
    std::puts("ok");
    return 0;
}
