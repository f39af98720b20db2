/*
 * dvo_upload_ring.h -- the landing pipeline of the frame uploads as one owning type.  Two landing buffers (and, for sources in
 * pageable host memory, their pinned mirrors) are filled through two copy streams while the consumer stream preprocesses the
 * other one.  A chunk takes one turn:
 *
 *     acquire      the next buffer; the copy streams wait for its previous consumer
 *     mirror_free  (mirror routes) the host waits until the mirror's previous copies have left
 *     ... the caller enqueues the chunk's copies or gathers on copy_stream(0) / copy_stream(1) ...
 *     copied       both copy streams are marked; the turn passes to the other buffer
 *     consumer_waits   the consumer stream sees the copies
 *     ... the caller enqueues the kernels that read the landing buffer ...
 *     consumed     the buffer is free again once those kernels have run
 *
 * The turn is committed by `copied`: an error further down leaves events and turn consistent.  Beside it SourceTable, the
 * address table of the sources that are read in place.  Needs only the HIP runtime API and dvo_buffers.h:
 * tests/host/upload_ring_main.cpp walks both over fakes of the HIP calls under a sanitizer.  Internal; not installed.
 */
#ifndef DVO_UPLOAD_RING_H_
#define DVO_UPLOAD_RING_H_

#include "dvo_buffers.h"

namespace dvo_host {

#define DVO_RING_TRY(expr)                        \
    do {                                          \
        const hipError_t ring_e_ = (expr);        \
        if (ring_e_ != hipSuccess) return ring_e_; \
    } while (0)

class UploadRing {
    DevBuf<unsigned char> up_buf[2];
    PinnedBuf<unsigned char> up_host[2];       /* pinned mirrors: small images are gathered here and go up in one copy */
    hipStream_t copy_[2] = {nullptr, nullptr};  /* two SDMA queues: frames alternate between them */
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_copied2[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    bool up_used[2] = {false, false};           /* the buffer has a pending ev_copied and, soon, ev_done */
    int up_next = 0;
public:
    UploadRing() = default;
    UploadRing(const UploadRing &) = delete;
    UploadRing &operator=(const UploadRing &) = delete;
    ~UploadRing() {
        for (hipStream_t s : copy_)
            if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        for (int b = 0; b < 2; b++)
            for (hipEvent_t e : {ev_copied[b], ev_copied2[b], ev_done[b]})
                if (e) (void)hipEventDestroy(e);
    }

    /* copy streams and events, at first use */
    hipError_t create() {
        if (copy_[0]) return hipSuccess;
        /* highest priority: the kernels that pull mapped host memory (DVO_UPLOAD_MAPPED) must not queue behind the
         * preprocessing of the previous chunk -- the PCIe link is the longer pole */
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        DVO_RING_TRY(hipStreamCreateWithPriority(&copy_[0], hipStreamNonBlocking, prio_hi));
        DVO_RING_TRY(hipStreamCreateWithPriority(&copy_[1], hipStreamNonBlocking, prio_hi));
        const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;      /* producers and consumers are kernels / DMAs of this device */
        for (int b = 0; b < 2; b++) {
            DVO_RING_TRY(hipEventCreateWithFlags(&ev_copied[b], evf));
            DVO_RING_TRY(hipEventCreateWithFlags(&ev_copied2[b], evf));
            DVO_RING_TRY(hipEventCreateWithFlags(&ev_done[b], evf));
        }
        return hipSuccess;
    }
    /* landing buffers of at least `bytes` each (+ their pinned mirrors when the sources are host buffers).  consumer_idle() waits
     * for the consumer stream.  Both landing buffers and both mirrors, or none: buffer 0's size speaks for its twin */
    template <class Wait>
    hipError_t grow(size_t bytes, bool mirrors, Wait &&consumer_idle) {
        const bool grow_dev = bytes > up_buf[0].size(), grow_host = mirrors && bytes > up_host[0].size();
        if (!grow_dev && !grow_host) return hipSuccess;
        DVO_RING_TRY(hipStreamSynchronize(copy_[0]));
        DVO_RING_TRY(hipStreamSynchronize(copy_[1]));
        DVO_RING_TRY(consumer_idle());
        hipError_t e = hipSuccess;
        for (int b = 0; b < 2; b++) {
            if (grow_dev && e == hipSuccess) e = up_buf[b].alloc(bytes);
            if (grow_host && e == hipSuccess) e = up_host[b].alloc(bytes);
            up_used[b] = false;
        }
        if (e != hipSuccess)
            for (int b = 0; b < 2; b++) { up_buf[b].reset(); up_host[b].reset(); }
        return e;
    }

    hipStream_t copy_stream(int i) const { return copy_[i]; }
    unsigned char *landing(int b) const { return up_buf[b]; }
    unsigned char *mirror(int b) const { return up_host[b]; }
    size_t landing_bytes() const { return up_buf[0].size(); }
    size_t mirror_bytes() const { return up_host[0].size(); }
    bool used(int b) const { return up_used[b]; }
    int next() const { return up_next; }

    hipError_t acquire(int *b) {
        *b = up_next;
        if (up_used[*b]) {                                  /* the buffer's previous consumer (two chunks back) has read it */
            DVO_RING_TRY(hipStreamWaitEvent(copy_[0], ev_done[*b], 0));
            DVO_RING_TRY(hipStreamWaitEvent(copy_[1], ev_done[*b], 0));
        }
        return hipSuccess;
    }
    /* the mirror's previous copies have left: both queues (the cameras path sends its depth half on the second) */
    hipError_t mirror_free(int b) {
        if (!up_used[b]) return hipSuccess;
        DVO_RING_TRY(hipEventSynchronize(ev_copied[b]));
        return hipEventSynchronize(ev_copied2[b]);
    }
    hipError_t copied(int b) {
        DVO_RING_TRY(hipEventRecord(ev_copied[b], copy_[0]));
        DVO_RING_TRY(hipEventRecord(ev_copied2[b], copy_[1]));
        up_used[b] = true;
        up_next = b ^ 1;
        return hipSuccess;
    }
    /* everything enqueued on `consumer` after this sees the copies */
    hipError_t consumer_waits(int b, hipStream_t consumer) {
        DVO_RING_TRY(hipStreamWaitEvent(consumer, ev_copied[b], 0));
        return hipStreamWaitEvent(consumer, ev_copied2[b], 0);
    }
    /* the kernels reading the landing buffer are enqueued */
    hipError_t consumed(int b, hipStream_t consumer) { return hipEventRecord(ev_done[b], consumer); }
};

/* Camera frames that already sit in HBM are read where they are (round 6): their addresses go up as a table, pinned staging ->
 * device, on the consumer stream. */
class SourceTable {
    DevBuf<void *> dev_;
    PinnedBuf<void *> host_;
    hipEvent_t sent_ = nullptr;
public:
    SourceTable() = default;
    SourceTable(const SourceTable &) = delete;
    SourceTable &operator=(const SourceTable &) = delete;
    ~SourceTable() { if (sent_) (void)hipEventDestroy(sent_); }

    /* room for n addresses, and a staging table nobody reads any more.  consumer_idle() waits for the consumer stream */
    template <class Wait>
    hipError_t reserve(size_t n, Wait &&consumer_idle) {
        if (n > host_.size()) {
            DVO_RING_TRY(consumer_idle());
            host_.reset();                          /* allocated last: its size speaks for both */
            DVO_RING_TRY(dev_.alloc(n));
            DVO_RING_TRY(host_.alloc(n));
        }
        if (!sent_) return hipEventCreateWithFlags(&sent_, hipEventDisableTiming);
        /* the staging table's previous copy has gone up; the DEVICE table's readers are ahead of this call's copy on the stream */
        return hipEventSynchronize(sent_);
    }
    void **staging() const { return host_; }
    void *const *device() const { return dev_; }
    size_t size() const { return host_.size(); }
    /* the first n staged addresses go up on `consumer` */
    hipError_t send(size_t n, hipStream_t consumer) {
        DVO_RING_TRY(hipMemcpyAsync(dev_, host_, sizeof(void *) * n, hipMemcpyHostToDevice, consumer));
        return hipEventRecord(sent_, consumer);
    }
};

#undef DVO_RING_TRY

}  // namespace dvo_host
#endif
