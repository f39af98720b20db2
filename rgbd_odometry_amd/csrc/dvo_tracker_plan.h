/*
 * dvo_tracker_plan.h -- what a tick of the multi-stream tracker does with the streams it lists, decided from each stream's four
 * counters: the frame-store bank of every new frame, the split into streams on their first frame and streams to align, the runs of
 * the frame upload, the host's part of the key-frame rule (TrackerEntry.flags), and how the counters move when the step ends.
 * dvo_capi_tracker.cpp asks here and carries the answer out; nothing in this file touches a tracker, the device or the environment.
 * Host only, no HIP header: tests/host/tracker_plan_main.cpp walks it under a sanitizer.  Internal; not installed.
 */
#ifndef DVO_TRACKER_PLAN_H_
#define DVO_TRACKER_PLAN_H_

#include "../../include/dvo_amd.h"      /* DVO_OK */

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace dvo_host {

/* DVO_TRK_* of dvo_launch.h, which this file cannot include; dvo_capi_tracker.cpp asserts they agree */
constexpr int PLAN_TRK_FORCED = 1;                 /* (nFrame - lastRefFrame) == keyFrameEvery (SolveDVO.cpp:2155-2160) */
constexpr int PLAN_TRK_MAY_SWITCH = 2;             /* lastRefFrame != nFrame - 1 (:2198) */

/* what the plan reads of a stream and the end of a step writes */
struct StreamClock {
    bool started = false;
    long n_frame = 0, last_ref = 0;                /* nFrame / lastRefFrame of SolveDVO::loop */
    int bank = -1;                                 /* bank of the stream's latest frame: slot bank * K + stream */
    /* processFirstFrame: lastRefFrame = 0; nFrame++ (:2014-2021) */
    void first_frame(int new_bank) { started = true; n_frame = 1; last_ref = 0; bank = new_bank; }
    /* an aligned frame whose step returned `event` (>= 2: the previous frame became the key frame, :2198-2232) */
    void aligned_frame(int event, int new_bank) {
        if (event >= 2) last_ref = n_frame - 1;
        n_frame++;
        bank = new_bank;
    }
};

/* consecutive streams (that go to the same bank, with by_bank) form one run: fn(a, b) for every [a, b) of the sorted entries */
template <typename F>
int for_runs(const std::vector<int> &sorted, const std::vector<int> &stream_of, const std::vector<int> &bank_of, bool by_bank, F fn) {
    for (size_t a = 0; a < sorted.size();) {
        size_t b = a + 1;
        while (b < sorted.size() && stream_of[sorted[b]] == stream_of[sorted[b - 1]] + 1 &&
               (!by_bank || bank_of[sorted[b]] == bank_of[sorted[a]]))
            b++;
        const int rc = fn(a, b);
        if (rc) return rc;
        a = b;
    }
    return DVO_OK;
}

struct StepPlan {
    std::vector<int> stream_of, bank_of;           /* per listed entry: its stream, the bank its new frame goes to */
    std::vector<int> order;                        /* the entries sorted by stream */
    std::vector<int> first, align;                 /* ... split: streams on their first frame, streams to align */
    std::vector<int> flags;                        /* PLAN_TRK_* of align[k] */
    std::vector<std::pair<size_t, size_t>> upload_runs;      /* [a, b) over `order`: consecutive streams in one bank */
};

/* banks: a stream's new frame goes to the bank its previous frame is not in; a first frame joins the bank most of the others write this
 * tick (a tie: bank 0), so that a stream that joins late still runs with them.  `clocks` is indexed by stream; its elements are
 * StreamClocks or derive from it */
template <typename Clocks>
StepPlan plan_step(const Clocks &clocks, int count, const int *streams, long key_frame_every) {
    StepPlan p;
    p.stream_of.assign(streams, streams + count);
    p.bank_of.resize(count);
    p.order.resize(count);
    int votes[2] = {0, 0};
    for (int i = 0; i < count; i++) {
        p.order[i] = i;
        const StreamClock &S = clocks[streams[i]];
        if (S.started) votes[p.bank_of[i] = 1 - S.bank]++;
    }
    const int join_bank = votes[1] > votes[0] ? 1 : 0;
    for (int i = 0; i < count; i++)
        if (!clocks[streams[i]].started) p.bank_of[i] = join_bank;
    std::sort(p.order.begin(), p.order.end(), [&](int a, int b) { return p.stream_of[a] < p.stream_of[b]; });
    for (int i : p.order) {
        const StreamClock &S = clocks[p.stream_of[i]];
        if (!S.started) { p.first.push_back(i); continue; }
        p.align.push_back(i);
        p.flags.push_back((S.n_frame - S.last_ref == key_frame_every ? PLAN_TRK_FORCED : 0) |
                          (S.last_ref != S.n_frame - 1 ? PLAN_TRK_MAY_SWITCH : 0));
    }
    for_runs(p.order, p.stream_of, p.bank_of, true, [&](size_t a, size_t b) { p.upload_runs.emplace_back(a, b); return DVO_OK; });
    return p;
}

}  // namespace dvo_host

#endif  // DVO_TRACKER_PLAN_H_
