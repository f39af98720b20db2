/*
 * dvo_launch_memo.h -- the KEY under which enqueue() (dvo_capi.cpp) remembers what a full pass over a resident batch decided, so
 * that a repeated request goes straight to the launch: the request itself, the context's host generation (bumped by every write
 * of the host state the stages read: dvo_ctx.h, Tracked) and the few things the stages read that change without it.  Also the
 * rule for which passes may be remembered at all, and the switch DVO_LAUNCH_MEMO.  The remembered Schedule and LaunchPlan are kept
 * beside the key in the context.  Nothing in this file touches a context, the device or the environment.
 * Host only, no HIP header: tests/host/launch_memo_main.cpp walks it under a sanitizer.  Internal; not installed.
 */
#ifndef DVO_LAUNCH_MEMO_H_
#define DVO_LAUNCH_MEMO_H_

#include "../../include/dvo_amd.h"      /* DVO_MAX_LEVELS */

#include <cstring>

namespace dvo_host {

enum MemoMode { MEMO_ON = 0, MEMO_OFF = 1, MEMO_VERIFY = 2 };
/* DVO_LAUNCH_MEMO: unset or "on" remembers; "off": every call takes the full pass; "verify": every hit also runs the full
 * stages and compares what they decide with what was remembered */
inline MemoMode memo_mode(const char *env) {
    if (env && std::strcmp(env, "off") == 0) return MEMO_OFF;
    if (env && std::strcmp(env, "verify") == 0) return MEMO_VERIFY;
    return MEMO_ON;
}

/* the request, by value (EnqueueRequest of dvo_capi.cpp carries pointers) */
struct MemoRequest {
    int first_pair = 0, n_pairs = 0;
    int n_levels = 0;
    int iters[DVO_MAX_LEVELS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int flags = 0;
    unsigned level_mask = ~0u;
    int forced_team = 0;
    bool listed = false;            /* index-list form: never remembered (the list is the caller's, per call) */
};
inline MemoRequest memo_request(int first_pair, int n_pairs, int n_levels, const int *iters, int flags, unsigned level_mask,
                                int forced_team, bool listed) {
    MemoRequest r;
    r.first_pair = first_pair; r.n_pairs = n_pairs; r.n_levels = n_levels; r.flags = flags;
    r.level_mask = level_mask; r.forced_team = forced_team; r.listed = listed;
    for (int l = 0; l < DVO_MAX_LEVELS; l++) r.iters[l] = (iters && l < n_levels) ? iters[l] : 0;
    return r;
}

struct MemoKey {
    MemoRequest q;
    unsigned long long host_gen = 0;        /* the context's host generation AFTER the remembered pass */
    /* read by the stages, changed without the generation */
    int sched_gen = 0;                      /* the output stamps (ensure_outputs bumps it when it re-allocates) */
    int final_cap = 0;
    unsigned long long energy_size = 0;     /* elements of d_energy */
    unsigned long long h_size = 0;          /* elements of d_H (DVO_FLAG_NORMAL_MATRIX) */
};

/* the first field in which two keys differ; NULL: equal */
inline const char *memo_key_mismatch(const MemoKey &a, const MemoKey &b) {
    if (a.q.first_pair != b.q.first_pair) return "first_pair";
    if (a.q.n_pairs != b.q.n_pairs) return "n_pairs";
    if (a.q.n_levels != b.q.n_levels) return "n_levels";
    if (std::memcmp(a.q.iters, b.q.iters, sizeof(a.q.iters)) != 0) return "iters";
    if (a.q.flags != b.q.flags) return "flags";
    if (a.q.level_mask != b.q.level_mask) return "level_mask";
    if (a.q.forced_team != b.q.forced_team) return "forced_team";
    if (a.q.listed != b.q.listed) return "listed";
    if (a.host_gen != b.host_gen) return "host_gen";
    if (a.sched_gen != b.sched_gen) return "sched_gen";
    if (a.final_cap != b.final_cap) return "final_cap";
    if (a.energy_size != b.energy_size) return "energy_size";
    if (a.h_size != b.h_size) return "h_size";
    return nullptr;
}

/* A pass may be remembered only when an identical second call would issue exactly one kernel launch and nothing else:
 *   - a range request over the whole schedule, with the context's own team size;
 *   - plan_team == 1: a team launch steps its exchange epoch per call (and small batches do not feel the per-pair walks);
 *   - tex16_pending: some now level of the request would still be decoded to 16-byte texels;
 *   - build_possible: some pair of the request wants, or could come to want through its use count, a compact build -- the hit
 *     skips NowState::used(), and `uses` is read only by wants_build of a form that is not built. */
inline bool memo_request_recordable(const MemoRequest &q) { return !q.listed && q.level_mask == ~0u && q.forced_team == 0; }
inline bool memo_recordable(const MemoRequest &q, int plan_team, bool tex16_pending, bool build_possible) {
    return memo_request_recordable(q) && plan_team == 1 && !tex16_pending && !build_possible;
}

struct LaunchMemo {
    bool valid = false;
    MemoKey key;
    unsigned long long full_passes = 0, hits = 0;       /* dvo_get_enqueue_counts */

    void forget() { valid = false; }
    bool matches(const MemoKey &now) const { return valid && memo_key_mismatch(key, now) == nullptr; }
    /* after a full pass: remember it under `now`, or forget what was remembered */
    void record(const MemoKey &now, MemoMode mode, int plan_team, bool tex16_pending, bool build_possible) {
        valid = mode != MEMO_OFF && memo_recordable(now.q, plan_team, tex16_pending, build_possible);
        if (valid) key = now;
    }
};

}  // namespace dvo_host
#endif
