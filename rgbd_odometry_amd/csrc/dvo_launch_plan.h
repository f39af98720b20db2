/*
 * dvo_launch_plan.h -- the SHAPE of a fused alignment launch, decided from a handful of integers: which kernel (packed or
 * one-point-per-lane), 256 / 512 / 1024 threads, the LDS budget of the resident point list, which forms the launch reads, the
 * team size; the tiers of team launches of the wide / tiled schedule; the count of the team exchange records; the
 * longest-first launch order.  dvo_capi.cpp gathers the facts (LaunchFacts) from the context, asks here and carries the answer
 * out on the device; nothing in this file touches a context, the device or the environment.
 * Host only, no HIP header: tests/host/launch_plan_main.cpp walks it under a sanitizer.  Internal; not installed.
 */
#ifndef DVO_LAUNCH_PLAN_H_
#define DVO_LAUNCH_PLAN_H_

#include "../../include/dvo_amd.h"      /* DVO_FLAG_*, DVO_OK, DVO_ERR_* */

#include <algorithm>

namespace dvo_host {

/* constants of HIP headers this file cannot include; dvo_capi.cpp asserts they agree */
constexpr int PLAN_NACC_PAD = 32;                  /* DVO_NACC_PAD of dvo_launch.h */
constexpr int PLAN_PALETTE_BYTES = 8 * 8192;       /* sizeof(float2) * DVO_PAL_MAX of dvo_palette.h */
constexpr int PLAN_SOLO_MAX = 6144;                /* DVO_TILED_SOLO_MAX_DEFAULT of dvo_launch.h */

/* everything the decisions read */
struct LaunchFacts {
    /* dvo_params, and the policy of DVO_COMPACT_NOW (0 default, 1 eager, 2 off) */
    int block_threads = 0, lds_point_bytes = 0, points_in_flight = 0;
    int engine_variant = 0, interpolate_dt = 0;
    int team_size = 0;              /* dvo_params.team_size, or the size a tier of the wide / tiled schedule forces */
    int compact_now_policy = 0;
    /* the launch */
    int n_cu = 256, n_pairs = 1;
    bool listed = false;            /* index-list form (the multi-stream tracker) */
    int flags = 0;
    bool compact = false;           /* every list of the launch has its compact twin (and the parameters allow reading it) */
    bool all_p4 = true;             /* every now level of the launch has its compact form (known after the compact builds) */
    int max_n = 0;                  /* the longest list over the levels that run */
    int n_fine = 0;                 /* the longest list at the schedule's last_level */
    bool pt4_rows_mismatch = false; /* some list's 4-byte twin was encoded against an image of another height than its now level */
    bool has_pair_K = false;        /* the context has per-pair camera models */
    /* static LDS of the candidate kernels, evaluated by the caller (PoseState lives in the .hip files) */
    int fused2_lds[3][2] = {{0, 0}, {0, 0}, {0, 0}};      /* fused2_static_lds(256 | 512 | 1024, with_h) */
    int pose_state_bytes = 0;
};

struct LaunchPlan {
    int err = DVO_OK;               /* a refusal: the error code and its message; nothing else is valid then */
    const char *msg = nullptr;
    bool packed = false;            /* the packed two-points-per-lane kernel (dvo_fused.hip), else the one-point-per-lane kernel */
    int block = 512;
    int points_in_flight = 1;       /* of the one-point-per-lane kernel */
    int lds_bytes = 0, lds_points = 0;
    int no_p4 = 0, no_pt4 = 0;
    int no_lds_tex = 0, force_exact = 0, force_e2 = 0, no_pt4_direct = 0;      /* the engine_variant test switches */
    bool needs_tex16 = false;       /* something in this launch may read 16-byte texels: decode them first */
    int team = 1;
    bool super_team = false;        /* a team over all XCDs (single pair) */
    bool team_fallback = false;     /* a team launch the runtime refuses runs again without teams (not where the size was asked for) */
};

/* engine_variant: 0 = auto (packed two-points-per-lane kernel whenever every list is compact), 1 = always the
 * one-point-per-lane kernel of dvo_kernels.hip (A/B measurements, parity tests of both) */
inline bool plan_packed(const LaunchFacts &f) { return f.compact && f.engine_variant != 1; }
/* the launch reads the compact form of its now levels (dvo_palette.h) where they have one: the caller builds what is due first */
inline bool plan_reads_compact_now(const LaunchFacts &f) { return !(f.engine_variant == 4 || !plan_packed(f) || f.compact_now_policy == 2); }
inline bool plan_block_fixed(int block) { return block == 256 || block == 512 || block == 1024; }
/* the block size the caller asked for, as far as this launch has it */
inline int plan_block_asked(const LaunchFacts &f) {
    int block = f.block_threads;
    /* the packed kernel carries H on both of its one-workgroup-per-pair shapes (round 5); 1024 threads have no such instantiation */
    if ((f.flags & DVO_FLAG_NORMAL_MATRIX) && (!plan_packed(f) || block == 1024)) block = plan_packed(f) ? 0 : 512;
    return block;
}
/* the shape is chosen here (the caller then gathers max_n) */
inline bool plan_block_auto(const LaunchFacts &f) { return !plan_block_fixed(plan_block_asked(f)); }
/* the 256-thread shape is chosen for launches that read the compact form: ask the device which pairs really have one
 * where that decides the shape (round 5, ADVICE r3/r4: `built` is also set for images the form could not hold) */
inline bool shape_depends_on_refusals(const LaunchFacts &f) {
    return !plan_block_fixed(f.block_threads) && (2 * f.n_pairs >= 3 * f.n_cu || f.n_pairs > f.n_cu);
}
/* the team size comes from the length of the finest list (the caller then gathers n_fine): an automatic size, and room for a team of two */
inline bool plan_team_by_n_fine(const LaunchFacts &f) {
    return !f.listed && plan_packed(f) && !(f.flags & DVO_FLAG_NORMAL_MATRIX) && f.team_size < 1 && 16 * ((f.n_pairs + 7) / 8) <= f.n_cu;
}
/* more than 5 % of a level on 16-byte texels: the request-bound shape */
inline bool too_many_refused(int refused, int n_pairs) { return 20 * refused > n_pairs; }

inline LaunchPlan plan_refusal(int code, const char *msg) { LaunchPlan p; p.err = code; p.msg = msg; return p; }

inline LaunchPlan plan_launch(const LaunchFacts &f) {
    LaunchPlan p;
    const int n_pairs = f.n_pairs, n_cu = f.n_cu;
    /* round 5: DVO_FLAG_NORMAL_MATRIX rides on the packed kernel too (its 512-thread shape, no teams: align_fused2_kernel<512, false, true>) */
    const bool with_h = (f.flags & DVO_FLAG_NORMAL_MATRIX) != 0;
    const bool packed = plan_packed(f);
    p.packed = packed;
    p.no_p4 = plan_reads_compact_now(f) ? 0 : 1;
    const bool all_p4 = !p.no_p4 && f.all_p4;
    if (with_h) {
        /* the H-carrying instantiation of the one-point-per-lane kernel exists for 512 threads only (dvo_kernels.hip): size the
         * LDS budget for that, and refuse the combination it has no instantiation for instead of returning unwritten memory */
        if (f.interpolate_dt)
            return plan_refusal(DVO_ERR_INVALID, "DVO_FLAG_NORMAL_MATRIX is not available together with dvo_params.interpolate_dt");
        /* the H-carrying instantiations read the context's K only (per-pair camera models would push them past their scratch budget) */
        if (f.has_pair_K)
            return plan_refusal(DVO_ERR_STATE, "DVO_FLAG_NORMAL_MATRIX is not available on a context with per-pair camera models");
    }
    if (f.listed && !packed) return plan_refusal(DVO_ERR_INVALID, "an index-list launch needs the packed kernel (compact lists, engine_variant != 1)");
    int block = plan_block_asked(f);
    int auto_lds = 0;
    const bool block_auto = !plan_block_fixed(block);
    if (block_auto) {
        /* auto: when the longest point list of the launch fits half a CU's LDS, two 256-thread workgroups
         * per CU overlap each other's serial phases (measured: 320x240x4x50 213 k -> 288 k aligns/s); otherwise
         * one 512-thread workgroup owns the CU and its LDS (640x480: 386 k vs 374 k) */
        const long long max_n = f.max_n;
        /* ... which only pays when there are enough pairs to put two workgroups on a CU: a launch of fewer pairs than
         * half the CUs is latency-bound and 512 threads finish an iteration sooner (single pair, 320x240x4x50:
         * 1.20 -> 1.06 ms) */
        if (max_n * 12 <= 77000 && !f.interpolate_dt && 2 * n_pairs > n_cu) { block = 256; auto_lds = 80 * 1024; }
        /* with the compact now form the loop is no longer request-bound and two workgroups per CU pay even when the lists do
         * not fit half the LDS (640x480x4x10, 1024 pairs: 510 k aligns/s with one 512-thread workgroup per CU, 593 k with two
         * of 256; 768 pairs 538 k vs 575 k, 384 pairs 403 k vs 453 k, 256 pairs 466 k vs 387 k -- so from 1.5 workgroups per CU) */
        else if (all_p4 && 2 * n_pairs >= 3 * n_cu && max_n * 8 <= 2 * 77000LL) { block = 256; auto_lds = 80 * 1024; }
        /* ... and, as soon as there are more pairs than CUs, for lists of any length (round 3; 1920x1080x5 with 4-byte streamed points:
         * 512 pairs 79.3 k -> 80.4 k aligns/s, 1024 pairs 78.5 k -> 80.1 k, 2048 pairs 81.4 k -> 84.7 k = 0.405 of the roofline) */
        else if (all_p4 && n_pairs > n_cu) { block = 256; auto_lds = 80 * 1024; }   /* 320 pairs 53.1 k -> 58.5 k, 384: 62.8 -> 65.3 k, 448: 72.5 -> 74.3 k;
                                                                                          640x480: 272 pairs 331 k -> 394 k, 288: 347 k -> 414 k (one round of 256-thread workgroups, all resident, instead of two of 512) */
        else if (max_n * 12 > 4 * 155000LL && !f.interpolate_dt) { block = 1024; auto_lds = 155000; }   /* lists far beyond the LDS
                                                                       budget are streamed: 16 waves hide that better (1920x1080x5, 256 pairs: 38.3 k -> 41.3 k aligns/s) */
        else { block = 512; auto_lds = 155000; }
    }
    /* LDS budget of the level's resident point list */
    {
        int bytes = f.lds_point_bytes;
        /* auto: one workgroup per CU for >= 512 threads (it owns the CU's LDS), two for 256 */
        if (bytes == 0) bytes = auto_lds ? auto_lds : ((block >= 512) ? 155000 : 80 * 1024);
        /* the CU has 160 KiB of LDS; the static part of the chosen kernel comes off the top */
        /* the packed kernel needs its 256-register budget: 1024 threads would halve it (measured, 1920x1080x5, 256 pairs:
         * 512 threads 45.2 k aligns/s, 1024 threads 41.3 k; the one-point-per-lane kernel: 43.7 k at 1024) */
        if (packed && block_auto && block == 1024) block = 512;
        const int static_lds = packed ? f.fused2_lds[block == 256 ? 0 : (block == 512 ? 1 : 2)][with_h ? 1 : 0]
                                      : (int)sizeof(double) * (block / 64) * PLAN_NACC_PAD + 256 + f.pose_state_bytes;
        /* 256 threads: two workgroups share the CU's LDS -- each gets exactly half, down to the last point that fits (at the
         * request ceiling every point kept out of the per-iteration stream counts: DESIGN.md section 6) */
        const int max_dyn = ((block == 256) ? 80 * 1024 : 160 * 1024) - static_lds - 64;
        if (bytes > max_dyn) bytes = max_dyn;
        if (bytes < 0) bytes = 0;
        bytes &= ~63;
        p.lds_bytes = bytes;
        p.no_lds_tex = (f.engine_variant == 2) ? 1 : 0;
        p.force_exact = (f.engine_variant == 3) ? 1 : 0;
        p.force_e2 = (f.engine_variant == 5) ? 1 : 0;
        p.no_pt4_direct = (f.engine_variant == 6) ? 1 : 0;
        /* 4-byte points from ONE times the LDS capacity (in 8-byte points) on (dvo_fused.hip).  Round 5 (3x through round 4).  Same-box
         * A/B, 640x480x4 at 8192 pairs: 3x 789-790 k aligns/s, 1x 801-803 k, always 764 k; 1920x1080x5 unchanged (its lists are far beyond
         * either bound) -- profiles/r05_experiments/pt4_factor_ab.txt.  The kernel now draws the HBM's whole achievable rate, so the 7 % of
         * its lines that were streamed 8-byte points of level 0 cost more than the 4-byte decode's instructions (round 4, when the issue
         * stage was the nearer ceiling: a wash) */
        /* pt4_decode rebuilds a point's pixel from its 16 x 16 block index with the number of block rows of the image the list was
         * ENCODED against; the kernel only knows the now level's rows.  Reference and now levels of different heights (nothing
         * forbids them) therefore read the 8-byte form, which carries absolute coordinates */
        p.no_pt4 = f.pt4_rows_mismatch ? 1 : 0;
        p.lds_points = bytes / (f.compact ? 8 : 12);
        if (f.lds_point_bytes < 0) { p.lds_points = 0; p.lds_bytes = 0; }
    }
    p.block = block;
    /* Who reads 16-byte texels in this launch?  Everything but the packed kernel on a compact form whose palette is certain to
     * fit the launch's LDS (the kernel decides per pair and level on the device; with less LDS than the largest palette it
     * could fall back to texels).  Now levels written by the engine's own distance-transform stage exist in the compact form
     * only (dvo_frames.hip): their texels are decoded first. */
    p.needs_tex16 = !packed || p.no_p4 || p.lds_bytes < PLAN_PALETTE_BYTES + 64;
    p.points_in_flight = (f.points_in_flight == 1 || f.points_in_flight == 2 || f.points_in_flight == 4) ? f.points_in_flight : 1;
    /* team mode (packed kernel only): with fewer pairs than half the compute units, G workgroups share each pair so that
     * the launch fills the GPU -- G = the largest power of two with 8*ceil(pairs/8)*G <= CUs (at most 16), all of them
     * resident at once (one 512-thread workgroup per CU).  dvo_params.team_size: 0 = auto, 1 = off, k = force k. */
    p.team_fallback = f.team_size <= 1;
    if (!f.listed && packed && !with_h && block == 512 && f.team_size != 1) {
        const int slots8 = 8 * ((n_pairs + 7) / 8);
        /* a team pays when the point phase it splits is longer than the exchange it adds (~2.2 us per iteration).  Measured,
         * one pair, ms per alignment by team size (tools/exp_team_single.py): 640x480x4x10 (14.8 k points at level 0) 1: 0.39,
         * 2: 0.34, 4: 0.30, 8: 0.28, 16: 0.30; 1920x1080x5 (130 k) 8: 0.55, 16: 0.47, 32: 0.49; 4096x3072x5 (629 k) 16: 1.03,
         * 32: 0.85; 320x240x4x50 (4.2 k) 1: 0.91, 2: 1.00, 4: 0.98.  Hence: no team below 5000 points, then double while every
         * member keeps >= 1800 points of the finest level; at most 8 (16 from 64 k points, 32 = a whole XCD from 256 k). */
        const int n_fine = f.n_fine;
        const int g_cap = (n_fine >= 262144) ? 32 : ((n_fine >= 65536) ? 16 : 8);
        int g = 1;
        if (n_fine >= 5000)
            while (g * 2 <= g_cap && slots8 * g * 2 <= n_cu && n_fine >= 1800 * g * 2) g *= 2;
        /* one very large frame: a team over all XCDs (8 x g1 workgroups, two-stage exchange, dvo_fused.hip).  Measured, ms per
         * alignment by team size: 4096x3072x5 (629 k points at level 0) 32: 0.94, 64: 0.65-0.73, 128: 0.61-0.62, 256: 0.66
         * (all-CU wide path 0.78-0.80); 1920x1080x5 (130 k) 16: 0.52-0.54, 32: 0.54, 64: 0.48-0.49, 128: 0.50, 256: 0.57 (wide 0.58) */
        bool super_team = (n_pairs == 1 && n_fine >= 100000 && n_cu >= 256);
        /* round 6, compact now levels, one host round trip per alignment: 4096x3072x5 128: 0.353, 256: 0.332; 1920x1080x5 64: 0.275, 128: 0.289;
         * a launch per tier of level sizes (32 / 128 / 256 members) 0.350 / 0.324: every launch stages its levels again and drains */
        if (super_team) g = (n_fine >= 400000) ? 256 : 64;
        if (f.team_size > 1) {
            g = f.team_size;
            super_team = (g == 64 || g == 128 || g == 256) && n_pairs == 1;
            if (super_team ? (g > n_cu) : (g > 32 || slots8 * g > n_cu))
                return plan_refusal(DVO_ERR_INVALID, "team_size: the launch would need more workgroups than compute units (members must be co-resident; 64 / 128 / 256 only for a single pair)");
        }
        p.team = g;
        p.super_team = g > 1 && super_team;
    }
    return p;
}

/* ---- the team exchange records ---------------------------------------------------------------------------------------------
 * A record is {value, tag}, tag = exchange count + 1.  Rounds 2-5 zeroed the records before every launch (two fills, ~10 us of
 * a 240 us single-pair alignment); since round 6 the count runs on from launch to launch, so whatever an earlier launch left
 * carries a tag below every tag this one waits for.  Zeroed only when the 32-bit count would wrap -- and always once a launch
 * was captured into a caller's graph (its replays would repeat their tags). */
/* exchanges a launch can make: the XCD check, per level one per iteration, one more per iteration whose energy takes the exact
 * sweep (dvo_fused.hip: the limbs travel through an exchange of their own); two more per level to spare */
inline unsigned team_exchanges_needed(const int *iters, int n_levels) {
    unsigned need = 2;
    for (int l = 0; l < n_levels; l++) if (iters[l] > 0) need += 2u * (unsigned)iters[l] + 2u;
    return need;
}
struct TeamEpochStep {
    bool zero_records;      /* fill the records with zeros in front of the launch */
    unsigned epoch0;        /* Schedule.team_epoch0 of the launch */
    unsigned next_epoch;    /* the context's count after it */
};
/* epoch: the context's count; legacy: a team launch was captured into a caller's graph once; first_use: the buffer was just made */
inline TeamEpochStep team_epoch_step(unsigned epoch, unsigned need, bool legacy, bool first_use) {
    const bool restart = legacy || epoch > 0xfffffff0u - need;
    TeamEpochStep s;
    s.zero_records = first_use || restart;
    s.epoch0 = restart ? 0u : epoch;
    s.next_epoch = legacy ? s.epoch0 : s.epoch0 + need;
    return s;
}

/* ---- tiers of team launches for the COARSE levels of the wide / tiled schedule -----------------------------------------------
 * Two tiers, measured on one 4096x3072x5 and one 1920x1080x5 pair (profiles/r06_final/wide_team_sweep.txt): levels of up to 80 k points
 * as a team of 32 inside ONE XCD (records as plain stores), levels of up to 350 k points as a team of 128 over all XCDs (two-stage
 * exchange); larger levels -- and always the finest one, whose final outputs the step path writes -- keep the step launches.
 * DVO_WIDE_TEAM_MAX=a,b overrides the two limits (0 switches the whole thing off; tests). */
/* allow_finest (one rank: nothing is sharded): a finest level of more than 350 k points joins as a third tier, a team of 256 over
 * the whole chip, with the final outputs written by that launch -- then no step launch is left at all. */
struct TeamTiers { int lim[2] = {80000, 350000}; int size[3] = {32, 128, 256}; };
struct WidePlan {
    bool whole_pyramid_one_launch = false;      /* every level that runs, as ONE fused launch with the team size plan_launch picks */
    unsigned tier[3] = {0u, 0u, 0u};            /* else: level masks of the launches with teams of size[0], size[1], size[2] (0: no such launch) */
};
/* N, compact_ok, iters: per level, of the one pair; possible: parameters, flags and device allow team launches at all */
inline WidePlan plan_wide_tiers(const int *N, const bool *compact_ok, const int *iters, int n_levels, const TeamTiers &tiers,
                                int n_cu, bool allow_finest, bool possible) {
    const int *lim = tiers.lim, *size = tiers.size;
    WidePlan w;
    if (!possible) return w;
    int finest = -1;
    for (int l = 0; l < n_levels; l++) if (iters[l] > 0) { finest = l; break; }
    /* the finest level joins only where it is what the third tier is for: a list no team of 128 should carry */
    const bool take_finest = allow_finest && finest >= 0 && N[finest] > lim[1] && n_cu >= size[2] && size[2] >= 2 && compact_ok[finest];
    /* One rank (nothing is sharded): the whole pyramid as ONE team launch of the fused kernel, team size by the finest level exactly as
     * dvo_align_batch picks it.  Measured on the compact now form, ms per alignment (tools/experiments/exp_team_single.py, PREP=1):
     * 4096x3072x5 0.332 (a launch per tier 0.350-0.363), 1920x1080x5 0.275 (0.312-0.324), 640x480x4 0.188 (one launch per level by one
     * workgroup, rounds 4-5: 0.246) -- every further launch stages its levels again and drains. */
    if (allow_finest && finest >= 0 && N[finest] >= 5000) {
        bool all_compact = true;
        for (int l = 0; l < n_levels; l++)
            if (iters[l] > 0 && !compact_ok[l]) all_compact = false;
        if (all_compact) { w.whole_pyramid_one_launch = true; return w; }
    }
    unsigned tier[3] = {0u, 0u, 0u};
    bool big_enough = false;
    for (int l = n_levels - 1; l >= (take_finest ? finest : finest + 1); l--) {               /* from the coarsest down */
        if (iters[l] <= 0) continue;
        if (!compact_ok[l]) break;
        if (N[l] > lim[1] && !(take_finest && l == finest)) break;
        const int k = (N[l] > lim[1]) ? 2 : ((N[l] <= lim[0] && !tier[1]) ? 0 : 1);          /* once a level went to a later tier the finer ones follow */
        if (k == 1 && (n_cu < size[1] || size[1] < 2)) break;
        tier[k] |= 1u << l;
        big_enough = big_enough || N[l] > PLAN_SOLO_MAX;
    }
    if (take_finest && !((tier[2] >> finest) & 1u)) tier[2] = 0;      /* the walk stopped above it: the finest level keeps its step launches */
    if (!big_enough) return w;       /* small levels are one launch each already */
    for (int k = 0; k < 3; k++) w.tier[k] = tier[k];
    return w;
}

/* a launch of more pairs than fit the GPU at once ends when its last workgroup ends: start the pairs with the most
 * point-iterations first (longest-processing-time order), so that the stragglers are the short ones; equal work keeps index order */
inline void launch_order(const long long *work, int n, int *out) {
    for (int p = 0; p < n; p++) out[p] = p;
    std::sort(out, out + n, [work](int a, int b) { return work[a] > work[b] || (work[a] == work[b] && a < b); });
}

}  // namespace dvo_host
#endif
