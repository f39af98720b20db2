/*
 * launch_plan_main.cpp -- walks the launch planner of the fused alignment (rgbd_odometry_amd/csrc/dvo_launch_plan.h): a table of
 * facts -> expected plan, the epoch rule of the team exchange records, the tiers of the wide / tiled schedule, the launch order.
 * Stand-alone: built and run by tests/test_launch_plan_cpu.py.
 *
 * The expected values of the table were written by the decision code of the commit BEFORE the planner existed (the block inside
 * enqueue() of dvo_capi.cpp and the walk of wide_coarse_levels_as_team, wrapped behind the same facts), never by the planner itself;
 * that code and the planner agreed on a full grid of 243 855 360 facts.  Each row names where it comes from: "comment:" rows are the
 * cases a measurement comment of the planner quotes.
 */
#include "dvo_launch_plan.h"

#include <cstdio>
#include <cstring>

using namespace dvo_host;

namespace {

int g_failed = 0;

void fail(int line, const char *what) {
    std::fprintf(stderr, "launch_plan_main.cpp:%d: %s\n", line, what);
    g_failed++;
}
#define CHECK(cond) do { if (!(cond)) fail(__LINE__, #cond); } while (0)

struct Facts {
    int block_threads, lds_point_bytes, points_in_flight, engine_variant, interpolate_dt, team_size, compact_now_policy;
    int n_cu, n_pairs, listed, flags, compact, all_p4, max_n, n_fine, pt4_rows_mismatch, has_pair_K;
};
struct Expect {
    int err, packed, block, points_in_flight, lds_bytes, lds_points, no_p4, no_pt4, no_lds_tex, force_exact, force_e2, no_pt4_direct,
        needs_tex16, team, super_team, team_fallback;
};
struct Row { const char *origin; Facts f; Expect e; const char *msg; };

/* static LDS of the kernels the table was written with: fused2_static_lds(256 | 512 | 1024, with_h) and pose_state_bytes() */
const int FUSED2_LDS[3][2] = {{1216, 1984}, {1472, 3008}, {1984, 5056}};
const int POSE_STATE_BYTES = 880;

LaunchFacts facts_of(const Facts &r) {
    LaunchFacts f;
    f.block_threads = r.block_threads; f.lds_point_bytes = r.lds_point_bytes; f.points_in_flight = r.points_in_flight;
    f.engine_variant = r.engine_variant; f.interpolate_dt = r.interpolate_dt; f.team_size = r.team_size; f.compact_now_policy = r.compact_now_policy;
    f.n_cu = r.n_cu; f.n_pairs = r.n_pairs; f.listed = r.listed != 0; f.flags = r.flags; f.compact = r.compact != 0; f.all_p4 = r.all_p4 != 0;
    f.max_n = r.max_n; f.n_fine = r.n_fine; f.pt4_rows_mismatch = r.pt4_rows_mismatch != 0; f.has_pair_K = r.has_pair_K != 0;
    std::memcpy(f.fused2_lds, FUSED2_LDS, sizeof(FUSED2_LDS));
    f.pose_state_bytes = POSE_STATE_BYTES;
    return f;
}

/* 320x240: 4.2 k points at level 0; 640x480: 14.8 k; 1920x1080: 130 k; 4096x3072: 629 k (the figures of the planner's comments).
 * The GPU twins of the 320x240 rows are the cases of tests/test_gpu_launch_plan.py. */
const Row ROWS[] = {
    /* origin,
     * {block_threads, lds_point_bytes, points_in_flight, engine_variant, interpolate_dt, team_size, compact_now_policy,
     *  n_cu, n_pairs, listed, flags, compact, all_p4, max_n, n_fine, pt4_rows_mismatch, has_pair_K},
     * {err, packed, block, points_in_flight, lds_bytes, lds_points, no_p4, no_pt4, no_lds_tex, force_exact, force_e2, no_pt4_direct,
     *  needs_tex16, team, super_team, team_fallback}, message of a refusal */
    {"comment: 320x240x4x50, single pair -> 512 threads, no team below 5000 points",
     {0, 0, 0, 0, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"comment: 320x240x4x50, 129 pairs (two workgroups per CU pay) -> 256 threads",
     {0, 0, 0, 0, 0, 0, 0, 256, 129, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240x4x50, 128 pairs (half the CUs exactly) -> 512 threads",
     {0, 0, 0, 0, 0, 0, 0, 256, 128, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240x4x50, 129 pairs, interpolate_dt -> never the half-LDS shape",
     {0, 0, 0, 0, 1, 0, 0, 256, 129, 0, 0, 0, 0, 4200, 4200, 0, 0},
     {DVO_OK, 0, 512, 1, 154944, 12912, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"comment: 640x480x4, 1024 pairs -> 256 threads",
     {0, 0, 0, 0, 0, 0, 0, 256, 1024, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"comment: 640x480x4, 768 pairs -> 256 threads",
     {0, 0, 0, 0, 0, 0, 0, 256, 768, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"comment: 640x480x4, 384 pairs (1.5 workgroups per CU) -> 256 threads",
     {0, 0, 0, 0, 0, 0, 0, 256, 384, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"640x480x4, 383 pairs -> 256 threads by the more-pairs-than-CUs rule",
     {0, 0, 0, 0, 0, 0, 0, 256, 383, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"comment: 640x480x4, 256 pairs -> 512 threads",
     {0, 0, 0, 0, 0, 0, 0, 256, 256, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"comment: 640x480, 272 pairs -> 256 threads (more pairs than CUs)",
     {0, 0, 0, 0, 0, 0, 0, 256, 272, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"640x480x4, 1024 pairs, now levels on 16-byte texels -> 512 threads",
     {0, 0, 0, 0, 0, 0, 0, 256, 1024, 0, 0, 1, 0, 14800, 14800, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"comment: 1920x1080x5, 256 pairs -> 512 threads, not 1024, on the packed kernel",
     {0, 0, 0, 0, 0, 0, 0, 256, 256, 0, 0, 1, 1, 130000, 130000, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"comment: 1920x1080x5, 256 pairs, one-point-per-lane kernel -> 1024 threads",
     {0, 0, 0, 1, 0, 0, 0, 256, 256, 0, 0, 1, 1, 130000, 130000, 0, 0},
     {DVO_OK, 0, 1024, 1, 154944, 19368, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"comment: 1920x1080x5, 512 pairs -> 256 threads for lists of any length",
     {0, 0, 0, 0, 0, 0, 0, 256, 512, 0, 0, 1, 1, 130000, 130000, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"comment: 4096x3072 single pair -> a team of 256",
     {0, 0, 0, 0, 0, 0, 0, 256, 1, 0, 0, 1, 1, 629000, 629000, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 256, 1, 1}, nullptr},
    {"comment: 1920x1080 single pair -> a team of 64",
     {0, 0, 0, 0, 0, 0, 0, 256, 1, 0, 0, 1, 1, 130000, 130000, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 64, 1, 1}, nullptr},
    {"1920x1080 single pair on 64 CUs -> no team over all XCDs: 8 members",
     {0, 0, 0, 0, 0, 0, 0, 64, 1, 0, 0, 1, 1, 130000, 130000, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 8, 0, 1}, nullptr},
    {"comment: 640x480 single pair (14.8 k points) -> a team of 8",
     {0, 0, 0, 0, 0, 0, 0, 256, 1, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 8, 0, 1}, nullptr},
    {"640x480, 9 pairs -> 16 slots, a team of 8",
     {0, 0, 0, 0, 0, 0, 0, 256, 9, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 8, 0, 1}, nullptr},
    {"640x480, 8 pairs, team_size 1 -> no team",
     {0, 0, 0, 0, 0, 1, 0, 256, 8, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240 single pair, team_size 2 forced",
     {0, 0, 0, 0, 0, 2, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0}, nullptr},
    {"320x240 single pair, block_threads 256",
     {256, 0, 0, 0, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240 single pair, block_threads 1024",
     {1024, 0, 0, 0, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 1024, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240 single pair, block_threads 512",
     {512, 0, 0, 0, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240 single pair, engine_variant 1 -> one-point-per-lane kernel, 16-byte texels",
     {0, 0, 0, 1, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 0, 512, 1, 154944, 19368, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"320x240 single pair, 3 x N float lists, points_in_flight 4",
     {0, 0, 4, 0, 0, 0, 0, 256, 1, 0, 0, 0, 1, 4200, 4200, 0, 0},
     {DVO_OK, 0, 512, 4, 154944, 12912, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"320x240 single pair, points_in_flight 3 -> 1",
     {0, 0, 3, 0, 0, 0, 0, 256, 1, 0, 0, 0, 1, 4200, 4200, 0, 0},
     {DVO_OK, 0, 512, 1, 154944, 12912, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"320x240 single pair, DVO_FLAG_NORMAL_MATRIX -> packed, 512 threads, no team",
     {0, 0, 0, 0, 0, 0, 0, 256, 1, 0, 4, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"640x480 single pair, DVO_FLAG_NORMAL_MATRIX -> no team",
     {0, 0, 0, 0, 0, 0, 0, 256, 1, 0, 4, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"DVO_FLAG_NORMAL_MATRIX, block_threads 1024 on the packed kernel -> auto",
     {1024, 0, 0, 0, 0, 0, 0, 256, 1, 0, 4, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"DVO_FLAG_NORMAL_MATRIX, block_threads 256, one-point-per-lane kernel -> 512 threads",
     {256, 0, 0, 1, 0, 0, 0, 256, 1, 0, 4, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 0, 512, 1, 154944, 19368, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"DVO_FLAG_NORMAL_MATRIX, block_threads 256 on the packed kernel",
     {256, 0, 0, 0, 0, 0, 0, 256, 1, 0, 4, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 256, 1, 79872, 9984, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"refusal: DVO_FLAG_NORMAL_MATRIX with interpolate_dt",
     {0, 0, 0, 0, 1, 0, 0, 256, 1, 0, 4, 0, 1, 4200, 4200, 0, 0},
     {DVO_ERR_INVALID}, "DVO_FLAG_NORMAL_MATRIX is not available together with dvo_params.interpolate_dt"},
    {"refusal: DVO_FLAG_NORMAL_MATRIX with per-pair camera models",
     {0, 0, 0, 0, 0, 0, 0, 256, 1, 0, 4, 1, 1, 4200, 4200, 0, 1},
     {DVO_ERR_STATE}, "DVO_FLAG_NORMAL_MATRIX is not available on a context with per-pair camera models"},
    {"refusal: index list with engine_variant 1",
     {0, 0, 0, 1, 0, 0, 0, 256, 300, 1, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_ERR_INVALID}, "an index-list launch needs the packed kernel (compact lists, engine_variant != 1)"},
    {"refusal: index list without compact lists",
     {0, 0, 0, 0, 0, 0, 0, 256, 300, 1, 0, 0, 1, 14800, 14800, 0, 0},
     {DVO_ERR_INVALID}, "an index-list launch needs the packed kernel (compact lists, engine_variant != 1)"},
    {"refusal: team_size 64 for two pairs",
     {0, 0, 0, 0, 0, 64, 0, 256, 2, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_ERR_INVALID}, "team_size: the launch would need more workgroups than compute units (members must be co-resident; 64 / 128 / 256 only for a single pair)"},
    {"refusal: team_size 32 for 9 pairs (16 slots x 32 > 256 CUs)",
     {0, 0, 0, 0, 0, 32, 0, 256, 9, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_ERR_INVALID}, "team_size: the launch would need more workgroups than compute units (members must be co-resident; 64 / 128 / 256 only for a single pair)"},
    {"refusal: team_size 256 for a single pair on 64 CUs",
     {0, 0, 0, 0, 0, 256, 0, 64, 1, 0, 0, 1, 1, 629000, 629000, 0, 0},
     {DVO_ERR_INVALID}, "team_size: the launch would need more workgroups than compute units (members must be co-resident; 64 / 128 / 256 only for a single pair)"},
    {"index list of 300 pairs -> 256 threads, no team",
     {0, 0, 0, 0, 0, 0, 0, 256, 300, 1, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"index list of 4 pairs -> 512 threads, no team",
     {0, 0, 0, 0, 0, 0, 0, 256, 4, 1, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"a tier of the wide schedule: team of 32 forced on 67 k points",
     {0, 0, 0, 0, 0, 32, 0, 256, 1, 0, 0, 1, 1, 67000, 67000, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 32, 0, 0}, nullptr},
    {"ADVICE r6 #1: tiers taken with block_threads = 256 -> the forced team is dropped (today's behaviour)",
     {256, 0, 0, 0, 0, 32, 0, 256, 1, 0, 0, 1, 1, 67000, 67000, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0}, nullptr},
    {"a tier of the wide schedule: team of 128 forced, single pair",
     {0, 0, 0, 0, 0, 128, 0, 256, 1, 0, 0, 1, 1, 300000, 300000, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 128, 1, 0}, nullptr},
    {"lds_point_bytes -1 -> every point from HBM",
     {0, -1, 0, 0, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"lds_point_bytes 4096 -> less LDS than a palette: 16-byte texels decoded",
     {0, 4096, 0, 0, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 4096, 512, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"lds_point_bytes 12 * 700 with block_threads 256, 3 x N lists",
     {256, 8400, 0, 0, 0, 0, 0, 256, 1, 0, 0, 0, 1, 4200, 4200, 0, 0},
     {DVO_OK, 0, 256, 1, 8384, 698, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"engine_variant 2 -> no_lds_tex",
     {0, 0, 0, 2, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"engine_variant 3 -> force_exact",
     {0, 0, 0, 3, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1}, nullptr},
    {"engine_variant 4 -> no compact now form",
     {0, 0, 0, 4, 0, 0, 0, 256, 1024, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"engine_variant 5 -> force_e2",
     {0, 0, 0, 5, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 1, 0, 0, 1, 0, 1}, nullptr},
    {"engine_variant 6 -> no_pt4_direct",
     {0, 0, 0, 6, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1}, nullptr},
    {"DVO_COMPACT_NOW=off -> no compact now form",
     {0, 0, 0, 0, 0, 0, 2, 256, 1024, 0, 0, 1, 1, 14800, 14800, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"a list encoded against another height -> no 4-byte points",
     {0, 0, 0, 0, 0, 0, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 1, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240 single pair, team_size 1",
     {0, 0, 0, 0, 0, 1, 0, 256, 1, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240, 9 pairs",
     {0, 0, 0, 0, 0, 0, 0, 256, 9, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240, 9 pairs, block_threads 256",
     {256, 0, 0, 0, 0, 0, 0, 256, 9, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 256, 1, 80640, 10080, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240, 9 pairs, block_threads 512",
     {512, 0, 0, 0, 0, 0, 0, 256, 9, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240, 9 pairs, block_threads 1024",
     {1024, 0, 0, 0, 0, 0, 0, 256, 9, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 1024, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240, 9 pairs, team_size 1",
     {0, 0, 0, 0, 0, 1, 0, 256, 9, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
    {"320x240, 9 pairs, team_size 2 forced",
     {0, 0, 0, 0, 0, 2, 0, 256, 9, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0}, nullptr},
    {"320x240, 9 pairs, engine_variant 1",
     {0, 0, 0, 1, 0, 0, 0, 256, 9, 0, 0, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 0, 512, 1, 154944, 19368, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1}, nullptr},
    {"320x240, 9 pairs, DVO_FLAG_NORMAL_MATRIX",
     {0, 0, 0, 0, 0, 0, 0, 256, 9, 0, 4, 1, 1, 4200, 4200, 0, 0},
     {DVO_OK, 1, 512, 1, 154944, 19368, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}, nullptr},
};

void check_row(const Row &r) {
    const LaunchPlan p = plan_launch(facts_of(r.f));
    const Expect &e = r.e;
    bool ok = p.err == e.err;
    if (ok && e.err) ok = r.msg && p.msg && std::strcmp(p.msg, r.msg) == 0;
    if (ok && !e.err)
        ok = p.packed == (e.packed != 0) && p.block == e.block && p.points_in_flight == e.points_in_flight && p.lds_bytes == e.lds_bytes &&
             p.lds_points == e.lds_points && p.no_p4 == e.no_p4 && p.no_pt4 == e.no_pt4 && p.no_lds_tex == e.no_lds_tex &&
             p.force_exact == e.force_exact && p.force_e2 == e.force_e2 && p.no_pt4_direct == e.no_pt4_direct &&
             p.needs_tex16 == (e.needs_tex16 != 0) && p.team == e.team && p.super_team == (e.super_team != 0) &&
             p.team_fallback == (e.team_fallback != 0);
    if (!ok) {
        std::fprintf(stderr, "row \"%s\": err %d (%s) packed %d block %d u %d lds %d / %d no_p4 %d no_pt4 %d switches %d %d %d %d tex16 %d team %d super %d fallback %d\n",
                     r.origin, p.err, p.msg ? p.msg : "", (int)p.packed, p.block, p.points_in_flight, p.lds_bytes, p.lds_points, p.no_p4, p.no_pt4,
                     p.no_lds_tex, p.force_exact, p.force_e2, p.no_pt4_direct, (int)p.needs_tex16, p.team, (int)p.super_team, (int)p.team_fallback);
        g_failed++;
    }
}

void expect_epoch(int line, unsigned epoch, unsigned need, bool legacy, bool first_use, bool zero, unsigned epoch0, unsigned next) {
    const TeamEpochStep s = team_epoch_step(epoch, need, legacy, first_use);
    if (s.zero_records != zero || s.epoch0 != epoch0 || s.next_epoch != next) {
        std::fprintf(stderr, "launch_plan_main.cpp:%d: team_epoch_step(%u, %u, %d, %d) = {%d, %u, %u}, expected {%d, %u, %u}\n", line, epoch, need,
                     (int)legacy, (int)first_use, (int)s.zero_records, s.epoch0, s.next_epoch, (int)zero, epoch0, next);
        g_failed++;
    }
}
#define EXPECT_EPOCH(...) expect_epoch(__LINE__, __VA_ARGS__)

void expect_wide(int line, const int *N, const bool *compact_ok, const int *iters, int n_levels, const TeamTiers &t, int n_cu, bool allow_finest,
                 bool possible, bool whole, unsigned t0, unsigned t1, unsigned t2) {
    const WidePlan w = plan_wide_tiers(N, compact_ok, iters, n_levels, t, n_cu, allow_finest, possible);
    if (w.whole_pyramid_one_launch != whole || w.tier[0] != t0 || w.tier[1] != t1 || w.tier[2] != t2) {
        std::fprintf(stderr, "launch_plan_main.cpp:%d: plan_wide_tiers = {%d, 0x%x, 0x%x, 0x%x}, expected {%d, 0x%x, 0x%x, 0x%x}\n", line,
                     (int)w.whole_pyramid_one_launch, w.tier[0], w.tier[1], w.tier[2], (int)whole, t0, t1, t2);
        g_failed++;
    }
}
#define EXPECT_WIDE(...) expect_wide(__LINE__, __VA_ARGS__)

}  // namespace

int main() {
    for (const Row &r : ROWS) check_row(r);
    {   /* the predicates the caller gathers by */
        LaunchFacts f = facts_of(ROWS[0].f);
        CHECK(plan_packed(f) && plan_reads_compact_now(f) && plan_block_auto(f) && plan_team_by_n_fine(f));
        CHECK(!shape_depends_on_refusals(f));                       /* one pair: the shape does not hang on the compact form */
        f.n_pairs = 384;
        CHECK(shape_depends_on_refusals(f) && !plan_team_by_n_fine(f));
        f.n_pairs = 257;
        CHECK(shape_depends_on_refusals(f));
        f.n_pairs = 256;
        CHECK(!shape_depends_on_refusals(f));
        f.n_pairs = 384; f.block_threads = 512;
        CHECK(!shape_depends_on_refusals(f) && !plan_block_auto(f));
        f.block_threads = 1024; f.flags = DVO_FLAG_NORMAL_MATRIX;   /* no H-carrying 1024-thread instantiation: chosen again */
        CHECK(plan_block_auto(f));
        f.engine_variant = 4;
        CHECK(plan_packed(f) && !plan_reads_compact_now(f));
        f.engine_variant = 1;
        CHECK(!plan_packed(f) && !plan_reads_compact_now(f) && !plan_block_auto(f));
        CHECK(!too_many_refused(1, 20) && too_many_refused(2, 39) && !too_many_refused(0, 1) && too_many_refused(1, 19));      /* more than 5 % */
    }
    {   /* the exchange records: 2, and per level that runs 2 per iteration + 2 */
        const int it4[4] = {10, 10, 10, 10}, skip[3] = {3, 0, 2};
        CHECK(team_exchanges_needed(it4, 4) == 90u);
        CHECK(team_exchanges_needed(skip, 3) == 16u);
        CHECK(team_exchanges_needed(it4, 1) == 24u);
        const unsigned need = 90u, edge = 0xfffffff0u - need;
        /*           epoch  need  legacy first   zero  epoch0 next */
        EXPECT_EPOCH(0u,    need, false, true,   true,  0u,    90u);          /* first use: the fresh buffer is zeroed */
        EXPECT_EPOCH(1000u, need, false, true,   true,  1000u, 1090u);        /* ... with a start count asked for (tests) */
        EXPECT_EPOCH(90u,   need, false, false,  false, 90u,   180u);         /* steady state: no fill, the count runs on */
        EXPECT_EPOCH(edge,  need, false, false,  false, edge,  0xfffffff0u);  /* the last launch that fits below the wrap */
        EXPECT_EPOCH(edge + 1u, need, false, false, true, 0u,  90u);          /* one above: zeroed, starts again */
        EXPECT_EPOCH(0xffffffffu, need, false, false, true, 0u, 90u);
        EXPECT_EPOCH(edge + 1u, need, false, true, true, 0u,   90u);
        EXPECT_EPOCH(0u,    need, true,  false,  true,  0u,    0u);           /* legacy (captured into a graph once): always zeroed, epoch stays 0 */
        EXPECT_EPOCH(5000u, need, true,  false,  true,  0u,    0u);
        EXPECT_EPOCH(edge + 1u, need, true, true, true, 0u,    0u);
    }
    {   /* tiers of the wide / tiled schedule */
        const TeamTiers def;
        CHECK(def.lim[0] == 80000 && def.lim[1] == 350000 && def.size[0] == 32 && def.size[1] == 128 && def.size[2] == 256);
        const bool all_ok[5] = {true, true, true, true, true};
        const int N1080[5] = {270000, 67000, 32000, 14000, 5500}, it1080[5] = {3, 3, 2, 3, 4};
        /* tests/test_gpu_tiled_ranks.py: 1920x1080x5 over two ranks, 67 k / 32 k / 14 k / 5.5 k points -> one team launch of 32 */
        EXPECT_WIDE(N1080, all_ok, it1080, 5, def, 256, false, true,   false, 0x1eu, 0u, 0u);
        /* one rank, a finest level of 5000 points or more, every list compact -> the whole pyramid as one launch */
        EXPECT_WIDE(N1080, all_ok, it1080, 5, def, 256, true, true,    true, 0u, 0u, 0u);
        const int N5k[2] = {5000, 1300}, N4999[2] = {4999, 1300}, it2[2] = {5, 5};
        EXPECT_WIDE(N5k, all_ok, it2, 2, def, 256, true, true,         true, 0u, 0u, 0u);
        EXPECT_WIDE(N4999, all_ok, it2, 2, def, 256, true, true,       false, 0u, 0u, 0u);       /* below: small levels are one launch each already */
        /* parameters, flags or device do not allow team launches */
        EXPECT_WIDE(N1080, all_ok, it1080, 5, def, 256, true, false,   false, 0u, 0u, 0u);
        /* a level that is not compact stops the walk (and the whole-pyramid launch) */
        const bool gap[5] = {true, true, false, true, true};
        EXPECT_WIDE(N1080, gap, it1080, 5, def, 256, false, true,      false, 0x18u, 0u, 0u);
        EXPECT_WIDE(N1080, gap, it1080, 5, def, 256, true, true,       false, 0x18u, 0u, 0u);
        /* ... unless that level does not run */
        const int it_skip[5] = {3, 3, 0, 3, 4};
        EXPECT_WIDE(N1080, gap, it_skip, 5, def, 256, false, true,     false, 0x1au, 0u, 0u);
        /* levels of 14 k and 5.5 k alone: big enough; 5.5 k alone: not */
        const int it_two[5] = {3, 0, 0, 3, 4}, it_one[5] = {3, 0, 0, 0, 4};
        EXPECT_WIDE(N1080, all_ok, it_two, 5, def, 256, false, true,   false, 0x18u, 0u, 0u);
        EXPECT_WIDE(N1080, all_ok, it_one, 5, def, 256, false, true,   false, 0u, 0u, 0u);
        /* DVO_WIDE_TEAM_MAX=0: lim = {0, 0} -> nothing (the caller also reports it as not possible) */
        TeamTiers off; off.lim[0] = off.lim[1] = 0;
        EXPECT_WIDE(N1080, all_ok, it1080, 5, off, 256, false, true,   false, 0u, 0u, 0u);
        EXPECT_WIDE(N1080, all_ok, it1080, 5, off, 256, false, false,  false, 0u, 0u, 0u);
        /* 4096x3072x5 over two ranks: 160 k goes to the team of 128, the coarser levels to the team of 32; the finest keeps its step launches */
        const int N4k[5] = {629000, 160000, 40000, 10000, 2500}, it5[5] = {4, 4, 4, 4, 4};
        EXPECT_WIDE(N4k, all_ok, it5, 5, def, 256, false, true,        false, 0x1cu, 0x2u, 0u);
        EXPECT_WIDE(N4k, all_ok, it5, 5, def, 64, false, true,         false, 0x1cu, 0u, 0u);      /* fewer CUs than the second tier's team: the walk stops */
        /* finest > 350 k on one rank with 256 CUs: what the third tier was made for is taken by the whole-pyramid launch first (team size
         * by plan_launch: 256) -- the walk never hands a level to the third tier while the finest list has 5000 points or more */
        EXPECT_WIDE(N4k, all_ok, it5, 5, def, 256, true, true,         true, 0u, 0u, 0u);
        /* the walk stopped above the finest level (a list that is not compact): no third tier, the coarse tier stays */
        const bool gap1[5] = {true, false, true, true, true};
        EXPECT_WIDE(N4k, gap1, it5, 5, def, 256, true, true,           false, 0x1cu, 0u, 0u);
        /* a finest list that is not compact itself */
        const bool gap0[5] = {false, true, true, true, true};
        EXPECT_WIDE(N4k, gap0, it5, 5, def, 256, true, true,           false, 0x1cu, 0x2u, 0u);
        /* lowered limits (DVO_WIDE_TEAM_MAX=1000,4000) and a finest list below 5000 points: the third tier's mask is formed, and dropped
         * with the rest because no level is big enough to pay for a team launch */
        TeamTiers low; low.lim[0] = 1000; low.lim[1] = 4000;
        const int Nlow[3] = {4800, 3000, 900}, it3[3] = {4, 4, 4};
        EXPECT_WIDE(Nlow, all_ok, it3, 3, low, 256, true, true,        false, 0u, 0u, 0u);
    }
    {   /* launch order: longest first, equal work keeps index order */
        const long long work[8] = {5, 9, 5, 1, 9, 0, 5, 9};
        int out[8];
        launch_order(work, 8, out);
        const int want[8] = {1, 4, 7, 0, 2, 6, 3, 5};
        CHECK(std::memcmp(out, want, sizeof(want)) == 0);
        const long long same[5] = {7, 7, 7, 7, 7};
        launch_order(same, 5, out);
        for (int i = 0; i < 5; i++) CHECK(out[i] == i);
        launch_order(work, 1, out);
        CHECK(out[0] == 0);
        launch_order(work, 0, out);                                 /* nothing to do, nothing touched */
        CHECK(out[0] == 0);
    }
    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("launch plan: %d rows ok\n", (int)(sizeof(ROWS) / sizeof(ROWS[0])));
    return 0;
}
