/* Walks the upload planner, rgbd_odometry_amd/csrc/dvo_upload_plan.h: a table of named rows computed by hand from the code the
 * planner replaced (routes, chunk sizes, strides, level sizes, refusals with their codes and messages, the pyramid layout and its
 * copy ranges), then a sweep of the arithmetic invariants over every count, format, depth and flag combination.  Stand-alone:
 * built with the address and undefined-behaviour sanitizers by tests/test_upload_plan_cpu.py; includes no HIP header. */
#include "dvo_upload_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace dvo_host;

namespace {
const char *g_row = "";
int g_checks = 0;
#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        g_checks++;                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: [%s] %s\n", __FILE__, __LINE__, g_row, #cond); std::exit(1); } \
    } while (0)
#define ROW(name) g_row = name

CameraFacts vga(int count, bool depth, int flags) {
    CameraFacts f;
    f.count = count; f.rows = 480; f.cols = 640; f.n_levels = 4; f.first_shift = 1;
    f.has_images = true; f.has_depth = depth; f.flags = flags; f.aligned = true;
    f.now_first_pair = -1; f.n_pairs = 300; f.n_slots = 512;
    return f;
}
bool refused(const UploadRefusal &p, const char *msg, bool late = false) {
    return p.err == DVO_ERR_INVALID && p.msg && !std::strcmp(p.msg, msg) && p.late == late;
}

void camera_routes() {
    ROW("640x480 BGR8 + f32 depth, pageable, flags 0, count 40");
    CameraPlan p = plan_camera_upload(vga(40, true, 0));
    CHECK(p.err == DVO_OK && p.bpp == 3 && p.dpp == 4 && p.b_img == 921600 && p.d_img == 1228800 && p.d_px == 307200);
    CHECK(p.route == ROUTE_MIRROR && p.chunk == 15 && !p.copies_ahead && p.mirror && !p.device_sources);
    CHECK(p.landing_bytes == (size_t)15 * (921600 + 1228800) && p.table_entries == 0);
    { int n[3], k = 0; for (int b = 0; b < 40; b += p.chunk) n[k++] = std::min(p.chunk, 40 - b); CHECK(k == 3 && n[0] == 15 && n[1] == 15 && n[2] == 10); }

    ROW("the same without depth");
    p = plan_camera_upload(vga(40, false, 0));
    CHECK(p.err == DVO_OK && p.route == ROUTE_MIRROR && p.chunk == 36 && p.d_img == 0 && p.d_px == 0 && p.landing_bytes == (size_t)36 * 921600);

    ROW("DVO_UPLOAD_DIRECT: one DMA per image, the first budget");
    p = plan_camera_upload(vga(40, true, DVO_UPLOAD_DIRECT));
    CHECK(p.err == DVO_OK && p.route == ROUTE_DMA && p.chunk == 15 && !p.copies_ahead && p.mirror);

    ROW("DVO_UPLOAD_MAPPED, BGR8 only, count 100");
    p = plan_camera_upload(vga(100, false, DVO_UPLOAD_MAPPED));
    CHECK(p.err == DVO_OK && p.route == ROUTE_GATHER && p.chunk == 64 && p.copies_ahead && !p.mirror && !p.device_sources);
    CHECK(p.gather_wgs(64) == 1 && p.gather_wgs(36) == 1 && p.gather_wgs(32) == 1 && p.gather_wgs(16) == 2 && p.gather_wgs(1) == 32);

    ROW("DVO_UPLOAD_MAPPED with f32 depth, count 40");
    p = plan_camera_upload(vga(40, true, DVO_UPLOAD_MAPPED));
    CHECK(p.err == DVO_OK && p.route == ROUTE_GATHER && p.chunk == 31 && p.copies_ahead);

    ROW("DVO_UPLOAD_DEVICE, all aligned, count 256");
    p = plan_camera_upload(vga(256, true, DVO_UPLOAD_DEVICE));
    CHECK(p.err == DVO_OK && p.route == ROUTE_IN_PLACE && p.chunk == 256 && p.landing_bytes == 0 && p.table_entries == 512 && p.device_sources);

    ROW("DVO_UPLOAD_DEVICE, a source off its alignment (image & 3, u16 depth & 7, f32 depth & 15: the caller's one fact)");
    CameraFacts f = vga(256, true, DVO_UPLOAD_DEVICE);
    f.aligned = false;
    p = plan_camera_upload(f);
    CHECK(p.err == DVO_OK && p.route == ROUTE_GATHER && p.device_sources && p.copies_ahead && !p.mirror && p.table_entries == 0);
    CHECK(p.chunk == 224 && p.gather_wgs(224) == 64 && p.gather_wgs(1) == 64);      /* 512 MiB / 2 150 400 = 249, whole gathers of 32 */
    CHECK(p.landing_bytes == (size_t)224 * 2150400);
    f.depth_format = DVO_DEPTH_U16;
    p = plan_camera_upload(f);
    CHECK(p.err == DVO_OK && p.route == ROUTE_GATHER && p.d_img == 614400 && p.chunk == 256 && p.gather_wgs(256) == 64);   /* 349 fit */
}

void camera_strides() {
    CameraFacts f = vga(1, true, 0);
    f.rows = 67; f.cols = 131; f.n_levels = 1; f.first_shift = 0;
    ROW("67x131 mono8 + u16 depth");
    f.image_format = DVO_CAM_MONO8; f.depth_format = DVO_DEPTH_U16;
    CameraPlan p = plan_camera_upload(f);
    CHECK(p.err == DVO_OK && p.bpp == 1 && p.dpp == 2 && p.b_img == 8784 && p.d_img == 17568 && p.d_px == 8784);
    ROW("67x131 BGR8 + f32 depth: float depth is not rounded");
    f.image_format = DVO_CAM_BGR8; f.depth_format = DVO_DEPTH_F32;
    p = plan_camera_upload(f);
    CHECK(p.err == DVO_OK && p.bpp == 3 && p.dpp == 4 && p.b_img == 26336 && p.d_img == 35108 && p.d_px == 8777);
    ROW("67x131 RGB8 is BGR8's size");
    f.image_format = DVO_CAM_RGB8;
    p = plan_camera_upload(f);
    CHECK(p.err == DVO_OK && p.bpp == 3 && p.b_img == 26336);
}

void camera_levels() {
    ROW("480x640, first_shift 1, 4 levels");
    CameraPlan p = plan_camera_upload(vga(1, true, 0));
    const int r[4] = {240, 120, 60, 30}, c[4] = {320, 160, 80, 40};
    for (int l = 0; l < 4; l++) CHECK(p.rows[l] == r[l] && p.cols[l] == c[l]);
    ROW("cvRound, half to even: 5 -> 2, 7 -> 4, 3 -> 2 rows at shift 1");
    CHECK(round_half_even_pos(2.5) == 2 && round_half_even_pos(3.5) == 4 && round_half_even_pos(1.5) == 2 && round_half_even_pos(0.5) == 0);
    CHECK(round_half_even_pos(2.25) == 2 && round_half_even_pos(2.75) == 3 && round_half_even_pos(7.0) == 7);
    const int in[3] = {5, 7, 3}, out[3] = {2, 4, 2};
    for (int k = 0; k < 3; k++) {
        CameraFacts f = vga(1, false, 0);
        f.rows = in[k]; f.cols = 64; f.n_levels = 1;
        p = plan_camera_upload(f);
        CHECK(p.err == DVO_OK && p.rows[0] == out[k] && p.cols[0] == 32);
    }
    ROW("1 row at shift 1 -> 0");
    CameraFacts f = vga(1, false, 0);
    f.rows = 1; f.cols = 64; f.n_levels = 1;
    CHECK(refused(plan_camera_upload(f), "pyramid level would be empty"));
    f = vga(1, false, 0);
    f.rows = 64; f.cols = 1; f.n_levels = 1;
    CHECK(refused(plan_camera_upload(f), "pyramid level would be empty"));
}

void camera_refusals() {
    CameraFacts f;
    ROW("unknown image format");
    f = vga(1, true, 0); f.image_format = 3;
    CHECK(refused(plan_camera_upload(f), "unknown image format (DVO_CAM_BGR8 / DVO_CAM_RGB8 / DVO_CAM_MONO8)"));
    f.image_format = -1; f.depth_format = 7;      /* the image format is looked at first */
    CHECK(refused(plan_camera_upload(f), "unknown image format (DVO_CAM_BGR8 / DVO_CAM_RGB8 / DVO_CAM_MONO8)"));
    ROW("unknown depth format");
    f = vga(1, true, 0); f.depth_format = 2;
    CHECK(refused(plan_camera_upload(f), "unknown depth format (DVO_DEPTH_F32 / DVO_DEPTH_U16)"));
    ROW("n_levels 0 and DVO_LEVELS + 1");
    f = vga(1, true, 0); f.n_levels = 0;
    CHECK(refused(plan_camera_upload(f), "bad camera frame arguments"));
    f.n_levels = PLAN_LEVELS + 1; f.first_shift = 0;
    CHECK(refused(plan_camera_upload(f), "bad camera frame arguments"));
    f.n_levels = PLAN_LEVELS; f.rows = 4096; f.cols = 4096;
    CHECK(plan_camera_upload(f).err == DVO_OK);
    ROW("first_shift + n_levels > 16");
    f = vga(1, true, 0); f.rows = 1 << 20; f.cols = 1 << 20; f.first_shift = 13; f.n_levels = 4;
    CHECK(refused(plan_camera_upload(f), "bad camera frame arguments"));
    f.first_shift = 12;
    CHECK(plan_camera_upload(f).err == DVO_OK);
    f.first_shift = -1;
    CHECK(refused(plan_camera_upload(f), "bad camera frame arguments"));
    ROW("count 0, no images, empty image");
    f = vga(0, true, 0);
    CHECK(refused(plan_camera_upload(f), "bad camera frame arguments"));
    f = vga(1, true, 0); f.has_images = false;
    CHECK(refused(plan_camera_upload(f), "bad camera frame arguments"));
    f = vga(1, true, 0); f.rows = 0;
    CHECK(refused(plan_camera_upload(f), "bad camera frame arguments"));
    f = vga(1, true, 0); f.cols = 0;
    CHECK(refused(plan_camera_upload(f), "bad camera frame arguments"));
    ROW("NULL camera image");
    f = vga(2, true, 0); f.null_image = true;
    CHECK(refused(plan_camera_upload(f), "NULL camera image"));
    ROW("now_first_pair range out of bounds");
    f = vga(4, true, 0); f.n_pairs = 8; f.now_first_pair = 5;
    CHECK(refused(plan_camera_upload(f), "now_first_pair range out of bounds"));
    f.now_first_pair = 8;
    CHECK(refused(plan_camera_upload(f), "now_first_pair range out of bounds"));
    f.now_first_pair = 4;
    CHECK(plan_camera_upload(f).err == DVO_OK);
    f.now_first_pair = -1;                                   /* nobody's now frames */
    CHECK(plan_camera_upload(f).err == DVO_OK);
    ROW("slot range out of bounds: after the caller's refusals, the plan valid beside it");
    f = vga(4, true, 0); f.n_slots = 6; f.first_slot = 3;
    CameraPlan p = plan_camera_upload(f);
    CHECK(refused(p, "frame slot range out of bounds (dvo_frames_reserve)", true) && p.rows[0] == 240 && p.cols[3] == 40 && p.chunk == 4);
    f.first_slot = 2;
    CHECK(plan_camera_upload(f).err == DVO_OK);
    f.first_slot = -1;
    CHECK(refused(plan_camera_upload(f), "frame slot range out of bounds (dvo_frames_reserve)", true));
    ROW("n_slots 0: the default capacity min(2 * n_pairs + 2, 64)");
    CHECK(frames_default_slots(1) == 4 && frames_default_slots(31) == 64 && frames_default_slots(300) == 64);
    f = vga(2, true, 0); f.n_slots = 0; f.n_pairs = 3; f.first_slot = 6;
    CHECK(plan_camera_upload(f).err == DVO_OK);
    f.first_slot = 7;
    CHECK(refused(plan_camera_upload(f), "frame slot range out of bounds (dvo_frames_reserve)", true));
    f.n_pairs = 300; f.first_slot = 62;
    CHECK(plan_camera_upload(f).err == DVO_OK);
    f.first_slot = 63;
    CHECK(refused(plan_camera_upload(f), "frame slot range out of bounds (dvo_frames_reserve)", true));
}

PyramidFacts pyramid(int count, int rows0, int cols0, int grey_dtype, int depth_dtype, int flags) {
    PyramidFacts f;
    f.count = count; f.n_levels = 4; f.has_grey = true; f.has_depth = true; f.flags = flags;
    for (int l = 0; l < 4; l++) { f.rows[l] = rows0 >> l; f.cols[l] = cols0 >> l; f.grey_dtype[l] = grey_dtype; f.depth_dtype[l] = depth_dtype; }
    f.now_first_pair = -1; f.n_pairs = 300; f.n_slots = 512;
    return f;
}

void pyramids() {
    ROW("u8 grey + u16 depth, 320x240 ... 40x30");
    PyramidPlan p = plan_pyramid_upload(pyramid(200, 240, 320, DVO_PIX_U8, DVO_PIX_U16, 0));
    CHECK(p.err == DVO_OK && p.frame_bytes == 306000 && p.chunk == 109 && !p.mapped && p.mirror && p.landing_bytes == (size_t)109 * 306000);
    CHECK(p.g_img[0] == 76800 && p.d_img[0] == 153600 && p.g_img[3] == 1200 && p.d_img[3] == 2400);
    CHECK(p.g_off[0] == 0 && p.d_off[0] == (size_t)109 * 76800 && p.g_off[1] == (size_t)109 * 230400 && p.d_off[3] == p.landing_bytes - (size_t)109 * 2400);
    for (int l = 0; l < 4; l++) CHECK(p.small[l]);
    CHECK(p.n_runs == 1 && p.run_lo[0] == 0 && p.run_hi[0] == p.landing_bytes);
    CHECK(plan_pyramid_upload(pyramid(109, 240, 320, DVO_PIX_U8, DVO_PIX_U16, 0)).chunk == 109);
    CHECK(plan_pyramid_upload(pyramid(108, 240, 320, DVO_PIX_U8, DVO_PIX_U16, 0)).chunk == 108);
    ROW("the same with DVO_UPLOAD_DIRECT: 76 800 x 2 bytes <= 256 KiB, still every level small");
    p = plan_pyramid_upload(pyramid(200, 240, 320, DVO_PIX_U8, DVO_PIX_U16, DVO_UPLOAD_DIRECT));
    CHECK(p.n_runs == 1 && p.small[0] && p.small[3]);

    ROW("f32 grey + f32 depth, 640x480 ... 80x60, DVO_UPLOAD_DIRECT");
    p = plan_pyramid_upload(pyramid(3, 480, 640, DVO_PIX_F32, DVO_PIX_F32, DVO_UPLOAD_DIRECT));
    CHECK(p.err == DVO_OK && p.chunk == 3 && p.frame_bytes == (size_t)8 * (307200 + 76800 + 19200 + 4800));
    CHECK(!p.small[0] && !p.small[1] && p.small[2] && p.small[3]);
    CHECK(p.n_runs == 1 && p.run_lo[0] == p.g_off[2] && p.run_hi[0] == p.landing_bytes && p.g_off[2] == (size_t)3 * 8 * (307200 + 76800));
    ROW("the same without the flag: everything through the mirror");
    p = plan_pyramid_upload(pyramid(3, 480, 640, DVO_PIX_F32, DVO_PIX_F32, 0));
    CHECK(p.small[0] && p.small[1] && p.n_runs == 1 && p.run_lo[0] == 0 && p.run_hi[0] == p.landing_bytes);
    ROW("a big level between small ones: two copy ranges");
    {
        PyramidFacts f = pyramid(2, 480, 640, DVO_PIX_F32, DVO_PIX_F32, DVO_UPLOAD_DIRECT);
        f.rows[0] = 60; f.cols[0] = 80;                     /* small, big, small, small */
        p = plan_pyramid_upload(f);
        CHECK(p.small[0] && !p.small[1] && p.small[2] && p.small[3] && p.n_runs == 2);
        CHECK(p.run_lo[0] == 0 && p.run_hi[0] == p.g_off[1] && p.run_lo[1] == p.g_off[2] && p.run_hi[1] == p.landing_bytes);
    }
    ROW("DVO_UPLOAD_MAPPED");
    p = plan_pyramid_upload(pyramid(500, 240, 320, DVO_PIX_U8, DVO_PIX_U16, DVO_UPLOAD_MAPPED));
    CHECK(p.err == DVO_OK && p.mapped && !p.mirror && p.n_runs == 0 && p.chunk == 219);      /* 64 MiB / 306 000 */
    for (int l = 0; l < 4; l++) CHECK(!p.small[l]);
    CHECK(mapped_gather_wgs(1) == 32 && mapped_gather_wgs(3) == 10 && mapped_gather_wgs(32) == 1 && mapped_gather_wgs(219) == 1);
    ROW("odd sizes: every image 16-byte aligned");
    {
        PyramidFacts f = pyramid(1, 67, 131, DVO_PIX_U8, DVO_PIX_F32, 0);
        f.n_levels = 1;
        p = plan_pyramid_upload(f);
        CHECK(p.g_img[0] == 8784 && p.d_img[0] == 35120 && p.frame_bytes == 43904 && p.d_off[0] == 8784);
        f.has_depth = false;
        p = plan_pyramid_upload(f);
        CHECK(p.d_img[0] == 0 && p.frame_bytes == 8784);
    }
    ROW("pyramid refusals");
    PyramidFacts f = pyramid(2, 240, 320, DVO_PIX_U8, DVO_PIX_U16, 0);
    f.has_grey = false;
    CHECK(refused(plan_pyramid_upload(f), "bad frame arguments"));
    f = pyramid(0, 240, 320, DVO_PIX_U8, DVO_PIX_U16, 0);
    CHECK(refused(plan_pyramid_upload(f), "bad frame arguments"));
    f = pyramid(2, 240, 320, DVO_PIX_U8, DVO_PIX_U16, 0); f.n_levels = 0;
    CHECK(refused(plan_pyramid_upload(f), "bad frame arguments"));
    f.n_levels = PLAN_LEVELS + 1;
    CHECK(refused(plan_pyramid_upload(f), "bad frame arguments"));
    f = pyramid(2, 240, 320, DVO_PIX_U8, DVO_PIX_U16, 0); f.n_slots = 2; f.first_slot = 1;
    p = plan_pyramid_upload(f);
    CHECK(refused(p, "frame slot range out of bounds (dvo_frames_reserve)", true) && p.frame_bytes == 306000);
    f.first_slot = 0; f.n_pairs = 2; f.now_first_pair = 2;
    CHECK(refused(plan_pyramid_upload(f), "now_first_pair range out of bounds", true));
    f.now_first_pair = 1;
    CHECK(refused(plan_pyramid_upload(f), "now_first_pair range out of bounds", true));
    f.first_slot = 2;                                        /* both wrong: the slot range speaks first */
    CHECK(refused(plan_pyramid_upload(f), "frame slot range out of bounds (dvo_frames_reserve)", true));
    f.first_slot = 0; f.now_first_pair = 0;
    CHECK(plan_pyramid_upload(f).err == DVO_OK);
    f.n_slots = 0; f.first_slot = 4;                         /* not reserved: min(2 * 2 + 2, 64) slots */
    CHECK(plan_pyramid_upload(f).err == DVO_OK);
    f.first_slot = 5;
    CHECK(refused(plan_pyramid_upload(f), "frame slot range out of bounds (dvo_frames_reserve)", true));
    ROW("an empty level is the caller's to refuse: the plan stays harmless");
    f = pyramid(2, 240, 320, DVO_PIX_U8, DVO_PIX_U16, 0);
    for (int l = 0; l < 4; l++) f.rows[l] = 0;
    p = plan_pyramid_upload(f);
    CHECK(p.err == DVO_OK && p.frame_bytes == 0 && p.chunk == 2 && p.landing_bytes == 0);
}

/* the arithmetic invariants, on every case */
int sweep() {
    int cases = 0;
    const int formats[3] = {DVO_CAM_BGR8, DVO_CAM_RGB8, DVO_CAM_MONO8}, depth_formats[2] = {DVO_DEPTH_F32, DVO_DEPTH_U16};
    const int flags[4] = {0, DVO_UPLOAD_DIRECT, DVO_UPLOAD_MAPPED, DVO_UPLOAD_DEVICE};
    const int sizes[3][2] = {{480, 640}, {67, 131}, {3072, 4096}};      /* the last: one BGR8 + f32 frame is beyond the 32 and 64 MiB budgets */
    ROW("sweep");
    for (int count = 1; count <= 300; count++)
        for (int fi = 0; fi < 3; fi++)
            for (int di = 0; di < 2; di++)
                for (int depth = 0; depth < 2; depth++)
                    for (int gi = 0; gi < 4; gi++)
                        for (int si = 0; si < 3; si++)
                            for (int aligned = 0; aligned < 2; aligned++) {
                                CameraFacts f = vga(count, depth != 0, flags[gi]);
                                f.image_format = formats[fi]; f.depth_format = depth_formats[di];
                                f.rows = sizes[si][0]; f.cols = sizes[si][1]; f.aligned = aligned != 0;
                                const CameraPlan p = plan_camera_upload(f);
                                cases++;
                                CHECK(p.err == DVO_OK);
                                CHECK(p.chunk >= 1 && p.chunk <= count);
                                const size_t per = p.b_img + p.d_img, npx = (size_t)f.rows * f.cols;
                                CHECK(p.b_img >= npx * p.bpp && p.b_img % 16 == 0 && p.d_img >= (depth ? npx * p.dpp : 0) && p.d_px * p.dpp == p.d_img);
                                const bool in_place = flags[gi] == DVO_UPLOAD_DEVICE && aligned;
                                const UploadRoute want = in_place ? ROUTE_IN_PLACE : (flags[gi] & (DVO_UPLOAD_DEVICE | DVO_UPLOAD_MAPPED)) ? ROUTE_GATHER
                                                       : (flags[gi] & DVO_UPLOAD_DIRECT) ? ROUTE_DMA : ROUTE_MIRROR;
                                CHECK(p.route == want);
                                CHECK(p.copies_ahead == (want == ROUTE_GATHER || want == ROUTE_IN_PLACE) && p.mirror == (want == ROUTE_DMA || want == ROUTE_MIRROR));
                                if (in_place) {
                                    CHECK(p.chunk == count && p.landing_bytes == 0 && p.table_entries == 2 * count);
                                } else {
                                    const size_t budget = flags[gi] == DVO_UPLOAD_DEVICE ? kDeviceHalf : (flags[gi] == DVO_UPLOAD_MAPPED ? kMappedHalf : kUploadHalf);
                                    CHECK(p.landing_bytes == per * p.chunk && p.table_entries == 0);
                                    CHECK(p.landing_bytes <= budget || (per > budget && p.chunk == 1));
                                    if (want == ROUTE_GATHER && p.chunk > 32) CHECK(p.chunk % 32 == 0);
                                    /* never a smaller chunk than the budget asks for, but for the tail that is no whole gather */
                                    const size_t fit = std::min<size_t>(std::max<size_t>(budget / per, 1), (size_t)count);
                                    CHECK(want == ROUTE_GATHER && fit > 32 ? (size_t)p.chunk + 32 > fit : (size_t)p.chunk == fit);
                                }
                                int covered = 0, chunks = 0;
                                for (int b = 0; b < count; b += p.chunk, chunks++) {            /* the chunks tile [0, count) */
                                    const int nc = std::min(p.chunk, count - b);
                                    CHECK(b == covered && nc >= 1);
                                    covered += nc;
                                    if (flags[gi] == DVO_UPLOAD_MAPPED) {
                                        const int wgs = p.gather_wgs(nc);
                                        CHECK(wgs >= 1 && (nc > 32 ? wgs == 1 : wgs * nc <= 32 && (wgs + 1) * nc > 32));
                                    } else if (flags[gi] == DVO_UPLOAD_DEVICE) {
                                        CHECK(p.gather_wgs(nc) == 64);
                                    }
                                }
                                CHECK(covered == count && chunks == (count + p.chunk - 1) / p.chunk);
                            }
    CHECK(cases == 300 * 3 * 2 * 2 * 4 * 3 * 2);
    return cases;
}
}  // namespace

int main() {
    camera_routes();
    camera_strides();
    camera_levels();
    camera_refusals();
    pyramids();
    const int cases = sweep();
    std::printf("ok: %d sweep cases, %d checks\n", cases, g_checks);
    return 0;
}
