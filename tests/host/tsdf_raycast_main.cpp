/*
 * tsdf_raycast_main.cpp -- dvo_tsdf::raycast (rgbd_odometry_amd/csrc/dvo_tsdf_raycast.h: the body of dvo_raycast_host) as a stand-alone
 * program, so that tests/test_tsdf_raycast_cpu.py can run it under the address and undefined-behaviour sanitizers.
 *
 *   tsdf_raycast_main VOLUME_FILE PARAMS_FILE WORDS_FILE VIEWS_FILE FORMAT ROWS COLS COUNT
 *
 * VOLUME_FILE: the bytes of one dvo_tsdf_volume.  PARAMS_FILE: one dvo_raycast_params.  WORDS_FILE: nx * ny * nz words.  VIEWS_FILE:
 * 4 COUNT doubles K4, then 12 COUNT doubles poses.  FORMAT 0 = float metres, 1 = 16-bit millimetres.
 * Output: "depth n" and the n pixels of all views (four hex digits each for 16-bit, eight for the floats' bit patterns) on one line;
 * "normals n" and the 3 n floats' bit patterns likewise; then "clipped equal 1" when the march clipped to the volume's box -- what the
 * kernel runs -- gave the same bytes as the whole march, "clipped equal 0" otherwise.
 * Exit status 3: the arguments were refused (nothing but "refused" is printed; the outputs are checked to be untouched).
 * Every buffer is allocated to its exact size, one allocation per image, so that an access past an end is the sanitizer's to see.
 */
#include "dvo_tsdf_raycast.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

static bool read_file(const char *path, void *dst, size_t bytes) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fread(dst, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

struct Images {
    std::vector<std::unique_ptr<unsigned char[]>> depth;
    std::vector<std::unique_ptr<float[]>> normals;
    std::vector<void *> dp;
    std::vector<float *> np;
    Images(size_t count, size_t depth_bytes, size_t pixels) {
        for (size_t i = 0; i < count; i++) {
            depth.emplace_back(new unsigned char[depth_bytes]);
            std::memset(depth.back().get(), 0xA5, depth_bytes);
            normals.emplace_back(new float[3 * pixels]);
            std::memset(normals.back().get(), 0xA5, 12 * pixels);
            dp.push_back(depth.back().get());
            np.push_back(normals.back().get());
        }
    }
};

int main(int argc, char **argv) {
    if (argc != 9) { std::fprintf(stderr, "usage: %s volume params words views format rows cols count\n", argv[0]); return 2; }
    const int format = std::atoi(argv[5]), rows = std::atoi(argv[6]), cols = std::atoi(argv[7]), count = std::atoi(argv[8]);
    dvo_tsdf_volume vol;
    dvo_raycast_params prm;
    if (!read_file(argv[1], &vol, sizeof(vol)) || !read_file(argv[2], &prm, sizeof(prm))) { std::fprintf(stderr, "cannot read the volume or the parameters\n"); return 2; }
    const bool vol_ok = dvo_tsdf::volume_ok(&vol);
    const size_t n = vol_ok ? dvo_tsdf::voxels_of(vol) : 1;
    std::unique_ptr<unsigned[]> words(new unsigned[n]);
    std::memset(words.get(), 0, 4 * n);
    if (vol_ok && !read_file(argv[3], words.get(), 4 * n)) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    const size_t c = count > 0 ? (size_t)count : 1;
    std::unique_ptr<double[]> K4(new double[4 * c]), poses(new double[12 * c]);
    {
        std::vector<double> both(16 * c, 0.0);
        if (count > 0 && !read_file(argv[4], both.data(), 8 * both.size())) { std::fprintf(stderr, "cannot read %s\n", argv[4]); return 2; }
        std::memcpy(K4.get(), both.data(), 32 * c);
        std::memcpy(poses.get(), both.data() + 4 * c, 96 * c);
    }
    const bool geometry = dvo_tsdf::format_ok(format) && rows >= 1 && cols >= 1;
    const size_t pixels = geometry ? (size_t)rows * (size_t)cols : 1, depth_bytes = geometry ? pixels * dvo_tsdf::depth_pixel_bytes(format) : 1;
    Images whole(c, depth_bytes, pixels), clipped(c, depth_bytes, pixels);
    if (!dvo_tsdf::raycast(&vol, words.get(), &prm, count, format, rows, cols, K4.get(), poses.get(), whole.dp.data(), whole.np.data())) {
        for (size_t i = 0; i < c; i++) {
            for (size_t k = 0; k < depth_bytes; k++)
                if (whole.depth[i][k] != 0xA5) { std::fprintf(stderr, "a refused call wrote a depth image\n"); return 4; }
            for (size_t k = 0; k < 12 * pixels; k++)
                if (reinterpret_cast<const unsigned char *>(whole.normals[i].get())[k] != 0xA5) { std::fprintf(stderr, "a refused call wrote a normal image\n"); return 4; }
        }
        std::printf("refused\n");
        return 3;
    }
    bool same = dvo_tsdf::raycast(&vol, words.get(), &prm, count, format, rows, cols, K4.get(), poses.get(), clipped.dp.data(), clipped.np.data(), true);
    for (size_t i = 0; same && i < c; i++)
        same = std::memcmp(whole.depth[i].get(), clipped.depth[i].get(), depth_bytes) == 0 &&
               std::memcmp(whole.normals[i].get(), clipped.normals[i].get(), 12 * pixels) == 0;
    std::printf("depth %zu\n", c * pixels);
    for (size_t i = 0; i < c; i++)
        for (size_t k = 0; k < pixels; k++) {
            if (format == dvo_tsdf::kFormatU16) {
                unsigned short m;
                std::memcpy(&m, whole.depth[i].get() + 2 * k, 2);
                std::printf("%04x", (unsigned)m);
            } else {
                unsigned bits;
                std::memcpy(&bits, whole.depth[i].get() + 4 * k, 4);
                std::printf("%08x", bits);
            }
        }
    std::printf("\nnormals %zu\n", c * pixels);
    for (size_t i = 0; i < c; i++)
        for (size_t k = 0; k < 3 * pixels; k++) {
            unsigned bits;
            std::memcpy(&bits, &whole.normals[i][k], 4);
            std::printf("%08x", bits);
        }
    std::printf("\nclipped equal %d\n", same ? 1 : 0);
    return 0;
}
