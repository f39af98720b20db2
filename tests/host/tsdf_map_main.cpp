/*
 * tsdf_map_main.cpp -- dvo_tsdf::integrate and dvo_tsdf::extract (rgbd_odometry_amd/csrc/dvo_tsdf_map.h: the bodies of
 * dvo_tsdf_integrate_host and dvo_tsdf_extract_host) as a stand-alone program, so that tests/test_tsdf_map_cpu.py can run them under the
 * address and undefined-behaviour sanitizers.
 *
 *   tsdf_map_main VOLUME_FILE PARAMS_FILE WORDS_FILE FRAMES_FILE DEPTH_FILE FORMAT ROWS COLS COUNT MIN_WEIGHT
 *
 * VOLUME_FILE: the bytes of one dvo_tsdf_volume.  PARAMS_FILE: one dvo_tsdf_params.  WORDS_FILE: nx * ny * nz words, the state before.
 * FRAMES_FILE: 4 COUNT doubles K4, then 12 COUNT doubles poses.  DEPTH_FILE: COUNT images of ROWS x COLS raw values, row-major, FORMAT
 * 0 = float metres, 1 = 16-bit millimetres.  COUNT 0: no integration, extraction only.
 * Output: "words n" and the n words as eight hex digits each on one line; "points n" and the 3 n floats' bit patterns likewise.
 * Exit status 3: the arguments were refused (nothing but "refused" is printed; the words are checked to be untouched).
 * Every buffer is allocated to its exact size, so that an access past an end is the sanitizer's to see.
 */
#include "dvo_tsdf_map.h"

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

int main(int argc, char **argv) {
    if (argc != 11) { std::fprintf(stderr, "usage: %s volume params words frames depth format rows cols count min_weight\n", argv[0]); return 2; }
    const int format = std::atoi(argv[6]), rows = std::atoi(argv[7]), cols = std::atoi(argv[8]), count = std::atoi(argv[9]),
              min_weight = std::atoi(argv[10]);
    dvo_tsdf_volume vol;
    dvo_tsdf_params prm;
    if (!read_file(argv[1], &vol, sizeof(vol)) || !read_file(argv[2], &prm, sizeof(prm))) { std::fprintf(stderr, "cannot read the volume or the parameters\n"); return 2; }
    const bool vol_ok = dvo_tsdf::volume_ok(&vol);
    const size_t n = vol_ok ? dvo_tsdf::voxels_of(vol) : 1;
    std::unique_ptr<unsigned[]> words(new unsigned[n]), before(new unsigned[n]);
    std::memset(words.get(), 0, 4 * n);
    if (vol_ok && !read_file(argv[3], words.get(), 4 * n)) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    std::memcpy(before.get(), words.get(), 4 * n);
    if (count != 0) {
        const size_t c = count > 0 ? (size_t)count : 1;
        std::unique_ptr<double[]> K4(new double[4 * c]), poses(new double[12 * c]);
        {
            std::vector<double> both(16 * c, 0.0);
            if (count > 0 && !read_file(argv[4], both.data(), 8 * both.size())) { std::fprintf(stderr, "cannot read %s\n", argv[4]); return 2; }
            std::memcpy(K4.get(), both.data(), 32 * c);
            std::memcpy(poses.get(), both.data() + 4 * c, 96 * c);
        }
        const bool geometry = dvo_tsdf::format_ok(format) && rows >= 1 && cols >= 1 && count > 0;      /* else: refused below, nothing to read */
        const size_t image = geometry ? (size_t)rows * (size_t)cols * dvo_tsdf::depth_pixel_bytes(format) : 1;
        std::vector<std::unique_ptr<unsigned char[]>> images;      /* one allocation per image: none may be read past its end */
        std::vector<const void *> depth;
        FILE *f = geometry ? std::fopen(argv[5], "rb") : nullptr;
        for (size_t i = 0; i < c; i++) {
            images.emplace_back(new unsigned char[image]);
            std::memset(images.back().get(), 0, image);
            if (geometry && (!f || std::fread(images.back().get(), 1, image, f) != image)) { std::fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
            depth.push_back(images.back().get());
        }
        if (f) std::fclose(f);
        if (!dvo_tsdf::integrate(&vol, words.get(), &prm, count, depth.data(), format, rows, cols, K4.get(), poses.get())) {
            if (std::memcmp(before.get(), words.get(), 4 * n) != 0) { std::fprintf(stderr, "a refused call wrote the words\n"); return 4; }
            std::printf("refused\n");
            return 3;
        }
    }
    long long n_points = -1;
    if (!dvo_tsdf::extract(&vol, words.get(), min_weight, nullptr, 0, &n_points)) {
        if (n_points != -1) { std::fprintf(stderr, "a refused call wrote the count\n"); return 4; }
        std::printf("refused\n");
        return 3;
    }
    const size_t np = (size_t)n_points;
    std::unique_ptr<float[]> xyz(new float[3 * np + (np ? 0 : 1)]);
    long long again = -1;
    if (!dvo_tsdf::extract(&vol, words.get(), min_weight, np ? xyz.get() : nullptr, n_points, &again) || again != n_points) {
        std::fprintf(stderr, "the second extraction disagrees with the first\n");
        return 4;
    }
    std::printf("words %zu\n", n);
    for (size_t i = 0; i < n; i++) std::printf("%08x", words[i]);
    std::printf("\npoints %lld\n", n_points);
    for (size_t i = 0; i < 3 * np; i++) {
        unsigned bits;
        std::memcpy(&bits, &xyz[i], 4);
        std::printf("%08x", bits);
    }
    std::printf("\n");
    return 0;
}
