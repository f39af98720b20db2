/*
 * tsdf_hpp_main.cpp -- the depth-fusion part of the C++ mirror (include/dvo_amd.hpp: TsdfFrames, tsdfIntegrateHost, tsdfExtractHost,
 * TsdfVolumes) as a program of tests/test_tsdf_map_cpu.py.  Plain g++, every warning on, linked against the library.
 *
 *   tsdf_hpp_main VOLUME_FILE WORDS_FILE FRAMES_FILE DEPTH_FILE FORMAT ROWS COLS COUNT MIN_WEIGHT [device]
 *
 * The files are those of tests/host/tsdf_map_main.cpp (the parameters are the defaults).  Output: "words n" and the words, "points n" and
 * the points, as that program prints them, from the mirror's host functions; with the last argument one more line, about the device:
 * "device equal 1" when TsdfVolumes gives the same words and points, "device none <message>" where there is no device.  Exit status
 * 3: refused.
 */
#include "dvo_amd.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static bool readFile(const char *path, void *dst, size_t bytes) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fread(dst, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv) {
    if (argc != 10 && !(argc == 11 && std::string(argv[10]) == "device")) {
        std::fprintf(stderr, "usage: %s volume words frames depth format rows cols count min_weight [device]\n", argv[0]);
        return 2;
    }
    const int format = std::atoi(argv[5]), rows = std::atoi(argv[6]), cols = std::atoi(argv[7]), count = std::atoi(argv[8]),
              minWeight = std::atoi(argv[9]);
    dvo_tsdf_volume vol;
    if (!readFile(argv[1], &vol, sizeof(vol)) || count < 1 || rows < 1 || cols < 1) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    std::vector<unsigned> start(dvo_amd::tsdfVoxels(vol));
    if (!readFile(argv[2], start.data(), 4 * start.size())) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::vector<double> both(16 * (size_t)count);
    if (!readFile(argv[3], both.data(), 8 * both.size())) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    const size_t image = (size_t)rows * (size_t)cols * (format == DVO_DEPTH_U16 ? 2 : 4);
    std::vector<unsigned char> images(image * (size_t)count);
    if (!readFile(argv[4], images.data(), images.size())) { std::fprintf(stderr, "cannot read %s\n", argv[4]); return 2; }
    dvo_amd::TsdfFrames frames;
    for (int i = 0; i < count; i++) frames.add(0, images.data() + image * (size_t)i, both.data() + 4 * (size_t)i, both.data() + 4 * (size_t)count + 12 * (size_t)i);

    std::vector<unsigned> words = start;
    std::vector<float> xyz;
    if (!dvo_amd::tsdfIntegrateHost(vol, words, frames, format, rows, cols) || !dvo_amd::tsdfExtractHost(vol, words, minWeight, xyz)) {
        std::printf("refused\n");
        return 3;
    }
    std::printf("words %zu\n", words.size());
    for (unsigned w : words) std::printf("%08x", w);
    std::printf("\npoints %zu\n", xyz.size() / 3);
    for (float v : xyz) {
        unsigned bits;
        std::memcpy(&bits, &v, 4);
        std::printf("%08x", bits);
    }
    std::printf("\n");
    if (argc == 10) return 0;
    try {
        dvo_amd::TsdfVolumes map(1, (long long)words.size());
        map.setVolume(0, vol);
        map.setVoxels(0, start);
        map.integrate(frames, format, rows, cols);
        int launches = 0, syncs = 0;
        map.stats(launches, syncs);
        const bool same = map.voxels(0) == words && map.points(0, minWeight) == xyz && launches == DVO_TSDF_INTEGRATE_LAUNCHES && syncs == 1;
        std::printf("device equal %d\n", same ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("device none %s\n", e.what());
    }
    return 0;
}
