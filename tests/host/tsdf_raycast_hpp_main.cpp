/*
 * tsdf_raycast_hpp_main.cpp -- the ray-cast part of the C++ mirror (include/dvo_amd.hpp: RaycastViews, RaycastImages, tsdfRaycastHost,
 * TsdfVolumes::raycast) as a program of tests/test_tsdf_raycast_cpu.py.  Plain g++, every warning on, linked against the library.
 *
 *   tsdf_raycast_hpp_main VOLUME_FILE WORDS_FILE VIEWS_FILE FORMAT ROWS COLS COUNT [device]
 *
 * The files are those of tests/host/tsdf_raycast_main.cpp (the parameters are the defaults).  Output: "depth n" and the pixels,
 * "normals n" and the normals, as that program prints them, from the mirror's host function; with the last argument one more line, about
 * the device: "device equal 1" when TsdfVolumes::raycast gives the same bytes, "device none <message>" where there is no device.  Exit
 * status 3: refused.
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
    if (argc != 8 && !(argc == 9 && std::string(argv[8]) == "device")) {
        std::fprintf(stderr, "usage: %s volume words views format rows cols count [device]\n", argv[0]);
        return 2;
    }
    const int format = std::atoi(argv[4]), rows = std::atoi(argv[5]), cols = std::atoi(argv[6]), count = std::atoi(argv[7]);
    dvo_tsdf_volume vol;
    if (!readFile(argv[1], &vol, sizeof(vol)) || count < 1 || rows < 1 || cols < 1) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    if (vol.nx < 1 || vol.ny < 1 || vol.nz < 1 || vol.nx > DVO_TSDF_MAX_DIM || vol.ny > DVO_TSDF_MAX_DIM || vol.nz > DVO_TSDF_MAX_DIM) { std::printf("refused\n"); return 3; }
    std::vector<unsigned> words(dvo_amd::tsdfVoxels(vol));
    if (!readFile(argv[2], words.data(), 4 * words.size())) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::vector<double> both(16 * (size_t)count);
    if (!readFile(argv[3], both.data(), 8 * both.size())) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    dvo_amd::RaycastViews views;
    for (int i = 0; i < count; i++) views.add(0, both.data() + 4 * (size_t)i, both.data() + 4 * (size_t)count + 12 * (size_t)i);

    dvo_amd::RaycastImages img;
    if (!dvo_amd::tsdfRaycastHost(vol, words, views, format, rows, cols, true, img)) {
        std::printf("refused\n");
        return 3;
    }
    const size_t pixels = (size_t)rows * (size_t)cols * (size_t)count;
    std::printf("depth %zu\n", pixels);
    for (size_t k = 0; k < pixels; k++) {
        if (format == DVO_DEPTH_U16) {
            unsigned short m;
            std::memcpy(&m, img.depth.data() + 2 * k, 2);
            std::printf("%04x", (unsigned)m);
        } else {
            unsigned bits;
            std::memcpy(&bits, img.depth.data() + 4 * k, 4);
            std::printf("%08x", bits);
        }
    }
    std::printf("\nnormals %zu\n", pixels);
    for (float v : img.normals) {
        unsigned bits;
        std::memcpy(&bits, &v, 4);
        std::printf("%08x", bits);
    }
    std::printf("\n");
    if (argc == 8) return 0;
    try {
        dvo_amd::TsdfVolumes map(1, (long long)words.size());
        map.setVolume(0, vol);
        map.setVoxels(0, words);
        const dvo_amd::RaycastImages dev = map.raycast(views, format, rows, cols, true);
        int launches = 0, syncs = 0;
        map.stats(launches, syncs);
        const dvo_amd::RaycastImages alone = map.raycast(views, format, rows, cols);
        const bool same = dev.depth == img.depth && dev.normals.size() == img.normals.size() &&
                          std::memcmp(dev.normals.data(), img.normals.data(), 4 * img.normals.size()) == 0 && alone.depth == img.depth &&
                          alone.normals.empty() && alone.normalsOf(0) == nullptr && launches == DVO_RAYCAST_LAUNCHES && syncs == 1 &&
                          map.voxels(0) == words;
        std::printf("device equal %d\n", same ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("device none %s\n", e.what());
    }
    return 0;
}
