/*
 * tsdf_mesh_hpp_main.cpp -- the mesh part of the C++ mirror (include/dvo_amd.hpp: Mesh, tsdfMeshHost, TsdfVolumes::mesh) as a program
 * of tests/test_tsdf_mesh_cpu.py.  Plain g++, every warning on, linked against the library.
 *
 *   tsdf_mesh_hpp_main VOLUME_FILE WORDS_FILE MIN_WEIGHT [device]
 *
 * The files are those of tests/host/tsdf_mesh_main.cpp.  Output: "vertices n", "triangles m" and "checksum x" as that program prints
 * them, from the mirror's host function; with the last argument one more line, about the device: "device equal 1" when
 * TsdfVolumes::mesh gives the same bytes, "device none <message>" where there is no device.  Exit status 3: refused.
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

static unsigned long long fnv1a(unsigned long long h, const void *data, size_t bytes) {
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 0x100000001B3ull; }
    return h;
}

int main(int argc, char **argv) {
    if (argc != 4 && !(argc == 5 && std::string(argv[4]) == "device")) {
        std::fprintf(stderr, "usage: %s volume words min_weight [device]\n", argv[0]);
        return 2;
    }
    const int minWeight = std::atoi(argv[3]);
    dvo_tsdf_volume vol;
    if (!readFile(argv[1], &vol, sizeof(vol))) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    if (vol.nx < 1 || vol.ny < 1 || vol.nz < 1 || vol.nx > DVO_TSDF_MAX_DIM || vol.ny > DVO_TSDF_MAX_DIM || vol.nz > DVO_TSDF_MAX_DIM) { std::printf("refused\n"); return 3; }
    std::vector<unsigned> words(dvo_amd::tsdfVoxels(vol));
    if (!readFile(argv[2], words.data(), 4 * words.size())) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    dvo_amd::Mesh mesh;
    if (!dvo_amd::tsdfMeshHost(vol, words, minWeight, mesh)) {
        std::printf("refused\n");
        return 3;
    }
    unsigned long long h = 0xCBF29CE484222325ull;
    h = fnv1a(h, mesh.xyz.data(), 4 * mesh.xyz.size());
    h = fnv1a(h, mesh.tri.data(), 4 * mesh.tri.size());
    std::printf("vertices %zu\ntriangles %zu\nchecksum %016llx\n", mesh.vertices(), mesh.triangles(), h);
    if (argc == 4) return 0;
    try {
        dvo_amd::TsdfVolumes map(1, (long long)words.size());
        map.setVolume(0, vol);
        map.setVoxels(0, words);
        const dvo_amd::Mesh dev = map.mesh(0, minWeight);
        int launches = 0, syncs = 0;
        map.stats(launches, syncs);
        const bool same = dev.xyz.size() == mesh.xyz.size() && (mesh.xyz.empty() || std::memcmp(dev.xyz.data(), mesh.xyz.data(), 4 * mesh.xyz.size()) == 0) &&
                          dev.tri == mesh.tri && launches == DVO_MESH_LAUNCHES && syncs == 1 && map.voxels(0) == words;
        std::printf("device equal %d\n", same ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("device none %s\n", e.what());
    }
    return 0;
}
