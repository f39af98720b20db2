/*
 * tsdf_colour_hpp_main.cpp -- the colour part of the C++ mirror (include/dvo_amd.hpp: TsdfFrames::image, RaycastImages::image,
 * Mesh::rgb, tsdfIntegrateColourHost, tsdfRaycastColourHost, tsdfMeshColourHost and the colour methods of TsdfVolumes) as a program of
 * tests/test_tsdf_colour_cpu.py.  Plain g++, every warning on, linked against the library.
 *
 *   tsdf_colour_hpp_main VOLUME_FILE DEPTH_FILE IMAGE_FILE POSES_FILE COUNT ROWS COLS IMAGE_FORMAT MIN_WEIGHT FX FY CX CY [device]
 *
 * The files and the output are those of tests/host/tsdf_colour_main.cpp, from the mirror's host functions; with the last argument one
 * more line, about the device: "device equal 1" when the colour methods of TsdfVolumes give the same bytes with the launches and
 * synchronisations the constants state, "device none <message>" where there is no device.  Exit status 3: refused.
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

static const unsigned long long kSeed = 0xCBF29CE484222325ull;

static unsigned long long meshSum(const dvo_amd::Mesh &m) {
    unsigned long long h = fnv1a(kSeed, m.xyz.data(), 4 * m.xyz.size());
    h = fnv1a(h, m.rgb.data(), m.rgb.size());
    return fnv1a(h, m.tri.data(), 4 * m.tri.size());
}

static unsigned long long viewsSum(const dvo_amd::RaycastImages &v) {
    unsigned long long h = fnv1a(kSeed, v.depth.data(), v.depth.size());
    h = fnv1a(h, v.normals.data(), 4 * v.normals.size());
    return fnv1a(h, v.image.data(), v.image.size());
}

int main(int argc, char **argv) {
    if (argc != 14 && !(argc == 15 && std::string(argv[14]) == "device")) {
        std::fprintf(stderr, "usage: %s volume depth images poses count rows cols image_format min_weight fx fy cx cy [device]\n", argv[0]);
        return 2;
    }
    const int count = std::atoi(argv[5]), rows = std::atoi(argv[6]), cols = std::atoi(argv[7]), imageFormat = std::atoi(argv[8]);
    const int minWeight = std::atoi(argv[9]);
    const double K4[4] = {std::atof(argv[10]), std::atof(argv[11]), std::atof(argv[12]), std::atof(argv[13])};
    dvo_tsdf_volume vol;
    if (count < 1 || rows < 1 || cols < 1 || !readFile(argv[1], &vol, sizeof(vol))) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    if (vol.nx < 1 || vol.ny < 1 || vol.nz < 1 || vol.nx > DVO_TSDF_MAX_DIM || vol.ny > DVO_TSDF_MAX_DIM || vol.nz > DVO_TSDF_MAX_DIM) { std::printf("refused\n"); return 3; }
    const size_t pixels = (size_t)rows * (size_t)cols, bpp = imageFormat == DVO_CAM_MONO8 ? 1 : 3;
    std::vector<unsigned short> depth(pixels * (size_t)count);
    std::vector<unsigned char> image(pixels * bpp * (size_t)count);
    std::vector<double> poses(12 * (size_t)count);
    if (!readFile(argv[2], depth.data(), 2 * depth.size()) || !readFile(argv[3], image.data(), image.size()) || !readFile(argv[4], poses.data(), 8 * poses.size())) {
        std::fprintf(stderr, "cannot read the frames\n");
        return 2;
    }
    dvo_amd::TsdfFrames frames;
    dvo_amd::RaycastViews views;
    for (int i = 0; i < count; i++) {
        frames.add(0, depth.data() + pixels * (size_t)i, image.data() + pixels * bpp * (size_t)i, K4, poses.data() + 12 * (size_t)i);
        views.add(0, K4, poses.data() + 12 * (size_t)i);
    }
    std::vector<unsigned> words(dvo_amd::tsdfVoxels(vol), 0u);
    std::vector<unsigned long long> colours(words.size(), 0ull);
    dvo_amd::Mesh mesh;
    dvo_amd::RaycastImages cast;
    if (!dvo_amd::tsdfIntegrateColourHost(vol, words, colours, frames, DVO_DEPTH_U16, imageFormat, rows, cols) ||
        !dvo_amd::tsdfMeshColourHost(vol, words, colours, minWeight, mesh) ||
        !dvo_amd::tsdfRaycastColourHost(vol, words, colours, views, DVO_DEPTH_U16, imageFormat, rows, cols, true, cast)) {
        std::printf("refused\n");
        return 3;
    }
    std::printf("words %016llx\ncolours %016llx\n", fnv1a(kSeed, words.data(), 4 * words.size()), fnv1a(kSeed, colours.data(), 8 * colours.size()));
    std::printf("vertices %zu\ntriangles %zu\nmesh %016llx\nviews %016llx\n", mesh.vertices(), mesh.triangles(), meshSum(mesh), viewsSum(cast));
    if (argc == 14) return 0;
    try {
        dvo_amd::TsdfVolumes map(1, (long long)words.size());
        map.setVolume(0, vol);
        map.enableColour();
        int launches = 0, syncs = 0;
        map.integrateColour(frames, DVO_DEPTH_U16, imageFormat, rows, cols);
        map.stats(launches, syncs);
        bool same = launches == DVO_TSDF_INTEGRATE_LAUNCHES && syncs == 1 && map.voxels(0) == words && map.colours(0) == colours;
        const dvo_amd::Mesh devMesh = map.meshColour(0, minWeight);
        map.stats(launches, syncs);
        same = same && launches == DVO_MESH_LAUNCHES && syncs == 1 && devMesh.vertices() == mesh.vertices() && meshSum(devMesh) == meshSum(mesh);
        const dvo_amd::RaycastImages devCast = map.raycastColour(views, DVO_DEPTH_U16, imageFormat, rows, cols, true);
        map.stats(launches, syncs);
        same = same && launches == DVO_RAYCAST_LAUNCHES && syncs == 1 && viewsSum(devCast) == viewsSum(cast);
        map.setColours(0, colours);
        same = same && map.colours(0) == colours;
        std::printf("device equal %d\n", same ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("device none %s\n", e.what());
    }
    return 0;
}
