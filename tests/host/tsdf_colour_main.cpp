/*
 * tsdf_colour_main.cpp -- dvo_tsdf::integrate_colour, mesh_colour and raycast_colour (rgbd_odometry_amd/csrc/dvo_tsdf_colour.h: the
 * bodies of dvo_colour_integrate_host, dvo_colour_mesh_host and dvo_colour_raycast_host) as a stand-alone program, so that
 * tests/test_tsdf_colour_cpu.py can run it under the address and undefined-behaviour sanitizers.  It includes the definition header and
 * nothing else of the library.
 *
 *   tsdf_colour_main VOLUME_FILE DEPTH_FILE IMAGE_FILE POSES_FILE COUNT ROWS COLS IMAGE_FORMAT MIN_WEIGHT FX FY CX CY
 *
 * VOLUME_FILE: the bytes of one dvo_tsdf_volume.  DEPTH_FILE: COUNT images of ROWS x COLS 16-bit millimetres.  IMAGE_FILE: COUNT images
 * of ROWS x COLS pixels of IMAGE_FORMAT (0 bgr8, 1 rgb8, 2 mono8).  POSES_FILE: COUNT poses of 12 doubles.
 * The frames are fused into a cleared volume with default parameters; the volume is meshed with MIN_WEIGHT; it is ray-cast from the
 * same poses with default parameters into 16-bit depth, normals and images of IMAGE_FORMAT.
 * Output: "words x", "colours x", "vertices n", "triangles m", "mesh x" (vertex bytes, colour bytes, triangle bytes) and "views x"
 * (depth, normals, images), x the 64-bit FNV-1a of the bytes.  Exit status 3: the arguments were refused ("refused" is printed).
 * Every buffer is allocated to its exact size, so that an access past an end is the sanitizer's to see.
 */
#include "dvo_tsdf_colour.h"

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

static unsigned long long fnv1a(unsigned long long h, const void *data, size_t bytes) {
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 0x100000001B3ull; }
    return h;
}

static const unsigned long long kSeed = 0xCBF29CE484222325ull;

int main(int argc, char **argv) {
    using namespace dvo_tsdf;
    if (argc != 14) { std::fprintf(stderr, "usage: %s volume depth images poses count rows cols image_format min_weight fx fy cx cy\n", argv[0]); return 2; }
    const int count = std::atoi(argv[5]), rows = std::atoi(argv[6]), cols = std::atoi(argv[7]), image_format = std::atoi(argv[8]);
    const int min_weight = std::atoi(argv[9]);
    if (count < 1 || rows < 1 || cols < 1) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    dvo_tsdf_volume vol;
    if (!read_file(argv[1], &vol, sizeof(vol))) { std::fprintf(stderr, "cannot read the volume\n"); return 2; }
    const size_t n = volume_ok(&vol) ? voxels_of(vol) : 1, pixels = (size_t)rows * (size_t)cols;
    const size_t bpp = image_format_ok(image_format) ? image_pixel_bytes(image_format) : 1;
    std::vector<std::unique_ptr<unsigned short[]>> depth;
    std::vector<std::unique_ptr<unsigned char[]>> image;
    std::vector<const void *> dp, ip;
    {
        std::unique_ptr<unsigned short[]> all_d(new unsigned short[pixels * (size_t)count]);
        std::unique_ptr<unsigned char[]> all_i(new unsigned char[pixels * bpp * (size_t)count]);
        if (!read_file(argv[2], all_d.get(), 2 * pixels * (size_t)count) || !read_file(argv[3], all_i.get(), pixels * bpp * (size_t)count)) {
            std::fprintf(stderr, "cannot read the frames\n");
            return 2;
        }
        for (int i = 0; i < count; i++) {                                /* every image in an allocation of its own */
            depth.emplace_back(new unsigned short[pixels]);
            image.emplace_back(new unsigned char[pixels * bpp]);
            std::memcpy(depth.back().get(), all_d.get() + pixels * (size_t)i, 2 * pixels);
            std::memcpy(image.back().get(), all_i.get() + pixels * bpp * (size_t)i, pixels * bpp);
            dp.push_back(depth.back().get());
            ip.push_back(image.back().get());
        }
    }
    std::unique_ptr<double[]> poses(new double[12 * (size_t)count]), K4(new double[4 * (size_t)count]);
    if (!read_file(argv[4], poses.get(), 96 * (size_t)count)) { std::fprintf(stderr, "cannot read the poses\n"); return 2; }
    for (int i = 0; i < count; i++)
        for (int k = 0; k < 4; k++) K4[4 * (size_t)i + k] = std::atof(argv[10 + k]);

    std::unique_ptr<unsigned[]> words(new unsigned[n]);
    std::unique_ptr<unsigned long long[]> colours(new unsigned long long[n]);
    std::memset(words.get(), 0, 4 * n);
    std::memset(colours.get(), 0, 8 * n);
    dvo_tsdf_params p;
    params_default(&p);
    if (!integrate_colour(&vol, words.get(), colours.get(), &p, count, dp.data(), kFormatU16, ip.data(), image_format, rows, cols, K4.get(), poses.get())) {
        for (size_t a = 0; a < n; a++)
            if (words[a] || colours[a]) { std::fprintf(stderr, "a refused call wrote a word\n"); return 4; }
        std::printf("refused\n");
        return 3;
    }
    /* the words are those of the uncoloured definition */
    {
        std::unique_ptr<unsigned[]> plain(new unsigned[n]);
        std::memset(plain.get(), 0, 4 * n);
        if (!integrate(&vol, plain.get(), &p, count, dp.data(), kFormatU16, rows, cols, K4.get(), poses.get()) || std::memcmp(plain.get(), words.get(), 4 * n) != 0) {
            std::fprintf(stderr, "the words differ from integrate()'s\n");
            return 4;
        }
    }
    std::printf("words %016llx\ncolours %016llx\n", fnv1a(kSeed, words.get(), 4 * n), fnv1a(kSeed, colours.get(), 8 * n));

    long long nv = -1, nt = -1;
    if (!mesh_colour(&vol, words.get(), colours.get(), min_weight, nullptr, nullptr, 0, nullptr, 0, &nv, &nt)) {
        if (nv != -1 || nt != -1) { std::fprintf(stderr, "a refused call wrote a count\n"); return 4; }
        std::printf("refused\n");
        return 3;
    }
    std::unique_ptr<float[]> xyz(new float[3 * (size_t)nv + (nv ? 0 : 1)]);
    std::unique_ptr<unsigned char[]> rgb(new unsigned char[3 * (size_t)nv + (nv ? 0 : 1)]);
    std::unique_ptr<int[]> tri(new int[3 * (size_t)nt + (nt ? 0 : 1)]);
    long long nv2 = -1, nt2 = -1;
    if (!mesh_colour(&vol, words.get(), colours.get(), min_weight, nv ? xyz.get() : nullptr, nv ? rgb.get() : nullptr, nv, nt ? tri.get() : nullptr, nt,
                     &nv2, &nt2) || nv2 != nv || nt2 != nt) {
        std::fprintf(stderr, "the second call disagrees with the first\n");
        return 4;
    }
    if (nv > 1 && nt > 1) {                                              /* one entry short on each side, exact allocations */
        std::unique_ptr<float[]> xyz_short(new float[3 * (size_t)(nv - 1)]);
        std::unique_ptr<unsigned char[]> rgb_short(new unsigned char[3 * (size_t)(nv - 1)]);
        std::unique_ptr<int[]> tri_short(new int[3 * (size_t)(nt - 1)]);
        if (!mesh_colour(&vol, words.get(), colours.get(), min_weight, xyz_short.get(), rgb_short.get(), nv - 1, tri_short.get(), nt - 1, &nv2, &nt2) ||
            nv2 != nv || nt2 != nt || std::memcmp(xyz_short.get(), xyz.get(), 12 * (size_t)(nv - 1)) != 0 ||
            std::memcmp(rgb_short.get(), rgb.get(), 3 * (size_t)(nv - 1)) != 0 || std::memcmp(tri_short.get(), tri.get(), 12 * (size_t)(nt - 1)) != 0) {
            std::fprintf(stderr, "a call with short buffers disagrees with the full one\n");
            return 4;
        }
    }
    {
        unsigned long long h = fnv1a(kSeed, xyz.get(), 12 * (size_t)nv);
        h = fnv1a(h, rgb.get(), 3 * (size_t)nv);
        h = fnv1a(h, tri.get(), 12 * (size_t)nt);
        std::printf("vertices %lld\ntriangles %lld\nmesh %016llx\n", nv, nt, h);
    }

    dvo_raycast_params rp;
    raycast_params_default(&rp);
    std::vector<std::unique_ptr<unsigned short[]>> out_d;
    std::vector<std::unique_ptr<float[]>> out_n;
    std::vector<std::unique_ptr<unsigned char[]>> out_i;
    std::vector<void *> odp, oip;
    std::vector<float *> onp;
    for (int i = 0; i < count; i++) {
        out_d.emplace_back(new unsigned short[pixels]);
        out_n.emplace_back(new float[3 * pixels]);
        out_i.emplace_back(new unsigned char[pixels * bpp]);
        odp.push_back(out_d.back().get()); onp.push_back(out_n.back().get()); oip.push_back(out_i.back().get());
    }
    if (!raycast_colour(&vol, words.get(), colours.get(), &rp, count, kFormatU16, rows, cols, K4.get(), poses.get(), odp.data(), onp.data(), oip.data(),
                        image_format)) {
        std::printf("refused\n");
        return 3;
    }
    unsigned long long h = kSeed;
    for (int i = 0; i < count; i++) h = fnv1a(h, out_d[(size_t)i].get(), 2 * pixels);
    for (int i = 0; i < count; i++) h = fnv1a(h, out_n[(size_t)i].get(), 12 * pixels);
    for (int i = 0; i < count; i++) h = fnv1a(h, out_i[(size_t)i].get(), pixels * bpp);
    std::printf("views %016llx\n", h);
    return 0;
}
