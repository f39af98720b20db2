/*
 * esdf_main.cpp -- the definition of the distance fields (rgbd_odometry_amd/csrc/dvo_esdf.h) as a stand-alone program of
 * tests/test_esdf_cpu.py: the same code the library compiles, built with -fsanitize=address,undefined, every buffer allocated to its
 * exact size.
 *
 *   esdf_main VOLUME_FILE WORDS_FILE MIN_WEIGHT SITES POINTS_FILE COUNT
 *
 * VOLUME_FILE: one dvo_tsdf_volume; WORDS_FILE: its nx * ny * nz TSDF words; POINTS_FILE: COUNT points of three doubles.  Prints the
 * 64-bit FNV-1a of the ESDF words, of their metres and of the query records, one per line.  Exit status 3: refused.
 */
#include "dvo_esdf.h"

#include <cstdio>
#include <cstdlib>
#include <memory>

static bool readFile(const char *path, void *dst, size_t bytes) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fread(dst, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

static unsigned long long fnv1a(const void *data, size_t bytes) {
    unsigned long long h = 0xCBF29CE484222325ull;
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 0x100000001B3ull; }
    return h;
}

int main(int argc, char **argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s volume words min_weight sites points count\n", argv[0]);
        return 2;
    }
    dvo_esdf_params p;
    p.min_weight = std::atoi(argv[3]); p.sites = std::atoi(argv[4]);
    const int count = std::atoi(argv[6]);
    dvo_tsdf_volume vol;
    if (count < 1 || !readFile(argv[1], &vol, sizeof(vol))) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    if (!dvo_tsdf::volume_ok(&vol)) { std::printf("refused\n"); return 3; }
    const size_t n = dvo_tsdf::voxels_of(vol);
    std::unique_ptr<unsigned[]> tsdf(new unsigned[n]), words(new unsigned[n]);
    std::unique_ptr<float[]> metres(new float[n]);
    std::unique_ptr<double[]> points(new double[3 * (size_t)count]);
    std::unique_ptr<dvo_esdf_sample[]> records(new dvo_esdf_sample[(size_t)count]);
    if (!readFile(argv[2], tsdf.get(), 4 * n) || !readFile(argv[5], points.get(), 24 * (size_t)count)) { std::fprintf(stderr, "cannot read the inputs\n"); return 2; }
    if (!dvo_tsdf::esdf(&vol, tsdf.get(), &p, words.get()) || !dvo_tsdf::esdf_distances(&vol, words.get(), metres.get()) ||
        !dvo_tsdf::esdf_query(&vol, words.get(), count, points.get(), records.get())) {
        std::printf("refused\n");
        return 3;
    }
    std::printf("words %016llx\nmetres %016llx\nrecords %016llx\n", fnv1a(words.get(), 4 * n), fnv1a(metres.get(), 4 * n),
                fnv1a(records.get(), sizeof(dvo_esdf_sample) * (size_t)count));
    return 0;
}
