/*
 * esdf_hpp_main.cpp -- the distance-field part of the C++ mirror (include/dvo_amd.hpp: esdfHost, esdfDistancesHost, esdfQueryHost and
 * the members enableEsdf, updateEsdf, esdfWords, esdfDistances and esdfQuery of TsdfVolumes) as a program of tests/test_esdf_cpu.py.
 * Plain g++, every warning on, linked against the library.
 *
 *   esdf_hpp_main VOLUME_FILE WORDS_FILE MIN_WEIGHT SITES POINTS_FILE COUNT [device]
 *
 * The files and the output are those of tests/host/esdf_main.cpp, from the mirror's host functions; with the last argument one more
 * line, about the device: "device equal 1" when TsdfVolumes gives the same bytes with the launches and synchronisations the constants
 * state and refuses a stale field, "device none <message>" where there is no device.  Exit status 3: refused.
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

static unsigned long long fnv1a(const void *data, size_t bytes) {
    unsigned long long h = 0xCBF29CE484222325ull;
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 0x100000001B3ull; }
    return h;
}

int main(int argc, char **argv) {
    if (argc != 7 && !(argc == 8 && std::string(argv[7]) == "device")) {
        std::fprintf(stderr, "usage: %s volume words min_weight sites points count [device]\n", argv[0]);
        return 2;
    }
    dvo_esdf_params p;
    p.min_weight = std::atoi(argv[3]); p.sites = std::atoi(argv[4]);
    const int count = std::atoi(argv[6]);
    dvo_tsdf_volume vol;
    if (count < 1 || !readFile(argv[1], &vol, sizeof(vol))) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    if (vol.nx < 1 || vol.ny < 1 || vol.nz < 1 || vol.nx > DVO_TSDF_MAX_DIM || vol.ny > DVO_TSDF_MAX_DIM || vol.nz > DVO_TSDF_MAX_DIM) { std::printf("refused\n"); return 3; }
    std::vector<unsigned> tsdf(dvo_amd::tsdfVoxels(vol)), words;
    std::vector<double> points(3 * (size_t)count);
    if (!readFile(argv[2], tsdf.data(), 4 * tsdf.size()) || !readFile(argv[5], points.data(), 8 * points.size())) {
        std::fprintf(stderr, "cannot read the inputs\n");
        return 2;
    }
    std::vector<float> metres;
    std::vector<dvo_esdf_sample> records;
    if (!dvo_amd::esdfHost(vol, tsdf, words, &p) || !dvo_amd::esdfDistancesHost(vol, words, metres) || !dvo_amd::esdfQueryHost(vol, words, points, records)) {
        std::printf("refused\n");
        return 3;
    }
    std::printf("words %016llx\nmetres %016llx\nrecords %016llx\n", fnv1a(words.data(), 4 * words.size()), fnv1a(metres.data(), 4 * metres.size()),
                fnv1a(records.data(), sizeof(dvo_esdf_sample) * records.size()));
    if (argc == 7) return 0;
    try {
        dvo_amd::TsdfVolumes map(1, (long long)tsdf.size());
        map.setVolume(0, vol);
        map.enableEsdf();
        map.setVoxels(0, tsdf);
        int launches = 0, syncs = 0;
        map.updateEsdf({0}, &p);
        map.stats(launches, syncs);
        bool same = launches == DVO_ESDF_UPDATE_LAUNCHES && syncs == 1 && map.esdfWords(0) == words;
        const std::vector<float> devMetres = map.esdfDistances(0, 0, vol.nz);
        map.stats(launches, syncs);
        same = same && launches == 1 && syncs == 1 && devMetres.size() == metres.size() &&
               std::memcmp(devMetres.data(), metres.data(), 4 * metres.size()) == 0;
        const std::vector<dvo_esdf_sample> devRecords = map.esdfQuery(0, points);
        map.stats(launches, syncs);
        same = same && launches == 1 && syncs == 1 && devRecords.size() == records.size() &&
               std::memcmp(devRecords.data(), records.data(), sizeof(dvo_esdf_sample) * records.size()) == 0;
        map.setVoxels(0, tsdf);                     /* the field is stale now: every reader refuses */
        bool refused = false;
        try { map.esdfWords(0); } catch (const std::exception &) { refused = true; }
        std::printf("device equal %d\n", same && refused ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("device none %s\n", e.what());
    }
    return 0;
}
