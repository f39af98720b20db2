/*
 * icp_prepare_hpp_main.cpp -- the depth front end of the C++ mirror (include/dvo_amd.hpp: IcpPrepared, icpPrepareHost, the now normals
 * of IcpViews, IcpAligner::prepare) as a program of tests/test_icp_prepare_cpu.py.  Plain g++, every warning on, linked against the
 * library.
 *
 *   icp_prepare_hpp_main PREPARE_PARAMS_FILE PARAMS_FILE VIEWS_FILE NOW_FORMAT MODEL_FORMAT ROWS COLS COUNT COS_MIN [device]
 *
 * The arguments and the output are those of tests/host/icp_prepare_main.cpp, from the mirror's host functions; with the last argument
 * one more line, about the device: "device equal 1" when IcpAligner::prepare and the gated IcpAligner::align give the same bytes with
 * the launches and the one synchronisation of their contracts, "device none <message>" where there is no device.  Exit status 3: refused.
 */
#include "dvo_amd.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static void hex_line(const void *p, size_t n) {
    for (size_t k = 0; k < n; k++) std::printf("%02x", (unsigned)static_cast<const unsigned char *>(p)[k]);
}
static bool same_images(const std::vector<std::vector<float>> &a, const std::vector<std::vector<float>> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].size() != b[i].size() || std::memcmp(a[i].data(), b[i].data(), 4 * a[i].size()) != 0) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 10 && !(argc == 11 && std::string(argv[10]) == "device")) {
        std::fprintf(stderr, "usage: %s prepare_params params views now_format model_format rows cols count cos_min_bits [device]\n", argv[0]);
        return 2;
    }
    const int nowFormat = std::atoi(argv[4]), modelFormat = std::atoi(argv[5]), rows = std::atoi(argv[6]), cols = std::atoi(argv[7]),
              count = std::atoi(argv[8]);
    if (count < 1 || rows < 1 || cols < 1 || (nowFormat != DVO_DEPTH_F32 && nowFormat != DVO_DEPTH_U16) ||
        (modelFormat != DVO_DEPTH_F32 && modelFormat != DVO_DEPTH_U16)) {
        std::fprintf(stderr, "bad arguments\n");
        return 2;
    }
    double cosMin;
    const unsigned long long cosBits = std::strtoull(argv[9], nullptr, 16);
    std::memcpy(&cosMin, &cosBits, 8);
    dvo_icp_prepare_params fp;
    dvo_icp_params prm;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(&fp, 1, sizeof(fp), f) != sizeof(fp)) { std::fprintf(stderr, "cannot read the prepare parameters\n"); return 2; }
    std::fclose(f);
    f = std::fopen(argv[2], "rb");
    if (!f || std::fread(&prm, 1, sizeof(prm), f) != sizeof(prm)) { std::fprintf(stderr, "cannot read the parameters\n"); return 2; }
    std::fclose(f);
    const size_t c = (size_t)count, pixels = (size_t)rows * (size_t)cols;
    const size_t nowBytes = pixels * (nowFormat == DVO_DEPTH_U16 ? 2 : 4), modelBytes = pixels * (modelFormat == DVO_DEPTH_U16 ? 2 : 4);
    std::vector<double> head(28 * c);
    std::vector<std::vector<unsigned char>> now(c, std::vector<unsigned char>(nowBytes)), model(c, std::vector<unsigned char>(modelBytes));
    std::vector<std::vector<float>> normals(c, std::vector<float>(3 * pixels));
    f = std::fopen(argv[3], "rb");
    bool ok = f && std::fread(head.data(), 8, head.size(), f) == head.size();
    for (size_t i = 0; ok && i < c; i++)
        ok = std::fread(now[i].data(), 1, nowBytes, f) == nowBytes && std::fread(model[i].data(), 1, modelBytes, f) == modelBytes &&
             std::fread(normals[i].data(), 4, 3 * pixels, f) == 3 * pixels;
    if (f) std::fclose(f);
    if (!ok) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    std::vector<const void *> depth;
    for (size_t i = 0; i < c; i++) depth.push_back(now[i].data());
    const std::vector<double> K4(head.begin(), head.begin() + 4 * (long)c);

    dvo_amd::IcpPrepared prepared;
    if (!dvo_amd::icpPrepareHost(depth, nowFormat, rows, cols, K4, prepared, true, &fp)) {
        std::printf("refused\n");
        return 3;
    }
    dvo_amd::IcpViews views;
    for (size_t i = 0; i < c; i++) {
        views.add(now[i].data(), model[i].data(), normals[i].data(), head.data() + 4 * i, head.data() + 4 * c + 12 * i, head.data() + 16 * c + 12 * i);
        views.setNowNormals((int)i, prepared.normals[i].data());
    }
    views.normalCosMin = cosMin;
    dvo_amd::IcpResult res;
    if (!dvo_amd::icpAlignHost(views, nowFormat, modelFormat, rows, cols, res, &prm)) {
        std::printf("refused\n");
        return 3;
    }
    std::printf("depth %zu\n", c);
    for (size_t i = 0; i < c; i++) hex_line(prepared.depth[i].data(), 4 * pixels);
    std::printf("\nnormals %zu\n", c);
    for (size_t i = 0; i < c; i++) hex_line(prepared.normals[i].data(), 12 * pixels);
    std::printf("\nposes %zu\n", c);
    for (double v : res.poses12) {
        unsigned long long bits;
        std::memcpy(&bits, &v, 8);
        std::printf("%016llx", bits);
    }
    std::printf("\nrecords %zu\n", c);
    hex_line(res.records.data(), sizeof(dvo_icp_record) * c);
    std::printf("\n");
    if (argc == 10) return 0;
    try {
        dvo_amd::IcpAligner icp(count);
        icp.params = prm;
        icp.prepareParams = fp;
        const dvo_amd::IcpPrepared dev = icp.prepare(depth, nowFormat, rows, cols, K4);
        int launches = 0, syncs = 0, sweeps = 1;
        icp.stats(launches, syncs);
        bool same = same_images(dev.depth, prepared.depth) && same_images(dev.normals, prepared.normals) && launches == DVO_ICP_PREPARE_LAUNCHES && syncs == 1;
        for (size_t i = 0; i < c; i++) views.setNowNormals((int)i, dev.normals[i].data());
        const dvo_amd::IcpResult aligned = icp.align(views, nowFormat, modelFormat, rows, cols);
        icp.stats(launches, syncs);
        for (int l = 0; l < prm.levels; l++) sweeps += prm.iterations[l];
        same = same && aligned.poses12.size() == res.poses12.size() &&
               std::memcmp(aligned.poses12.data(), res.poses12.data(), 8 * res.poses12.size()) == 0 && aligned.records.size() == res.records.size() &&
               std::memcmp(aligned.records.data(), res.records.data(), sizeof(dvo_icp_record) * res.records.size()) == 0 &&
               launches == DVO_ICP_LAUNCHES_PER_SWEEP * sweeps && syncs == 1;
        std::printf("device equal %d\n", same ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("device none %s\n", e.what());
    }
    return 0;
}
