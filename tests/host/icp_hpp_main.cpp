/*
 * icp_hpp_main.cpp -- the alignment part of the C++ mirror (include/dvo_amd.hpp: IcpViews, IcpResult, icpAlignHost, IcpAligner) as a
 * program of tests/test_icp_cpu.py.  Plain g++, every warning on, linked against the library.
 *
 *   icp_hpp_main PARAMS_FILE VIEWS_FILE NOW_FORMAT MODEL_FORMAT ROWS COLS COUNT [device]
 *
 * The files are those of tests/host/icp_main.cpp.  Output: "poses n" and "records n" with their bytes, as that program prints them, from
 * the mirror's host function; with the last argument one more line, about the device: "device equal 1" when IcpAligner::align gives the
 * same bytes with the launches and the one synchronisation of the contract, "device none <message>" where there is no device.  Exit
 * status 3: refused.
 */
#include "dvo_amd.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 8 && !(argc == 9 && std::string(argv[8]) == "device")) {
        std::fprintf(stderr, "usage: %s params views now_format model_format rows cols count [device]\n", argv[0]);
        return 2;
    }
    const int nowFormat = std::atoi(argv[3]), modelFormat = std::atoi(argv[4]), rows = std::atoi(argv[5]), cols = std::atoi(argv[6]),
              count = std::atoi(argv[7]);
    if (count < 1 || rows < 1 || cols < 1 || (nowFormat != DVO_DEPTH_F32 && nowFormat != DVO_DEPTH_U16) ||
        (modelFormat != DVO_DEPTH_F32 && modelFormat != DVO_DEPTH_U16)) {
        std::fprintf(stderr, "bad arguments\n");
        return 2;
    }
    dvo_icp_params prm;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(&prm, 1, sizeof(prm), f) != sizeof(prm)) { std::fprintf(stderr, "cannot read the parameters\n"); return 2; }
    std::fclose(f);
    const size_t c = (size_t)count, pixels = (size_t)rows * (size_t)cols;
    const size_t nowBytes = pixels * (nowFormat == DVO_DEPTH_U16 ? 2 : 4), modelBytes = pixels * (modelFormat == DVO_DEPTH_U16 ? 2 : 4);
    std::vector<double> head(28 * c);
    std::vector<std::vector<unsigned char>> now(c, std::vector<unsigned char>(nowBytes)), model(c, std::vector<unsigned char>(modelBytes));
    std::vector<std::vector<float>> normals(c, std::vector<float>(3 * pixels));
    f = std::fopen(argv[2], "rb");
    bool ok = f && std::fread(head.data(), 8, head.size(), f) == head.size();
    for (size_t i = 0; ok && i < c; i++)
        ok = std::fread(now[i].data(), 1, nowBytes, f) == nowBytes && std::fread(model[i].data(), 1, modelBytes, f) == modelBytes &&
             std::fread(normals[i].data(), 4, 3 * pixels, f) == 3 * pixels;
    if (f) std::fclose(f);
    if (!ok) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    dvo_amd::IcpViews views;
    for (size_t i = 0; i < c; i++)
        views.add(now[i].data(), model[i].data(), normals[i].data(), head.data() + 4 * i, head.data() + 4 * c + 12 * i, head.data() + 16 * c + 12 * i);

    dvo_amd::IcpResult res;
    if (!dvo_amd::icpAlignHost(views, nowFormat, modelFormat, rows, cols, res, &prm)) {
        std::printf("refused\n");
        return 3;
    }
    std::printf("poses %zu\n", c);
    for (double v : res.poses12) {
        unsigned long long bits;
        std::memcpy(&bits, &v, 8);
        std::printf("%016llx", bits);
    }
    std::printf("\nrecords %zu\n", c);
    const unsigned char *rb = reinterpret_cast<const unsigned char *>(res.records.data());
    for (size_t k = 0; k < sizeof(dvo_icp_record) * c; k++) std::printf("%02x", (unsigned)rb[k]);
    std::printf("\n");
    if (argc == 8) return 0;
    try {
        dvo_amd::IcpAligner icp(count);
        icp.params = prm;
        const dvo_amd::IcpResult dev = icp.align(views, nowFormat, modelFormat, rows, cols);
        int launches = 0, syncs = 0, sweeps = 1;
        icp.stats(launches, syncs);
        for (int l = 0; l < prm.levels; l++) sweeps += prm.iterations[l];
        const bool same = dev.poses12.size() == res.poses12.size() && std::memcmp(dev.poses12.data(), res.poses12.data(), 8 * res.poses12.size()) == 0 &&
                          dev.records.size() == res.records.size() &&
                          std::memcmp(dev.records.data(), res.records.data(), sizeof(dvo_icp_record) * res.records.size()) == 0 &&
                          launches == DVO_ICP_LAUNCHES_PER_SWEEP * sweeps && syncs == 1;
        std::printf("device equal %d\n", same ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("device none %s\n", e.what());
    }
    return 0;
}
