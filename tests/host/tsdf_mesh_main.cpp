/*
 * tsdf_mesh_main.cpp -- dvo_tsdf::mesh (rgbd_odometry_amd/csrc/dvo_tsdf_mesh.h: the body of dvo_mesh_host) as a stand-alone program, so
 * that tests/test_tsdf_mesh_cpu.py can run it under the address and undefined-behaviour sanitizers.  It includes the definition
 * header and nothing else of the library.
 *
 *   tsdf_mesh_main VOLUME_FILE WORDS_FILE MIN_WEIGHT
 *
 * VOLUME_FILE: the bytes of one dvo_tsdf_volume.  WORDS_FILE: nx * ny * nz words.
 * Output: "table ok" once the generated orientation table agrees with a geometric re-derivation done here in floating point, then
 * "vertices n", "triangles m" and "checksum x": the 64-bit FNV-1a of the vertex bytes followed by the triangle bytes.
 * Exit status 3: the arguments were refused (nothing but "refused" is printed; no count was written).
 * Every buffer is allocated to its exact size, so that an access past an end is the sanitizer's to see.
 */
#include "dvo_tsdf_mesh.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

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

/* every triangle of every (p, mask) of the table: its edges join an inside and an outside corner of the tetrahedron, its three vertices
 * are distinct, and with the vertices at the midpoints its normal has a positive dot product with (mean outside - mean inside) */
static bool table_ok() {
    using namespace dvo_tsdf;
    for (int p = 0; p < 6; p++)
        for (int m = 0; m < 16; m++) {
            const MeshCase &c = kMeshTable.c[p][m];
            const int n_in = mesh_popcount4(m);
            if (c.n != (n_in == 0 || n_in == 4 ? 0 : n_in == 2 ? 2 : 1)) return false;
            double in[3] = {0, 0, 0}, out[3] = {0, 0, 0};
            int corner_inside[8];
            for (int k = 0; k < 8; k++) corner_inside[k] = -1;
            for (int i = 0; i < 4; i++) {
                const int k = mesh_tet_corner(p, i);
                corner_inside[k] = (m >> i) & 1;
                for (int ax = 0; ax < 3; ax++) ((m >> i) & 1 ? in : out)[ax] += (double)((k >> ax) & 1);
            }
            for (int t = 0; t < c.n; t++) {
                double P[3][3];
                for (int v = 0; v < 3; v++) {
                    const int code = c.e[3 * t + v], a = code & 7, d = code >> 3;
                    if (d < 0 || d >= kMeshEdges) return false;
                    const int b = a | mesh_dir_corner(d);
                    if ((a & mesh_dir_corner(d)) != 0 || corner_inside[a] < 0 || corner_inside[b] < 0 || corner_inside[a] == corner_inside[b]) return false;
                    for (int ax = 0; ax < 3; ax++) P[v][ax] = 0.5 * (double)(((a >> ax) & 1) + ((b >> ax) & 1));
                }
                if (c.e[3 * t] == c.e[3 * t + 1] || c.e[3 * t] == c.e[3 * t + 2] || c.e[3 * t + 1] == c.e[3 * t + 2]) return false;
                double u[3], v[3];
                for (int ax = 0; ax < 3; ax++) { u[ax] = P[1][ax] - P[0][ax]; v[ax] = P[2][ax] - P[0][ax]; }
                const double cr[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
                double dot = 0.0;
                for (int ax = 0; ax < 3; ax++) dot += cr[ax] * (out[ax] / (double)(4 - n_in) - in[ax] / (double)n_in);
                if (!(dot > 0.0)) return false;
            }
        }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s volume words min_weight\n", argv[0]); return 2; }
    const int min_weight = std::atoi(argv[3]);
    dvo_tsdf_volume vol;
    if (!read_file(argv[1], &vol, sizeof(vol))) { std::fprintf(stderr, "cannot read the volume\n"); return 2; }
    const bool vol_ok = dvo_tsdf::volume_ok(&vol);
    const size_t n = vol_ok ? dvo_tsdf::voxels_of(vol) : 1;
    std::unique_ptr<unsigned[]> words(new unsigned[n]);
    std::memset(words.get(), 0, 4 * n);
    if (vol_ok && !read_file(argv[2], words.get(), 4 * n)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    if (!table_ok()) { std::fprintf(stderr, "the generated table disagrees with the geometry\n"); return 4; }
    std::printf("table ok\n");
    long long nv = -1, nt = -1;
    if (!dvo_tsdf::mesh(&vol, words.get(), min_weight, nullptr, 0, nullptr, 0, &nv, &nt)) {
        if (nv != -1 || nt != -1) { std::fprintf(stderr, "a refused call wrote a count\n"); return 4; }
        std::printf("refused\n");
        return 3;
    }
    std::unique_ptr<float[]> xyz(new float[3 * (size_t)nv + (nv ? 0 : 1)]);
    std::unique_ptr<int[]> tri(new int[3 * (size_t)nt + (nt ? 0 : 1)]);
    long long nv2 = -1, nt2 = -1;
    if (!dvo_tsdf::mesh(&vol, words.get(), min_weight, nv ? xyz.get() : nullptr, nv, nt ? tri.get() : nullptr, nt, &nv2, &nt2) || nv2 != nv || nt2 != nt) {
        std::fprintf(stderr, "the second call disagrees with the first\n");
        return 4;
    }
    /* one entry short on each side: the prefixes must be the same bytes and nothing past them may be touched (exact allocations) */
    if (nv > 0 && nt > 0) {
        std::unique_ptr<float[]> xyz_short(new float[3 * (size_t)(nv - 1) + (nv > 1 ? 0 : 1)]);
        std::unique_ptr<int[]> tri_short(new int[3 * (size_t)(nt - 1) + (nt > 1 ? 0 : 1)]);
        if (!dvo_tsdf::mesh(&vol, words.get(), min_weight, nv > 1 ? xyz_short.get() : nullptr, nv - 1, nt > 1 ? tri_short.get() : nullptr, nt - 1, &nv2, &nt2) ||
            nv2 != nv || nt2 != nt || std::memcmp(xyz_short.get(), xyz.get(), 12 * (size_t)(nv - 1)) != 0 ||
            std::memcmp(tri_short.get(), tri.get(), 12 * (size_t)(nt - 1)) != 0) {
            std::fprintf(stderr, "a call with short buffers disagrees with the full one\n");
            return 4;
        }
    }
    unsigned long long h = 0xCBF29CE484222325ull;
    h = fnv1a(h, xyz.get(), 12 * (size_t)nv);
    h = fnv1a(h, tri.get(), 12 * (size_t)nt);
    std::printf("vertices %lld\ntriangles %lld\nchecksum %016llx\n", nv, nt, h);
    return 0;
}
