/*
 * archive_blob_main.cpp -- the host-side validation of the key-frame archive blob (rgbd_odometry_amd/csrc/dvo_archive_blob.h) as a
 * stand-alone program: the code the library compiles, run without a device, under -fsanitize=address,undefined
 * (tests/test_archive_blob_cpu.py).
 *
 *   archive_blob_main FILE
 * reads FILE into an allocation of exactly its size -- a validator that reads one byte beyond a truncated blob is caught -- and prints
 *   ok VERSION ROWS COLS N_LEVELS FIRST_SHIFT PLACES_LEVEL D N_KEY_FRAMES TOTAL_BYTES   and, per key frame, one line
 *   kf ORIGIN_ID ORIGIN_STREAM ORIGIN_FRAME HAS_DESC PAYLOAD_OFFSET PAYLOAD_BYTES PAYLOAD_CHECKSUM N... PT4_OK...
 * exit status 0; or "refused: DEFECT", exit status 3, for a blob whose header, table or payload checksums are not valid.
 */
#include <cstdio>
#include <cstdlib>

#include "dvo_archive_blob.h"

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    unsigned char *blob = static_cast<unsigned char *>(std::malloc(size > 0 ? (size_t)size : 1));
    if (!blob || (size > 0 && std::fread(blob, 1, (size_t)size, f) != (size_t)size)) { std::fprintf(stderr, "read failed\n"); return 2; }
    std::fclose(f);

    dvo_blob::Info info;
    std::vector<dvo_blob::Record> table;
    std::string defect = dvo_blob::validate(blob, (size_t)size, &info, &table);
    if (defect.empty()) defect = dvo_blob::validate_payloads(blob, table);
    if (!defect.empty()) {
        std::printf("refused: %s\n", defect.c_str());
        std::free(blob);
        return 3;
    }
    std::printf("ok %u %d %d %d %d %d %d %d %llu\n", dvo_blob::kVersion, info.rows, info.cols, info.n_levels, info.first_shift, info.places_level,
                info.D, info.n_key_frames, (unsigned long long)info.total_bytes);
    for (const dvo_blob::Record &r : table) {
        std::printf("kf %lld %d %lld %d %llu %llu %llu", (long long)r.origin_id, r.origin_stream, (long long)r.origin_frame, r.has_desc,
                    (unsigned long long)r.payload_offset, (unsigned long long)r.payload_bytes, (unsigned long long)r.payload_checksum);
        for (int l = 0; l < dvo_blob::kMaxLevels; l++) std::printf(" %d", r.N[l]);
        for (int l = 0; l < dvo_blob::kMaxLevels; l++) std::printf(" %d", r.pt4_ok[l]);
        std::printf("\n");
    }
    /* the size arithmetic the kernels share: the sections of every payload tile it exactly */
    for (const dvo_blob::Record &r : table) {
        uint64_t o = 0;
        for (int l = 0; l < info.n_levels; l++)
            for (int s = 0; s < 4; s++) {
                if (dvo_blob::section_offset(r.N, l, s) != o) { std::printf("section_offset disagrees\n"); return 4; }
                o += dvo_blob::pad16(dvo_blob::section_bytes(s, r.N[l]));
            }
        if (o != dvo_blob::levels_bytes(r.N, info.n_levels) || dvo_blob::payload_bytes(r.N, info.n_levels, r.has_desc, info.D) != r.payload_bytes) {
            std::printf("payload arithmetic disagrees\n");
            return 4;
        }
    }
    std::free(blob);
    return 0;
}
