/*
 * dvo_archive_blob.h -- the key-frame archive blob, format version 1 (include/dvo_amd.h, "export and import of the key-frame archive"):
 * the layout, the size and offset arithmetic, the checksum and the host-side validation, in plain C++.  No device, no context, no other
 * header of the library: dvo_capi_tracker_archive.cpp and dvo_tracker_archive_blob.hip compile it (the arithmetic is shared with the kernels),
 * and a stand-alone program can include the file as it is (tests/host/archive_blob_main.cpp).
 *
 * Little-endian throughout.  Every offset counts from the start of the blob and is a multiple of 16.
 *   [header: 80 bytes] [table: n_key_frames records of 144 bytes] [payloads]
 * The payload of a key frame is, for l = 0 .. n_levels - 1, the four sections cpts (8 N_l bytes), cidx (4 N_l), cpt4 (4 N_l) and chdr
 * (4 ceil(N_l / 64)) of the slot, then the D descriptor bytes where has_desc; every section is zero-padded to a multiple of 16 bytes.
 *
 * The checksum guards against truncation and bit rot.  It is NOT a security boundary: whoever can write a blob can write its checksums.
 */
#ifndef DVO_ARCHIVE_BLOB_H_
#define DVO_ARCHIVE_BLOB_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define DVO_BLOB_HD __host__ __device__ inline
#else
#define DVO_BLOB_HD inline
#endif

namespace dvo_blob {

constexpr int kMaxLevels = 8;      /* == DVO_MAX_LEVELS */
constexpr uint32_t kVersion = 1;
constexpr char kMagic[9] = "DVOKFAR1";

struct Header {
    char magic[8];                 /* "DVOKFAR1" */
    uint32_t version;              /* 1 */
    uint32_t zero0;
    uint64_t header_bytes;         /* sizeof(Header) */
    uint64_t record_bytes;         /* sizeof(Record) */
    uint64_t total_bytes;          /* the whole blob */
    int32_t n_key_frames;
    int32_t rows, cols, n_levels, first_shift;      /* the exporting tracker's geometry */
    int32_t places_level;          /* -1: no descriptors */
    int32_t D;                     /* bytes of a descriptor, 0: none */
    int32_t zero1;
    uint64_t table_checksum;       /* of the n_key_frames records */
};
static_assert(sizeof(Header) == 80 && sizeof(Header) % 16 == 0, "the header of format 1 has 80 bytes");

struct Record {
    int64_t origin_id;             /* the id the key frame had in the tracker that made it */
    int32_t origin_stream;
    int32_t zero0;
    int64_t origin_frame;
    float K[4];                    /* fx, fy, cx, cy: the bits the slot holds */
    int32_t N[kMaxLevels];         /* zero beyond n_levels */
    int32_t pt4_ok[kMaxLevels];    /* 0 or 1; zero beyond n_levels */
    int32_t has_desc;              /* 0 or 1 */
    int32_t zero1;
    uint64_t payload_offset, payload_bytes, payload_checksum;
    uint64_t zero2;
};
static_assert(sizeof(Record) == 144 && sizeof(Record) % 16 == 0, "a record of format 1 has 144 bytes");

/* ---- sizes and offsets (shared with the kernels) ---- */
DVO_BLOB_HD uint64_t pad16(uint64_t bytes) { return (bytes + 15u) & ~(uint64_t)15u; }
enum { SEC_CPTS = 0, SEC_CIDX = 1, SEC_CPT4 = 2, SEC_CHDR = 3 };
/* unpadded bytes of section `sec` of a level with N points */
DVO_BLOB_HD uint64_t section_bytes(int sec, int N) {
    const uint64_t n = N > 0 ? (uint64_t)N : 0;
    return sec == SEC_CPTS ? 8 * n : (sec == SEC_CHDR ? 4 * ((n + 63) / 64) : 4 * n);
}
DVO_BLOB_HD uint64_t level_bytes(int N) {
    return pad16(section_bytes(SEC_CPTS, N)) + pad16(section_bytes(SEC_CIDX, N)) + pad16(section_bytes(SEC_CPT4, N)) +
           pad16(section_bytes(SEC_CHDR, N));
}
/* offset of section `sec` of level `level` inside a payload */
DVO_BLOB_HD uint64_t section_offset(const int32_t *N, int level, int sec) {
    uint64_t o = 0;
    for (int l = 0; l < level; l++) o += level_bytes(N[l]);
    for (int s = 0; s < sec; s++) o += pad16(section_bytes(s, N[level]));
    return o;
}
/* offset of the descriptor = end of the levels */
DVO_BLOB_HD uint64_t levels_bytes(const int32_t *N, int n_levels) {
    uint64_t o = 0;
    for (int l = 0; l < n_levels; l++) o += level_bytes(N[l]);
    return o;
}
DVO_BLOB_HD uint64_t payload_bytes(const int32_t *N, int n_levels, int has_desc, int D) {
    return levels_bytes(N, n_levels) + (has_desc ? pad16((uint64_t)(D > 0 ? D : 0)) : 0);
}

/* ---- checksum: sum_i mix(w_i | (i + 1) << 32) mod 2^64 over the u32 words of a range; mix = the splitmix64 finaliser ---- */
DVO_BLOB_HD uint64_t mix_word(uint32_t w, uint64_t index) {
    uint64_t z = (uint64_t)w | ((index + 1) << 32);
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
inline uint64_t checksum(const void *bytes, uint64_t n_bytes) {      /* n_bytes: a multiple of 4 */
    const unsigned char *p = static_cast<const unsigned char *>(bytes);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n_bytes / 4; i++) {
        uint32_t w;
        memcpy(&w, p + 4 * i, 4);
        sum += mix_word(w, i);
    }
    return sum;
}

/* ---- validation of header and table: an empty string, or the first defect found ---- */
struct Info {
    int rows = 0, cols = 0, n_levels = 0, first_shift = 0, places_level = -1, D = 0, n_key_frames = 0;
    uint64_t total_bytes = 0;
};

inline std::string validate(const void *blob, size_t bytes, Info *info, std::vector<Record> *table = nullptr) {
    const unsigned char *p = static_cast<const unsigned char *>(blob);
    if (bytes < sizeof(Header)) return "the blob is shorter than a header (" + std::to_string(bytes) + " bytes)";
    Header h;
    memcpy(&h, p, sizeof(Header));
    if (memcmp(h.magic, kMagic, 8) != 0) return "bad magic: not a key-frame archive blob";
    if (h.version != kVersion) return "format version " + std::to_string(h.version) + ", this library reads version 1";
    if (h.header_bytes != sizeof(Header) || h.record_bytes != sizeof(Record)) return "header_bytes / record_bytes are not those of format 1";
    if (h.zero0 != 0 || h.zero1 != 0) return "the header's padding is not zero";
    if (h.n_key_frames < 0) return "n_key_frames is negative";
    if (h.rows < 1 || h.cols < 1 || h.n_levels < 1 || h.n_levels > kMaxLevels || h.first_shift < 0) return "bad geometry in the header";
    if (h.places_level < -1 || h.places_level >= h.n_levels || h.D < 0 || (h.places_level < 0) != (h.D == 0))
        return "places_level and D of the header do not go together";
    const uint64_t table_end = sizeof(Header) + (uint64_t)h.n_key_frames * sizeof(Record);
    if (h.total_bytes % 16 != 0 || h.total_bytes < table_end) return "total_bytes does not hold the table";
    if (h.total_bytes != (uint64_t)bytes)
        return "the blob has " + std::to_string(bytes) + " bytes, its header says " + std::to_string(h.total_bytes) +
               (h.total_bytes > (uint64_t)bytes ? " (truncated)" : " (trailing bytes)");
    if (checksum(p + sizeof(Header), table_end - sizeof(Header)) != h.table_checksum) return "the table checksum does not match";
    std::vector<Record> recs((size_t)h.n_key_frames);
    if (h.n_key_frames > 0) memcpy(recs.data(), p + sizeof(Header), (size_t)h.n_key_frames * sizeof(Record));
    std::vector<std::pair<uint64_t, uint64_t>> spans;
    for (int i = 0; i < h.n_key_frames; i++) {
        const Record &r = recs[(size_t)i];
        const std::string who = "key frame " + std::to_string(i) + ": ";
        if (r.zero0 != 0 || r.zero1 != 0 || r.zero2 != 0) return who + "the record's padding is not zero";
        for (int l = 0; l < kMaxLevels; l++) {
            if (r.N[l] < 0) return who + "N is negative";
            if (r.pt4_ok[l] != 0 && r.pt4_ok[l] != 1) return who + "pt4_ok is neither 0 nor 1";
            if (l >= h.n_levels && (r.N[l] != 0 || r.pt4_ok[l] != 0)) return who + "N / pt4_ok are not zero beyond n_levels";
        }
        if (r.has_desc != 0 && r.has_desc != 1) return who + "has_desc is neither 0 nor 1";
        if (r.has_desc && h.D == 0) return who + "has_desc in a blob without descriptors";
        if (r.payload_bytes != payload_bytes(r.N, h.n_levels, r.has_desc, h.D)) return who + "payload_bytes is not what N, has_desc and D imply";
        if (r.payload_offset % 16 != 0 || r.payload_offset < table_end || r.payload_offset > h.total_bytes ||
            r.payload_bytes > h.total_bytes - r.payload_offset)
            return who + "payload offset out of range";
        if (r.payload_bytes > 0) spans.emplace_back(r.payload_offset, r.payload_bytes);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); i++)
        if (spans[i - 1].first + spans[i - 1].second > spans[i].first) return "overlapping payloads";
    if (info) {
        info->rows = h.rows; info->cols = h.cols; info->n_levels = h.n_levels; info->first_shift = h.first_shift;
        info->places_level = h.places_level; info->D = h.D; info->n_key_frames = h.n_key_frames; info->total_bytes = h.total_bytes;
    }
    if (table) table->swap(recs);
    return std::string();
}

/* the payload checksums as the host computes them (the library recomputes them on the device; the stand-alone program here) */
inline std::string validate_payloads(const void *blob, const std::vector<Record> &table) {
    const unsigned char *p = static_cast<const unsigned char *>(blob);
    for (size_t i = 0; i < table.size(); i++)
        if (checksum(p + table[i].payload_offset, table[i].payload_bytes) != table[i].payload_checksum)
            return "key frame " + std::to_string(i) + ": the payload checksum does not match";
    return std::string();
}

/* the header of a blob whose table (n records at blob + sizeof(Header)) is complete */
inline void write_header(void *blob, int n_key_frames, uint64_t total_bytes, int rows, int cols, int n_levels, int first_shift,
                         int places_level, int D) {
    Header h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, kMagic, 8);
    h.version = kVersion;
    h.header_bytes = sizeof(Header); h.record_bytes = sizeof(Record); h.total_bytes = total_bytes;
    h.n_key_frames = n_key_frames;
    h.rows = rows; h.cols = cols; h.n_levels = n_levels; h.first_shift = first_shift;
    h.places_level = places_level; h.D = D;
    h.table_checksum = checksum(static_cast<unsigned char *>(blob) + sizeof(Header), (uint64_t)n_key_frames * sizeof(Record));
    memcpy(blob, &h, sizeof(h));
}

}  // namespace dvo_blob
#endif
