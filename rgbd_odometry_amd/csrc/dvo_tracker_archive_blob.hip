/*
 * dvo_tracker_archive_blob.hip -- export and import of the key-frame archive (include/dvo_amd.h: dvo_tracker_archive_export,
 * dvo_tracker_archive_import; the blob's format: dvo_archive_blob.h; host side dvo_capi_tracker_archive.cpp).
 *
 * Three kernels, none of which touches the alignment or the tracker's context:
 *   archive_export_kernel   the listed slots of the ring -> one dense blob in a device staging buffer: ONE launch, grid = key frames x
 *                           (levels + descriptor) x EXPORT_Z sharing workgroups, like archive_store_kernel.  A workgroup gathers its
 *                           share of the ragged sections (zero padding included, zeros for the 4-byte twins of a level without valid
 *                           ones) and, while copying, forms its part of the key frame's checksum; the parts are added into the record of
 *                           the table with 64-bit atomic adds.  The checksum is a sum mod 2^64 of position-dependent terms: it has one
 *                           value whatever the order of the additions.  The workgroup (level 0, share 0) writes the rest of the record.
 *   archive_blob_sum_kernel the payload checksums of an uploaded blob, recomputed: one 64-bit sum per key frame.
 *   archive_import_kernel   the payloads of an uploaded, verified blob -> the slots the host chose: lists, ArchiveHeader, descriptor row
 *                           (padded with 128) and mark.  ONE launch, the export's grid.
 *
 * Every index is bounded: counts are clamped to the slot capacity, offsets were validated by the host against the blob's size
 * (dvo_blob::validate) before anything was uploaded.
 *
 * Compile with -ffp-contract=off.
 */
#include "dvo_launch.h"
#include "dvo_archive_blob.h"

namespace dvo {

namespace {

constexpr int BLOB_BLOCK = 256;
constexpr int EXPORT_Z = 4, SUM_Z = 8, IMPORT_Z = 4;      /* workgroups that share one (key frame, level) / one payload */

/* the workgroup's 64-bit sum -> *dst by one atomic add (addition mod 2^64: the order does not matter) */
DVO_DEV void block_add(unsigned long long sum, unsigned long long *dst, unsigned long long *red) {
    for (int o = 32; o > 0; o >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < BLOB_BLOCK / 64; w++) s += red[w];
        atomicAdd(dst, s);
    }
}

DVO_DEV int clamp_n(int N, int cap) { return N < 0 ? 0 : (N > cap ? cap : N); }

/* word i of a descriptor row of D bytes: bytes at or beyond D as `fill` */
DVO_DEV unsigned desc_word(const unsigned *row, int i, int D, unsigned fill) {
    if (4 * i + 4 <= D) return row[i];
    unsigned v = 0;
    const unsigned w = 4 * i < D ? row[i] : 0u;
    for (int b = 0; b < 4; b++) v |= (4 * i + b < D ? (w >> (8 * b)) & 255u : fill) << (8 * b);
    return v;
}

DVO_DEV dvo_blob::Record *record_of(unsigned char *blob, int index) {
    return reinterpret_cast<dvo_blob::Record *>(blob + sizeof(dvo_blob::Header)) + index;
}

}  // namespace

__global__ void __launch_bounds__(BLOB_BLOCK)
archive_export_kernel(const BlobEntry *__restrict__ entries, ArchiveView A, PlaceView P, unsigned char *__restrict__ blob) {
    __shared__ unsigned long long red[BLOB_BLOCK / 64];
    const BlobEntry &e = entries[blockIdx.x];
    const int y = blockIdx.y;
    if (e.slot < 0 || e.slot >= A.n_slots) return;
    dvo_blob::Record *rec = record_of(blob, e.record);
    unsigned *pay = reinterpret_cast<unsigned *>(blob + e.payload_offset);
    const ArchiveHeader &h = A.hdr[e.slot];
    const size_t first = (size_t)blockIdx.z * BLOB_BLOCK + threadIdx.x, step = (size_t)gridDim.z * BLOB_BLOCK;
    unsigned long long sum = 0;
    if (y < A.n_levels) {
        const ArchiveLevel &L = A.l[y];
        const int N = e.N[y];
        const int n = clamp_n(N, L.cap);                  /* the host lists what fits; a clamped list is written as zeros beyond n */
        const bool pt4 = h.pt4_ok[y] != 0;
        const unsigned *src[4] = {reinterpret_cast<const unsigned *>(L.cpts + (size_t)e.slot * L.cap), L.cidx + (size_t)e.slot * L.cap,
                                  L.cpt4 + (size_t)e.slot * L.cap, L.chdr + (size_t)e.slot * (L.cap / 64)};
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const size_t have = (s >= dvo_blob::SEC_CPT4 && !pt4) ? 0 : (size_t)(dvo_blob::section_bytes(s, n) / 4);
            const size_t words = (size_t)(dvo_blob::pad16(dvo_blob::section_bytes(s, N)) / 4);
            const size_t base = (size_t)(dvo_blob::section_offset(e.N, y, s) / 4);
            for (size_t i = first; i < words; i += step) {
                const unsigned w = i < have ? src[s][i] : 0u;
                pay[base + i] = w;
                sum += dvo_blob::mix_word(w, base + i);
            }
        }
        if (blockIdx.z == 0 && threadIdx.x == 0) rec->pt4_ok[y] = pt4 ? 1 : 0;
    } else if (e.has_desc && P.desc && P.D > 0 && P.D <= P.stride && e.slot < P.n_slots) {
        const unsigned *row = reinterpret_cast<const unsigned *>(P.desc + (size_t)e.slot * P.stride);
        const size_t words = (size_t)(dvo_blob::pad16((uint64_t)P.D) / 4);
        const size_t base = (size_t)(dvo_blob::levels_bytes(e.N, A.n_levels) / 4);
        for (size_t i = first; i < words; i += step) {
            const unsigned w = desc_word(row, (int)i, P.D, 0u);
            pay[base + i] = w;
            sum += dvo_blob::mix_word(w, base + i);
        }
    }
    if (y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {      /* everything of the record but pt4_ok and the checksum (zeroed by the host) */
        rec->origin_id = e.origin_id; rec->origin_stream = e.origin_stream; rec->origin_frame = e.origin_frame;
        rec->K[0] = h.K.x; rec->K[1] = h.K.y; rec->K[2] = h.K.z; rec->K[3] = h.K.w;
        for (int l = 0; l < DVO_LEVELS; l++) rec->N[l] = l < A.n_levels ? e.N[l] : 0;
        rec->has_desc = e.has_desc;
        rec->payload_offset = e.payload_offset; rec->payload_bytes = e.payload_bytes;
    }
    block_add(sum, reinterpret_cast<unsigned long long *>(&rec->payload_checksum), red);
}

__global__ void __launch_bounds__(BLOB_BLOCK)
archive_blob_sum_kernel(const BlobEntry *__restrict__ entries, const unsigned char *__restrict__ blob, unsigned long long *__restrict__ sums) {
    __shared__ unsigned long long red[BLOB_BLOCK / 64];
    const BlobEntry &e = entries[blockIdx.x];
    const unsigned *pay = reinterpret_cast<const unsigned *>(blob + e.payload_offset);
    const size_t words = (size_t)(e.payload_bytes / 4);
    unsigned long long sum = 0;
    for (size_t i = (size_t)blockIdx.y * BLOB_BLOCK + threadIdx.x; i < words; i += (size_t)gridDim.y * BLOB_BLOCK) sum += dvo_blob::mix_word(pay[i], i);
    block_add(sum, sums + blockIdx.x, red);
}

__global__ void __launch_bounds__(BLOB_BLOCK)
archive_import_kernel(const BlobEntry *__restrict__ entries, const unsigned char *__restrict__ blob, ArchiveView A, PlaceView P) {
    const BlobEntry &e = entries[blockIdx.x];
    const int y = blockIdx.y;
    if (e.slot < 0 || e.slot >= A.n_slots) return;        /* refused by the host, or evicted by a later key frame of the same blob */
    const dvo_blob::Record *rec = record_of(const_cast<unsigned char *>(blob), e.record);
    const unsigned *pay = reinterpret_cast<const unsigned *>(blob + e.payload_offset);
    const size_t first = (size_t)blockIdx.z * BLOB_BLOCK + threadIdx.x, step = (size_t)gridDim.z * BLOB_BLOCK;
    if (y < A.n_levels) {
        const ArchiveLevel &L = A.l[y];
        const int N = e.N[y];
        const int n = clamp_n(N, L.cap);
        unsigned *dst[4] = {reinterpret_cast<unsigned *>(L.cpts + (size_t)e.slot * L.cap), L.cidx + (size_t)e.slot * L.cap,
                            L.cpt4 + (size_t)e.slot * L.cap, L.chdr + (size_t)e.slot * (L.cap / 64)};
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const size_t words = (size_t)(dvo_blob::section_bytes(s, n) / 4);
            const size_t base = (size_t)(dvo_blob::section_offset(e.N, y, s) / 4);
            for (size_t i = first; i < words; i += step) dst[s][i] = pay[base + i];
        }
        if (blockIdx.z == 0 && threadIdx.x == 0) {
            ArchiveHeader &h = A.hdr[e.slot];
            h.N[y] = (n == N) ? N : 0;                    /* a clamped list is no list */
            h.pt4_ok[y] = (n == N) ? rec->pt4_ok[y] : 0;
            if (y == 0) {
                h.K = make_float4(rec->K[0], rec->K[1], rec->K[2], rec->K[3]);
                h.stream = -1; h.pad_ = 0;                /* foreign: no stream of this tracker made it */
                h.frame = rec->origin_frame;
            }
        }
    } else if (P.desc && P.mark && e.slot < P.n_slots) {
        /* the slot's descriptor row: the blob's D bytes and the padding of 128, or no descriptor at all */
        const bool take = e.has_desc && P.D > 0 && P.D <= P.stride;
        if (take) {
            unsigned *row = reinterpret_cast<unsigned *>(P.desc + (size_t)e.slot * P.stride);
            const unsigned *src = pay + (size_t)(dvo_blob::levels_bytes(e.N, A.n_levels) / 4);
            const size_t have = (size_t)(dvo_blob::pad16((uint64_t)P.D) / 4);
            for (size_t i = first; i < (size_t)(P.stride >> 2); i += step)
                row[i] = i < have ? desc_word(src, (int)i, P.D, 128u) : 0x80808080u;
        }
        if (blockIdx.z == 0 && threadIdx.x == 0) P.mark[e.slot] = take ? 1 : 0;
    }
}

hipError_t launch_archive_export(const BlobEntry *entries, int count, const ArchiveView &A, const PlaceView &P, unsigned char *blob, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(archive_export_kernel, dim3(count, A.n_levels + 1, EXPORT_Z), dim3(BLOB_BLOCK), 0, s, entries, A, P, blob);
    return hipGetLastError();
}

hipError_t launch_archive_blob_sums(const BlobEntry *entries, int count, const unsigned char *blob, unsigned long long *sums, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(archive_blob_sum_kernel, dim3(count, SUM_Z), dim3(BLOB_BLOCK), 0, s, entries, blob, sums);
    return hipGetLastError();
}

hipError_t launch_archive_import(const BlobEntry *entries, int count, const unsigned char *blob, const ArchiveView &A, const PlaceView &P,
                                 hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(archive_import_kernel, dim3(count, A.n_levels + 1, IMPORT_Z), dim3(BLOB_BLOCK), 0, s, entries, blob, A, P);
    return hipGetLastError();
}

}  // namespace dvo
