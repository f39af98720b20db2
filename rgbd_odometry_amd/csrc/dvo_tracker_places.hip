/*
 * dvo_tracker_places.hip -- place descriptors of the key-frame archive and their top-k retrieval (include/dvo_amd.h:
 * dvo_tracker_set_places, dvo_tracker_archive_get_descriptor, dvo_tracker_query_places; host side dvo_capi_tracker_places.cpp).
 *
 * The descriptor of a frame is the grey image of one pyramid level as the frame store holds it (u8, column-major, D = rows * cols
 * bytes a_i), shifted to the mean 128:  S = sum a_i,  m = (2 S + D) / (2 D)  (the mean, rounded half up),  b_i = clamp(a_i - m + 128,
 * 0, 255).  A row is padded with 128 to a multiple of 16 bytes; the distance of two rows is sum |b_i - b'_i| in 32 bits, to which the
 * padding adds nothing.  All of it is integer arithmetic: a descriptor and a distance have ONE value, whatever the order of summation,
 * the grid or the tile -- the tests compare with a numpy restatement for equality.
 *
 * Four kernels, none of which touches the alignment:
 *   place_store_kernel     a step's new key frames: one workgroup per entry {frame-store slot, row}; block_descriptor() below.
 *   place_distance_kernel  the hot path.  A workgroup takes PLACE_TQ queries and PLACE_CHUNK archive slots.  It first computes the
 *                          queries' descriptors into LDS -- block_descriptor() again, from the streams' current frames in the frame
 *                          store -- then every wave walks its slots of the chunk: each lane loads 16 bytes of the slot's row ONCE and
 *                          accumulates v_sad_u8 (four bytes per lane-instruction) against the same 16 bytes of the PLACE_TQ query rows,
 *                          read from LDS by ds_read_b128 (consecutive lanes, consecutive 16-byte pieces: no bank conflicts); then an
 *                          integer wave reduction.  The exclusion rules are evaluated per (query, slot) from ArchiveHeader and the
 *                          slot's mark before the walk; a slot that no query of the tile may see is not read at all.
 *   place_select_kernel    one workgroup per query: k rounds of block-minimum over the row of the distance matrix, on the 64-bit keys
 *                          (distance << 32) | (id - id_base), each round taking the smallest key above the previous round's.  The
 *                          matrix is only read, the order (distance, id) is total, so the result does not depend on any decomposition.
 *   place_shift_kernel     dvo_tracker_place_shifts: one workgroup per candidate {archive slot, frame-store slot}.  The slot's stored row
 *                          and the query's row (block_descriptor() once more) go to LDS; then the table of (2 r + 1)^2 SADs over the
 *                          central window.  In the column-major store a shift (dy, dx) is the byte offset dx * rows + dy and a window
 *                          column is one contiguous run of rows - 2 r bytes in both rows, so a work item is {shift, window column}: the
 *                          run as dwords through v_sad_u8, each dword put together from two aligned LDS dwords by v_alignbyte_b32 (both
 *                          runs start at any byte), the run's last dword masked on both operands; the item's sum joins its shift's table
 *                          entry by an LDS atomic (integers: any order gives the same sum).  Consecutive lanes take consecutive shifts of
 *                          one column, dy fastest (table entry s = (dx + r) * (2 r + 1) + dy + r): the key's dwords are broadcast, the
 *                          query's of neighbouring lanes lie one byte apart.  The best and the runner-up are block minima over 64-bit keys
 *                          (SAD, |dy| + |dx|, dy, dx), the pattern of place_select_kernel.
 *
 * Every index is bounded by the capacities the host passes.
 */
#include "dvo_launch.h"

#include <mutex>
#include <vector>

namespace dvo {

namespace {

constexpr int PLACE_BLOCK = 256;        /* store and select */
constexpr int PLACE_DIST_BLOCK = 512;   /* 8 waves: PLACE_CHUNK / 8 slots each */
constexpr int PLACE_TQ = 8;             /* query rows per workgroup: 8 x DVO_PLACE_MAX_D = 150 KB of the 160 KB LDS at the largest descriptor */
constexpr int PLACE_CHUNK = 64;         /* archive slots per workgroup: the queries' descriptors cost 1/8 of the chunk's walk */

DVO_DEV unsigned sad4(unsigned a, unsigned b, unsigned acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }

/* bytes i4 .. i4 + 3 of the image as one dword, bytes at or beyond D as `fill` */
DVO_DEV unsigned grey_dword(const unsigned char *__restrict__ img, int i4, int D, bool aligned, unsigned fill) {
    if (aligned && i4 + 4 <= D) return *reinterpret_cast<const unsigned *>(img + i4);
    unsigned v = 0;
    for (int b = 0; b < 4; b++) v |= (i4 + b < D ? (unsigned)img[i4 + b] : fill) << (8 * b);
    return v;
}

DVO_DEV unsigned shift_byte(unsigned a, int m) {
    const int t = (int)a - m + 128;
    return (unsigned)(t < 0 ? 0 : (t > 255 ? 255 : t));
}

/* the whole workgroup (BLOCK threads): the descriptor of the D-byte image `img` -> the stride bytes at dst (global memory or LDS,
 * 4-byte aligned).  red: BLOCK / 64 + 1 words of LDS.  Ends with a barrier: dst is complete for every thread */
template <int BLOCK>
DVO_DEV void block_descriptor(const unsigned char *__restrict__ img, int D, int stride, unsigned *dst, unsigned *red) {
    const bool aligned = (reinterpret_cast<uintptr_t>(img) & 3) == 0;
    const int n_dw = stride >> 2;
    unsigned sum = 0;
    for (int i = threadIdx.x; 4 * i < D; i += BLOCK) sum = sad4(grey_dword(img, 4 * i, D, aligned, 0u), 0u, sum);
    for (int o = 32; o > 0; o >>= 1) sum += (unsigned)__shfl_xor((int)sum, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned S = 0;
        for (int w = 0; w < BLOCK / 64; w++) S += red[w];
        red[BLOCK / 64] = (2u * S + (unsigned)D) / (2u * (unsigned)D);      /* S <= 255 * DVO_PLACE_MAX_D: no overflow */
    }
    __syncthreads();
    const int m = (int)red[BLOCK / 64];
    for (int i = threadIdx.x; i < n_dw; i += BLOCK) {
        unsigned v = 0x80808080u;
        if (4 * i < D) {
            const unsigned a = grey_dword(img, 4 * i, D, aligned, 0u);
            v = 0;
            for (int b = 0; b < 4; b++) v |= (4 * i + b < D ? shift_byte((a >> (8 * b)) & 255u, m) : 128u) << (8 * b);
        }
        dst[i] = v;
    }
    __syncthreads();
}

DVO_DEV bool same_model(const float4 &a, const float4 &b) {
    return __float_as_uint(a.x) == __float_as_uint(b.x) && __float_as_uint(a.y) == __float_as_uint(b.y) &&
           __float_as_uint(a.z) == __float_as_uint(b.z) && __float_as_uint(a.w) == __float_as_uint(b.w);
}

}  // namespace

__global__ void __launch_bounds__(PLACE_BLOCK)
place_store_kernel(const PlaceEntry *__restrict__ entries, PlaceGrey G, PlaceView P) {
    __shared__ unsigned red[PLACE_BLOCK / 64 + 1];
    const PlaceEntry e = entries[blockIdx.x];
    if (e.frame_slot < 0 || e.frame_slot >= G.n_slots || e.row < 0 || e.row >= P.n_slots || (size_t)P.D > G.npx || P.D > P.stride) return;
    block_descriptor<PLACE_BLOCK>(G.grey + (size_t)e.frame_slot * G.npx, P.D, P.stride,
                                  reinterpret_cast<unsigned *>(P.desc + (size_t)e.row * P.stride), red);
    if (threadIdx.x == 0) P.mark[e.row] = 1;
}

__global__ void __launch_bounds__(PLACE_DIST_BLOCK)
place_distance_kernel(const PlaceQuery *__restrict__ queries, int n, long long min_gap, PlaceGrey G, PlaceView P,
                      const ArchiveHeader *__restrict__ hdr, unsigned *__restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];      /* PLACE_TQ rows of P.stride bytes, then the reduction's words */
    unsigned *red = reinterpret_cast<unsigned *>(lds + (size_t)PLACE_TQ * P.stride);
    const int q0 = blockIdx.x * PLACE_TQ;
    const int s0 = blockIdx.y * PLACE_CHUNK;
    const int n_dw = P.stride >> 2, n_v = P.stride >> 4;

    /* the tile's query rows; a query beyond n is a row of 128 whose distances are not written, one whose frame-store slot is out of range
     * sees no slot */
    unsigned valid = 0;
    for (int j = 0; j < PLACE_TQ; j++) {
        unsigned *row = reinterpret_cast<unsigned *>(lds + (size_t)j * P.stride);
        const int fs = q0 + j < n ? queries[q0 + j].frame_slot : -1;
        if (fs >= 0 && fs < G.n_slots && (size_t)P.D <= G.npx && P.D <= P.stride) {
            block_descriptor<PLACE_DIST_BLOCK>(G.grey + (size_t)fs * G.npx, P.D, P.stride, row, red);
            valid |= 1u << j;
        } else {
            for (int i = threadIdx.x; i < n_dw; i += PLACE_DIST_BLOCK) row[i] = 0x80808080u;
        }
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int s = s0 + wave; s < s0 + PLACE_CHUNK && s < P.n_slots; s += PLACE_DIST_BLOCK / 64) {
        /* which of the tile's queries may see slot s: wave-uniform */
        unsigned see = 0;
        if (P.mark[s]) {
            const ArchiveHeader &h = hdr[s];
            for (int j = 0; j < PLACE_TQ; j++) {
                if (!((valid >> j) & 1)) continue;
                const PlaceQuery &Q = queries[q0 + j];
                const bool own_stream_near = min_gap > 0 && h.stream == Q.stream && Q.frame - h.frame < min_gap;
                if (same_model(h.K, Q.K) && s != Q.own_slot && !own_stream_near) see |= 1u << j;
            }
        }
        see = __builtin_amdgcn_readfirstlane(see);
        unsigned acc[PLACE_TQ];
#pragma unroll
        for (int j = 0; j < PLACE_TQ; j++) acc[j] = 0;
        if (see) {
            const uint4 *__restrict__ arow = reinterpret_cast<const uint4 *>(P.desc + (size_t)s * P.stride);
            for (int i = lane; i < n_v; i += 64) {
                const uint4 a = arow[i];
#pragma unroll
                for (int j = 0; j < PLACE_TQ; j++) {
                    const uint4 b = *reinterpret_cast<const uint4 *>(lds + (size_t)j * P.stride + (size_t)i * 16);
                    acc[j] = sad4(a.x, b.x, acc[j]);
                    acc[j] = sad4(a.y, b.y, acc[j]);
                    acc[j] = sad4(a.z, b.z, acc[j]);
                    acc[j] = sad4(a.w, b.w, acc[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < PLACE_TQ; j++)
                for (int o = 32; o > 0; o >>= 1) acc[j] += (unsigned)__shfl_xor((int)acc[j], o, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < PLACE_TQ; j++)
                if (q0 + j < n) dist[(size_t)(q0 + j) * P.n_slots + s] = ((see >> j) & 1) ? acc[j] : DVO_PLACE_NONE;
        }
    }
}

__global__ void __launch_bounds__(PLACE_BLOCK)
place_select_kernel(int k, long long id_base, int n_slots, const ArchiveHeader *__restrict__ hdr, const unsigned *__restrict__ dist,
                    PlaceOut *__restrict__ out, int *__restrict__ n_found) {
    __shared__ unsigned long long red[PLACE_BLOCK / 64];
    __shared__ unsigned long long best;
    const int q = blockIdx.x;
    const unsigned *__restrict__ row = dist + (size_t)q * n_slots;
    /* rel = id - id_base in [0, n_slots): the slot's place in the order of ids */
    long long r0 = -id_base % n_slots;                     /* rel of slot 0 */
    if (r0 < 0) r0 += n_slots;
    const unsigned long long none = ~0ull;
    unsigned long long last = 0;
    bool first = true;
    int found = 0;
    for (int j = 0; j < k; j++) {
        unsigned long long mine = none;
        for (int s = threadIdx.x; s < n_slots; s += PLACE_BLOCK) {
            const unsigned d = row[s];
            if (d == DVO_PLACE_NONE) continue;
            const unsigned rel = (unsigned)((r0 + s) % n_slots);
            const unsigned long long key = ((unsigned long long)d << 32) | rel;
            if ((first || key > last) && key < mine) mine = key;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = (unsigned long long)__shfl_xor((long long)mine, o, 64);
            mine = other < mine ? other : mine;
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long b = red[0];
            for (int w = 1; w < PLACE_BLOCK / 64; w++) b = red[w] < b ? red[w] : b;
            best = b;
        }
        __syncthreads();
        const unsigned long long b = best;
        __syncthreads();                                   /* red and best are rewritten by the next round */
        if (threadIdx.x == 0) {
            PlaceOut &o = out[(size_t)q * k + j];
            if (b != none) {
                const unsigned rel = (unsigned)(b & 0xFFFFFFFFull);
                long long s = ((long long)rel - r0) % n_slots;
                if (s < 0) s += n_slots;
                o.key_id = id_base + rel;
                o.frame = hdr[s].frame;
                o.stream = hdr[s].stream;
                o.distance = (unsigned)(b >> 32);
            } else {
                o.key_id = -1; o.frame = -1; o.stream = -1; o.distance = DVO_PLACE_NONE;
            }
        }
        if (b != none) { found++; last = b; first = false; }
        else { last = none; first = false; }               /* nothing is above `none`: the remaining rounds find nothing either */
    }
    if (threadIdx.x == 0) n_found[q] = found;
}

/* ---- dvo_tracker_place_shifts ---- */
constexpr int SHIFT_PAD = 16;           /* bytes behind each LDS row: a run's last dword pair may end one dword beyond the row */

/* the dword at any byte offset of an LDS row, from the two aligned dwords that hold it */
DVO_DEV unsigned dword_at(unsigned lo, unsigned hi, int byte) { return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)(byte & 3)); }

/* the order of the search as one 64-bit key: (SAD, |dy| + |dx|, dy, dx) */
DVO_DEV unsigned long long shift_key(unsigned sad, int dy, int dx) {
    const unsigned l1 = (unsigned)((dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx));
    return ((unsigned long long)sad << 32) | (l1 << 16) | ((unsigned)(dy + DVO_PLACE_SHIFT_MAX_R) << 8) | (unsigned)(dx + DVO_PLACE_SHIFT_MAX_R);
}

/* the whole workgroup: the smallest of the threads' keys.  red: PLACE_BLOCK / 64 words; ends with red free for the next call */
DVO_DEV unsigned long long block_min_key(unsigned long long mine, unsigned long long *red) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)mine, o, 64);
        mine = other < mine ? other : mine;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
    __syncthreads();
    unsigned long long b = red[0];
    for (int w = 1; w < PLACE_BLOCK / 64; w++) b = red[w] < b ? red[w] : b;
    __syncthreads();
    return b;
}

__global__ void __launch_bounds__(PLACE_BLOCK)
place_shift_kernel(const PlaceShiftCand *__restrict__ cands, int rows, int cols, int radius, PlaceGrey G, PlaceView P,
                   PlaceShiftOut *__restrict__ out) {
    /* the key's row, the query's row (P.stride + SHIFT_PAD bytes each), the SAD table, the reductions' words */
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int pitch = P.stride + SHIFT_PAD;
    const int side = 2 * radius + 1, n_shift = side * side;
    unsigned *krow = reinterpret_cast<unsigned *>(lds);
    unsigned *qrow = reinterpret_cast<unsigned *>(lds + pitch);
    unsigned *table = reinterpret_cast<unsigned *>(lds + 2 * (size_t)pitch);
    unsigned long long *red64 = reinterpret_cast<unsigned long long *>(table + ((n_shift + 3) & ~3));
    unsigned *red = reinterpret_cast<unsigned *>(red64 + PLACE_BLOCK / 64);
    const PlaceShiftCand e = cands[blockIdx.x];
    const int h = rows - 2 * radius, w = cols - 2 * radius;
    if (e.slot < 0 || e.slot >= P.n_slots || e.frame_slot < 0 || e.frame_slot >= G.n_slots || (size_t)P.D > G.npx || P.D > P.stride ||
        (P.stride & 15) || P.stride > (DVO_PLACE_MAX_D + 15) / 16 * 16 || rows < 1 || cols < 1 || (long long)rows * cols != P.D ||
        radius < 0 || radius > DVO_PLACE_SHIFT_MAX_R || h < 1 || w < 1)
        return;

    {
        const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(P.desc + (size_t)e.slot * P.stride);
        uint4 *dst = reinterpret_cast<uint4 *>(krow);
        for (int i = threadIdx.x; i < (P.stride >> 4); i += PLACE_BLOCK) dst[i] = src[i];
    }
    if (threadIdx.x < SHIFT_PAD / 4) {
        krow[(P.stride >> 2) + threadIdx.x] = 0x80808080u;
        qrow[(P.stride >> 2) + threadIdx.x] = 0x80808080u;
    }
    for (int s = threadIdx.x; s < n_shift; s += PLACE_BLOCK) table[s] = 0;
    block_descriptor<PLACE_BLOCK>(G.grey + (size_t)e.frame_slot * G.npx, P.D, P.stride, qrow, red);      /* ends with a barrier */

    /* item = {window column, shift}: SAD of the column's run of h bytes, key at kb, query at kb + dx * rows + dy */
    const int n_dw = (h + 3) >> 2;
    const unsigned tail = (h & 3) ? (1u << (8 * (h & 3))) - 1u : 0xFFFFFFFFu;
    for (int item = threadIdx.x; item < w * n_shift; item += PLACE_BLOCK) {
        const int x = radius + item / n_shift, s = item % n_shift;
        const int dy = s % side - radius, dx = s / side - radius;
        const int kb = x * rows + radius, qb = kb + dx * rows + dy;      /* 0 <= qb, qb + h <= D */
        const unsigned *kp = krow + (kb >> 2), *qp = qrow + (qb >> 2);
        unsigned klo = kp[0], qlo = qp[0], acc = 0;
        for (int j = 1; j <= n_dw; j++) {
            const unsigned khi = kp[j], qhi = qp[j];                     /* at most dword (D + 3) / 4 of the row: inside the pad */
            unsigned a = dword_at(klo, khi, kb), b = dword_at(qlo, qhi, qb);
            if (j == n_dw) { a &= tail; b &= tail; }
            acc = sad4(a, b, acc);
            klo = khi; qlo = qhi;
        }
        atomicAdd(&table[s], acc);
    }
    __syncthreads();

    unsigned long long mine = ~0ull;
    for (int s = threadIdx.x; s < n_shift; s += PLACE_BLOCK) {
        const unsigned long long key = shift_key(table[s], s % side - radius, s / side - radius);
        mine = key < mine ? key : mine;
    }
    const unsigned long long best = block_min_key(mine, red64);
    const int bdy = (int)((best >> 8) & 255u) - DVO_PLACE_SHIFT_MAX_R, bdx = (int)(best & 255u) - DVO_PLACE_SHIFT_MAX_R;
    mine = ~0ull;
    for (int s = threadIdx.x; s < n_shift; s += PLACE_BLOCK) {
        const int dy = s % side - radius, dx = s / side - radius;
        const int ay = dy - bdy < 0 ? bdy - dy : dy - bdy, ax = dx - bdx < 0 ? bdx - dx : dx - bdx;
        if (ay < 2 && ax < 2) continue;
        const unsigned long long key = shift_key(table[s], dy, dx);
        mine = key < mine ? key : mine;
    }
    const unsigned long long second = block_min_key(mine, red64);
    if (threadIdx.x == 0) {
        PlaceShiftOut &o = out[blockIdx.x];
        o.dy = bdy; o.dx = bdx;
        o.sad = (unsigned)(best >> 32);
        o.sad_zero = table[radius * side + radius];
        o.sad_second = second == ~0ull ? DVO_PLACE_NONE : (unsigned)(second >> 32);
        o.area = h * w;
    }
}

hipError_t launch_place_store(const PlaceEntry *entries, int count, const PlaceGrey &G, const PlaceView &P, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(place_store_kernel, dim3(count), dim3(PLACE_BLOCK), 0, s, entries, G, P);
    return hipGetLastError();
}

hipError_t launch_place_query(const PlaceQuery *queries, int n, int k, long long min_gap, long long id_base, const PlaceGrey &G,
                              const PlaceView &P, const ArchiveHeader *hdr, unsigned *dist, PlaceOut *out, int *n_found, hipStream_t s) {
    if (n <= 0 || k <= 0 || P.n_slots <= 0) return hipSuccess;
    const size_t dyn = (size_t)PLACE_TQ * P.stride + sizeof(unsigned) * (PLACE_DIST_BLOCK / 64 + 1);
    /* once per process and device: the attribute belongs to the kernel, not to a launch */
    static std::mutex once_mutex;
    static std::vector<char> once_done;
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(once_mutex);
        if ((size_t)dev >= once_done.size()) once_done.resize((size_t)dev + 1, 0);
        if (!once_done[dev]) {
            const size_t most = (size_t)PLACE_TQ * ((DVO_PLACE_MAX_D + 15) / 16 * 16) + sizeof(unsigned) * (PLACE_DIST_BLOCK / 64 + 1);
            e = hipFuncSetAttribute((const void *)place_distance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
            if (e != hipSuccess) return e;
            once_done[dev] = 1;
        }
    }
    hipLaunchKernelGGL(place_distance_kernel, dim3((n + PLACE_TQ - 1) / PLACE_TQ, (P.n_slots + PLACE_CHUNK - 1) / PLACE_CHUNK),
                       dim3(PLACE_DIST_BLOCK), dyn, s, queries, n, min_gap, G, P, hdr, dist);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(place_select_kernel, dim3(n), dim3(PLACE_BLOCK), 0, s, k, id_base, P.n_slots, hdr, dist, out, n_found);
    return hipGetLastError();
}

hipError_t launch_place_shifts(const PlaceShiftCand *cands, int n, int rows, int cols, int radius, const PlaceGrey &G, const PlaceView &P,
                               PlaceShiftOut *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int side = 2 * radius + 1;
    const size_t dyn = 2 * (size_t)(P.stride + SHIFT_PAD) + sizeof(unsigned) * (size_t)((side * side + 3) & ~3) +
                       sizeof(unsigned long long) * (PLACE_BLOCK / 64) + sizeof(unsigned) * (PLACE_BLOCK / 64 + 1);      /* < 40 KB */
    hipLaunchKernelGGL(place_shift_kernel, dim3(n), dim3(PLACE_BLOCK), dyn, s, cands, rows, cols, radius, G, P, out);
    return hipGetLastError();
}

}  // namespace dvo
