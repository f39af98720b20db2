/*
 * dvo_tracker_info.h -- the per-point walk shared by the tracker's accumulating kernels: the pose information of a step
 * (dvo_tracker_info.hip) and the scoring of archived key frames (dvo_tracker_archive.hip).  One 512-thread workgroup walks ONE compact
 * reference list against ONE now level at one float pose and leaves the engine's 32 accumulators (dvo_kernel_common.h) in every lane's
 * Acc; the caller reduces them with block_reduce (lanes, then the waves in wave order), so a result depends on that list, that now
 * level and that pose alone.  The per-point arithmetic is the scalar code of dvo_device_math.h (project_point, jacobian_row) and
 * acc_add<true>, hence the oracle's floats.
 *
 * The alignment kernels' sources stay as they are (the committed traffic profiles carry their hash, bench.py): the three helpers of
 * dvo_fused.hip this walk needs -- U3, the byte offset of a rank word, p4_texel -- are restated below in plain form.
 *
 * Internal; compile with -ffp-contract=off.
 */
#ifndef DVO_TRACKER_INFO_H_
#define DVO_TRACKER_INFO_H_

#include "dvo_kernel_common.h"
#include "dvo_palette.h"

namespace dvo {
namespace {

/* restated from dvo_fused.hip: three consecutive dwords at any 4-byte boundary (one global_load_dwordx3) */
struct __attribute__((packed, aligned(4))) InfoU3 { unsigned a, b, c; };

/* the plain form of p4_line_offset (dvo_palette.h) + 128, as dvo_fused.hip once had it: byte offset of the rank word ABOVE pixel (yy, xx) in the compact image; the 12 bytes
 * from there are above / centre / below.  yy / 6 by multiplication (exact for yy < 98 000) */
DVO_DEV unsigned info_p4_byte_offset(int yy, int xx, unsigned p4_col_bytes /* p4_tiles_per_col * 128 */) {
    static_assert(DVO_P4_ROWS == 6, "written for 6 interior rows per line");
    const unsigned ty = __umul24((unsigned)yy, 43691u) >> 18;
    return __umul24((unsigned)(xx >> 2), p4_col_bytes) + 128u /* the sentinel line */ + (((unsigned)xx & 3u) << 5) + ((unsigned)yy << 2) + __umul24(ty, 104u);
}

/* restated from dvo_fused.hip (p4_texel): {DT, gx, gy, w} from the three rank words of a pixel and the palette.  The words of the
 * sentinel line (offset 0) point at palette entry n = {0, 0}: exact zeros */
DVO_DEV float4 info_p4_texel(const InfoU3 &w, const float2 *pal_lds) {
    const int c = (int)((w.b >> 3) & 0x1fffu);
    const int cr = c + __builtin_amdgcn_sbfe((int)w.b, 16, 8), cl = c + (((int)w.b) >> 24);
    const float2 pc = pal_lds[c];
    const float pr = pal_lds[cr].x, pl = pal_lds[cl].x, pu = pal_lds[(w.a >> 3) & 0x1fffu].x, pd = pal_lds[(w.c >> 3) & 0x1fffu].x;
    return make_float4(pc.x, (pr - pl) * 0.5f, (pd - pu) * 0.5f, pc.y);      /* imageGradient, SolveDVO.cpp:1063-1098 */
}

constexpr int INFO_BLOCK = 512;
constexpr int INFO_U = 4;          /* points per lane in flight: their look-ups are issued before any Jacobian arithmetic */

struct InfoPoint {
    float xn, yn, zn;
    bool vis;
};

/* points [base, base + INFO_U * INFO_BLOCK) of the list: project (the trip count is the workgroup's, so the visible count can be
 * taken from ballots); returns the look-up position of each (pixel 0, 0 and vis = false where there is nothing to look up) */
DVO_DEV void info_project(const IterConst &c, const uint2 *__restrict__ pts, int base, int N, InfoPoint (&b)[INFO_U], int (&px)[INFO_U],
                          int (&py)[INFO_U], Acc &a) {
#pragma unroll
    for (int u = 0; u < INFO_U; u++) {
        const int i = base + u * INFO_BLOCK + (int)threadIdx.x;
        const bool valid = i < N;
        const uint2 v = pts[valid ? i : (N - 1)];
        float X, Y, Z, uu, vv;
        expand_compact(c, v.x, __uint_as_float(v.y), X, Y, Z);
        const bool vis = project_point(c, X, Y, Z, b[u].xn, b[u].yn, b[u].zn, uu, vv) && valid;
        b[u].vis = vis;
        px[u] = vis ? (int)uu : 0;                  /* :376-377 == floor for u, v >= 0 */
        py[u] = vis ? (int)vv : 0;
        if (!vis) { b[u].xn = 0.0f; b[u].yn = 0.0f; b[u].zn = 1.0f; }      /* finite dummy: exact zeros in every sum */
        a.nvis += __popcll(__ballot(vis));
    }
}

DVO_DEV void info_add(const IterConst &c, const InfoPoint &b, const float4 &t, Acc &a) {
    float J[6];
    jacobian_row(c, b.xn, b.yn, b.zn, b.vis ? t.y : 0.0f, b.vis ? t.z : 0.0f, J);
    acc_add<true>(a, J, b.vis ? t.x : 0.0f, b.vis ? t.w : 0.0f);
}

/* the float pose every evaluation runs at: 12 doubles {R column-major, t} narrowed (cR.cast<float>(), SolveDVO.cpp:673-674) */
DVO_DEV void info_set_pose(IterConst &c, const double *__restrict__ P) {
    c.r[0] = uniform_f((float)P[0]); c.r[1] = uniform_f((float)P[1]); c.r[2] = uniform_f((float)P[2]);      /* cR.cast<float>() :673 */
    c.r[3] = uniform_f((float)P[3]); c.r[4] = uniform_f((float)P[4]); c.r[5] = uniform_f((float)P[5]);
    c.r[6] = uniform_f((float)P[6]); c.r[7] = uniform_f((float)P[7]); c.r[8] = uniform_f((float)P[8]);
    c.t[0] = uniform_f((float)P[9]); c.t[1] = uniform_f((float)P[10]); c.t[2] = uniform_f((float)P[11]);    /* :674 */
}

/* the whole walk: the N points of `pts` against the now level of pair p in slab L, at the pose and level constants in c.  The now
 * level is read in its compact form where it is complete (palette staged in pal_lds: DVO_PAL_MAX entries of dynamic LDS); a partial
 * form's or a refused image's real form is its 16-byte texels (dvo_palette.h), and so is that of a level the context keeps as texels */
DVO_DEV void info_accumulate(const IterConst &c, const uint2 *__restrict__ pts, int N, const LevelSlab &L, int p, int use_p4,
                             float2 *pal_lds, Acc &a) {
    const int pal_n_raw = (use_p4 && L.pal_n) ? __builtin_amdgcn_readfirstlane(L.pal_n[p]) : 0;
    const int n_pal = pal_count(pal_n_raw);
    const bool p4 = n_pal > 0 && !pal_partial(pal_n_raw);
    if (p4) {
        const float2 *__restrict__ pg = L.pal + (size_t)p * DVO_PAL_MAX;
        for (int k = threadIdx.x; k <= n_pal; k += INFO_BLOCK) pal_lds[k] = pg[k];      /* + the sentinel entry {0, 0} */
        __syncthreads();
        const char *__restrict__ img = reinterpret_cast<const char *>(L.p4 + (size_t)p * L.p4_stride);
        const unsigned col_bytes = (unsigned)p4_tiles_per_col(L.rows) * 128u;
        for (int base = 0; base < N; base += INFO_U * INFO_BLOCK) {
            InfoPoint b[INFO_U];
            int px[INFO_U], py[INFO_U];
            InfoU3 w[INFO_U];
            info_project(c, pts, base, N, b, px, py, a);
#pragma unroll
            for (int u = 0; u < INFO_U; u++)       /* a lane without a visible point reads the sentinel line */
                w[u] = *reinterpret_cast<const InfoU3 *>(img + (b[u].vis ? info_p4_byte_offset(py[u], px[u], col_bytes) : 0u));
#pragma unroll
            for (int u = 0; u < INFO_U; u++) info_add(c, b[u], info_p4_texel(w[u], pal_lds), a);
        }
    } else {
        const float4 *__restrict__ tex = L.tex + (size_t)p * L.tex_stride;
        for (int base = 0; base < N; base += INFO_U * INFO_BLOCK) {
            InfoPoint b[INFO_U];
            int px[INFO_U], py[INFO_U];
            float4 t[INFO_U];
            info_project(c, pts, base, N, b, px, py, a);
#pragma unroll
            for (int u = 0; u < INFO_U; u++) t[u] = tex[texel_index(py[u], px[u], c.tiles_per_col)];
#pragma unroll
            for (int u = 0; u < INFO_U; u++) info_add(c, b[u], t[u], a);
        }
    }
}

}  // namespace
}  // namespace dvo
#endif
