/*
 * dvo_tsdf_mesh.h -- the triangle mesh of a fused volume (include/dvo_amd.h, "the surface as a triangle mesh"): the definition, in
 * plain C++.  It follows the rules of dvo_tsdf_map.h, which it includes: no device, no context, IEEE double in the order written,
 * nothing fused (-ffp-contract=off).  dvo_mesh_host is mesh() below; the kernels (dvo_tsdf_mesh.hip) call the per-voxel and per-cell
 * functions -- mesh_corner_words, mesh_edge_mask, mesh_vertex, mesh_cell_inside, mesh_cell_triangles, mesh_cell_emit -- as they are.
 *
 * Marching tetrahedra on the Kuhn split of the voxel lattice: no case table to transcribe, no ambiguous case, consistent between
 * neighbouring cells by construction.
 * Vertices.  Voxel a = (ix, iy, iz) owns seven lattice edges, direction d = 0, 1, 2: the axes (1,0,0), (0,1,0), (0,0,1); d = 3, 4, 5:
 *   the face diagonals (1,1,0), (1,0,1), (0,1,1); d = 6: the body diagonal (1,1,1).  b = a + dir(d).  The edge carries a vertex iff b is
 *   inside the volume, both weights are >= min_weight and (qa < 0) != (qb < 0) -- the crossing rule of the surface points.  Then
 *   lambda = (double)qa / (double)(qa - qb) and the vertex is centre(a) + (lambda voxel_size) dir(d): every component whose direction
 *   component is 1 gets c + lambda voxel_size, the others stay c (centre: the direct formula origin + voxel_size i); output as three
 *   floats.  Vertices are numbered in voxel index order and, within a voxel, in the order of d: those with d < 3, in order, are byte for
 *   byte the surface points of extract() with the same min_weight.
 * Cells.  Cell a exists when ix + 1 < nx, iy + 1 < ny and iz + 1 < nz; its corners are c_k = a + (k & 1, (k >> 1) & 1, (k >> 2) & 1); it
 *   is valid iff all eight corners have w >= min_weight (the validity of a ray-cast sample).  A valid cell is split into six tetrahedra,
 *   one per permutation p of the axes (0, 1, 2) in lexicographic order: v0 = c_0, v1 = c_[1 << p0], v2 = c_[(1 << p0) | (1 << p1)],
 *   v3 = c_7.  Every edge of every tetrahedron is an owned edge of some corner voxel of the cell; E(i, j) = the vertex on the edge
 *   between v_i and v_j.
 * Triangles of one tetrahedron.  The inside corners are those with q < 0.  None or four: nothing.  One corner i that differs from the
 *   other three j < k < l: (E(i,j), E(i,k), E(i,l)).  Two inside i < j and two outside k < l: (E(i,k), E(i,l), E(j,l)) then (E(i,k),
 *   E(j,l), E(j,k)).  The second and third index of a triangle are swapped when that is needed for its normal (right-hand rule) to point
 *   from the inside corners to the outside ones; the sign is decided on the unit lattice with every vertex at its edge's midpoint -- the
 *   sign of cross(P1 - P0, P2 - P0) . (mean of the outside corners - mean of the inside corners), never zero (mesh_make_table checks) --
 *   so it is a function of (p, inside mask) alone: kMeshTable, generated below at compile time.  Positive q lies in front of a surface:
 *   the normals point to the viewer's side, like the ray caster's.  Triangles are numbered in cell index order, then p, then as listed;
 *   indices are 32-bit.
 *
 * Properties, none of them a defect.  A vertex whose surrounding cells are all invalid or outside the volume is referenced by no
 * triangle (only at the rim of the observed region).  A voxel with q == 0 exactly is "outside" with lambda = 0: its vertices coincide
 * with its centre and the triangles between them have zero area; their indices are still distinct.  No vertex is shared across a
 * sign-consistent pair: the mesh of a closed surface that lies wholly inside valid cells is a closed oriented 2-manifold.
 *
 * What an implementation may skip (host and kernels do): a voxel whose own weight is below min_weight owns no vertex and is the first
 * corner of no valid cell, whatever its neighbours say; and a corner outside the volume may be read as word 0 (never seen), which
 * fails every min_weight >= 1 exactly as "outside" does.
 *
 * A mesh of more than 2^31 - 1 vertices is refused after the counts are set and before anything is written; that needs a volume of
 * gigabytes and is not tested.
 */
#ifndef DVO_TSDF_MESH_H_
#define DVO_TSDF_MESH_H_

#include "dvo_tsdf_map.h"

#include <vector>

namespace dvo_tsdf {

constexpr int kMeshEdges = 7;                          /* owned edges of a voxel */
constexpr int kMeshCellTriangles = 12;                 /* at most, per cell: two per tetrahedron */
constexpr long long kMeshMaxVertices = 0x7FFFFFFFll;   /* indices are 32-bit */

/* direction d as corner bits (bit 0: x, bit 1: y, bit 2: z), and back */
DVO_TSDF_HD constexpr int mesh_dir_corner(int d) { return d < 3 ? 1 << d : d == 3 ? 3 : d == 4 ? 5 : d == 5 ? 6 : 7; }
DVO_TSDF_HD constexpr int mesh_corner_dir(int bits) { return bits == 1 ? 0 : bits == 2 ? 1 : bits == 4 ? 2 : bits == 3 ? 3 : bits == 5 ? 4 : bits == 6 ? 5 : 6; }
/* corner k (0 .. 3) of tetrahedron p (0 .. 5: the permutations of the axes in lexicographic order) as a corner index of the cell */
DVO_TSDF_HD constexpr int mesh_tet_corner(int p, int k) {
    const int p0 = p >> 1, lo = p0 == 0 ? 1 : 0, hi = p0 == 2 ? 1 : 2, p1 = (p & 1) ? hi : lo;
    return k == 0 ? 0 : k == 1 ? 1 << p0 : k == 2 ? (1 << p0) | (1 << p1) : 7;
}
DVO_TSDF_HD constexpr int mesh_popcount4(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }

/* ---- the table: the triangles of tetrahedron p with inside mask m (bit i: v_i has q < 0) ---- */
struct MeshCase {
    unsigned char n;                                   /* triangles: 0, 1 or 2 */
    unsigned char e[6];                                /* triangle t: e[3 t .. 3 t + 2]; an entry = owner corner of the cell | d << 3 */
};
struct MeshTable {
    MeshCase c[6][16];
    bool ok;                                           /* no orientation sign was zero */
};

/* E(i, j) of tetrahedron p: the lower corner owns the edge */
constexpr unsigned char mesh_edge_code(int p, int i, int j) {
    const int a = mesh_tet_corner(p, i < j ? i : j), b = mesh_tet_corner(p, i < j ? j : i);
    return (unsigned char)(a | (mesh_corner_dir(a ^ b) << 3));
}
/* twice the midpoint of the edge `code` on the unit lattice, axis k */
constexpr int mesh_mid2(unsigned char code, int k) {
    const int a = code & 7, b = a | mesh_dir_corner(code >> 3);
    return ((a >> k) & 1) + ((b >> k) & 1);
}
/* the sign of cross(P1 - P0, P2 - P0) . (mean outside - mean inside), scaled by positive factors into integers */
constexpr int mesh_orientation(int p, int m, unsigned char e0, unsigned char e1, unsigned char e2) {
    int u[3] = {0, 0, 0}, v[3] = {0, 0, 0}, in[3] = {0, 0, 0}, out[3] = {0, 0, 0};
    const int n_in = mesh_popcount4(m), n_out = 4 - n_in;
    for (int k = 0; k < 3; k++) {
        u[k] = mesh_mid2(e1, k) - mesh_mid2(e0, k);
        v[k] = mesh_mid2(e2, k) - mesh_mid2(e0, k);
        for (int i = 0; i < 4; i++) {
            const int bit = (mesh_tet_corner(p, i) >> k) & 1;
            if ((m >> i) & 1) in[k] += bit; else out[k] += bit;
        }
    }
    const int cr[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    int dot = 0;
    for (int k = 0; k < 3; k++) dot += cr[k] * (n_in * out[k] - n_out * in[k]);
    return dot;
}
constexpr MeshTable mesh_make_table() {
    MeshTable T = {};
    T.ok = true;
    for (int p = 0; p < 6; p++)
        for (int m = 0; m < 16; m++) {
            MeshCase &c = T.c[p][m];
            const int n_in = mesh_popcount4(m);
            if (n_in == 0 || n_in == 4) continue;
            if (n_in == 2) {
                int in[2] = {0, 0}, out[2] = {0, 0}, ni = 0, no = 0;
                for (int i = 0; i < 4; i++) { if ((m >> i) & 1) in[ni++] = i; else out[no++] = i; }
                const int i = in[0], j = in[1], k = out[0], l = out[1];
                c.n = 2;
                c.e[0] = mesh_edge_code(p, i, k); c.e[1] = mesh_edge_code(p, i, l); c.e[2] = mesh_edge_code(p, j, l);
                c.e[3] = mesh_edge_code(p, i, k); c.e[4] = mesh_edge_code(p, j, l); c.e[5] = mesh_edge_code(p, j, k);
            } else {
                int i = 0, rest[3] = {0, 0, 0}, nr = 0;
                for (int t = 0; t < 4; t++) { if ((((m >> t) & 1) == 1) == (n_in == 1)) i = t; else rest[nr++] = t; }
                c.n = 1;
                c.e[0] = mesh_edge_code(p, i, rest[0]); c.e[1] = mesh_edge_code(p, i, rest[1]); c.e[2] = mesh_edge_code(p, i, rest[2]);
            }
            for (int t = 0; t < c.n; t++) {
                const int s = mesh_orientation(p, m, c.e[3 * t], c.e[3 * t + 1], c.e[3 * t + 2]);
                if (s == 0) T.ok = false;
                if (s < 0) { const unsigned char x = c.e[3 * t + 1]; c.e[3 * t + 1] = c.e[3 * t + 2]; c.e[3 * t + 2] = x; }
            }
        }
    return T;
}
constexpr MeshTable kMeshTable = mesh_make_table();
static_assert(kMeshTable.ok, "an orientation sign of the marching-tetrahedra table is zero");

/* ---- the per-voxel and per-cell functions, shared with the device ---- */

/* the word offset from voxel a to corner k of its cell */
DVO_TSDF_HD size_t mesh_corner_step(const VolumeConst &vc, int k) {
    return (size_t)(k & 1) + (size_t)((k >> 1) & 1) * (size_t)vc.nx + (size_t)((k >> 2) & 1) * ((size_t)vc.nx * (size_t)vc.ny);
}
/* w[k] = the word of corner k of the cell of voxel a = (x, y, z); 0 (never seen) for a corner outside the volume */
DVO_TSDF_HD void mesh_corner_words(const unsigned *words, const VolumeConst &vc, int x, int y, int z, size_t a, unsigned w[8]) {
    const bool in_x = x + 1 < vc.nx, in_y = y + 1 < vc.ny, in_z = z + 1 < vc.nz;
    const size_t sy = (size_t)vc.nx, sz = (size_t)vc.nx * (size_t)vc.ny;
    w[0] = words[a];
    w[1] = in_x ? words[a + 1] : 0u;
    w[2] = in_y ? words[a + sy] : 0u;
    w[3] = in_x && in_y ? words[a + sy + 1] : 0u;
    w[4] = in_z ? words[a + sz] : 0u;
    w[5] = in_x && in_z ? words[a + sz + 1] : 0u;
    w[6] = in_y && in_z ? words[a + sz + sy] : 0u;
    w[7] = in_x && in_y && in_z ? words[a + sz + sy + 1] : 0u;
}
/* bit d: the owned edge d of the voxel carries a vertex */
DVO_TSDF_HD unsigned mesh_edge_mask(const unsigned w[8], int min_weight) {
    if (word_w(w[0]) < min_weight) return 0u;
    const bool inside = word_q(w[0]) < 0;
    unsigned mask = 0u;
    for (int d = 0; d < kMeshEdges; d++) {
        const unsigned wb = w[mesh_dir_corner(d)];
        if (word_w(wb) >= min_weight && (word_q(wb) < 0) != inside) mask |= 1u << d;
    }
    return mask;
}
/* the vertex on the owned edge d between a (word wa, centre cx, cy, cz) and b (word wb); the edge carries one */
DVO_TSDF_HD void mesh_vertex(unsigned wa, unsigned wb, int d, double cx, double cy, double cz, double voxel_size, float *xyz) {
    const int qa = word_q(wa), qb = word_q(wb), dir = mesh_dir_corner(d);
    const double lambda = (double)qa / (double)(qa - qb);
    const double move = lambda * voxel_size;
    xyz[0] = (float)((dir & 1) ? cx + move : cx);
    xyz[1] = (float)((dir & 2) ? cy + move : cy);
    xyz[2] = (float)((dir & 4) ? cz + move : cz);
}
/* the cell of the voxel: -1 when it is not valid, else bit k = corner k has q < 0 */
DVO_TSDF_HD int mesh_cell_inside(const unsigned w[8], int min_weight) {
    int inside = 0;
    for (int k = 0; k < 8; k++) {
        if (word_w(w[k]) < min_weight) return -1;
        if (word_q(w[k]) < 0) inside |= 1 << k;
    }
    return inside;
}
/* the inside mask of tetrahedron p: bit i = v_i */
DVO_TSDF_HD int mesh_tet_mask(int inside8, int p) {
    return (inside8 & 1) | (((inside8 >> mesh_tet_corner(p, 1)) & 1) << 1) | (((inside8 >> mesh_tet_corner(p, 2)) & 1) << 2) | (((inside8 >> 7) & 1) << 3);
}
/* the triangles of a valid cell: 0 .. kMeshCellTriangles */
DVO_TSDF_HD int mesh_cell_triangles(int inside8) {
    if (inside8 == 0 || inside8 == 255) return 0;
    int n = 0;
    for (int p = 0; p < 6; p++) {
        const int k = mesh_popcount4(mesh_tet_mask(inside8, p));
        n += k == 2 ? 2 : (k == 1 || k == 3) ? 1 : 0;
    }
    return n;
}
/* the triangles of a valid cell in the definition's order: emit(i0, i1, i2) per triangle, with vertex_of(corner, d) = the number of the
 * vertex on the owned edge d of corner `corner` of the cell */
template <class VertexOf, class Emit>
DVO_TSDF_HD void mesh_cell_emit(int inside8, VertexOf vertex_of, Emit emit) {
    for (int p = 0; p < 6; p++) {
        const MeshCase &c = kMeshTable.c[p][mesh_tet_mask(inside8, p)];
        for (int t = 0; t < c.n; t++) {
            const int e0 = c.e[3 * t], e1 = c.e[3 * t + 1], e2 = c.e[3 * t + 2];
            emit(vertex_of(e0 & 7, e0 >> 3), vertex_of(e1 & 7, e1 >> 3), vertex_of(e2 & 7, e2 >> 3));
        }
    }
}
/* the number of the vertex on owned edge d of a voxel whose first vertex is `first` and whose edge mask is `mask` */
DVO_TSDF_HD int mesh_vertex_number(int first, unsigned mask, int d) { return first + __builtin_popcount(mask & ((1u << d) - 1u)); }

/* ---- the entry point ---- */

/* The mesh of a volume.  *n_vertices, *n_triangles: the full counts; the first vertex_capacity vertices go to xyz (3 floats each) and
 * the first triangle_capacity triangles to tri (3 ints each); either may be NULL with capacity 0.  A triangle may name a vertex beyond
 * vertex_capacity.  False: refused, nothing written -- the arguments extract() refuses, for either buffer, with no count set; or more
 * than kMeshMaxVertices vertices, with both counts set */
/* on_vertex(o, a, b, d): vertex o < vertex_capacity, on owned edge d between voxels a and b, has just been written (the colour path,
 * dvo_tsdf_colour.h, hangs its three bytes on it) */
template <class OnVertex>
inline bool mesh_walk(const dvo_tsdf_volume *vol, const unsigned *voxels, int min_weight, float *xyz, long long vertex_capacity, int *tri,
                      long long triangle_capacity, long long *n_vertices, long long *n_triangles, OnVertex on_vertex) {
    if (!volume_ok(vol) || !voxels || min_weight < 1 || vertex_capacity < 0 || (vertex_capacity > 0 && !xyz) || triangle_capacity < 0 ||
        (triangle_capacity > 0 && !tri) || !n_vertices || !n_triangles)
        return false;
    const VolumeConst vc = volume_const(*vol);
    const size_t n = voxels_of(*vol);
    /* per voxel: the number of its first vertex, its edge mask and the triangles of its cell */
    std::vector<int> first(n);
    std::vector<unsigned char> mask(n), cell(n);
    long long nv = 0, nt = 0;
    size_t a = 0;
    for (int z = 0; z < vc.nz; z++)
        for (int y = 0; y < vc.ny; y++)
            for (int x = 0; x < vc.nx; x++, a++) {
                first[a] = (int)nv;
                mask[a] = 0; cell[a] = 0;
                if (word_w(voxels[a]) < min_weight) continue;
                unsigned w[8];
                mesh_corner_words(voxels, vc, x, y, z, a, w);
                const unsigned m = mesh_edge_mask(w, min_weight);
                const int inside8 = mesh_cell_inside(w, min_weight);
                const int t = inside8 < 0 ? 0 : mesh_cell_triangles(inside8);
                mask[a] = (unsigned char)m; cell[a] = (unsigned char)t;
                nv += __builtin_popcount(m);
                nt += t;
            }
    *n_vertices = nv;
    *n_triangles = nt;
    if (nv > kMeshMaxVertices) return false;
    long long at = 0;
    a = 0;
    for (int z = 0; z < vc.nz; z++)
        for (int y = 0; y < vc.ny; y++)
            for (int x = 0; x < vc.nx; x++, a++) {
                if (!mask[a] && !cell[a]) continue;
                unsigned w[8];
                mesh_corner_words(voxels, vc, x, y, z, a, w);
                if (mask[a] && first[a] < vertex_capacity) {
                    const double cx = centre(vc.origin[0], vc.voxel_size, x), cy = centre(vc.origin[1], vc.voxel_size, y),
                                 cz = centre(vc.origin[2], vc.voxel_size, z);
                    long long o = first[a];
                    for (int d = 0; d < kMeshEdges; d++) {
                        if (!(mask[a] & (1u << d))) continue;
                        if (o < vertex_capacity) {
                            mesh_vertex(w[0], w[mesh_dir_corner(d)], d, cx, cy, cz, vc.voxel_size, xyz + 3 * o);
                            on_vertex(o, a, a + mesh_corner_step(vc, mesh_dir_corner(d)), d);
                        }
                        o++;
                    }
                }
                if (cell[a]) {
                    if (at < triangle_capacity)
                        mesh_cell_emit(mesh_cell_inside(w, min_weight),
                                       [&](int corner, int d) {
                                           const size_t b = a + mesh_corner_step(vc, corner);
                                           return mesh_vertex_number(first[b], mask[b], d);
                                       },
                                       [&](int i0, int i1, int i2) {
                                           if (at < triangle_capacity) { tri[3 * at] = i0; tri[3 * at + 1] = i1; tri[3 * at + 2] = i2; }
                                           at++;
                                       });
                    else
                        at += cell[a];
                }
            }
    return true;
}
inline bool mesh(const dvo_tsdf_volume *vol, const unsigned *voxels, int min_weight, float *xyz, long long vertex_capacity, int *tri,
                 long long triangle_capacity, long long *n_vertices, long long *n_triangles) {
    return mesh_walk(vol, voxels, min_weight, xyz, vertex_capacity, tri, triangle_capacity, n_vertices, n_triangles,
                     [](long long, size_t, size_t, int) {});
}

}  // namespace dvo_tsdf
#endif
