/*
 * dexnerf_hip_mesh.h - the Dex threshold surface {x : sigma(x) > m_thres} of a sampled density field as an indexed triangle mesh, as
 * entry points of libdexnerf_hip.so beside dexnerf_hip.h, dexnerf_hip_ext.h, dexnerf_hip_anneal.h, dexnerf_hip_exposure.h,
 * dexnerf_hip_normals.h and dexnerf_hip_quantile.h, whose tables and DN_ABI_VERSION stay as they are.  Same conventions: device
 * pointers, caller-owned buffers, work enqueued on `stream`, 0 / DN_E_* / -(hipError_t), dn_last_error; every argument is judged
 * before any GPU work; the library never allocates; plain vector stores, no atomics; no host read: every launch can be captured
 * into a HIP graph.
 *
 * Definition.
 *
 * Grid.  Three strictly increasing fp32 coordinate arrays in device memory, xs[nx], ys[ny], zs[nz], each of length >= 2 (strict
 * monotonicity is the caller's to check: the arrays live in device memory; the Python binding checks on the host).  Grid vertex
 * (i,j,k) sits at (xs[i], ys[j], zs[k]); its linear index is (i*ny + j)*nz + k, z fastest.  The field is f[i,j,k] in fp32, read as
 * field[linear * field_stride]: stride 1 is a dense field, stride 4 on a pointer advanced by 3 floats reads the .w column of the
 * network's (P,4) rows.
 *
 * Inside.  Vertex v is inside iff f[v] is finite and f[v] > level: a strict fp32 comparison, the Dex comparison.  This is exact
 * integer work: no tolerance enters the topology.  A non-finite sample makes every tetrahedron that touches it emit nothing, an
 * edge with a non-finite end carries no vertex, and the number of non-finite samples is reported in the counts record.  `level` is
 * passed by value: the caller validates that it is finite.
 *
 * Cells.  Each cell (i,j,k) is cut into the six Kuhn tetrahedra, one per permutation p of the axes in lexicographic order: xyz,
 * xzy, yxz, yzx, zxy, zyx, with corners c0 = (0,0,0), c1 = c0 + e_p1, c2 = c1 + e_p2, c3 = (1,1,1).  Translated copies agree on
 * every shared face, so the surface is watertight without a case table of the cube (marching tetrahedra).
 *
 * Vertices lie on the edges of that triangulation.  Grid vertex (i,j,k) owns the seven edges to (i+dx, j+dy, k+dz), (dx,dy,dz) in
 * {0,1}^3 without 0, slot = 4dx + 2dy + dz - 1: three axis edges, three face diagonals, the body diagonal.  An edge carries a mesh
 * vertex iff both ends are finite and exactly one is inside.  Its position is a + (b - a) * t with t = (level - f_a) / (f_b - f_a),
 * a the owner, b the far end, f_a and f_b the field there: formed in fp64 from the fp32 inputs, per coordinate, multiply then add
 * (no FMA), and rounded to fp32 once.  Vertices are numbered ascending by (owner linear index, slot).
 *
 * Triangles, per tetrahedron, with v(c, d) the vertex on the edge between corners c and d:
 *   one corner inside, a, the outside ones o1 < o2 < o3 in corner number    (v(a,o1), v(a,o2), v(a,o3))
 *   three inside a1 < a2 < a3, one outside o                                (v(a1,o), v(a2,o), v(a3,o))
 *   two inside a < b, two outside o < p                                     the quad q0 = v(a,o), q1 = v(a,p), q2 = v(b,p), q3 = v(b,o),
 *                                                                           split as (q0,q1,q2), (q0,q2,q3)
 * and then the last two indices are swapped where needed so that (v1 - v0) x (v2 - v0) points from the inside corners to the
 * outside ones: toward decreasing density, the direction of -grad sigma that the normal render composites.  For increasing
 * coordinates the swap depends on the tetrahedron and the case alone.  Triangles are ordered ascending by (cell linear index,
 * tetrahedron 0..5, triangle 0..1), cell linear index (i*(ny-1) + j)*(nz-1) + k.
 *
 * Determinism.  The output is a function of the field: the same bits on every run, in this order (count, exclusive scan, emit; the
 * scan is the multi-launch kind: block totals, scan of the totals, add - no workgroup waits on another).
 *
 * Limits.  The scan has three levels of DN_ISO_SCAN_BLOCK elements per workgroup; together with int32 indices the entry points
 * accept nx*ny*nz <= DN_ISO_MAX_GRID_VERTICES (2^28: 512^3 is 2^27) and 12 * (nx-1)*(ny-1)*(nz-1) < 2^31, and refuse anything larger
 * (DN_E_INVAL) before any launch.
 */
#ifndef DEXNERF_HIP_MESH_H
#define DEXNERF_HIP_MESH_H

#include "dexnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DN_ISO_SCAN_BLOCK 1024
#define DN_ISO_MAX_GRID_VERTICES 268435456

/* Bytes of the workspace of the two calls below for this grid (256-byte aligned, caller-owned); 0 for a grid they refuse. */
size_t dn_isosurface_workspace_bytes(int nx, int ny, int nz);

/* ---- classify and scan --------------------------------------------------------------------------------------------------------------
 * Classifies every grid vertex and cell, scans the per-vertex edge counts and the per-cell triangle counts into `workspace`, and
 * writes d_counts, a device record of four uint32: {n_vertices, n_triangles, n_nonfinite, reserved (0)} - always the true totals. */
int dn_isosurface_count(const float* field, int field_stride, const float* xs, const float* ys, const float* zs, int nx, int ny, int nz,
                        float level, void* workspace, unsigned* d_counts, dn_stream_t stream);

/* ---- emit ---------------------------------------------------------------------------------------------------------------------------
 * Runs on the workspace dn_isosurface_count filled for the same field, grid and level, on the same stream.  vertices (V,3) fp32,
 * triangles (T,3) int32; rows at or past max_vertices / max_triangles are not written (the counts record carries the true totals, so
 * a caller with generous capacities needs no host read).  A capacity of 0 leaves its output alone (the pointer may be NULL). */
int dn_isosurface_emit(const float* field, int field_stride, const float* xs, const float* ys, const float* zs, int nx, int ny, int nz,
                       float level, const void* workspace, int64_t max_vertices, int64_t max_triangles, float* vertices, int* triangles,
                       dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_MESH_H */
