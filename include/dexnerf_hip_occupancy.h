/*
 * dexnerf_hip_occupancy.h - an occupancy bit grid of the density field and the compaction of ray samples against it, for a depth-only
 * render that evaluates the network only where the scene is not empty.  Entry points of libdexnerf_hip.so beside dexnerf_hip.h,
 * dexnerf_hip_ext.h, dexnerf_hip_anneal.h, dexnerf_hip_exposure.h, dexnerf_hip_normals.h, dexnerf_hip_quantile.h and
 * dexnerf_hip_mesh.h, whose tables and DN_ABI_VERSION stay as they are.  Same conventions: device pointers, caller-owned buffers, work
 * enqueued on `stream`, 0 / DN_E_* / -(hipError_t), dn_last_error; every argument is judged before any GPU work; the library never
 * allocates; plain vector stores, no atomics; the same bits on every run.
 *
 * No entry point here reads device memory on the host.  The culled render built from them does: the number of kept samples sizes
 * the network launch, so the caller reads the record between dn_occupancy_compact_count and dn_occupancy_compact_emit - one host
 * read per network pass, two per ray chunk of a coarse + fine render.  That chain cannot be captured into a HIP graph.
 *
 * Definition.
 *
 * Grid.  Bounds (x0,y0,z0,x1,y1,z1), finite, x1 > x0, y1 > y0, z1 > z0.  Cells (cx,cy,cz), each in 1 .. DN_OCC_MAX_AXIS_CELLS, their
 * product at most DN_OCC_MAX_CELLS.  Cell (i,j,k) has the linear index c = (i*cy + j)*cz + k, z fastest, and is bit c & 31 of uint32
 * word c >> 5: dn_occupancy_words(cx,cy,cz) = ceil(cx*cy*cz / 32) words.  The grid lives in the network's input space.
 *
 * Build.  The vertex field f is (cx+1, cy+1, cz+1) fp32, vertex (i,j,k) read as field[((i*(cy+1) + j)*(cz+1) + k) * field_stride]
 * (stride 1: a dense field; stride 4 on a pointer advanced by 3 floats: the .w column of the network's (P,4) rows).  A vertex is hot
 * iff its value is not finite, or is finite and > level: a strict fp32 comparison, the Dex comparison; a non-finite value counts as
 * occupied, so that the grid errs on the side of evaluating.  The raw bit of a cell is 1 iff one of its 8 corners is hot.  The
 * stored bit of cell (i,j,k) is the OR of the raw bits of the cells (i+di, j+dj, k+dk), |di|,|dj|,|dk| <= dilate, that lie in the
 * grid.  With `accumulate` the result is OR-ed into the word already there (a second network into the same grid), else it replaces
 * it; the computed bits past the last cell in the last word are 0.  `level` is passed by value: the caller checks that it is finite.
 *
 * Classification of a ray sample.  Rays are rows of ray_stride >= 8 floats (origin 0..2, direction 3..5); sample p = r*n_samples + s
 * of P = n_rays*n_samples has the depth z[p] and, per axis a, the point x_a = ro_a + rd_a * z: fp32, multiply, then add (no FMA) -
 * the bits the fused network kernels form from the same rays and depths.  t_a = (x_a - b0_a) * s_a in fp32, subtract then multiply,
 * with s_a = cells_a / (b1_a - b0_a) formed in float64 by the caller, rounded to fp32 once and passed by value (finite, > 0).  The
 * sample is kept iff on all three axes t_a >= 0 and t_a < (float)cells_a, as fp32 comparisons - a NaN fails them: culled -, and the
 * bit of cell ((int)t_x, (int)t_y, (int)t_z) is set.  (float)cells_a is exact: DN_OCC_MAX_AXIS_CELLS is 2^24.
 *
 * Compaction.  slot[p] = the number of kept samples q < p if p is kept, else -1: the kept samples in ascending p.  The exclusive scan
 * is the multi-launch kind of dexnerf_hip_mesh.h (block totals, scan of the totals, add; three levels of 1024), so
 * P <= DN_OCC_MAX_SAMPLES.  Row slot[p] of pts (n_kept,3) is the point x of p.
 *
 * Gather.  rf[p][3] = net_out[slot[p]][3] if 0 <= slot[p] < n_rows, else DN_OCC_FILL = -FLT_MAX, the most negative finite fp32: its
 * ReLU is 0, it exceeds no threshold, it is finite (the non-finite counters of the compositing passes stay silent), and noise of any
 * finite size added to it stays negative.  Columns 0..2 of rf are not written.
 */
#ifndef DEXNERF_HIP_OCCUPANCY_H
#define DEXNERF_HIP_OCCUPANCY_H

#include "dexnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DN_OCC_MAX_AXIS_CELLS 16777216
#define DN_OCC_MAX_CELLS 1073741824
#define DN_OCC_MAX_DILATE 8
#define DN_OCC_MAX_SAMPLES 1073741824
#define DN_OCC_MAX_SAMPLES_PER_RAY 2048
#define DN_OCC_FILL (-3.402823466e+38f)

/* uint32 words of the bit grid; 0 for cells the entry points refuse. */
int64_t dn_occupancy_words(int cx, int cy, int cz);

/* ---- build --------------------------------------------------------------------------------------------------------------------------
 * bits: dn_occupancy_words words.  scratch: as many words of the caller's for the raw bits, 4-byte aligned; needed for dilate > 0
 * (NULL otherwise is fine).  dilate in 0 .. DN_OCC_MAX_DILATE.  Each thread owns whole words. */
int dn_occupancy_build(const float* field, int field_stride, int cx, int cy, int cz, float level, int dilate, int accumulate,
                       unsigned* scratch, unsigned* bits, dn_stream_t stream);

/* Bytes of the workspace of dn_occupancy_compact_count (and of a counting dn_occupancy_gather) for P = n_rays * n_samples samples
 * (256-byte aligned, caller-owned); 0 for sizes they refuse: n_rays < 1, n_samples outside 1 .. DN_OCC_MAX_SAMPLES_PER_RAY,
 * P > DN_OCC_MAX_SAMPLES. */
size_t dn_occupancy_compact_workspace_bytes(int64_t n_rays, int n_samples);

/* ---- classify and scan --------------------------------------------------------------------------------------------------------------
 * Writes slot[P] (int32) and d_record, a device record of four uint32: {n_kept, P, 0, 0}.  The bounds and the three scales travel
 * by value. */
int dn_occupancy_compact_count(const float* rays, int ray_stride, const float* z, int64_t n_rays, int n_samples, const unsigned* bits,
                               int cx, int cy, int cz, float x0, float y0, float z0, float x1, float y1, float z1, float sx, float sy,
                               float sz, void* workspace, int* slot, unsigned* d_record, dn_stream_t stream);

/* ---- emit ---------------------------------------------------------------------------------------------------------------------------
 * Runs on the slots dn_occupancy_compact_count wrote for the same rays and depths, on the same stream.  pts (max_points,3) fp32; rows
 * at or past max_points are not written (the record carries the true count).  max_points == 0 launches nothing (pts may be NULL). */
int dn_occupancy_compact_emit(const float* rays, int ray_stride, const float* z, int64_t n_rays, int n_samples, const int* slot,
                              int64_t max_points, float* pts, dn_stream_t stream);

/* ---- gather -------------------------------------------------------------------------------------------------------------------------
 * The sigma column of rf (n_points,4) from net_out (n_rows,4) by the slots; n_rows == 0: every sample gets DN_OCC_FILL (net_out may
 * be NULL).  d_record and workspace both given: word 2 of the record becomes the number of gathered values that are not finite
 * (a second small launch sums the workgroups' counts in a fixed order); both NULL: no count. */
int dn_occupancy_gather(const int* slot, const float* net_out, int64_t n_rows, int64_t n_points, float* rf, void* workspace,
                        unsigned* d_record, dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_OCCUPANCY_H */
