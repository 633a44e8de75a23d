/*
 * dexnerf_hip_span.h - the occupied span of a ray: each ray walks the occupancy bit grid once and its [near, far] is tightened to the
 * depth range in which it can meet a set cell, so that the render that follows spends its samples where the scene is.  An entry point
 * of libdexnerf_hip.so beside dexnerf_hip.h, dexnerf_hip_ext.h, dexnerf_hip_anneal.h, dexnerf_hip_exposure.h, dexnerf_hip_normals.h,
 * dexnerf_hip_quantile.h, dexnerf_hip_mesh.h, dexnerf_hip_occupancy.h, dexnerf_hip_cull.h and dexnerf_hip_refine.h, whose tables and
 * DN_ABI_VERSION stay as they are.  Same conventions: device pointers, caller-owned buffers, work enqueued on `stream`, 0 / DN_E_* /
 * -(hipError_t), dn_last_error; every argument is judged before any GPU work; the library never allocates; plain vector stores, no
 * atomics; no host read: the launch can be captured into a HIP graph; the same bits on every run.
 *
 * The grid, its bit layout, the bounds and the three fp32 scales s_a = cells_a / (b1_a - b0_a) - formed in float64 by the caller and
 * rounded once - are those of dexnerf_hip_occupancy.h's dn_occupancy_compact_count.  Rays are rows of ray_stride >= 8 floats: origin
 * 0..2, direction 3..5, near, far.
 *
 * Definition of the span of one ray.  Everything is fp32; the library is compiled with -ffp-contract=off, so a multiply followed by
 * an add is two roundings.  max(a,b) is b > a ? b : a and min(a,b) is b < a ? b : a.
 *
 * Non-finite rows.  A row with a non-finite value in columns 0..7 is a miss.
 *
 * Cell coordinates.  Per axis o_a = (ro_a - b0_a) * s_a, d_a = rd_a * s_a and c_a = (float)cells_a.
 *
 * Slab clip.  Start with t_in = near and t_out = far.  For an axis with d_a == 0, the ray is a miss unless o_a >= 0 && o_a < c_a;
 * that axis adds no constraint and its tn_a is +inf.  For any other axis:
 *   inv_a = 1.0f / d_a, a correctly rounded division;
 *   ta = (0 - o_a) * inv_a and tb = (c_a - o_a) * inv_a;
 *   (lo, hi) = ta <= tb ? (ta, tb) : (tb, ta);
 *   t_in = max(t_in, lo) and t_out = min(t_out, hi).
 * The ray is a miss unless t_in < t_out after all three axes.
 *
 * Start cell.  p_a = o_a + d_a * t_in.  i_a = (int)min(max(floorf(p_a), 0), c_a - 1).  step_a is the sign of d_a.
 * tn_a = ((float)(i_a + (d_a > 0)) - o_a) * inv_a.  (The integer is clamped to 0 .. cells_a - 1 once more after the conversion: that
 * changes nothing unless p_a is NaN - coordinates that overflowed fp32 -, which then starts in cell 0 of that axis.)
 *
 * Walk.  Start with t_cur = t_in.  Repeat:
 *   a is the axis with the smallest tn; on a tie the lowest axis wins;
 *   t_exit = min(tn_a, t_out);
 *   if the bit of cell (i_x, i_y, i_z) is set: on the first such cell lo = t_cur; on every such cell hi = t_exit and the visit count
 *   goes up by one;
 *   stop unless tn_a < t_out;
 *   i_a += step_a; stop if i_a has left 0 .. cells_a - 1;
 *   t_cur = tn_a;
 *   tn_a is recomputed from the integer by the formula above and never accumulated.
 * The loop runs at most cx + cy + cz + 1 times.
 *
 * Result.  A ray with no visit is a miss.
 *   Miss: span = (near, far), copied bit for bit; visits = 0; the row is not written.
 *   Hit:  pad = pad_cells / max(|d_x|, |d_y|, |d_z|); span = (max(near, lo - pad), min(far, hi + pad)); visits is the count; with
 *         `apply`, columns 6 and 7 of the row receive the span.
 *
 * What the span does not promise.  A ray that grazes a cell boundary within fp32 rounding can lose samples that the classification of
 * dexnerf_hip_occupancy.h would keep: pad_cells and the grid's dilation are the margins for that.  The grid is a sampled approximation
 * of the field.  A render of the tightened rows treats everything past the tightened far as what the grid says it is: empty.
 */
#ifndef DEXNERF_HIP_SPAN_H
#define DEXNERF_HIP_SPAN_H

#include "dexnerf_hip_occupancy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rays (n_rays, ray_stride) read, 4-byte aligned; bits: dn_occupancy_words words; span (n_rays,2) fp32 and visits (n_rays) int32 may
 * each be NULL, span only when apply != 0.  apply != 0 also writes columns 6 and 7 of every hit ray's row - no other column, and no
 * column of a missed row.  pad_cells finite and >= 0; cells within DN_OCC_MAX_AXIS_CELLS and DN_OCC_MAX_CELLS.  One thread per ray.
 * n_rays == 0 returns 0 after the checks. */
int dn_occupancy_ray_spans(float* rays, int ray_stride, int64_t n_rays, const unsigned* bits, int cx, int cy, int cz, float x0, float y0,
                           float z0, float x1, float y1, float z1, float sx, float sy, float sz, float pad_cells, int apply, float* span,
                           int* visits, dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_SPAN_H */
