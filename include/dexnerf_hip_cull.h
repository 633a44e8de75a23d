/*
 * dexnerf_hip_cull.h - the two pieces the occupancy compaction of dexnerf_hip_occupancy.h lacks for renders that read more than the
 * sigma column: an emit that also writes a view direction per kept point, and a gather of whole rows.  With them the full colour
 * render and the normal render run their networks only on the samples whose occupancy cell is set.  Entry points of
 * libdexnerf_hip.so beside dexnerf_hip_occupancy.h and the older headers, whose tables and DN_ABI_VERSION stay as they are.  Same
 * conventions: device pointers, caller-owned buffers, work enqueued on `stream`, 0 / DN_E_* / -(hipError_t), dn_last_error; every
 * argument is judged before any GPU work; the library never allocates; plain vector stores, no atomics; the same bits on every run;
 * no entry point reads device memory on the host.
 *
 * Both run on the slots dn_occupancy_compact_count wrote (slot[p] = the rank of sample p among the kept samples, or -1), on the same
 * stream, and take the sizes that entry point takes.
 *
 * Emit with directions.  Rays are rows of ray_stride >= 11 floats: origin 0..2, direction 3..5, near, far, view direction 8..10.
 * Row slot[p] of pts (max_points,3) is the point of sample p = r*n_samples + s, x = ro + rd * z[p] per axis in fp32, multiply, then
 * add (no FMA): the bits dn_occupancy_compact_emit writes.  Row slot[p] of dirs (max_points,3) is columns 8..10 of ray row r,
 * copied bit for bit: one direction row per kept point, what dn_run_network reads with samples_per_ray = 1.
 *
 * Gather of rows.  For c < width: dst[p*dst_stride + c] = src[slot[p]*src_stride + c] if 0 <= slot[p] < n_rows, else fill_c.  Copies
 * of bits, no arithmetic: NaN payloads and the sign of zero survive.  The other columns of a dst row are not written.  With
 * width = 1, src = net_out + 3, dst = rf + 3, both strides 4 and fill0 = DN_OCC_FILL it is dn_occupancy_gather, record included.
 */
#ifndef DEXNERF_HIP_CULL_H
#define DEXNERF_HIP_CULL_H

#include "dexnerf_hip_occupancy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DN_CULL_MAX_WIDTH 4

/* ---- emit with directions -----------------------------------------------------------------------------------------------------------
 * pts and dirs (max_points,3) fp32, written by one launch; rows at or past max_points are not written (the record of
 * dn_occupancy_compact_count carries the true count).  max_points == 0 launches nothing (pts and dirs may be NULL). */
int dn_occupancy_compact_emit_dirs(const float* rays, int ray_stride, const float* z, int64_t n_rays, int n_samples, const int* slot,
                                   int64_t max_points, float* pts, float* dirs, dn_stream_t stream);

/* ---- gather of rows -----------------------------------------------------------------------------------------------------------------
 * width in 1 .. DN_CULL_MAX_WIDTH; src_stride and dst_stride in floats, each >= width; the fills travel by value and may hold any
 * bits (fills at or past width are not read).  n_points in 1 .. DN_OCC_MAX_SAMPLES, n_rows in 0 .. n_points; n_rows == 0: every row
 * gets the fills (src may be NULL).  workspace (dn_occupancy_compact_workspace_bytes of the same samples, 256-byte aligned) and
 * d_record both given: word 2 of the record becomes the number of copied values, over all `width` columns of the kept rows, that are
 * not finite - fills are never counted; a second small launch sums the workgroups' counts in a fixed order.  Both NULL: no count.
 * Rows of 16 bytes (width 4, both strides 4, src and dst 16-byte aligned) move as one 16-byte load and store: the same bits. */
int dn_occupancy_gather_rows(const int* slot, const float* src, int src_stride, int64_t n_rows, int64_t n_points, int width, float fill0,
                             float fill1, float fill2, float fill3, float* dst, int dst_stride, void* workspace, unsigned* d_record,
                             dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_CULL_H */
