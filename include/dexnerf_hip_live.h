/*
 * dexnerf_hip_live.h - an occupancy grid kept live beside networks that are still training: a running maximum of the density at one
 * jittered point per cell, refreshed on the device every few steps, and the bit grid of dexnerf_hip_occupancy.h derived from it.  The
 * training step consumes the bits through dexnerf_hip_span.h's dn_occupancy_ray_spans.  Entry points of libdexnerf_hip.so beside
 * dexnerf_hip.h, dexnerf_hip_ext.h, dexnerf_hip_anneal.h, dexnerf_hip_exposure.h, dexnerf_hip_normals.h, dexnerf_hip_quantile.h,
 * dexnerf_hip_mesh.h, dexnerf_hip_occupancy.h, dexnerf_hip_cull.h, dexnerf_hip_refine.h, dexnerf_hip_span.h and dexnerf_hip_layers.h,
 * whose tables and DN_ABI_VERSION stay as they are.  Same conventions: device pointers, caller-owned buffers, work enqueued on
 * `stream`, 0 / DN_E_* / -(hipError_t), dn_last_error; every argument is judged before any GPU work; the library never allocates;
 * plain vector stores, no atomics, no workgroup waits on another; no host read: the launches can be captured into a HIP graph; the
 * same bits on every run.  Everything is fp32 and the library is compiled with -ffp-contract=off: a multiply followed by an add is
 * two roundings.
 *
 * The grid, its cells, its linear index c = (i*cy + j)*cz + k and its bit layout are those of dexnerf_hip_occupancy.h.
 *
 * The rng record.  {seed_lo, seed_hi, cur, nxt}, four uint32 on the device, as the training step's (csrc/dn_rng.h) - but the grid's
 * OWN record, not the step's: the refreshes count by themselves, and every rank of a data-parallel run that starts from the same
 * seed draws the same points.  dn_occupancy_cell_points with c0 == 0 draws from `nxt` and copies it to `cur`, as dn_select_rays_draw
 * does for the step; with c0 != 0 it draws from `cur`.  dn_occupancy_ema_update writes nxt = cur + 1.  One refresh is therefore: the
 * cell points in ascending slabs, the first one at c0 == 0; the networks; one update.
 *
 * Definition of the cell points.  Cell c = (i_x*cy + i_y)*cz + i_z gets, per axis a = 0, 1, 2,
 *   x_a = b0_a + ((float)i_a + u_a) * h_a          the sum in the brackets rounded to fp32, then a multiply, then an add: two more roundings
 * with h_a = (b1_a - b0_a) / cells_a formed in float64 by the caller, rounded to fp32 once and passed by value (finite, > 0),
 * u_a = rng_to_uniform(w[a]) = (float)(w[a] >> 8) * 2^-24 in [0, 1), and w = rng_words(seed_lo, seed_hi, iteration, kRngStreamCell, c):
 * Philox-4x32-10 on the counter (c low, c high, stream 6, iteration) under the key (seed_lo, seed_hi).  (float)i_a is exact:
 * DN_OCC_MAX_AXIS_CELLS is 2^24.  Row c - c0 of pts receives (x_0, x_1, x_2).
 *
 * Definition of the update.  One or two columns of raw density, a[c * stride_a] and b[c * stride_b] (stride 4 on a pointer advanced
 * by 3 floats: the .w column of dn_run_network's (n,4) rows, read in place); b may be NULL.  max(p,q) is q > p ? q : p.  Per cell c:
 *   hot   = a given column's value is not finite (its exponent bits are all ones);
 *   s     = the value of a, or max(a, b) with two columns;
 *   e'    = hot ? ema[c] * decay : max(ema[c] * decay, s)      ema starts at 0 and so stays >= 0; a hot cell's s does not enter it
 *   raw_c = hot || e' > level                                  a strict fp32 comparison: the Dex comparison
 * ema[c] = e' is stored.  With write_bits == 0 nothing else but the record is written: the warm-up, in which the bits stay what the
 * caller initialised them to.  With write_bits != 0 the stored bit of cell (i,j,k) is the OR of raw over the cells
 * (i+di, j+dj, k+dk), |di|,|dj|,|dk| <= dilate, that lie in the grid - dn_occupancy_build's dilation, the same code -, replacing the
 * word that was there; the bits past the last cell in the last word are 0.
 *
 * What this does not promise.  A cell point within one rounding of its cell's upper face may classify into the neighbouring cell
 * under dexnerf_hip_occupancy.h's (int)((x - b0) * s); its density is attributed to c by index regardless.  One point per cell and
 * refresh is a sample: a cell whose density exceeds the level only away from the points drawn so far is clear until a draw finds
 * it - the dilation, the decay (how long a found value lasts) and the warm-up are the margins.  The level is compared with the
 * density the networks have NOW; early in training that is not the scene.
 */
#ifndef DEXNERF_HIP_LIVE_H
#define DEXNERF_HIP_LIVE_H

#include "dexnerf_hip_occupancy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pts (n,3) fp32, 4-byte aligned: the points of the cells c0 .. c0 + n - 1; c0 >= 0, n >= 1, c0 + n <= cx*cy*cz.  The lower bounds
 * and the three cell sizes travel by value (finite, sizes > 0).  rng_state: the grid's record, read and (c0 == 0: word 2) written.
 * One thread per cell, 256-thread workgroups. */
int dn_occupancy_cell_points(int cx, int cy, int cz, float x0, float y0, float z0, float hx, float hy, float hz, int64_t c0, int64_t n,
                             unsigned* rng_state, float* pts, dn_stream_t stream);

/* Bytes of the scratch of dn_occupancy_ema_update: the raw words ahead of the dilation, 4 bytes per word of the grid (needed
 * for write_bits != 0 with dilate > 0; NULL otherwise is fine).  0 for cells outside the limits of dexnerf_hip_occupancy.h or a dilate
 * outside 0 .. DN_OCC_MAX_DILATE. */
size_t dn_occupancy_ema_workspace_bytes(int cx, int cy, int cz, int dilate);

/* sigma_a (required) and sigma_b (may be NULL): one value per cell at the given stride in floats (>= 1).  ema (cx*cy*cz) fp32 read
 * and written.  decay in (0, 1]; level finite and >= 0; dilate in 0 .. DN_OCC_MAX_DILATE.  bits: dn_occupancy_words words, required
 * with write_bits != 0; scratch: as many words of the caller's, not the grid's, required with write_bits != 0 and dilate > 0.
 * rng_state: the grid's record; word 3 is written.  One lane per cell: a wave's 64 predicates are two words. */
int dn_occupancy_ema_update(const float* sigma_a, int stride_a, const float* sigma_b, int stride_b, int cx, int cy, int cz, float decay,
                            float level, int write_bits, int dilate, float* ema, unsigned* bits, unsigned* scratch, unsigned* rng_state,
                            dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_LIVE_H */
