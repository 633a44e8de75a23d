/*
 * dexnerf_hip_layers.h - Dex depth layers: EVERY entry into and exit from the region {sigma > m} along a ray, not the first entry
 * alone - the back face and the wall thickness of a glass, the second wall of a hollow object, the thin floater in front of the
 * surface.  Entry points of libdexnerf_hip.so beside dexnerf_hip.h and the other headers, whose tables and DN_ABI_VERSION stay as
 * they are.  Same conventions as dexnerf_hip_refine.h, whose record and bisection step are reused: device pointers, contiguous fp32
 * (count: int32), caller-owned buffers, work enqueued on `stream`, 0 / DN_E_* / -(hipError_t), dn_last_error; every argument is judged
 * before any GPU work; plain vector stores, no atomics (but the non-finite count of the render's status block); no host read: every
 * launch can be captured into a HIP graph; the same bits on every run.
 *
 * Definitions.  For one ray with raw densities s_j (the .w column of its rows; NO density noise: the entry points take none), depths
 * z_j, j = 0 .. S-1, and a threshold m >= 0 (in DEVICE memory: the caller validates it, as for the refine header):
 *   above      above_j = (s_j > m) in fp32: NaN is not above, +inf is; above_{-1} = false.
 *   event      an event lies at every j with above_j != above_{j-1}, in ascending j.  Events 0, 2, ... are entries, events 1, 3, ...
 *              exits (the states alternate from "not above").  The end of the ray is no event: a ray still above at S-1 has an open
 *              last layer and an odd number of events.
 *   count      (K,N) int32: the number of events of the ray, NOT capped.
 *   record     the first 2L events are stored (1 <= L <= DN_MAX_LAYERS), one record of four floats (z_lo, z_hi, s_lo, s_hi) each -
 *              the refine header's, with s_lo <= m < s_hi (or s_lo NaN) - as br (N,K,2L,4): ray-major, 16-byte rows
 *                entry at j >= 1      (z_{j-1}, z_j, s_{j-1}, s_j)
 *                entry at j == 0      (z_0, z_0, s_0, s_0)
 *                exit at j (>= 1)     (z_j, z_{j-1}, s_j, s_{j-1})   - the lo end is the sample that is not above: z_lo >= z_hi
 *                no such event        (z_0, z_0, +inf, -inf)          - the refine header's "none"
 *   midpoint   z_mid = z_lo + 0.5f * (z_hi - z_lo) in fp32 (no fused multiply-add), stored as z_mid (N,K*2L): dn_run_network's
 *              rays-mode depth array with samples_per_ray = K*2L
 *   one step   dn_dex_bisect's, unchanged: s > m moves the hi end, anything else (NaN included) the lo end, a record with
 *              z_lo == z_hi is never touched.  The rule does not ask which end is deeper, so exits need no step of their own.  On
 *              the records of this header dn_dex_bisect is called with n_thres = K*2L and the thresholds repeated: threshold k at
 *              positions k*2L .. k*2L + 2L-1.
 *   finish     events (K,2L,N) and width (K,2L,N)
 *                none                 depth +inf (the ray never gets there - also the exit of an open layer), width -1
 *                sample mode          the depth of the sample at which the state changes: z_hi of an entry, z_lo of an exit;
 *                                     width = |z_hi - z_lo|
 *                interpolated mode    z_lo == z_hi: z_lo, width 0; otherwise t = (m - s_lo) / (s_hi - s_lo) if both ends are finite,
 *                                     else 0.5; depth = z_lo + (z_hi - z_lo) * t in fp64 from the fp32 ends, rounded to fp32 once;
 *                                     width = |z_hi - z_lo|
 * Where count > 0, event 0 of the sample mode carries the Dex depth's bits, and event 0 of the interpolated mode after R steps
 * carries dn_render_rays_depth_refined's `refined` bits for the same R.
 *
 * As in the refine header, a refined event is A crossing inside its sample bracket: where the field changes state three times between
 * two samples it need not be the first of them, and a layer thinner than the sample spacing can be stepped over altogether.
 */
#ifndef DEXNERF_HIP_LAYERS_H
#define DEXNERF_HIP_LAYERS_H

#include "dexnerf_hip_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DN_MAX_LAYERS 8
#define DN_MAX_LAYER_RECORDS 2048 /* K*2L per ray: dn_run_network's samples per ray */

/* ---- dn_composite_density without noise that also enumerates the events of every threshold ------------------------------------------------
 * rf (N,S,4) raw rows (.w read, 16-byte aligned), z (N,S), rd rows of rd_stride >= 3 floats, d_m_thres: n_thres >= 1 thresholds in
 * DEVICE memory, 1 <= n_layers <= DN_MAX_LAYERS.  depth (N), acc (N), dex (K,N) carry dn_composite_density's bits for the same inputs
 * with noise NULL / noise_std 0; any of the three may be NULL.  br (N,K,2L,4), 16-byte aligned, z_mid (N,K*2L) and count (K,N) int32
 * are required.  One wave per ray and one more pass over the ray's densities per threshold; the grid is a function of N alone.
 * n_rays == 0: a valid no-op. */
int dn_composite_density_layers(const float* rf, const float* z, const float* rd, int rd_stride, const float* d_m_thres, int n_thres,
                                int n_layers, int64_t n_rays, int n_samples, float* depth, float* acc, float* dex, float* br,
                                float* z_mid, int* count, dn_stream_t stream);

/* ---- the event depths and bracket widths of the records ------------------------------------------------------------------------------------
 * br (N,K,2L,4) read, 16-byte aligned; interp 0: sample mode, 1: interpolated mode; events (K,2L,N) required; width (K,2L,N) or NULL.
 * At most 2^31 - 1 records (n_rays * n_thres * 2 n_layers). */
int dn_dex_layers_finish(const float* br, const float* d_m_thres, int n_thres, int n_layers, int interp, int64_t n_rays, float* events,
                         float* width, dn_stream_t stream);

/* ---- dn_render_rays_depth with the layers of its last pass -----------------------------------------------------------------------------------
 * The workspace holds dn_render_depth_workspace_bytes' regions up to its status block, then br (N,K,2L,4), z_mid (N,K*2L),
 * rf_mid (N,K*2L,4) and the K*2L repeated thresholds - each region rounded up to 256 bytes - then the 256-byte status block.
 * 0 for arguments the render would refuse. */
size_t dn_render_depth_layers_workspace_bytes(int64_t n_rays, int num_coarse, int num_fine, int n_thres, int n_layers);

/* dn_render_rays_depth's arguments, launches and status words, plus n_layers, refine_steps, events (K,2L,N), count (K,N) int32 and
 * width (K,2L,N) or NULL.  The last compositing launch is dn_composite_density_layers' kernel.  refine_steps == -1: sample mode - the
 * finish follows at once, no network launch.  0 .. DN_MAX_REFINE_STEPS: interpolated mode - refine_steps times the pair { the last
 * pass's density network on (rays, z_mid) with samples_per_ray = K*2L, reporting into the same fp16 range word as the last pass;
 * dn_dex_bisect's kernel on the repeated thresholds }, then the finish.  depth_*, acc_*, dex_f carry dn_render_rays_depth's bits.
 * Refuses what dn_render_rays_depth refuses, and n_thres == 0, n_layers outside 1 .. DN_MAX_LAYERS, K*2L > DN_MAX_LAYER_RECORDS,
 * N*K*2L > 2^31 - 1, refine_steps outside -1 .. DN_MAX_REFINE_STEPS, noise_std != 0 and a missing `events` or `count`. */
int dn_render_rays_depth_layers(const dn_mlp_desc* desc_coarse_density, const void* packed_coarse, const dn_mlp_desc* desc_fine_density,
                                const void* packed_fine, int precision, const float* rays, int ray_stride, int64_t n_rays,
                                int num_coarse, int num_fine, int lindisp, float noise_std, const float* d_m_thres, int n_thres,
                                const float* t_rand, const float* noise_c, const float* u, const float* noise_f, float* depth_c,
                                float* acc_c, float* depth_f, float* acc_f, float* dex_f, int n_layers, int refine_steps, float* events,
                                int* count, float* width, void* workspace, dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_LAYERS_H */
