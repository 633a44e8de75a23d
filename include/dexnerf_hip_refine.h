/*
 * dexnerf_hip_refine.h - sub-sample Dex depths: the first threshold crossing of a ray, bracketed by the compositing pass and then
 * bisected on the density network, as entry points of libdexnerf_hip.so beside dexnerf_hip.h, dexnerf_hip_ext.h, dexnerf_hip_anneal.h,
 * dexnerf_hip_exposure.h, dexnerf_hip_normals.h, dexnerf_hip_quantile.h, dexnerf_hip_mesh.h, dexnerf_hip_occupancy.h and
 * dexnerf_hip_cull.h, whose tables and DN_ABI_VERSION stay as they are.  Same conventions: device pointers, contiguous fp32,
 * caller-owned buffers, work enqueued on `stream`, 0 / DN_E_* / -(hipError_t), dn_last_error; every argument is judged before any GPU
 * work; plain vector stores, no atomics (but the non-finite count of the render's status block); no host read: every launch can be
 * captured into a HIP graph; the same bits on every run.
 *
 * Definitions.  For one ray with raw densities s_j (the .w column of its rows; NO density noise: the entry points take none), depths
 * z_j, j = 0 .. S-1, and a threshold m >= 0 (the thresholds live in DEVICE memory, so the C layer cannot read them: the caller
 * validates them - the Python binding does, on the host, before any GPU work):
 *   i          the first index with s_i > m in fp32, or -1: exactly the index of dn_composite_density's Dex depth (for m >= 0 and no
 *              noise relu(s) > m iff s > m).  NaN never crosses, +inf does.
 *   record     four floats (z_lo, z_hi, s_lo, s_hi), stored as br (N, K, 4): ray-major, 16-byte rows
 *                proper, i >= 1          (z_{i-1}, z_i, s_{i-1}, s_i)
 *                first sample, i == 0    (z_0, z_0, s_0, s_0)
 *                no crossing             (z_0, z_0, +inf, -inf)   - no other record has s_hi == -inf: this marks "none"
 *   midpoint   z_mid = z_lo + 0.5f * (z_hi - z_lo) in fp32 (no fused multiply-add), stored as z_mid (N, K): dn_run_network's rays-mode
 *              depth array with samples_per_ray = K
 *   one step   reads s = rf_mid[ray, k, 3], the network's raw density at the midpoint.  A record with z_lo == z_hi is never changed;
 *              otherwise s > m gives (z_hi, s_hi) = (z_mid, s) and anything else, NaN included, gives (z_lo, s_lo) = (z_mid, s).  The
 *              step then writes the next z_mid.
 *   finish     no crossing:   refined = z_0 (the Dex fallback), width = -1 - the width map doubles as the hit mask the Dex depth lacks
 *              z_lo == z_hi:  refined = z_lo, width = 0
 *              otherwise:     t = (m - s_lo) / (s_hi - s_lo) if both ends are finite, else t = 0.5;
 *                             refined = z_lo + (z_hi - z_lo) * t, formed in fp64 from the fp32 inputs and rounded to fp32 once;
 *                             width = z_hi - z_lo in fp32
 * Layout: refined (K, N) and width (K, N), like dex (K, N).
 *
 * The refinement finds A crossing inside the first bracket [z_{i-1}, z_i].  Where the field crosses m three (or any odd number above
 * one) times between two samples this need not be the first crossing; where 64 samples step over a thin first crossing altogether, the
 * bracket - like the Dex depth - belongs to a later one.
 */
#ifndef DEXNERF_HIP_REFINE_H
#define DEXNERF_HIP_REFINE_H

#include "dexnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DN_MAX_REFINE_STEPS 24

/* ---- dn_composite_density without noise that also writes the bracket records and the first midpoints -----------------------------------
 * rf (N,S,4) raw rows (.w read, 16-byte aligned), z (N,S), rd rows of rd_stride >= 3 floats, d_m_thres: n_thres >= 1 thresholds in
 * DEVICE memory (any count: thresholds past 64 take one more pass each 64 over the ray's densities).  depth (N), acc (N), dex (K,N)
 * carry dn_composite_density's bits for the same inputs with noise NULL / noise_std 0; any of the three may be NULL.  br (N,K,4),
 * 16-byte aligned, and z_mid (N,K) are required.  One wave per ray; the grid is a function of N alone.  n_rays == 0: a valid no-op. */
int dn_composite_density_brackets(const float* rf, const float* z, const float* rd, int rd_stride, const float* d_m_thres, int n_thres,
                                  int64_t n_rays, int n_samples, float* depth, float* acc, float* dex, float* br, float* z_mid,
                                  dn_stream_t stream);

/* ---- one bisection step on every record ----------------------------------------------------------------------------------------------------
 * br (N,K,4) read and written, 16-byte aligned; rf_mid (N,K,4), 16-byte aligned: the density network's rows at z_mid (.w read);
 * z_mid (N,K) written: the next midpoints.  Elementwise, one record per thread. */
int dn_dex_bisect(float* br, const float* rf_mid, const float* d_m_thres, int n_thres, int64_t n_rays, float* z_mid, dn_stream_t stream);

/* ---- the refined depths and bracket widths of the records ------------------------------------------------------------------------------------
 * br (N,K,4) read; refined (K,N) required; width (K,N) or NULL. */
int dn_dex_refine_finish(const float* br, const float* d_m_thres, int n_thres, int64_t n_rays, float* refined, float* width,
                         dn_stream_t stream);

/* ---- dn_render_rays_depth with refined Dex depths ------------------------------------------------------------------------------------------
 * The workspace holds dn_render_depth_workspace_bytes' regions up to its status block, then br (N,K,4), z_mid (N,K), rf_mid (N,K,4) -
 * each region rounded up to 256 bytes - then the 256-byte status block: br starts 256 bytes before the end of a
 * dn_render_depth_workspace_bytes workspace for the same rays and sample counts.
 * 0 for arguments the render would refuse. */
size_t dn_render_depth_refined_workspace_bytes(int64_t n_rays, int num_coarse, int num_fine, int n_thres);

/* dn_render_rays_depth's arguments, launches and status words, plus refine_steps, refined (K,N) and width (K,N) or NULL.  The last
 * compositing launch is dn_composite_density_brackets' kernel; then refine_steps times the pair { the last pass's density network
 * on (rays, z_mid) with samples_per_ray = n_thres, reporting into the same fp16 range word as the last pass; dn_dex_bisect's kernel };
 * then dn_dex_refine_finish's kernel.  depth_*, acc_*, dex_f carry dn_render_rays_depth's bits.  Refuses what dn_render_rays_depth
 * refuses, and n_thres == 0, refine_steps outside 0 .. DN_MAX_REFINE_STEPS, noise_std != 0 and a missing `refined`. */
int dn_render_rays_depth_refined(const dn_mlp_desc* desc_coarse_density, const void* packed_coarse,
                                 const dn_mlp_desc* desc_fine_density, const void* packed_fine, int precision, const float* rays,
                                 int ray_stride, int64_t n_rays, int num_coarse, int num_fine, int lindisp, float noise_std,
                                 const float* d_m_thres, int n_thres, const float* t_rand, const float* noise_c, const float* u,
                                 const float* noise_f, float* depth_c, float* acc_c, float* depth_f, float* acc_f, float* dex_f,
                                 int refine_steps, float* refined, float* width, void* workspace, dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_REFINE_H */
