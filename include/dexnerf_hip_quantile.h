/*
 * dexnerf_hip_quantile.h - opacity-quantile (median) depth maps beside the expected depth and the Dex depths, as entry points of
 * libdexnerf_hip.so beside dexnerf_hip.h, dexnerf_hip_ext.h, dexnerf_hip_anneal.h, dexnerf_hip_exposure.h and dexnerf_hip_normals.h,
 * whose tables and DN_ABI_VERSION stay as they are.  Same conventions: device pointers, contiguous fp32, caller-owned buffers, work
 * enqueued on `stream`, 0 / DN_E_* / -(hipError_t), dn_last_error; every argument is judged before any GPU work; plain vector stores;
 * no host read: every launch can be captured into a HIP graph.
 *
 * Definitions.  For one ray with samples s = 0 .. S-1, depths z_s and compositing weights w_s:
 *   w_s       the fp32 values dn_composite_density / dn_volume_render form (sample terms, fp64 transmittance scan, alpha * trans);
 *             density noise enters exactly as in dn_composite_density
 *   C_s       the inclusive prefix sum of the fp32 w_j, j <= s, accumulated in fp64 (a wave scan per 64-sample chunk plus a carry
 *             between chunks); C_{-1} = 0
 *   i(q)      the crossing index: the smallest s with C_s >= (double)q, or -1 if there is none (acc < q).  Exact in q, monotone in q.
 *   q         0 < q < 1 strictly.  The quantiles live in DEVICE memory, so the C layer cannot read them: the caller validates them
 *             (the Python binding does, on the host, before any GPU work).  At most DN_MAX_QUANTILES per call; the number of Dex
 *             thresholds stays unlimited.
 * Two modes, chosen per call by `interp`:
 *   interp = 0 (sample)   qdepth[k, ray] = z_i, the convention of the Dex depth
 *   interp = 1 (linear)   z_i + (z_{i+1} - z_i) * (q - C_{i-1}) / w_i - the piecewise-linear CDF inversion of the fine-depth sampler -
 *                         formed in fp64 from the fp32 inputs and rounded to fp32 once; for i = S-1 (the 1e10 interval) the value is
 *                         z_{S-1}
 *   no crossing (i = -1)  both modes give z_{S-1}: the ray went through.  This differs ON PURPOSE from the Dex depth's fallback to
 *                         z[0], which restates the reference's argmax of an all-false row.
 * Layout: qdepth (Q, N), like dex (K, N).
 */
#ifndef DEXNERF_HIP_QUANTILE_H
#define DEXNERF_HIP_QUANTILE_H

#include "dexnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DN_MAX_QUANTILES 64

/* ---- dn_composite_density that also reads out the opacity-quantile depths ---------------------------------------------------------------
 * rf (N,S,4) raw rows (.w read), z (N,S), rd rows of rd_stride floats, noise (N,S) or NULL, d_m_thres: n_thres >= 0 thresholds in
 * DEVICE memory - all as in dn_composite_density - and d_quantiles: 0 <= n_quant <= DN_MAX_QUANTILES quantiles in DEVICE memory.
 * depth (N), acc (N), dex (K,N) carry dn_composite_density's bits for the same inputs; qdepth (Q,N).  depth and acc may be NULL; dex
 * is required with n_thres > 0, qdepth with n_quant > 0.  One wave per ray; the grid is a function of (N, S) alone. */
int dn_composite_density_quantiles(const float* rf, const float* z, const float* rd, int rd_stride, const float* noise, float noise_std,
                                   const float* d_m_thres, int n_thres, const float* d_quantiles, int n_quant, int interp,
                                   int64_t n_rays, int n_samples, float* depth, float* acc, float* dex, float* qdepth,
                                   dn_stream_t stream);

/* ---- dn_render_rays_depth whose last pass also reads out the quantile depths ------------------------------------------------------------
 * dn_render_rays_depth's arguments, launches, workspace (dn_render_depth_workspace_bytes) and status words; the last pass (the fine
 * one, or the coarse one with num_fine == 0) is composited by dn_composite_density_quantiles' kernel when n_quant > 0.  Refuses what
 * dn_render_rays_depth refuses, and n_quant outside 0 .. DN_MAX_QUANTILES, quantiles without d_quantiles / qdepth, interp outside
 * {0, 1}. */
int dn_render_rays_depth_quantiles(const dn_mlp_desc* desc_coarse_density, const void* packed_coarse,
                                   const dn_mlp_desc* desc_fine_density, const void* packed_fine, int precision, const float* rays,
                                   int ray_stride, int64_t n_rays, int num_coarse, int num_fine, int lindisp, float noise_std,
                                   const float* d_m_thres, int n_thres, const float* t_rand, const float* noise_c, const float* u,
                                   const float* noise_f, float* depth_c, float* acc_c, float* depth_f, float* acc_f, float* dex_f,
                                   const float* d_quantiles, int n_quant, int interp, float* qdepth, void* workspace,
                                   dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_QUANTILE_H */
