/*
 * dexnerf_hip_normals.h - the surface-normal render: density-gradient normals composited beside the Dex depths, as entry points of
 * libdexnerf_hip.so beside dexnerf_hip.h, dexnerf_hip_ext.h, dexnerf_hip_anneal.h and dexnerf_hip_exposure.h, whose tables and
 * DN_ABI_VERSION stay as they are.  Same conventions: device pointers, contiguous fp32, caller-owned buffers, work enqueued on `stream`,
 * 0 / DN_E_* / -(hipError_t), dn_last_error; every argument is judged before any GPU work; plain vector stores, no atomics; no host
 * read: every launch can be captured into a HIP graph.
 *
 * Definitions.  For sample s of a ray, g_s = d sigma_raw / d x at the sample point: sigma_raw is the network's raw density output
 * (before noise and ReLU), x the network's INPUT space - world space, or NDC space for forward-facing scenes; nothing converts it.
 *   sample normal    n_s = -g_s / |g_s|; the norm is formed in fp64 from the three fp32 components, each component is rounded to fp32
 *                    once; n_s = (0,0,0) when |g_s| is 0 or not finite (no NaN leaves the kernel)
 *   expected normal  normal[ray] = sum_s w_s n_s with dn_composite_density's compositing weights w_s, summed in the order of that
 *                    kernel's depth sum (lane-local over ascending 64-sample chunks, then the wave butterfly).  Not renormalised: its
 *                    length is at most acc and works as a confidence.
 *   Dex normal       dex_normal[k, ray, :] = n at the first sample with sigma > m_k - the sample whose z the Dex depth reports -
 *                    and (0,0,0) when no sample crosses (the Dex depth then falls back to z[0]); the zero vector is the only
 *                    "no surface" marker.  Layout (K, N, 3).
 */
#ifndef DEXNERF_HIP_NORMALS_H
#define DEXNERF_HIP_NORMALS_H

#include "dexnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dn_composite_density that also composites per-sample normals --------------------------------------------------------------------
 * rf (N,S,4) raw rows (.w read), z (N,S), rd rows of rd_stride floats, noise (N,S) or NULL, d_m_thres: n_thres >= 0 thresholds in
 * DEVICE memory - all as in dn_composite_density - and g_pts (N,S,3) = g_s.  depth (N), acc (N), dex (K,N) carry dn_composite_density's
 * bits for the same inputs; normal (N,3); dex_normal (K,N,3).  Every output may be NULL, but with n_thres > 0 not both dex and
 * dex_normal.  One wave per ray; the grid is a function of (N, S) alone. */
int dn_composite_normals(const float* rf, const float* z, const float* rd, int rd_stride, const float* noise, float noise_std,
                         const float* g_pts, const float* d_m_thres, int n_thres, int64_t n_rays, int n_samples, float* depth,
                         float* acc, float* dex, float* normal, float* dex_normal, dn_stream_t stream);

/* ---- the normal render: dn_render_rays_depth with the last pass differentiated ---------------------------------------------------------
 * Launches: coarse depths -> coarse density network (inference kernel) -> dn_density_resample -> fine density network on the TRAINING
 * forward (its saved tensors stay in the workspace) -> the seed g_out = (0,0,0,1) per point -> dn_mlp_backward_data -> the per-point
 * input gradient (dn_mlp_backward_input's first launch, points formed from rays + z) -> dn_composite_normals.  With num_fine == 0 the
 * coarse network is the one differentiated (and depth_c / acc_c are not written: the coarse pass is the last one).
 *   desc_* / packed_*   density descriptors (dn_mlp_density_desc: use_viewdirs == 0) and their forward packs (dn_mlp_pack_density)
 *   packed_bwd / _ig    dn_mlp_pack_backward / dn_mlp_pack_input_grad streams of the DIFFERENTIATED density network (the fine one, or the
 *                       coarse one with num_fine == 0), packed from [layer1, trunk..., head (4,W) = zeros with row 3 = fc_alpha.weight]
 *   precision           DN_PREC_F32, or DN_PREC_BF16 (16-bit saved tensors); DN_PREC_F16 and DN_PREC_BF16_S8: DN_E_UNSUPPORTED, as in
 *                       dn_mlp_backward_input
 *   rays, draws, d_m_thres, sample counts: dn_render_rays_depth's - ray_stride >= 8; with a fine pass 10 <= num_coarse <= 512 and
 *                       num_coarse + num_fine <= 2048
 *   depth_c, acc_c (N)  the coarse pass (num_fine > 0), may be NULL
 *   depth, acc (N), dex (K,N), normal (N,3), dex_normal (K,N,3): the last pass; each may be NULL, but with n_thres > 0 not both dex and
 *                       dex_normal
 *   workspace           256-byte aligned, at least dn_render_normals_workspace_bytes(...) bytes
 * The last pass's sigma comes from the training-forward kernel: depth / acc / dex may differ from dn_render_rays_depth's in the last
 * bits. */
size_t dn_render_normals_workspace_bytes(const dn_mlp_desc* desc_coarse, const dn_mlp_desc* desc_fine, int precision, int64_t n_rays,
                                         int num_coarse, int num_fine);   /* 0: bad sizes, or a descriptor / precision not supported */
int dn_render_rays_normals(const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine, const void* packed_fine,
                           const void* packed_bwd, const void* packed_ig, int precision, const float* rays, int ray_stride, int64_t n_rays,
                           int num_coarse, int num_fine, int lindisp, float noise_std, const float* d_m_thres, int n_thres,
                           const float* t_rand, const float* noise_c, const float* u, const float* noise_f, float* depth_c, float* acc_c,
                           float* depth, float* acc, float* dex, float* normal, float* dex_normal, void* workspace, size_t workspace_bytes,
                           dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_NORMALS_H */
