/*
 * dexnerf_hip_ext.h - entry points of libdexnerf_hip.so added after ABI version 2 (dexnerf_hip.h, whose table and DN_ABI_VERSION stay as
 * they are: a caller built against it alone keeps working).  Same conventions: device pointers, contiguous fp32, caller-owned outputs
 * and workspaces, work enqueued on `stream`, 0 / DN_E_* / -(hipError_t), dn_last_error.
 */
#ifndef DEXNERF_HIP_EXT_H
#define DEXNERF_HIP_EXT_H

#include "dexnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the distortion regulariser (mip-NeRF 360, eq. 15) on compositing's weights and depths -----------------------------------------------
 * Per ray, with m_i = (z_i + z_{i+1}) / 2 and delta_i = z_{i+1} - z_i for i < S-1, m_{S-1} = z_{S-1}, delta_{S-1} = 0 (compositing's last
 * interval is a constant), both times k = 1 / (far - near):
 *     L_ray = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i
 * formed in O(S) by fp64 prefix sums over the samples in their (sorted) order; tied depths get the subgradient of that order.
 *   weights, z : (N, S), S in 1..1024; z ascending along a ray
 *   near_far   : near of ray r at near_far[r * stride], far at near_far[r * stride + 1], stride >= 2 (ray rows: rays + 6, ray_stride).
 *                far - near is a normalisation constant: no gradient; a ray without far > near yields exact zeros everywhere
 *   g_weights  : (N, S)  = scale * dL_ray/dw
 *   g_z        : (N, S)  = scale * dL_ray/dz, stored (accumulate_z == 0) or added to what is there; may be NULL
 *   ray_loss   : (N) fp64, L_ray (not scaled)
 *   mean_loss  : one float: the unweighted mean of L_ray over the rays, summed in a fixed order
 * Two launches whose grids are functions of N and S alone; no atomics: two runs give the same bits.  n_rays == 0 returns 0 before any
 * check; otherwise every argument is judged before GPU work (NULL pointers, S, stride, a non-finite scale: DN_E_INVAL). */
int dn_distortion_loss(const float* weights, const float* z, const float* near_far, int stride, int64_t n_rays, int n_samples, float scale,
                       float* g_weights, float* g_z, int accumulate_z, double* ray_loss, float* mean_loss, dn_stream_t stream);

/* ---- dn_render_rays_backward_ws with the distortion regulariser of either network -----------------------------------------------------------
 * The arguments of dn_render_rays_backward_ws, then: the weight of the coarse and of the fine network's term (finite, >= 0), a workspace of
 * dn_render_reg_workspace_bytes(n_rays, num_coarse, num_fine) bytes (256-byte aligned; contents undefined before and after), and reg2 =
 * [mean L_ray coarse, mean L_ray fine] (two floats; a half writes its own word, and only when its weight is non-zero).
 * For a network in `nets` whose weight is non-zero, before its compositing backward: its sample weights (coarse: as the forward left
 * them in the training workspace; fine: composited again from the saved rows, the same noise stream, the same bits), then
 * dn_distortion_loss with scale = weight / n_rays, whose g_weights the compositing backward adds to every sample's upstream gradient.
 * With both weights 0 this is dn_render_rays_backward_ws bit for bit (reg_workspace and reg2 may then be NULL). */
size_t dn_render_reg_workspace_bytes(int64_t n_rays, int num_coarse, int num_fine);
int dn_render_rays_backward_reg(const dn_mlp_desc* desc_coarse, const void* packed_bwd_coarse, const dn_mlp_desc* desc_fine,
                                const void* packed_bwd_fine, int precision, const float* rays, int ray_stride, int64_t n_rays,
                                int num_coarse, int num_fine, float noise_std, int white_background, const float* noise_c,
                                const float* noise_f, const float* g_rgb_c, const float* g_depth_c, const float* g_acc_c,
                                const float* g_rgb_f, const float* g_depth_f, const float* g_acc_f, void* workspace,
                                const void* act_c, const void* masks_c, void* grads_c, const void* act_f, const void* masks_f,
                                void* grads_f, float* const* h_dW_c, float* const* h_db_c, float* const* h_dW_f,
                                float* const* h_db_f, int nets, const uint32_t* rng_state, void* wg_scratch, size_t wg_scratch_bytes,
                                float dist_weight_c, float dist_weight_f, void* reg_workspace, size_t reg_workspace_bytes, float* reg2,
                                dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_EXT_H */
