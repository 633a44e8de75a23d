/*
 * dexnerf_hip_exposure.h - per-view exposure (photometric calibration) in the loss head, as an entry point of libdexnerf_hip.so beside
 * dexnerf_hip.h, dexnerf_hip_ext.h and dexnerf_hip_anneal.h, whose tables and DN_ABI_VERSION stay as they are.  Same conventions: device
 * pointers, contiguous fp32, caller-owned buffers, work enqueued on `stream`, 0 / DN_E_* / -(hipError_t), dn_last_error; every argument
 * is judged before any GPU work; plain vector stores, no atomics; every launch can be captured into a HIP graph.
 *
 * Each view v of a capture has an exposure row eps[v] of P floats; with s = exposure_scale (> 0) the rendered colour c of a ray of
 * view v - coarse and fine alike - enters the colour terms of the loss as
 *     P = 1  "gain"    c^_k = exp(s a) c_k                      eps[v] = [a]
 *     P = 6  "affine"  c^_k = exp(s a_k) c_k + s b_k            eps[v] = [a_r, a_g, a_b, b_r, b_g, b_b]
 * (with `luminance` per channel first, the 0.299 / 0.587 / 0.114 mix after it).  The depth term does not see the exposure.
 */
#ifndef DEXNERF_HIP_EXPOSURE_H
#define DEXNERF_HIP_EXPOSURE_H

#include "dexnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dn_render_loss with the exposure correction ------------------------------------------------------------------------------------------------
 * The arguments of dn_render_loss, with the same meaning and the same checks, and
 *   eps            : (n_views, P) exposure rows;  P in {1, 6};  n_views in [1, 65535];  exposure_scale finite and > 0
 *   view_index     : (n_rays) int32, the view of every ray - also the view the depth targets are gathered at when pixel_index is given;
 *                    NULL: every ray is of view *view (device int32 word; NULL too: view 0).  Unlike dn_render_loss both may be given
 *                    without pixel_index.  A ray whose view lies outside [0, n_views) is not corrected and enters no row of g_eps.
 *   view_mask      : (n_views) int32 or NULL: row v of g_eps is formed where view_mask[v] != 0 (NULL: everywhere).  The correction itself
 *                    is applied to every view, masked or not.
 *   g_eps          : (n_views, P) out, or NULL (loss and colour gradients only: one launch less)
 *
 * A ray whose row is all zeros (of either sign) takes dn_render_loss's expressions by a branch: with eps == 0 loss6, g_rgb_* and g_depth_*
 * are dn_render_loss's bits.  Otherwise the gain exp(s a_k) is formed in fp64 and rounded to fp32 once, c^_k = gain * c_k + s * b_k in
 * fp32 (a multiply, an add: no FMA), and
 *   loss6          : as dn_render_loss lays it out, the two mse on c^
 *   g_rgb_*        : dn_render_loss's gradient expression on c^, times the gain (d c^_k / d c_k); the depth gradients are dn_render_loss's
 *   g_eps[v]       : the gradient of loss6[0] with respect to eps[v]: over the rays of view v and both passes p (weights w_p),
 *                      d/da_k = sum w_p (dmse_p / dc^_k) s exp(s a_k) c_pk   ("gain": summed over k as well, a_k = a)
 *                      d/db_k = sum w_p (dmse_p / dc^_k) s
 *                    each ray's terms in fp64 from the fp32 inputs.  One workgroup of 1024 threads per view walks all rays (i = thread,
 *                    thread + 1024, ...: a lane's rays ascending), then wave_sum's butterfly over the 64 lanes, then the 16 waves through
 *                    LDS in wave order; the fp64 sum is rounded to fp32 once.  The order of every sum is a function of (n_rays, n_views)
 *                    and the view indices alone: the same bits on any device.  A view without a ray, and a masked view: exact +0.
 * rng_state given: its iteration counter is advanced as dn_render_loss advances it.
 * Launches: the head (one workgroup of 1024 threads, like dn_render_loss), and with g_eps the per-view reduction (n_views workgroups).
 * No scratch. */
int dn_render_loss_exposure(const float* rgb_coarse, const float* rgb_fine, const float* target, const float* depth_coarse,
                            const float* depth_fine, const float* depth_src, const int64_t* pixel_index, const int32_t* view_index,
                            const int32_t* view, int64_t hw, int64_t n_rays, int luminance, float w_rgb_coarse, float w_rgb_fine,
                            float w_depth_coarse, float w_depth_fine, float depth_lo, float depth_hi, const float* eps, int P, int n_views,
                            float exposure_scale, const int32_t* view_mask, float* loss6, float* g_rgb_coarse, float* g_rgb_fine,
                            float* g_depth_coarse, float* g_depth_fine, float* g_eps, uint32_t* rng_state, dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_EXPOSURE_H */
