/*
 * dexnerf_hip_anneal.h - the coarse-to-fine positional encoding (BARF, Lin et al. 2021, eq. 14) as entry points of libdexnerf_hip.so
 * beside dexnerf_hip.h and dexnerf_hip_ext.h, whose tables and DN_ABI_VERSION stay as they are.  Same conventions: device pointers,
 * contiguous fp32, caller-owned buffers, work enqueued on `stream`, 0 / DN_E_* / -(hipError_t), dn_last_error; every argument is
 * judged before any GPU work; plain vector stores, no atomics; every launch can be captured into a HIP graph.
 *
 * A per-band amplitude a on the encoding is a per-column scale of the weights that multiply it: W (a * enc) = (W diag(a)) enc.  The
 * kernels here form a on the device (so a replayed graph follows the iteration counter), scale fp32 copies of the weights BEFORE they
 * are packed - forward and input gradient of every precision then come out of the unchanged network kernels - and scale the weight
 * gradient's encoding columns afterwards: dL/dW = (dL/dW_eff) diag(a).
 *
 * The layers that read an encoding, in the reference parameter order (index into the pointer lists):
 *     layer1            index 0                     columns [0, 3 + 6 L_xyz)              of 3 + 6 L_xyz
 *     layers_xyz[i]     index 1 + i, i a skip layer columns [W, W + 3 + 6 L_xyz)          of W + 3 + 6 L_xyz
 *     layers_dir.0      index D (view directions)   columns [W, W + 3 + 6 L_dir)          of W + 3 + 6 L_dir
 * Column c of such a block: c < 3 is the raw input (amplitude 1, always), else band (c - 3) / 6 in the order of the encoding, whether
 * its frequencies are sampled log or linear.
 */
#ifndef DEXNERF_HIP_ANNEAL_H
#define DEXNERF_HIP_ANNEAL_H

#include "dexnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the amplitude table ----------------------------------------------------------------------------------------------------------------------
 * amp[l_xyz + l_dir] fp32: the bands of the xyz encoding, then those of the view-direction encoding.  With the iteration `it`,
 *     p = clamp((it - start) / (end - start), 0, 1)   (end == start: a step, p = 1 from it >= start on)
 *     a_k = (1 - cos(pi * clamp(p L - k, 0, 1))) / 2   per encoding, L its number of bands
 * in fp64, rounded to fp32 once; the clamped ends are exact +0.0f and exact 1.0f by branch.  anneal_dir == 0: the l_dir view-direction
 * amplitudes are 1.0f.
 *   rng_state : the training loop's device record {seed_lo, seed_hi, cur, nxt} (dn_select_rays_draw), or NULL.  Given: `it` is its `nxt`
 *               word, read by the kernel - the number of the iteration being enqueued from the end of the previous loss head to this
 *               one's, before and after the draw kernel publishes it as `cur`.  NULL: `it` = iteration (>= 0).
 *   start, end: iterations, finite, 0 <= start <= end;  l_xyz in 1..32, l_dir in 0..32.
 * One launch of one workgroup. */
int dn_encoding_anneal_amplitudes(const uint32_t* rng_state, int64_t iteration, double start, double end, int l_xyz, int l_dir,
                                  int anneal_dir, float* amp, dn_stream_t stream);

/* ---- scaled weight copies -------------------------------------------------------------------------------------------------------------------------
 * h_weights, h_scaled: HOST arrays of device pointers, one per nn.Linear weight in the reference parameter order (dn_mlp_pack).  For each
 * layer that reads an encoding (above) the whole (out, in) matrix is written to h_scaled[i]: hidden columns and the three raw-input
 * columns copied, band columns multiplied by their amplitude - one fp32 multiply per element.  Other entries of h_scaled are not read.
 * amp: the table of dn_encoding_anneal_amplitudes for this descriptor's L_xyz / L_dir (nets without view directions: the xyz part).
 * The copies must not overlap the weights or each other.  One launch per network. */
int dn_encoding_anneal_scale_weights(const dn_mlp_desc* desc, const float* const* h_weights, const float* amp, float* const* h_scaled,
                                     dn_stream_t stream);

/* ---- gradient column scale --------------------------------------------------------------------------------------------------------------------------
 * h_dW: HOST array of device pointers to the weight gradients, (out, in) row-major, in the reference parameter order
 * (dn_mlp_weight_grad_all).  In place on the band columns of the layers that read an encoding: g <- g * a; where a is +0.0f the result is
 * +0.0f.  Every other element is left alone.
 * PRECONDITION: the arrays hold the contribution of ONE backward run on the scaled weights, nothing accumulated from another source - a
 * gradient already in the array would be scaled with it.  (The fused training steps clear their gradient bucket before every backward.)
 * One launch per network. */
int dn_encoding_anneal_scale_grads(const dn_mlp_desc* desc, const float* amp, float* const* h_dW, dn_stream_t stream);

/* ---- both networks of a training step in one launch ---------------------------------------------------------------------------------------------------
 * The two entry points above for a coarse and a fine network that read ONE table (they must agree on L_xyz / L_dir and on having view
 * directions; their depths and widths may differ): the same stores, one launch instead of two. */
int dn_encoding_anneal_scale_weights_pair(const dn_mlp_desc* desc_a, const float* const* h_weights_a, float* const* h_scaled_a,
                                          const dn_mlp_desc* desc_b, const float* const* h_weights_b, float* const* h_scaled_b,
                                          const float* amp, dn_stream_t stream);
int dn_encoding_anneal_scale_grads_pair(const dn_mlp_desc* desc_a, float* const* h_dW_a, const dn_mlp_desc* desc_b, float* const* h_dW_b,
                                        const float* amp, dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXNERF_HIP_ANNEAL_H */
