// The opacity-quantile compositing of the depth path (include/dexnerf_hip_quantile.h): dn_composite_density's pass - expected depth,
// accumulation, Dex depths, the same bits - that also reads out, per quantile q_k, the depth at which the ray's accumulated opacity
// C_s = sum_{j <= s} w_j first reaches q_k (q = 0.5: the median depth).  One wave64 per ray, four rays per workgroup, built on
// forward_ray with its Quantiles<> argument: lane k tracks quantile k, the prefix sum is an fp64 wave scan with a carry between the
// 64-sample chunks, and a chunk is searched for quantile k only when its last C reaches q_k (a wave-uniform test).  Plain vector
// stores, no atomics (but the non-finite count of the render's status block); the grid is a function of (N, S) alone.
//
// Memory: HBM-bound like composite_density_kernel - 16 B (raw row, .w used) + 4 B (z) read per sample; the quantiles add Q floats
// read and Q floats written per ray and no pass over the samples.
#include "../../include/dexnerf_hip_quantile.h"
#include "composite_body.h"
#include "sampler_body.h"

namespace dn {

__global__ __launch_bounds__(256) void composite_quantile_kernel(const float4* __restrict__ rf, const float* __restrict__ z,
                                                                 const float* __restrict__ rd, int rd_stride, const float* __restrict__ noise,
                                                                 float noise_std, const float* __restrict__ d_thres, int n_thres,
                                                                 const float* __restrict__ d_quant, int n_quant, int interp, int64_t n_rays,
                                                                 int S, float* __restrict__ depth, float* __restrict__ acc,
                                                                 float* __restrict__ dex, float* __restrict__ qdepth,
                                                                 unsigned* __restrict__ nonfinite) {
  const int lane = lane_id();
  const int64_t ray = static_cast<int64_t>(blockIdx.x) * kSamplerWaves + (threadIdx.x >> 6);
  if (ray >= n_rays) return;  // wave-uniform exit; no block-level sync in this kernel
  forward_ray(SigmaColumn(rf + ray * S), TensorNoise{noise, noise_std, ray, S}, DeviceThres{d_thres, n_thres}, z + ray * S,
              rd + ray * rd_stride, ray, true, lane, n_rays, S, acc, depth, dex, nonfinite, [](int, bool, float, float) {}, NoFirstHook{},
              Quantiles<>{d_quant, n_quant, interp, qdepth, NoQuantileHook{}});
}

int quantile_args_check(const char* who, const float* d_quantiles, int n_quant, int interp, const float* qdepth) {
  DN_REQUIRE(n_quant >= 0 && n_quant <= DN_MAX_QUANTILES, "%s: need 0 <= n_quant <= %d quantiles per call", who, DN_MAX_QUANTILES);
  DN_REQUIRE(n_quant == 0 || (d_quantiles && qdepth), "%s: quantiles given without qdepth output", who);
  DN_REQUIRE(interp == 0 || interp == 1, "%s: interp must be 0 (sample) or 1 (linear)", who);
  return 0;
}

int composite_quantile_counting(const SigmaCompositeArgs& a, dn_stream_t stream) {
  if (int rc = sigma_composite_check("dn_composite_density_quantiles", a)) return rc;
  if (a.n_rays == 0) return 0;
  hipLaunchKernelGGL(composite_quantile_kernel, dim3(ray_grid(a.n_rays)), dim3(256), 0, as_stream(stream), reinterpret_cast<const float4*>(a.rf),
                     a.z, a.rd, a.rd_stride, a.noise, a.noise_std, a.d_m_thres, a.n_thres, a.d_quantiles, a.n_quant, a.interp, a.n_rays,
                     a.n_samples, a.depth, a.acc, a.n_thres > 0 ? a.dex : nullptr, a.n_quant > 0 ? a.qdepth : nullptr, a.nonfinite);
  return check_launch("dn_composite_density_quantiles");
}

}  // namespace dn

using namespace dn;

extern "C" int dn_composite_density_quantiles(const float* rf, const float* z, const float* rd, int rd_stride, const float* noise,
                                              float noise_std, const float* d_m_thres, int n_thres, const float* d_quantiles, int n_quant,
                                              int interp, int64_t n_rays, int n_samples, float* depth, float* acc, float* dex, float* qdepth,
                                              dn_stream_t stream) {
  return composite_quantile_counting({rf, z, rd, rd_stride, noise, noise_std, d_m_thres, n_thres, n_rays, n_samples, depth, acc, dex, nullptr,
                                      d_quantiles, n_quant, interp, qdepth}, stream);
}
