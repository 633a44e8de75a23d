// The surface-normal compositing of the normal render (dn_render_rays_normals, include/dexnerf_hip_normals.h): dn_composite_density's
// pass - expected depth, accumulation, Dex depths, the same bits - that also composites the per-sample unit normals
//     n_s = -g_s / |g_s|,   g_s = d sigma_raw / d x  (g_pts, (N,S,3)),
// into the expected normal sum_s w_s n_s and picks n at each threshold's first-crossing sample (the sample whose z the Dex depth
// reports).  One wave64 per ray, four rays per workgroup, built on forward_ray: the expected normal rides on its on_weight hook, the
// Dex normals on its on_first hook.  Plain stores, no atomics; the grid is a function of (N, S) alone.
//
// Memory: HBM-bound, 16 B (raw row, .w used) + 4 B (z) + 12 B (gradient) read per sample.  A lane reads its sample's three gradient
// components as three dwords 12 B apart; the wave's three loads cover ONE contiguous 768 B span between them, so every cache line
// fetched is used in full (the second and third load hit the lines the first brought in) - no staging through LDS.
#include "../../include/dexnerf_hip_normals.h"
#include "composite_body.h"
#include "sampler_body.h"

namespace dn {

// -g / |g|: the norm in fp64 from the three fp32 components, each quotient rounded to fp32 once; (0,0,0) when |g| is 0 or not finite
__device__ __forceinline__ void unit_normal(const float* __restrict__ g, float (&n)[3]) {
  const double gx = g[0], gy = g[1], gz = g[2];
  const double len = sqrt((gx * gx + gy * gy) + gz * gz);
  const bool ok = len > 0.0 && len <= 1.7976931348623157e308;   // (false for NaN and +inf)
  n[0] = ok ? static_cast<float>(-gx / len) : 0.0f;
  n[1] = ok ? static_cast<float>(-gy / len) : 0.0f;
  n[2] = ok ? static_cast<float>(-gz / len) : 0.0f;
}

__global__ __launch_bounds__(256) void composite_normals_kernel(const float4* __restrict__ rf, const float* __restrict__ z,
                                                                const float* __restrict__ rd, int rd_stride, const float* __restrict__ noise,
                                                                float noise_std, const float* __restrict__ g_pts,
                                                                const float* __restrict__ d_thres, int n_thres, int64_t n_rays, int S,
                                                                float* __restrict__ depth, float* __restrict__ acc, float* __restrict__ dex,
                                                                float* __restrict__ normal, float* __restrict__ dex_normal,
                                                                unsigned* __restrict__ nonfinite) {
  const int lane = lane_id();
  const int64_t ray = static_cast<int64_t>(blockIdx.x) * kSamplerWaves + (threadIdx.x >> 6);
  if (ray >= n_rays) return;  // wave-uniform exit; no block-level sync in this kernel
  const float* gr = g_pts + ray * S * 3;
  float s_n[3] = {0.0f, 0.0f, 0.0f};   // lane-local over ascending chunks, then wave_sum: the order of forward_ray's depth sum
  forward_ray(
      SigmaColumn(rf + ray * S), TensorNoise{noise, noise_std, ray, S}, DeviceThres{d_thres, n_thres}, z + ray * S, rd + ray * rd_stride, ray,
      true, lane, n_rays, S, acc, depth, dex, nonfinite,
      [&](int s, bool valid, float w, float) {
        if (!valid || normal == nullptr) return;
        float n[3];
        unit_normal(gr + 3 * s, n);
#pragma unroll
        for (int c = 0; c < 3; ++c) s_n[c] += w * n[c];
      },
      [&](int k, int first) {
        if (dex_normal == nullptr) return;
        float n[3] = {0.0f, 0.0f, 0.0f};   // no crossing: the zero vector is the "no surface" marker
        if (first >= 0) unit_normal(gr + 3 * first, n);
        float* out = dex_normal + (static_cast<int64_t>(k) * n_rays + ray) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = n[c];
      });
  if (normal == nullptr) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) s_n[c] = wave_sum(s_n[c]);
  if (lane < 3) normal[ray * 3 + lane] = lane == 0 ? s_n[0] : lane == 1 ? s_n[1] : s_n[2];
}

// the seed of the density gradient: g_out = (0, 0, 0, 1) per point - d sigma_raw / d(raw row)
__global__ __launch_bounds__(256) void density_seed_kernel(float4* __restrict__ g_out, long long n_points) {
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_points;
       i += static_cast<long long>(gridDim.x) * blockDim.x)
    g_out[i] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
}

int density_seed(float* g_out, int64_t n_points, dn_stream_t stream) {
  if (n_points == 0) return 0;
  DN_REQUIRE(g_out && n_points > 0 && (reinterpret_cast<uintptr_t>(g_out) & 15) == 0, "density_seed: bad arguments");
  const long long blocks = (n_points + 255) / 256;
  hipLaunchKernelGGL(density_seed_kernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<float4*>(g_out), static_cast<long long>(n_points));
  return check_launch("density_seed");
}

int composite_normals_counting(const SigmaCompositeArgs& a, dn_stream_t stream) {
  if (int rc = sigma_composite_check("dn_composite_normals", a, true)) return rc;
  if (a.n_rays == 0) return 0;
  hipLaunchKernelGGL(composite_normals_kernel, dim3(ray_grid(a.n_rays)), dim3(256), 0, as_stream(stream), reinterpret_cast<const float4*>(a.rf),
                     a.z, a.rd, a.rd_stride, a.noise, a.noise_std, a.g_pts, a.d_m_thres, a.n_thres, a.n_rays, a.n_samples, a.depth, a.acc,
                     a.n_thres > 0 ? a.dex : nullptr, a.normal, a.n_thres > 0 ? a.dex_normal : nullptr, a.nonfinite);
  return check_launch("dn_composite_normals");
}

}  // namespace dn

using namespace dn;

extern "C" int dn_composite_normals(const float* rf, const float* z, const float* rd, int rd_stride, const float* noise, float noise_std,
                                    const float* g_pts, const float* d_m_thres, int n_thres, int64_t n_rays, int n_samples, float* depth,
                                    float* acc, float* dex, float* normal, float* dex_normal, dn_stream_t stream) {
  SigmaCompositeArgs a{rf, z, rd, rd_stride, noise, noise_std, d_m_thres, n_thres, n_rays, n_samples, depth, acc, dex};
  a.g_pts = g_pts; a.normal = normal; a.dex_normal = dex_normal;
  return composite_normals_counting(a, stream);
}
