// The sigma-only render kernels of the depth path (dn_render_rays_depth): expected depth, accumulation and Dex depths need the
// density column alone (reference nerf/volume_rendering_utils.py:33-58), so neither kernel evaluates a sigmoid or a colour sum.
//   density_resample_kernel : coarse compositing fused with the fine-depth generation (nerf/train_utils.py:163-173) - one wave per
//                             ray forms the coarse weights in registers, drops weights[1:-1] + 1e-5 straight into the sampler's
//                             LDS row and runs the sampler's own code on it: the (N, Nc) weights never reach HBM.
//   composite_density_kernel: depth, acc and dex (K, N) for any K (thresholds in device memory, 64 per pass).
//   composite_brackets_kernel: the same without noise, plus the bracket record and first midpoint of every first crossing
//                             (include/dexnerf_hip_refine.h; the bisection and the finish are dex_refine.hip's).
// One wave64 per ray, four rays per workgroup, like composite.hip / the sampler.
#include "../../include/dexnerf_hip_refine.h"
#include "composite_body.h"
#include "sampler_body.h"

namespace dn {

__global__ __launch_bounds__(256) void density_resample_kernel(const float4* __restrict__ rf, const float* __restrict__ z,
                                                               const float* __restrict__ rd, int rd_stride, const float* __restrict__ noise,
                                                               float noise_std, const float* __restrict__ u, int64_t n_rays, int nc, int nf,
                                                               float* __restrict__ depth, float* __restrict__ acc, float* __restrict__ z_fine,
                                                               int sort_len, unsigned* __restrict__ nonfinite) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int64_t ray_raw = static_cast<int64_t>(blockIdx.x) * kSamplerWaves + wave;
  const bool live = ray_raw < n_rays;
  const int64_t ray = live ? ray_raw : (n_rays - 1);
  const int B = nc - 1;
  const int per_wave = 3 * (B + 1) + sort_len;   // sampler_kernel's rows (mode 1)
  float* w = lds + wave * per_wave;
  float* cdf = w + (B + 1);
  float* bins = cdf + (B + 1);
  float* sbuf = bins + (B + 1);
  const float* zc = z + ray * nc;
  for (int i = lane; i < B; i += 64) bins[i] = 0.5f * (zc[i + 1] + zc[i]);
  for (int i = lane; i < nc; i += 64) sbuf[i] = zc[i];
  forward_ray(SigmaColumn(rf + ray * nc), TensorNoise{noise, noise_std, ray, nc}, DeviceThres{nullptr, 0}, zc, rd + ray * rd_stride, ray, live,
              lane, n_rays, nc, acc, depth, static_cast<float*>(nullptr), nonfinite,
              [&](int s, bool valid, float wt, float) { if (valid && s >= 1 && s <= nc - 2) w[s - 1] = wt + 1e-5f; });   // weights[..., 1:-1] + 1e-5
  sampler_resample<1>(w, cdf, bins, sbuf, u, ray, live, B, nf, static_cast<float*>(nullptr), static_cast<int64_t*>(nullptr), z_fine,
                      sort_len, RngRef{nullptr, 0u});
}

__global__ __launch_bounds__(256) void composite_density_kernel(const float4* __restrict__ rf, const float* __restrict__ z,
                                                                const float* __restrict__ rd, int rd_stride, const float* __restrict__ noise,
                                                                float noise_std, const float* __restrict__ d_thres, int n_thres, int64_t n_rays,
                                                                int S, float* __restrict__ depth, float* __restrict__ acc,
                                                                float* __restrict__ dex, unsigned* __restrict__ nonfinite) {
  const int lane = lane_id();
  const int64_t ray = static_cast<int64_t>(blockIdx.x) * kSamplerWaves + (threadIdx.x >> 6);
  if (ray >= n_rays) return;  // wave-uniform exit; no block-level sync in this kernel
  forward_ray(SigmaColumn(rf + ray * S), TensorNoise{noise, noise_std, ray, S}, DeviceThres{d_thres, n_thres}, z + ray * S,
              rd + ray * rd_stride, ray, true, lane, n_rays, S, acc, depth, dex, nonfinite, [](int, bool, float, float) {});
}

// composite_density_kernel without noise whose first-crossing hook writes the bracket record (z_lo, z_hi, s_lo, s_hi) of every
// threshold and its first midpoint (include/dexnerf_hip_refine.h).  The hook runs once per (ray, threshold) in the lane that holds the
// threshold: two depths and two raw densities re-read from the ray's rows (L2-resident by then), one 16-byte store, one 4-byte store.
__global__ __launch_bounds__(256) void composite_brackets_kernel(const float4* __restrict__ rf, const float* __restrict__ z,
                                                                 const float* __restrict__ rd, int rd_stride, const float* __restrict__ d_thres,
                                                                 int n_thres, int64_t n_rays, int S, float* __restrict__ depth,
                                                                 float* __restrict__ acc, float* __restrict__ dex, float4* __restrict__ br,
                                                                 float* __restrict__ z_mid, unsigned* __restrict__ nonfinite) {
  const int lane = lane_id();
  const int64_t ray = static_cast<int64_t>(blockIdx.x) * kSamplerWaves + (threadIdx.x >> 6);
  if (ray >= n_rays) return;  // wave-uniform exit; no block-level sync in this kernel
  const SigmaColumn sig(rf + ray * S);
  const float* zr = z + ray * S;
  forward_ray(sig, TensorNoise{nullptr, 0.0f, ray, S}, DeviceThres{d_thres, n_thres}, zr, rd + ray * rd_stride, ray, true, lane, n_rays, S, acc,
              depth, dex, nonfinite, [](int, bool, float, float) {}, [&](int k, int idx) {
                float4 r;
                if (idx < 0) {
                  r = make_float4(zr[0], zr[0], __builtin_inff(), -__builtin_inff());
                } else {
                  const int lo = idx > 0 ? idx - 1 : 0;
                  r = make_float4(zr[lo], zr[idx], sig(lo), sig(idx));
                }
                const int64_t rec = ray * n_thres + k;
                br[rec] = r;
                z_mid[rec] = r.x + 0.5f * (r.y - r.x);
              });
}

static int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

int density_resample_counting(const float* rf, const float* z, const float* rd, int rd_stride, const float* noise, float noise_std,
                              const float* u, int64_t n_rays, int num_coarse, int num_fine, float* depth, float* acc, float* z_fine,
                              unsigned* nonfinite, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(rf && z && rd && z_fine && n_rays >= 0 && num_fine >= 1 && rd_stride >= 3, "dn_density_resample: bad arguments");
  DN_REQUIRE(num_coarse >= 10 && num_coarse <= 512 && num_coarse + num_fine <= 2048,
             "dn_density_resample: need 10 <= num_coarse <= 512 and num_coarse + num_fine <= 2048");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(rf) & 15) == 0, "dn_density_resample: rf must be 16-byte aligned");
  const int sort_len = next_pow2(num_coarse + num_fine);
  const size_t lds = static_cast<size_t>(kSamplerWaves) * (3 * num_coarse + sort_len) * sizeof(float);
  hipLaunchKernelGGL(density_resample_kernel, dim3(ray_grid(n_rays)), dim3(256), lds, as_stream(stream), reinterpret_cast<const float4*>(rf), z, rd,
                     rd_stride, noise, noise_std, u, n_rays, num_coarse, num_fine, depth, acc, z_fine, sort_len, nonfinite);
  return check_launch("dn_density_resample");
}

int sigma_composite_check(const char* who, const SigmaCompositeArgs& a, bool normals) {
  DN_REQUIRE(a.rf && a.z && a.rd && (!normals || a.g_pts) && a.n_rays >= 0 && a.n_samples >= 1 && a.rd_stride >= 3, "%s: bad arguments", who);
  DN_REQUIRE(a.n_thres >= 0, "%s: negative threshold count", who);
  if (normals)
    DN_REQUIRE(a.n_thres == 0 || (a.d_m_thres && (a.dex || a.dex_normal)), "%s: thresholds given without dex or dex_normal output", who);
  else
    DN_REQUIRE(a.n_thres == 0 || (a.d_m_thres && a.dex), "%s: thresholds given without dex output", who);
  if (int rc = quantile_args_check(who, a.d_quantiles, a.n_quant, a.interp, a.qdepth)) return rc;   // (n_quant == 0, interp == 0: passes)
  DN_REQUIRE((reinterpret_cast<uintptr_t>(a.rf) & 15) == 0, "%s: rf must be 16-byte aligned", who);
  return 0;
}
static_assert(kSamplerWaves == 4, "ray_grid (dn_common.h) counts four rays per workgroup");

int composite_density_counting(const SigmaCompositeArgs& a, dn_stream_t stream) {
  if (a.n_rays == 0) return 0;   // (before the checks, as ever: empty tensors carry NULL data pointers - _ops.composite_density)
  if (int rc = sigma_composite_check("dn_composite_density", a)) return rc;
  hipLaunchKernelGGL(composite_density_kernel, dim3(ray_grid(a.n_rays)), dim3(256), 0, as_stream(stream), reinterpret_cast<const float4*>(a.rf),
                     a.z, a.rd, a.rd_stride, a.noise, a.noise_std, a.d_m_thres, a.n_thres, a.n_rays, a.n_samples, a.depth, a.acc,
                     a.n_thres > 0 ? a.dex : nullptr, a.nonfinite);
  return check_launch("dn_composite_density");
}

int composite_brackets_counting(const SigmaCompositeArgs& a, float* br, float* z_mid, dn_stream_t stream) {
  const char* who = "dn_composite_density_brackets";
  if (a.n_rays == 0) return 0;   // (before the checks, like dn_composite_density: empty tensors carry NULL data pointers)
  DN_REQUIRE(a.rf && a.z && a.rd && br && z_mid && a.n_rays >= 0 && a.n_samples >= 1 && a.rd_stride >= 3, "%s: bad arguments", who);
  DN_REQUIRE(a.n_thres >= 1 && a.d_m_thres, "%s: needs at least one threshold", who);
  DN_REQUIRE(((reinterpret_cast<uintptr_t>(a.rf) | reinterpret_cast<uintptr_t>(br)) & 15) == 0, "%s: rf and br must be 16-byte aligned", who);
  hipLaunchKernelGGL(composite_brackets_kernel, dim3(ray_grid(a.n_rays)), dim3(256), 0, as_stream(stream), reinterpret_cast<const float4*>(a.rf),
                     a.z, a.rd, a.rd_stride, a.d_m_thres, a.n_thres, a.n_rays, a.n_samples, a.depth, a.acc, a.dex, reinterpret_cast<float4*>(br),
                     z_mid, a.nonfinite);
  return check_launch(who);
}

}  // namespace dn

using namespace dn;

extern "C" int dn_composite_density_brackets(const float* rf, const float* z, const float* rd, int rd_stride, const float* d_m_thres,
                                             int n_thres, int64_t n_rays, int n_samples, float* depth, float* acc, float* dex, float* br,
                                             float* z_mid, dn_stream_t stream) {
  return composite_brackets_counting({rf, z, rd, rd_stride, nullptr, 0.0f, d_m_thres, n_thres, n_rays, n_samples, depth, acc, dex}, br, z_mid,
                                     stream);
}

extern "C" int dn_density_resample(const float* rf, const float* z, const float* rd, int rd_stride, const float* noise,
                                   float noise_std, const float* u, int64_t n_rays, int num_coarse, int num_fine, float* depth,
                                   float* acc, float* z_fine, dn_stream_t stream) {
  return density_resample_counting(rf, z, rd, rd_stride, noise, noise_std, u, n_rays, num_coarse, num_fine, depth, acc, z_fine, nullptr, stream);
}

extern "C" int dn_composite_density(const float* rf, const float* z, const float* rd, int rd_stride, const float* noise,
                                    float noise_std, const float* d_m_thres, int n_thres, int64_t n_rays, int n_samples,
                                    float* depth, float* acc, float* dex, dn_stream_t stream) {
  return composite_density_counting({rf, z, rd, rd_stride, noise, noise_std, d_m_thres, n_thres, n_rays, n_samples, depth, acc, dex}, stream);
}
