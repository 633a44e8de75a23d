// dn_render_loss_exposure (include/dexnerf_hip_exposure.h): the general loss head with a per-view exposure correction of the rendered
// colours, and the per-view reduction of the exposure rows' gradient.  Compiled with -ffp-contract=off like loss_head.hip: with all-zero
// rows the head's sums and gradients are render_loss_kernel's expressions in its order, the same bits.
#include <cmath>

#include "dn_common.h"
#include "../../include/dexnerf_hip_exposure.h"

namespace dn {
struct ExposureLossArgs {
  const float *rgb_c, *rgb_f, *target, *depth_c, *depth_f, *depth_src;
  const int64_t* pixel_index;
  const int32_t *view_index, *view;
  int64_t hw, n;
  int luminance;
  float w_rgb_c, w_rgb_f, w_depth_c, w_depth_f, depth_lo, depth_hi;
  const float* eps;
  int p, n_views;
  float scale;
  const int32_t* view_mask;
  float *out6, *g_c, *g_f, *gd_c, *gd_f, *g_eps;
  uint32_t* rng_state;
};

constexpr int kExposureGradThreads = 1024;

__device__ __forceinline__ float exposure_target_depth(const ExposureLossArgs& a, int64_t i, int64_t view_base) {
  if (a.pixel_index == nullptr) return a.depth_src[i];
  const int64_t base = a.view_index != nullptr ? static_cast<int64_t>(a.view_index[i]) * a.hw : view_base;
  return a.depth_src[base + a.pixel_index[i]];
}

// the exposure row of ray i, or nullptr where the ray takes the uncorrected expressions: its view outside [0, V), or a row of zeros
__device__ __forceinline__ const float* exposure_row(const ExposureLossArgs& a, int64_t i, int one_view) {
  const int v = a.view_index != nullptr ? a.view_index[i] : one_view;
  if (v < 0 || v >= a.n_views) return nullptr;
  const float* row = a.eps + static_cast<int64_t>(v) * a.p;
  bool zero = true;
  for (int j = 0; j < a.p; ++j) zero = zero && row[j] == 0.0f;
  return zero ? nullptr : row;
}

// exp(s a_k) of channel k: formed in fp64, rounded to fp32 once
__device__ __forceinline__ float exposure_gain(const ExposureLossArgs& a, const float* row, int k) {
  return static_cast<float>(exp(static_cast<double>(a.scale) * static_cast<double>(row[a.p == 1 ? 0 : k])));
}

// c^_k: a multiply, then (affine rows) an add
__device__ __forceinline__ float exposure_apply(const ExposureLossArgs& a, const float* row, int k, float gain, float c) {
  return a.p == 1 ? gain * c : gain * c + a.scale * row[3 + k];
}

// render_loss_kernel (loss_head.hip) with c^ in the place of c in the colour terms: the same loops, sums and reductions in the same order;
// the depth term is its code unchanged.
__global__ __launch_bounds__(1024) void render_loss_exposure_kernel(const ExposureLossArgs a) {
  __shared__ float part[4][16];
  __shared__ int count[16];
  const int64_t n = a.n;
  const float wc = a.w_rgb_c, wf = a.w_rgb_f;
  const int one_view = a.view != nullptr ? *a.view : 0;
  float sc = 0.0f, sf = 0.0f;
  if (a.luminance) {
    const float inv = 2.0f / static_cast<float>(n);
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      const float lt = (0.299f * a.target[i * 3] + 0.587f * a.target[i * 3 + 1]) + 0.114f * a.target[i * 3 + 2];
      const float* src[2] = {a.rgb_c, a.rgb_f};
      float* dst[2] = {a.g_c, a.g_f};
      const float w[2] = {wc, wf};
      const float* row = exposure_row(a, i, one_view);
      float gain[3] = {1.0f, 1.0f, 1.0f};
      if (row != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gain[c] = exposure_gain(a, row, c);
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (src[k] == nullptr) continue;
        if (row == nullptr) {
          const float d = ((0.299f * src[k][i * 3] + 0.587f * src[k][i * 3 + 1]) + 0.114f * src[k][i * 3 + 2]) - lt;
          (k ? sf : sc) += d * d;
          if (dst[k] != nullptr) {
            dst[k][i * 3] = w[k] * (inv * d * 0.299f); dst[k][i * 3 + 1] = w[k] * (inv * d * 0.587f); dst[k][i * 3 + 2] = w[k] * (inv * d * 0.114f);
          }
        } else {
          const float r = exposure_apply(a, row, 0, gain[0], src[k][i * 3]), g = exposure_apply(a, row, 1, gain[1], src[k][i * 3 + 1]);
          const float b = exposure_apply(a, row, 2, gain[2], src[k][i * 3 + 2]);
          const float d = ((0.299f * r + 0.587f * g) + 0.114f * b) - lt;
          (k ? sf : sc) += d * d;
          if (dst[k] != nullptr) {
            dst[k][i * 3] = (w[k] * (inv * d * 0.299f)) * gain[0]; dst[k][i * 3 + 1] = (w[k] * (inv * d * 0.587f)) * gain[1];
            dst[k][i * 3 + 2] = (w[k] * (inv * d * 0.114f)) * gain[2];
          }
        }
      }
    }
  } else {
    const float inv = 2.0f / static_cast<float>(3 * n);
    for (int64_t e = threadIdx.x; e < 3 * n; e += blockDim.x) {
      const float t = a.target[e];
      const int64_t i = e / 3;
      const int k = static_cast<int>(e - 3 * i);
      const float* row = exposure_row(a, i, one_view);
      if (row == nullptr) {
        const float dc = a.rgb_c[e] - t;
        sc += dc * dc;
        if (a.g_c != nullptr) a.g_c[e] = wc * (inv * dc);
        if (a.rgb_f != nullptr) {
          const float df = a.rgb_f[e] - t;
          sf += df * df;
          if (a.g_f != nullptr) a.g_f[e] = wf * (inv * df);
        }
      } else {
        const float gain = exposure_gain(a, row, k);
        const float dc = exposure_apply(a, row, k, gain, a.rgb_c[e]) - t;
        sc += dc * dc;
        if (a.g_c != nullptr) a.g_c[e] = (wc * (inv * dc)) * gain;
        if (a.rgb_f != nullptr) {
          const float df = exposure_apply(a, row, k, gain, a.rgb_f[e]) - t;
          sf += df * df;
          if (a.g_f != nullptr) a.g_f[e] = (wf * (inv * df)) * gain;
        }
      }
    }
  }
  // the depth term: squared errors and the number of valid rays (the loop bound is uniform: every lane reaches the ballot)
  const bool depth = a.depth_src != nullptr;
  const int64_t view_base = (depth && a.view != nullptr) ? static_cast<int64_t>(*a.view) * a.hw : 0;
  float dc_sum = 0.0f, df_sum = 0.0f;
  int valid_rays = 0;
  if (depth) {
    for (int64_t base = 0; base < n; base += blockDim.x) {
      const int64_t i = base + threadIdx.x;
      bool valid = false;
      if (i < n) {
        const float d = exposure_target_depth(a, i, view_base);
        valid = d > a.depth_lo && d < a.depth_hi;
        if (valid) {
          const float ec = a.depth_c[i] - d;
          dc_sum += ec * ec;
          if (a.depth_f != nullptr) {
            const float ef = a.depth_f[i] - d;
            df_sum += ef * ef;
          }
        }
      }
      valid_rays += __popcll(__ballot(valid));
    }
  }
  sc = wave_sum(sc); sf = wave_sum(sf);
  dc_sum = wave_sum(dc_sum); df_sum = wave_sum(df_sum);
  const int wave = threadIdx.x >> 6;
  const int waves = static_cast<int>(blockDim.x >> 6);
  if ((threadIdx.x & 63) == 0) {
    part[0][wave] = sc; part[1][wave] = sf; part[2][wave] = dc_sum; part[3][wave] = df_sum;
    count[wave] = valid_rays;
  }
  __syncthreads();
  int m = 0;
  for (int w = 0; w < waves; ++w) m += count[w];
  const float m_div = static_cast<float>(m > 1 ? m : 1);
  if (depth && (a.gd_c != nullptr || a.gd_f != nullptr)) {
    const float inv = 2.0f / m_div;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      const float d = exposure_target_depth(a, i, view_base);
      const bool valid = d > a.depth_lo && d < a.depth_hi;
      if (a.gd_c != nullptr) a.gd_c[i] = valid ? a.w_depth_c * (inv * (a.depth_c[i] - d)) : 0.0f;
      if (a.gd_f != nullptr && a.depth_f != nullptr) a.gd_f[i] = valid ? a.w_depth_f * (inv * (a.depth_f[i] - d)) : 0.0f;
    }
  }
  if (threadIdx.x == 0) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int w = 0; w < waves; ++w) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += part[k][w];
    }
    const float denom = static_cast<float>(a.luminance ? n : 3 * n);
    const float mse_c = s[0] / denom, mse_f = s[1] / denom;
    const float d_c = s[2] / m_div, d_f = s[3] / m_div;
    float loss = wc * mse_c + wf * mse_f;
    if (depth) loss = loss + (a.w_depth_c * d_c + a.w_depth_f * d_f);
    a.out6[0] = loss; a.out6[1] = mse_c; a.out6[2] = mse_f; a.out6[3] = d_c; a.out6[4] = d_f; a.out6[5] = static_cast<float>(m);
    if (a.rng_state != nullptr) a.rng_state[3] = a.rng_state[2] + 1u;   // the next iteration's counter (dn_rng.h)
  }
}

// Workgroup v forms g_eps[v]: it walks the rays in camera_grad_views_kernel's stride order (one workgroup per view: i = thread, thread +
// 1024, ...) and adds, in fp64, the terms of those of view v; wave_sum's butterfly, the waves through LDS in wave order, one rounding to
// fp32.  acc[0:3] = d/da_k, acc[3:6] = d/db_k; "gain" rows store acc[0] + acc[1] + acc[2].  A masked view and a view without a ray: +0.
// 1024 threads: the walk is latency-bound (every workgroup reads all n view indices), a batch of 4096 rays is four trips of the loop.
__global__ __launch_bounds__(kExposureGradThreads) void exposure_grad_kernel(const ExposureLossArgs a) {
  __shared__ double part[kExposureGradThreads / 64][6];
  const int v = static_cast<int>(blockIdx.x);
  float* out = a.g_eps + static_cast<int64_t>(v) * a.p;
  if (a.view_mask != nullptr && a.view_mask[v] == 0) {      // (uniform over the workgroup: nobody reaches the barrier)
    if (static_cast<int>(threadIdx.x) < a.p) out[threadIdx.x] = 0.0f;
    return;
  }
  const float* row = a.eps + static_cast<int64_t>(v) * a.p;
  const double s = static_cast<double>(a.scale);
  double gain[3], off[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gain[k] = exp(s * static_cast<double>(row[a.p == 1 ? 0 : k]));
    off[k] = a.p == 1 ? 0.0 : s * static_cast<double>(row[3 + k]);
  }
  const int one_view = a.view != nullptr ? *a.view : 0;
  const double mix[3] = {static_cast<double>(0.299f), static_cast<double>(0.587f), static_cast<double>(0.114f)};
  const double inv = 2.0 / static_cast<double>(a.luminance ? a.n : 3 * a.n);
  const float* src[2] = {a.rgb_c, a.rgb_f};
  const double w[2] = {static_cast<double>(a.w_rgb_c), static_cast<double>(a.w_rgb_f)};
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < a.n; i += kExposureGradThreads) {
    if ((a.view_index != nullptr ? a.view_index[i] : one_view) != v) continue;
    double t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = static_cast<double>(a.target[i * 3 + k]);
    double ray[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (src[p] == nullptr) continue;
      double c[3], d[3];      // d_k = c^_k - t_k
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        c[k] = static_cast<double>(src[p][i * 3 + k]);
        d[k] = (gain[k] * c[k] + off[k]) - t[k];
      }
      const double lum = (mix[0] * d[0] + mix[1] * d[1]) + mix[2] * d[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double dm = w[p] * (inv * (a.luminance ? lum * mix[k] : d[k]));     // w_p dmse_p / dc^_k
        ray[k] += dm * (s * gain[k] * c[k]);
        ray[3 + k] += dm * s;
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[j] += ray[j];
  }
  if (a.p == 1) acc[0] = (acc[0] + acc[1]) + acc[2];
  const int wave = threadIdx.x >> 6;
  for (int j = 0; j < a.p; ++j) {
    const double sum = wave_sum(acc[j]);
    if (lane_id() == 0) part[wave][j] = sum;
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < a.p) {
    double sum = part[0][threadIdx.x];
    for (int wv = 1; wv < kExposureGradThreads / 64; ++wv) sum += part[wv][threadIdx.x];
    out[threadIdx.x] = static_cast<float>(sum);
  }
}
}  // namespace dn

using namespace dn;

extern "C" int dn_render_loss_exposure(const float* rgb_coarse, const float* rgb_fine, const float* target, const float* depth_coarse,
                                       const float* depth_fine, const float* depth_src, const int64_t* pixel_index, const int32_t* view_index,
                                       const int32_t* view, int64_t hw, int64_t n_rays, int luminance, float w_rgb_coarse, float w_rgb_fine,
                                       float w_depth_coarse, float w_depth_fine, float depth_lo, float depth_hi, const float* eps, int P,
                                       int n_views, float exposure_scale, const int32_t* view_mask, float* loss6, float* g_rgb_coarse,
                                       float* g_rgb_fine, float* g_depth_coarse, float* g_depth_fine, float* g_eps, uint32_t* rng_state,
                                       dn_stream_t stream) {
  DN_REQUIRE(rgb_coarse && target && loss6 && n_rays >= 1,
             "dn_render_loss_exposure: bad arguments (rgb_coarse, target, loss6 must be given, n_rays >= 1)");
  DN_REQUIRE(std::isfinite(w_rgb_coarse) && std::isfinite(w_rgb_fine) && std::isfinite(w_depth_coarse) && std::isfinite(w_depth_fine),
             "dn_render_loss_exposure: the four weights must be finite");
  if (depth_src != nullptr) {
    DN_REQUIRE(depth_coarse != nullptr, "dn_render_loss_exposure: a depth target needs depth_coarse");
    DN_REQUIRE(!std::isnan(depth_lo) && !std::isnan(depth_hi), "dn_render_loss_exposure: depth_lo / depth_hi must not be NaN");
    DN_REQUIRE(n_rays <= (1LL << 24), "dn_render_loss_exposure: the valid-ray count is reported as a float (n_rays <= 2^24 with a depth target)");
    DN_REQUIRE(pixel_index == nullptr || hw >= 1, "dn_render_loss_exposure: gathered depth targets need hw = H W >= 1");
  }
  DN_REQUIRE(pixel_index == nullptr || depth_src != nullptr, "dn_render_loss_exposure: pixel_index without depth_src");
  DN_REQUIRE(eps != nullptr, "dn_render_loss_exposure: the exposure rows must be given");
  DN_REQUIRE(P == 1 || P == 6, "dn_render_loss_exposure: P is 1 (gain) or 6 (affine) (got %d)", P);
  DN_REQUIRE(n_views >= 1 && n_views <= 65535, "dn_render_loss_exposure: n_views must be in [1, 65535]");
  DN_REQUIRE(std::isfinite(exposure_scale) && exposure_scale > 0.0f, "dn_render_loss_exposure: exposure_scale must be finite and > 0");
  const ExposureLossArgs args{rgb_coarse, rgb_fine, target, depth_coarse, depth_fine, depth_src, pixel_index, view_index, view, hw, n_rays,
                              luminance, w_rgb_coarse, w_rgb_fine, w_depth_coarse, w_depth_fine, depth_lo, depth_hi, eps, P, n_views,
                              exposure_scale, view_mask, loss6, g_rgb_coarse, g_rgb_fine, g_depth_coarse, g_depth_fine, g_eps, rng_state};
  hipLaunchKernelGGL(render_loss_exposure_kernel, dim3(1), dim3(1024), 0, as_stream(stream), args);
  if (g_eps != nullptr) {
    const int rc = check_launch("dn_render_loss_exposure");
    if (rc != 0) return rc;
    hipLaunchKernelGGL(exposure_grad_kernel, dim3(static_cast<unsigned>(n_views)), dim3(kExposureGradThreads), 0, as_stream(stream), args);
  }
  return check_launch("dn_render_loss_exposure");
}
