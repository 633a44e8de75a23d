// The loss heads of a training step (dn_mse2_loss, dn_render_loss, dn_render_loss_exposure: three instances of one kernel), the
// per-view reduction of the exposure rows' gradient (include/dexnerf_hip_exposure.h) and dn_rng_fill.  One-workgroup / elementwise
// kernels; compiled with -ffp-contract=off so plain mul/add sequences round like ATen's.
#include <cmath>
#include <type_traits>

#include "dn_common.h"
#include "dn_rng.h"
#include "../../include/dexnerf_hip_exposure.h"

namespace dn {
// The arguments of every loss head; an entry point leaves what it lacks at zero.  out: [loss, mse_c, mse_f], and behind them
// [D_c, D_f, M] from the general heads.
struct LossHeadArgs {
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
  float *out, *g_c, *g_f, *gd_c, *gd_f, *g_eps;
  uint32_t* rng_state;
};

constexpr int kExposureGradThreads = 1024;

__device__ __forceinline__ float loss_target_depth(const LossHeadArgs& a, int64_t i, int64_t view_base) {
  if (a.pixel_index == nullptr) return a.depth_src[i];
  const int64_t base = a.view_index != nullptr ? static_cast<int64_t>(a.view_index[i]) * a.hw : view_base;
  return a.depth_src[base + a.pixel_index[i]];
}

// the exposure row of ray i, or nullptr where the ray takes the uncorrected expressions: its view outside [0, V), or a row of zeros
__device__ __forceinline__ const float* exposure_row(const LossHeadArgs& a, int64_t i, int one_view) {
  const int v = a.view_index != nullptr ? a.view_index[i] : one_view;
  if (v < 0 || v >= a.n_views) return nullptr;
  const float* row = a.eps + static_cast<int64_t>(v) * a.p;
  bool zero = true;
  for (int j = 0; j < a.p; ++j) zero = zero && row[j] == 0.0f;
  return zero ? nullptr : row;
}

// exp(s a_k) of channel k: formed in fp64, rounded to fp32 once
__device__ __forceinline__ float exposure_gain(const LossHeadArgs& a, const float* row, int k) {
  return static_cast<float>(exp(static_cast<double>(a.scale) * static_cast<double>(row[a.p == 1 ? 0 : k])));
}

// c^_k: a multiply, then (affine rows) an add
__device__ __forceinline__ float exposure_apply(const LossHeadArgs& a, const float* row, int k, float gain, float c) {
  return a.p == 1 ? gain * c : gain * c + a.scale * row[3 + k];
}

// ---- The loss head on the device, its upstream gradients written where dn_render_rays_backward reads them, and the RNG state's
// iteration counter advanced.  One workgroup: per-lane partial sums in ray order, wave_sum, the waves through LDS in wave order
// (deterministic; n is a training batch, <= a few thousand rays).  No atomics.
//
// Every head: mse_c = mse(rgb_coarse, target), mse_f = mse(rgb_fine, target) (train_dexnerf_rgb.py:264-277; with `luminance` the IR
// head of train_nerf_ir.py:260-263: both sides through 0.299 r + 0.587 g + 0.114 b first).
// GENERAL (dn_render_loss): w_rgb_c mse_c + w_rgb_f mse_f + w_depth_c D_c + w_depth_f D_f, D_p the mean squared depth error over the
// M rays whose target depth d lies in (depth_lo, depth_hi) (a NaN d compares false: invalid).  d is read in place - depth_src[i], or
// gathered from (V, H W) depth maps at (view, pixel_index[i]) - so a depth-supervised step launches nothing more than a photometric
// one.  M is counted in the same pass (ballots, integers), published through LDS, and the depth gradients are written after the
// barrier.  Without it (dn_mse2_loss) the weights are not applied (w = 1 gives the same bits: x * 1.0f is exact) and `out` has 3 floats.
// EXPOSURE (dn_render_loss_exposure): c^ in the place of c in the colour terms of every ray that has a usable exposure row; the other
// rays - all of them without EXPOSURE - take the uncorrected expressions (not gain * c + 0: that loses the sign of a zero).
template <bool EXPOSURE, bool GENERAL>
__global__ __launch_bounds__(1024) void loss_head_kernel(const LossHeadArgs a) {
  __shared__ float part[GENERAL ? 4 : 2][16];
  __shared__ int count[GENERAL ? 16 : 1];
  const int64_t n = a.n;
  const float* src[2] = {a.rgb_c, a.rgb_f};
  float* dst[2] = {a.g_c, a.g_f};
  const float w[2] = {a.w_rgb_c, a.w_rgb_f};
  auto weighted = [&](int k, float x) { return GENERAL ? w[k] * x : x; };
  const int one_view = (EXPOSURE && a.view != nullptr) ? *a.view : 0;
  float sum[2] = {0.0f, 0.0f};
  if (a.luminance) {
    const float mix[3] = {0.299f, 0.587f, 0.114f};
    const float inv = 2.0f / static_cast<float>(n);
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      const float lt = (0.299f * a.target[i * 3] + 0.587f * a.target[i * 3 + 1]) + 0.114f * a.target[i * 3 + 2];
      const float* row = EXPOSURE ? exposure_row(a, i, one_view) : nullptr;
      float gain[3] = {1.0f, 1.0f, 1.0f};
      if (row != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gain[c] = exposure_gain(a, row, c);
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (src[k] == nullptr) continue;
        float c[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = row != nullptr ? exposure_apply(a, row, j, gain[j], src[k][i * 3 + j]) : src[k][i * 3 + j];
        const float d = ((0.299f * c[0] + 0.587f * c[1]) + 0.114f * c[2]) - lt;
        sum[k] += d * d;
        if (dst[k] == nullptr) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float g = weighted(k, inv * d * mix[j]);
          dst[k][i * 3 + j] = row != nullptr ? g * gain[j] : g;
        }
      }
    }
  } else {
    const float inv = 2.0f / static_cast<float>(3 * n);
    for (int64_t e = threadIdx.x; e < 3 * n; e += blockDim.x) {
      const float t = a.target[e];
      const int j = EXPOSURE ? static_cast<int>(e - 3 * (e / 3)) : 0;
      const float* row = EXPOSURE ? exposure_row(a, e / 3, one_view) : nullptr;
      // one element's terms; `corrected` (a type): its ray has a usable row - ONE branch per element, below, around both the coarse and
      // the fine term (a select per term is 7 % slower; the luminance loop selects: branching there costs four more SGPR spills)
      auto element_terms = [&](auto corrected) {
        constexpr bool kRow = decltype(corrected)::value;
        float gain = 1.0f;
        if constexpr (kRow) gain = exposure_gain(a, row, j);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (k == 1 && src[k] == nullptr) continue;   // (rgb_c is always given)
          const float d = (kRow ? exposure_apply(a, row, j, gain, src[k][e]) : src[k][e]) - t;
          sum[k] += d * d;
          if (dst[k] == nullptr) continue;
          const float g = weighted(k, inv * d);
          dst[k][e] = kRow ? g * gain : g;
        }
      };
      if (EXPOSURE && row != nullptr) element_terms(std::true_type{});
      else element_terms(std::false_type{});
    }
  }
  // the depth term: squared errors and the number of valid rays (the loop bound is uniform: every lane reaches the ballot)
  const bool depth = GENERAL && a.depth_src != nullptr;
  const int64_t view_base = (depth && a.view != nullptr) ? static_cast<int64_t>(*a.view) * a.hw : 0;
  float dc_sum = 0.0f, df_sum = 0.0f;
  int valid_rays = 0;
  if (depth) {
    for (int64_t base = 0; base < n; base += blockDim.x) {
      const int64_t i = base + threadIdx.x;
      bool valid = false;
      if (i < n) {
        const float d = loss_target_depth(a, i, view_base);
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
  const int wave = threadIdx.x >> 6;
  const int waves = static_cast<int>(blockDim.x >> 6);
  const float sc = wave_sum(sum[0]), sf = wave_sum(sum[1]);
  if constexpr (GENERAL) { dc_sum = wave_sum(dc_sum); df_sum = wave_sum(df_sum); }
  if ((threadIdx.x & 63) == 0) {
    part[0][wave] = sc; part[1][wave] = sf;
    if constexpr (GENERAL) { part[2][wave] = dc_sum; part[3][wave] = df_sum; count[wave] = valid_rays; }
  }
  __syncthreads();
  int m = 0;
  if constexpr (GENERAL) {
    for (int wv = 0; wv < waves; ++wv) m += count[wv];
  }
  const float m_div = static_cast<float>(m > 1 ? m : 1);
  if (depth && (a.gd_c != nullptr || a.gd_f != nullptr)) {
    const float inv = 2.0f / m_div;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      const float d = loss_target_depth(a, i, view_base);
      const bool valid = d > a.depth_lo && d < a.depth_hi;
      if (a.gd_c != nullptr) a.gd_c[i] = valid ? a.w_depth_c * (inv * (a.depth_c[i] - d)) : 0.0f;
      if (a.gd_f != nullptr && a.depth_f != nullptr) a.gd_f[i] = valid ? a.w_depth_f * (inv * (a.depth_f[i] - d)) : 0.0f;
    }
  }
  if (threadIdx.x == 0) {
    float s[GENERAL ? 4 : 2] = {};
    for (int wv = 0; wv < waves; ++wv) {
#pragma unroll
      for (int k = 0; k < (GENERAL ? 4 : 2); ++k) s[k] += part[k][wv];
    }
    const float denom = static_cast<float>(a.luminance ? n : 3 * n);
    const float mse_c = s[0] / denom, mse_f = s[1] / denom;
    float loss = weighted(0, mse_c) + weighted(1, mse_f);
    if constexpr (GENERAL) {
      const float d_c = s[2] / m_div, d_f = s[3] / m_div;
      if (depth) loss = loss + (a.w_depth_c * d_c + a.w_depth_f * d_f);
      a.out[3] = d_c; a.out[4] = d_f; a.out[5] = static_cast<float>(m);
    }
    a.out[0] = loss; a.out[1] = mse_c; a.out[2] = mse_f;
    if (a.rng_state != nullptr) a.rng_state[3] = a.rng_state[2] + 1u;   // the next iteration's counter (dn_rng.h)
  }
}

// Workgroup v forms g_eps[v]: it walks the rays in camera_grad_views_kernel's stride order (one workgroup per view: i = thread, thread +
// 1024, ...) and adds, in fp64, the terms of those of view v; wave_sum's butterfly, the waves through LDS in wave order, one rounding to
// fp32.  acc[0:3] = d/da_k, acc[3:6] = d/db_k; "gain" rows store acc[0] + acc[1] + acc[2].  A masked view and a view without a ray: +0.
// 1024 threads: the walk is latency-bound (every workgroup reads all n view indices), a batch of 4096 rays is four trips of the loop.
__global__ __launch_bounds__(kExposureGradThreads) void exposure_grad_kernel(const LossHeadArgs a) {
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


__global__ void rng_fill_kernel(const uint32_t* __restrict__ state, uint32_t stream, int64_t n, int normal, float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const RngRef r{state, stream};
  out[i] = normal ? rng_normal(r, static_cast<uint64_t>(i)) : rng_uniform(r, static_cast<uint64_t>(i));
}
}  // namespace dn

using namespace dn;

extern "C" int dn_rng_fill(const uint32_t* rng_state, uint32_t stream_id, int64_t n, int normal, float* out, dn_stream_t stream) {
  if (n == 0) return 0;
  DN_REQUIRE(rng_state && out && n >= 0, "dn_rng_fill: bad arguments");
  hipLaunchKernelGGL(rng_fill_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, as_stream(stream), rng_state, stream_id, n, normal, out);
  return check_launch("dn_rng_fill");
}

extern "C" int dn_mse2_loss(const float* rgb_coarse, const float* rgb_fine, const float* target, int64_t n_rays, int luminance,
                            float* loss3, float* g_rgb_coarse, float* g_rgb_fine, uint32_t* rng_state, dn_stream_t stream) {
  DN_REQUIRE(rgb_coarse && target && loss3 && n_rays >= 1, "dn_mse2_loss: bad arguments");
  LossHeadArgs args{};
  args.rgb_c = rgb_coarse; args.rgb_f = rgb_fine; args.target = target; args.n = n_rays; args.luminance = luminance;
  args.out = loss3; args.g_c = g_rgb_coarse; args.g_f = g_rgb_fine; args.rng_state = rng_state;
  hipLaunchKernelGGL((loss_head_kernel<false, false>), dim3(1), dim3(1024), 0, as_stream(stream), args);
  return check_launch("dn_mse2_loss");
}

// what the general heads ask of their arguments (`name`: the entry point, for messages)
static int check_render_loss(const char* name, const LossHeadArgs& a) {
  DN_REQUIRE(a.rgb_c && a.target && a.out && a.n >= 1, "%s: bad arguments (rgb_coarse, target, loss6 must be given, n_rays >= 1)", name);
  DN_REQUIRE(std::isfinite(a.w_rgb_c) && std::isfinite(a.w_rgb_f) && std::isfinite(a.w_depth_c) && std::isfinite(a.w_depth_f),
             "%s: the four weights must be finite", name);
  if (a.depth_src != nullptr) {
    DN_REQUIRE(a.depth_c != nullptr, "%s: a depth target needs depth_coarse", name);
    DN_REQUIRE(!std::isnan(a.depth_lo) && !std::isnan(a.depth_hi), "%s: depth_lo / depth_hi must not be NaN", name);
    DN_REQUIRE(a.n <= (1LL << 24), "%s: the valid-ray count is reported as a float (n_rays <= 2^24 with a depth target)", name);
    DN_REQUIRE(a.pixel_index == nullptr || a.hw >= 1, "%s: gathered depth targets need hw = H W >= 1", name);
  }
  DN_REQUIRE(a.pixel_index == nullptr || a.depth_src != nullptr, "%s: pixel_index without depth_src", name);
  return 0;
}

extern "C" int dn_render_loss(const float* rgb_coarse, const float* rgb_fine, const float* target, const float* depth_coarse,
                              const float* depth_fine, const float* depth_src, const int64_t* pixel_index, const int32_t* view_index,
                              const int32_t* view, int64_t hw, int64_t n_rays, int luminance, float w_rgb_coarse, float w_rgb_fine,
                              float w_depth_coarse, float w_depth_fine, float depth_lo, float depth_hi, float* loss6, float* g_rgb_coarse,
                              float* g_rgb_fine, float* g_depth_coarse, float* g_depth_fine, uint32_t* rng_state, dn_stream_t stream) {
  const LossHeadArgs args{rgb_coarse, rgb_fine, target, depth_coarse, depth_fine, depth_src, pixel_index, view_index, view, hw, n_rays, luminance,
                          w_rgb_coarse, w_rgb_fine, w_depth_coarse, w_depth_fine, depth_lo, depth_hi, nullptr, 0, 0, 0.0f, nullptr, loss6,
                          g_rgb_coarse, g_rgb_fine, g_depth_coarse, g_depth_fine, nullptr, rng_state};
  if (const int rc = check_render_loss("dn_render_loss", args)) return rc;
  DN_REQUIRE((view_index == nullptr && view == nullptr) || pixel_index != nullptr, "dn_render_loss: view_index / view without pixel_index");
  hipLaunchKernelGGL((loss_head_kernel<false, true>), dim3(1), dim3(1024), 0, as_stream(stream), args);
  return check_launch("dn_render_loss");
}

extern "C" int dn_render_loss_exposure(const float* rgb_coarse, const float* rgb_fine, const float* target, const float* depth_coarse,
                                       const float* depth_fine, const float* depth_src, const int64_t* pixel_index, const int32_t* view_index,
                                       const int32_t* view, int64_t hw, int64_t n_rays, int luminance, float w_rgb_coarse, float w_rgb_fine,
                                       float w_depth_coarse, float w_depth_fine, float depth_lo, float depth_hi, const float* eps, int P,
                                       int n_views, float exposure_scale, const int32_t* view_mask, float* loss6, float* g_rgb_coarse,
                                       float* g_rgb_fine, float* g_depth_coarse, float* g_depth_fine, float* g_eps, uint32_t* rng_state,
                                       dn_stream_t stream) {
  const LossHeadArgs args{rgb_coarse, rgb_fine, target, depth_coarse, depth_fine, depth_src, pixel_index, view_index, view, hw, n_rays,
                          luminance, w_rgb_coarse, w_rgb_fine, w_depth_coarse, w_depth_fine, depth_lo, depth_hi, eps, P, n_views,
                          exposure_scale, view_mask, loss6, g_rgb_coarse, g_rgb_fine, g_depth_coarse, g_depth_fine, g_eps, rng_state};
  if (const int rc = check_render_loss("dn_render_loss_exposure", args)) return rc;
  DN_REQUIRE(eps != nullptr, "dn_render_loss_exposure: the exposure rows must be given");
  DN_REQUIRE(P == 1 || P == 6, "dn_render_loss_exposure: P is 1 (gain) or 6 (affine) (got %d)", P);
  DN_REQUIRE(n_views >= 1 && n_views <= 65535, "dn_render_loss_exposure: n_views must be in [1, 65535]");
  DN_REQUIRE(std::isfinite(exposure_scale) && exposure_scale > 0.0f, "dn_render_loss_exposure: exposure_scale must be finite and > 0");
  hipLaunchKernelGGL((loss_head_kernel<true, true>), dim3(1), dim3(1024), 0, as_stream(stream), args);
  if (g_eps != nullptr) {
    const int rc = check_launch("dn_render_loss_exposure");
    if (rc != 0) return rc;
    hipLaunchKernelGGL(exposure_grad_kernel, dim3(static_cast<unsigned>(n_views)), dim3(kExposureGradThreads), 0, as_stream(stream), args);
  }
  return check_launch("dn_render_loss_exposure");
}
