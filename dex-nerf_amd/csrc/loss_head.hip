// The loss heads of a training step (dn_mse2_loss, dn_render_loss) and dn_rng_fill.  One-workgroup / elementwise kernels; compiled with
// -ffp-contract=off so plain mul/add sequences round like ATen's.
#include "dn_common.h"
#include "dn_rng.h"

// ---- S9 loss head on the device: mse(rgb_coarse, target) + mse(rgb_fine, target) (train_dexnerf_rgb.py:264-277; with
// `luminance` the IR head of train_nerf_ir.py:260-263: both sides through 0.299 r + 0.587 g + 0.114 b first), the upstream
// gradients of the two rgb maps written where dn_render_rays_backward reads them, and the RNG state's iteration counter advanced.
// One workgroup: the sums are formed in a fixed order (deterministic); n is a training batch (<= a few thousand rays).
namespace dn {
__global__ __launch_bounds__(1024) void mse2_loss_kernel(const float* __restrict__ rgb_c, const float* __restrict__ rgb_f,
                                                         const float* __restrict__ target, int64_t n, int luminance,
                                                         float* __restrict__ out3, float* __restrict__ g_c, float* __restrict__ g_f,
                                                         uint32_t* __restrict__ rng_state) {
  __shared__ float part[2][16];
  float sc = 0.0f, sf = 0.0f;
  if (luminance) {
    const float inv = 2.0f / static_cast<float>(n);
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      const float lt = (0.299f * target[i * 3] + 0.587f * target[i * 3 + 1]) + 0.114f * target[i * 3 + 2];
      const float* src[2] = {rgb_c, rgb_f};
      float* dst[2] = {g_c, g_f};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (src[k] == nullptr) continue;
        const float d = ((0.299f * src[k][i * 3] + 0.587f * src[k][i * 3 + 1]) + 0.114f * src[k][i * 3 + 2]) - lt;
        (k ? sf : sc) += d * d;
        if (dst[k] != nullptr) { dst[k][i * 3] = inv * d * 0.299f; dst[k][i * 3 + 1] = inv * d * 0.587f; dst[k][i * 3 + 2] = inv * d * 0.114f; }
      }
    }
  } else {
    const float inv = 2.0f / static_cast<float>(3 * n);
    for (int64_t e = threadIdx.x; e < 3 * n; e += blockDim.x) {
      const float t = target[e];
      const float dc = rgb_c[e] - t;
      sc += dc * dc;
      if (g_c != nullptr) g_c[e] = inv * dc;
      if (rgb_f != nullptr) {
        const float df = rgb_f[e] - t;
        sf += df * df;
        if (g_f != nullptr) g_f[e] = inv * df;
      }
    }
  }
  sc = wave_sum(sc); sf = wave_sum(sf);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[0][wave] = sc; part[1][wave] = sf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.0f, b = 0.0f;
    for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) { a += part[0][w]; b += part[1][w]; }
    const float denom = static_cast<float>(luminance ? n : 3 * n);
    out3[1] = a / denom; out3[2] = b / denom; out3[0] = a / denom + b / denom;
    if (rng_state != nullptr) rng_state[3] = rng_state[2] + 1u;   // the next iteration's counter (dn_rng.h)
  }
}

// ---- the general loss head: w_rgb_c mse_c + w_rgb_f mse_f + w_depth_c D_c + w_depth_f D_f, D_p the mean squared depth error over the
// M rays whose target depth d lies in (depth_lo, depth_hi) (a NaN d compares false: invalid).  d is read in place - depth_src[i], or
// gathered from (V, H W) depth maps at (view, pixel_index[i]) - so a depth-supervised step launches nothing more than a photometric
// one.  The colour sums and gradients are mse2_loss_kernel's expressions in its order (w = 1: the same bits; x * 1.0f is exact).
// One workgroup like mse2_loss_kernel: per-lane partial sums in ray order, wave_sum, the waves through LDS in wave order; M is counted
// in the same pass (ballots, integers), published through LDS, and the depth gradients are written after the barrier.  No atomics.
struct RenderLossArgs {
  const float *rgb_c, *rgb_f, *target, *depth_c, *depth_f, *depth_src;
  const int64_t* pixel_index;
  const int32_t *view_index, *view;
  int64_t hw, n;
  int luminance;
  float w_rgb_c, w_rgb_f, w_depth_c, w_depth_f, depth_lo, depth_hi;
  float *out6, *g_c, *g_f, *gd_c, *gd_f;
  uint32_t* rng_state;
};

__device__ __forceinline__ float loss_target_depth(const RenderLossArgs& a, int64_t i, int64_t view_base) {
  if (a.pixel_index == nullptr) return a.depth_src[i];
  const int64_t base = a.view_index != nullptr ? static_cast<int64_t>(a.view_index[i]) * a.hw : view_base;
  return a.depth_src[base + a.pixel_index[i]];
}

__global__ __launch_bounds__(1024) void render_loss_kernel(const RenderLossArgs a) {
  __shared__ float part[4][16];
  __shared__ int count[16];
  const int64_t n = a.n;
  const float wc = a.w_rgb_c, wf = a.w_rgb_f;
  float sc = 0.0f, sf = 0.0f;
  if (a.luminance) {
    const float inv = 2.0f / static_cast<float>(n);
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      const float lt = (0.299f * a.target[i * 3] + 0.587f * a.target[i * 3 + 1]) + 0.114f * a.target[i * 3 + 2];
      const float* src[2] = {a.rgb_c, a.rgb_f};
      float* dst[2] = {a.g_c, a.g_f};
      const float w[2] = {wc, wf};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (src[k] == nullptr) continue;
        const float d = ((0.299f * src[k][i * 3] + 0.587f * src[k][i * 3 + 1]) + 0.114f * src[k][i * 3 + 2]) - lt;
        (k ? sf : sc) += d * d;
        if (dst[k] != nullptr) {
          dst[k][i * 3] = w[k] * (inv * d * 0.299f); dst[k][i * 3 + 1] = w[k] * (inv * d * 0.587f); dst[k][i * 3 + 2] = w[k] * (inv * d * 0.114f);
        }
      }
    }
  } else {
    const float inv = 2.0f / static_cast<float>(3 * n);
    for (int64_t e = threadIdx.x; e < 3 * n; e += blockDim.x) {
      const float t = a.target[e];
      const float dc = a.rgb_c[e] - t;
      sc += dc * dc;
      if (a.g_c != nullptr) a.g_c[e] = wc * (inv * dc);
      if (a.rgb_f != nullptr) {
        const float df = a.rgb_f[e] - t;
        sf += df * df;
        if (a.g_f != nullptr) a.g_f[e] = wf * (inv * df);
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
      const float d = loss_target_depth(a, i, view_base);
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
  hipLaunchKernelGGL(mse2_loss_kernel, dim3(1), dim3(1024), 0, as_stream(stream), rgb_coarse, rgb_fine, target, n_rays, luminance, loss3,
                     g_rgb_coarse, g_rgb_fine, rng_state);
  return check_launch("dn_mse2_loss");
}

extern "C" int dn_render_loss(const float* rgb_coarse, const float* rgb_fine, const float* target, const float* depth_coarse,
                              const float* depth_fine, const float* depth_src, const int64_t* pixel_index, const int32_t* view_index,
                              const int32_t* view, int64_t hw, int64_t n_rays, int luminance, float w_rgb_coarse, float w_rgb_fine,
                              float w_depth_coarse, float w_depth_fine, float depth_lo, float depth_hi, float* loss6, float* g_rgb_coarse,
                              float* g_rgb_fine, float* g_depth_coarse, float* g_depth_fine, uint32_t* rng_state, dn_stream_t stream) {
  DN_REQUIRE(rgb_coarse && target && loss6 && n_rays >= 1, "dn_render_loss: bad arguments (rgb_coarse, target, loss6 must be given, n_rays >= 1)");
  DN_REQUIRE(std::isfinite(w_rgb_coarse) && std::isfinite(w_rgb_fine) && std::isfinite(w_depth_coarse) && std::isfinite(w_depth_fine),
             "dn_render_loss: the four weights must be finite");
  if (depth_src != nullptr) {
    DN_REQUIRE(depth_coarse != nullptr, "dn_render_loss: a depth target needs depth_coarse");
    DN_REQUIRE(!std::isnan(depth_lo) && !std::isnan(depth_hi), "dn_render_loss: depth_lo / depth_hi must not be NaN");
    DN_REQUIRE(n_rays <= (1LL << 24), "dn_render_loss: the valid-ray count is reported as a float (n_rays <= 2^24 with a depth target)");
    DN_REQUIRE(pixel_index == nullptr || hw >= 1, "dn_render_loss: gathered depth targets need hw = H W >= 1");
  }
  DN_REQUIRE(pixel_index == nullptr || depth_src != nullptr, "dn_render_loss: pixel_index without depth_src");
  DN_REQUIRE((view_index == nullptr && view == nullptr) || pixel_index != nullptr, "dn_render_loss: view_index / view without pixel_index");
  const RenderLossArgs args{rgb_coarse, rgb_fine, target, depth_coarse, depth_fine, depth_src, pixel_index, view_index, view, hw, n_rays, luminance,
                            w_rgb_coarse, w_rgb_fine, w_depth_coarse, w_depth_fine, depth_lo, depth_hi, loss6, g_rgb_coarse, g_rgb_fine,
                            g_depth_coarse, g_depth_fine, rng_state};
  hipLaunchKernelGGL(render_loss_kernel, dim3(1), dim3(1024), 0, as_stream(stream), args);
  return check_launch("dn_render_loss");
}
