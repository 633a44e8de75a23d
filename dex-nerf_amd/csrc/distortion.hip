// The distortion regulariser of mip-NeRF 360 (Barron et al. 2022, eq. 15) on the weights and depths of the compositing kernels:
//   L_ray = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i
// with compositing's own intervals: m_i = (z_i + z_{i+1}) / 2, delta_i = z_{i+1} - z_i; the last sample's interval (the constant 1e10 in
// compositing) is degenerate here: m_{S-1} = z_{S-1}, delta_{S-1} = 0.  Both are scaled by k = 1 / (far - near) of the ray's own columns.
//
// Linear time by prefix sums over the sorted samples (W_<i = sum_{j<i} w_j, M_<i = sum_{j<i} w_j m_j, W_>i / M_>i likewise for j > i):
//   L_ray      = 2 sum_i w_i (m_i W_<i - M_<i) + (1/3) sum_i w_i^2 delta_i
//   dL/dw_i    = 2 [(m_i W_<i - M_<i) + (M_>i - m_i W_>i)] + (2/3) w_i delta_i
//   dL/dm_i    = 2 w_i (W_<i - W_>i) ;  dL/ddelta_i = w_i^2 / 3
//   dL/dz_s    = k [ (s < S-1 ? dm_s / 2 - ddelta_s : dm_s) + (s >= 1 ? dm_{s-1} / 2 + ddelta_{s-1} : 0) ]
// (where depths tie, |m_i - m_j| has no derivative: this is the subgradient of the sorted order).  L_ray depends on depth differences
// only, so near drops out; the span far - near is a normalisation constant and gets no gradient.  A ray without far > near gives zeros.
//
// One wave64 per ray, sample s = 64*chunk + lane as in composite.hip: every wave instruction reads or writes one coalesced run of the
// row.  The four running sums are fp64 wave scans with a carry between the chunks; W_> and M_> are the totals minus the prefixes (fp64:
// the cancellation stays ~1e-16 of the totals).  Inputs are fp32, every output is rounded to fp32 once.  Plain vector stores, no atomics;
// the mean over the rays is a second, one-workgroup kernel over the per-ray fp64 values in a fixed order, so two runs give the same bits.
// HBM- or launch-bound: 8 B/sample in, 4 (g_weights) to 8 (+ g_z; 12 with the read of accumulate mode) B/sample out.
#include <cmath>

#include "../../include/dexnerf_hip_ext.h"
#include "dn_common.h"

namespace dn {

constexpr int kDistRaysPerBlock = 4;   // 256 threads

template <int MAXC>
__global__ __launch_bounds__(256) void distortion_kernel(const float* __restrict__ weights, const float* __restrict__ z,
                                                         const float* __restrict__ near_far, int stride, int64_t n_rays, int S, float scale,
                                                         float* __restrict__ g_weights, float* __restrict__ g_z, int accumulate_z,
                                                         double* __restrict__ ray_loss) {
  const int lane = lane_id();
  const int64_t ray = static_cast<int64_t>(blockIdx.x) * kDistRaysPerBlock + (threadIdx.x >> 6);
  if (ray >= n_rays) return;   // wave-uniform exit; no block-level sync in this kernel
  const float near = near_far[ray * stride], far = near_far[ray * stride + 1];
  const bool live = far > near;   // (false for a NaN too)
  const double k = live ? 1.0 / (static_cast<double>(far) - static_cast<double>(near)) : 0.0;
  const float* wr = weights + ray * S;
  const float* zr = z + ray * S;

  float w_[MAXC], z0_[MAXC], z1_[MAXC];
  double wlt_[MAXC], mlt_[MAXC];
  double carry_w = 0.0, carry_m = 0.0;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int s = c * 64 + lane;
    const bool valid = s < S;
    const int sc = valid ? s : S - 1;
    const float w = valid ? wr[sc] : 0.0f;
    const float z0 = zr[sc];
    const float z1 = (sc + 1 < S) ? zr[sc + 1] : z0;   // the last sample: m = z, delta = 0
    w_[c] = w; z0_[c] = z0; z1_[c] = z1;
    const double m = 0.5 * (static_cast<double>(z0) + static_cast<double>(z1)) * k;
    const double wd = static_cast<double>(w);
    const double incl_w = wave_scan_add(wd), incl_m = wave_scan_add(wd * m);
    wlt_[c] = carry_w + wave_shift_up1(incl_w, 0.0);
    mlt_[c] = carry_m + wave_shift_up1(incl_m, 0.0);
    carry_w += wave_last(incl_w);
    carry_m += wave_last(incl_m);
  }
  // second pass, ascending: the values, and the previous sample's share of dL/dz (lane 63 of the chunk before as the carry)
  double loss = 0.0, prev_last = 0.0;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int s = c * 64 + lane;
    const bool valid = s < S;
    const double w = static_cast<double>(w_[c]);
    const double z0 = static_cast<double>(z0_[c]), z1 = static_cast<double>(z1_[c]);
    const double m = 0.5 * (z0 + z1) * k, delta = (z1 - z0) * k;
    const double wlt = wlt_[c], mlt = mlt_[c];
    const double wgt = (carry_w - wlt) - w, mgt = (carry_m - mlt) - w * m;
    const double before = m * wlt - mlt, after = mgt - m * wgt;
    loss += w * (2.0 * before) + (w * w) * delta * (1.0 / 3.0);
    const double gw = 2.0 * (before + after) + (2.0 / 3.0) * w * delta;
    const double dm = 2.0 * w * (wlt - wgt), dd = (w * w) * (1.0 / 3.0);
    const bool last = s == S - 1;
    const double to_next = (valid && !last) ? 0.5 * dm + dd : 0.0;
    const double prev = wave_shift_up1(to_next, prev_last);
    prev_last = wave_last(to_next);
    if (valid) {
      const int64_t at = ray * S + s;
      g_weights[at] = live ? static_cast<float>(static_cast<double>(scale) * gw) : 0.0f;
      if (g_z != nullptr) {
        const double own = last ? dm : 0.5 * dm - dd;
        const float g = live ? static_cast<float>(static_cast<double>(scale) * k * (own + prev)) : 0.0f;
        g_z[at] = accumulate_z ? g_z[at] + g : g;
      }
    }
  }
  loss = wave_sum(loss);
  if (lane == 0) ray_loss[ray] = live ? loss : 0.0;
}

// the mean of the per-ray values: one workgroup, lane-strided fp64 partial sums in ray order, wave_sum, the waves through LDS in wave order
__global__ __launch_bounds__(1024) void distortion_mean_kernel(const double* __restrict__ ray_loss, int64_t n_rays, float* __restrict__ mean) {
  __shared__ double part[16];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n_rays; i += blockDim.x) s += ray_loss[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) total += part[w];
    *mean = static_cast<float>(total / static_cast<double>(n_rays));
  }
}

using DistortionKernel = decltype(&distortion_kernel<1>);

static DistortionKernel distortion_instance(int chunks) {
  if (chunks <= 1) return distortion_kernel<1>;
  if (chunks <= 2) return distortion_kernel<2>;
  if (chunks <= 4) return distortion_kernel<4>;
  if (chunks <= 8) return distortion_kernel<8>;
  return distortion_kernel<16>;
}

}  // namespace dn

using namespace dn;

extern "C" int dn_distortion_loss(const float* weights, const float* z, const float* near_far, int stride, int64_t n_rays, int n_samples,
                                  float scale, float* g_weights, float* g_z, int accumulate_z, double* ray_loss, float* mean_loss,
                                  dn_stream_t stream) {
  if (n_rays == 0) return 0;
  // every argument is judged before any GPU work
  DN_REQUIRE(weights && z && near_far && g_weights && ray_loss && mean_loss && n_rays >= 0,
             "dn_distortion_loss: bad arguments (weights, z, near_far, g_weights, ray_loss, mean_loss must be given, n_rays >= 0)");
  DN_REQUIRE(n_samples >= 1 && n_samples <= 1024, "dn_distortion_loss: 1 to 1024 samples per ray (got %d)", n_samples);
  DN_REQUIRE(stride >= 2, "dn_distortion_loss: near_far stride must be >= 2 (near, far per ray)");
  DN_REQUIRE(std::isfinite(scale), "dn_distortion_loss: scale must be finite");
  const unsigned grid = static_cast<unsigned>((n_rays + kDistRaysPerBlock - 1) / kDistRaysPerBlock);
  hipLaunchKernelGGL(distortion_instance((n_samples + 63) / 64), dim3(grid), dim3(256), 0, as_stream(stream), weights, z, near_far, stride,
                     n_rays, n_samples, scale, g_weights, g_z, accumulate_z, ray_loss);
  int rc = check_launch("dn_distortion_loss");
  if (rc) return rc;
  hipLaunchKernelGGL(distortion_mean_kernel, dim3(1), dim3(1024), 0, as_stream(stream), ray_loss, n_rays, mean_loss);
  return check_launch("dn_distortion_loss");
}
