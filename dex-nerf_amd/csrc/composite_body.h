// The forward compositing of ONE ray by one wave (volume_render_radiance_field, reference nerf/volume_rendering_utils.py:6-70).
// forward_ray is the one chunk loop: the sample terms, the fp64 transmittance scan, expected depth, accumulation, the non-finite
// count and the Dex first-crossing depths.  Its clients add their own sums through its per-sample hook and finish in their own epilogue:
//   composite_ray            colour, disparity, the weights map - composite_fwd_kernel (composite.hip: raw rows from HBM) and the
//                            fused network kernel's epilogue (mlp_fused48_kernel.h: the rows the wave tile has just staged in LDS)
//   the sigma-only kernels   composite_density.hip, composite_quantile.hip (forward_ray's Quantiles<> argument), composite_normals.hip
// One body, so for the same sigma and depths every client's depth / acc / weights / dex carry the same bits.  What differs between
// the clients is passed as types (the row accessor, the noise source, the threshold source): none of it is decided at run time.
#pragma once
#include "dn_common.h"
#include "dn_rng.h"
#include <type_traits>

namespace dn {

constexpr int kMaxThres = 64;

struct ThresArgs {
  float m[kMaxThres];
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

struct SampleTerms {
  float sigma, alpha, one_m_alpha, dist;
};

// relu(raw sigma + noise): what the Dex thresholds are compared with
__device__ __forceinline__ float sample_sigma(float raw_sigma, float noise, float noise_std) {
  float raw = raw_sigma;
  if (noise_std > 0.0f) raw = raw + noise * noise_std;
  return fmaxf(raw, 0.0f);
}

__device__ __forceinline__ SampleTerms sample_terms(float raw_sigma, float noise, float noise_std, float z0, float z1,
                                                    bool last, float rd_norm) {
  SampleTerms t;
  t.sigma = sample_sigma(raw_sigma, noise, noise_std);
  t.dist = (last ? 1e10f : (z1 - z0)) * rd_norm;
  t.alpha = 1.0f - expf(-t.sigma * t.dist);
  t.one_m_alpha = (1.0f - t.alpha) + 1e-10f;
  return t;
}

// Where the density noise of sample sc of `ray` comes from (std: its scale; 0: none).  TensorNoise: an (N,S) tensor, or nothing.
// DrawnNoise: a tensor; without one the in-kernel draw, a pure function of (seed, iteration, stream, element), so a backward
// regenerates the forward's.
struct TensorNoise {
  const float* noise;
  float std;
  int64_t ray;
  int S;
  __device__ float operator()(int sc) const { return (std > 0.0f && noise != nullptr) ? noise[ray * S + sc] : 0.0f; }
};
struct DrawnNoise {
  const float* noise;
  RngRef rng;
  float std;
  int64_t ray;
  int S;
  __device__ float operator()(int sc) const {
    if (!(std > 0.0f)) return 0.0f;
    if (noise != nullptr) return noise[ray * S + sc];
    return rng.state != nullptr ? rng_normal(rng, static_cast<uint64_t>(ray) * S + sc) : 0.0f;
  }
};

// One 64-sample chunk of the transmittance T_s = prod_{j < s} (1 - alpha_j + 1e-10) and the weight alpha_s T_s: a wave-level fp64
// scan with `carry` (the product over the chunks before) - the reference's cumprod accumulates in fp64 and rounds each prefix to fp32,
// rolled by one, [0] = 1.
struct ScanStep {
  float trans, w;
};
__device__ __forceinline__ ScanStep transmittance_step(float alpha, float one_m_alpha, bool valid, int s, double& carry) {
  const double f = valid ? static_cast<double>(one_m_alpha) : 1.0;
  const double incl = wave_scan_mul(f) * carry;
  const double excl = wave_shift_up1(incl, carry);
  carry = wave_last(incl);
  ScanStep r;
  r.trans = (s == 0) ? 1.0f : static_cast<float>(excl);
  r.w = valid ? alpha * r.trans : 0.0f;
  return r;
}

// what the fused network kernel needs to composite the rays it has finished (FwdParams::comp; rgb == NULL: not requested)
struct CompParams {
  float* rgb; float* disp; float* acc; float* weights; float* depth; float* dex;
  unsigned* nonfinite;
  int64_t n_rays;
  int n_thres, white;
  ThresArgs th;
};

// one dword / one double of lane `src` (wave-uniform) as a wave-uniform value
__device__ __forceinline__ float read_lane(float v, int src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}
__device__ __forceinline__ double read_lane(double v, int src) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<unsigned>(b)), src));
  const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<unsigned>(b >> 32)), src));
  return __builtin_bit_cast(double, (static_cast<unsigned long long>(hi) << 32) | lo);
}

// ---- what forward_ray's clients choose, as types ----
// The raw rows: raw_at(sc) returns the whole row (float4: colour clients) or its sigma alone (float); the non-finite probe is as wide
// as what was read.  x - x is 0 for every finite x and NaN for +-inf / NaN.
struct SigmaColumn {   // the .w of (S,4) rows in HBM
  const float* sig;
  __device__ explicit SigmaColumn(const float4* rows) : sig(reinterpret_cast<const float*>(rows) + 3) {}
  __device__ float operator()(int sc) const { return sig[4 * sc]; }
};
__device__ __forceinline__ float raw_sigma(float raw) { return raw; }
__device__ __forceinline__ float raw_sigma(float4 raw) { return raw.w; }
__device__ __forceinline__ float finite_probe(float raw) { return raw - raw; }
__device__ __forceinline__ float finite_probe(float4 raw) { return ((raw.x - raw.x) + (raw.y - raw.y)) + ((raw.z - raw.z) + (raw.w - raw.w)); }

// The Dex thresholds; lane k of a wave tracks threshold 64 g + k of group g, and at(m_lane, k) is threshold k of the group as a
// wave-uniform value.  HostThres: at most kMaxThres of them in the kernel arguments, one group.  DeviceThres: any count in device
// memory; a lane keeps its own in a register (lane_value) and the others read it from there.
struct HostThres {
  static constexpr bool kGroups = false;
  const ThresArgs& th;
  int n;
  __device__ float lane_value(int, int, int) const { return 0.0f; }
  __device__ float at(float, int k) const { return th.m[k]; }
};
struct DeviceThres {
  static constexpr bool kGroups = true;
  const float* d;
  int n;
  __device__ float lane_value(int first, int kn, int lane) const { return (lane < kn) ? d[first + lane] : 0.0f; }
  __device__ float at(float m_lane, int k) const { return read_lane(m_lane, k); }
};

struct NoFirstHook {};   // forward_ray without the first-crossing hook
struct NoQuantiles {};   // forward_ray without the opacity-quantile readout
struct NoQuantileHook {};

// The opacity-quantile readout of forward_ray (include/dexnerf_hip_quantile.h): d_q: n_q <= 64 quantiles in DEVICE memory - lane k of
// the wave tracks quantile k; qdepth (Q,N) or NULL; interp 0: z at the crossing sample, 1: the piecewise-linear CDF inversion.
// on_quantile(k, idx) - optional - is called by the lane that holds quantile k with the crossing index i(q_k) (-1: acc < q_k).
template <class OnQuantile = NoQuantileHook>
struct Quantiles {
  const float* d_q;
  int n_q, interp;
  float* qdepth;
  OnQuantile on_quantile;
};

// First crossings of one chunk for the kn thresholds of one group (volume_rendering_utils.py:51-58: the first sample whose sigma
// exceeds m_k, per threshold).  A ballot per threshold per chunk doubled the compositing kernel's time (346 vs 190 us for 160,000 x
// 192 samples, K = 20); most (chunk, threshold) pairs cannot hit: the threshold was crossed in an earlier chunk, or no sigma of this
// chunk reaches it.  Both are wave-uniform facts - a found mask and the chunk's maximum - so those pairs cost two scalar branches.
template <class Thres>
__device__ __forceinline__ void dex_chunk(const Thres& thres, float m_lane, int kn, float sigma, bool valid, int base, int lane, int& first,
                                          unsigned long long& fnd) {
  float cmax = valid ? sigma : -__builtin_inff();
  cmax = wave_max(cmax);
  const float cmax_u = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, cmax)));
  for (int k = 0; k < kn; ++k) {
    if ((fnd >> k) & 1ull) continue;
    const float mk = thres.at(m_lane, k);
    if (!(cmax_u > mk)) continue;
    const unsigned long long hit = __ballot(valid && (sigma > mk));   // non-empty: cmax > m
    if (lane == k) first = base + __builtin_ctzll(hit);
    fnd |= 1ull << k;
  }
}

struct RaySums {   // wave-uniform: sum_s w_s z_s and sum_s w_s
  float depth, acc;
};

// raw_at(sc): the ray's raw row of sample sc (above); noise_at(sc): its density noise (above); zr: its depths; rd3: its direction; live:
// false for a wave that works on a ray of another wave's and stores nothing.
// on_sample(s, valid, w, raw): called once per lane and chunk with the sample's compositing weight (valid false: past the ray's end,
// w = 0 and raw the last sample's).
// thres: group 0 rides in the compositing pass, every further group (DeviceThres) is one more pass over the ray's sigma column
// (L2-resident by then).  on_first(k, idx) - optional - is called by the lane that holds threshold k with the index of the first
// sample whose sigma exceeds it (-1: none; the Dex depth then falls back to z[0]), for every threshold, whether or not `dex` is given.
// quant - optional, a Quantiles<> - adds the opacity-quantile depths: C_s, the inclusive prefix sum of the fp32 weights in fp64
// (wave_scan_add per chunk plus a carry), is non-decreasing, so a chunk can hold quantile k's crossing (the first s with C_s >= q_k)
// only if its last C reaches q_k - a wave-uniform test, like the Dex pass's chunk maximum; on a hit the owning lane takes z_i, z_{i+1},
// w_i and C_{i-1} from the hit lane.  No crossing: z[S-1] - the ray went through (NOT the Dex depth's z[0]).  Without it (NoQuantiles)
// none of that code exists.
template <class RawAt, class NoiseAt, class Thres, class OnSample, class OnFirst = NoFirstHook, class Quant = NoQuantiles>
__device__ __forceinline__ RaySums forward_ray(RawAt raw_at, NoiseAt noise_at, Thres thres, const float* __restrict__ zr,
                                               const float* __restrict__ rd3, int64_t ray, bool live, int lane, int64_t n_rays, int S,
                                               float* __restrict__ acc, float* __restrict__ depth, float* __restrict__ dex,
                                               unsigned* __restrict__ nonfinite, OnSample on_sample, OnFirst on_first = OnFirst{},
                                               Quant quant = Quant{}) {
  constexpr bool kFirstHook = !std::is_same<OnFirst, NoFirstHook>::value;
  constexpr bool kQuant = !std::is_same<Quant, NoQuantiles>::value;
  unsigned n_bad = 0;   // non-finite raw values of this lane's samples (counted only when the caller asks: fp16 overflow guard)
  const float noise_std = noise_at.std;
  const float dx = rd3[0], dy = rd3[1], dz = rd3[2];
  const float rd_norm = sqrtf((dx * dx + dy * dy) + dz * dz);
  double carry = 1.0;  // prod_{j < chunk start} (1 - alpha_j + 1e-10), kept in fp64
  float s_d = 0.f, s_a = 0.f;
  const int n_thres = thres.n;
  const int k0 = (!Thres::kGroups || n_thres < 64) ? n_thres : 64;   // thresholds of group 0 (HostThres: all of them, <= kMaxThres)
  const float m_lane = thres.lane_value(0, k0, lane);
  int first_idx = -1;
  unsigned long long found = 0ull;   // wave-uniform: thresholds whose first crossing is already known
  // quantile k rides in lane k: its crossing index and, for the linear mode, z_i, z_{i+1}, w_i, C_{i-1} of the crossing sample
  int q_n = 0, q_idx = -1;
  float q_lane = 0.0f, q_z0 = 0.0f, q_z1 = 0.0f, q_w = 0.0f;
  double q_carry = 0.0, q_cprev = 0.0;
  unsigned long long q_found = 0ull;
  if constexpr (kQuant) {
    q_n = quant.n_q < 64 ? quant.n_q : 64;
    q_lane = (lane < q_n) ? quant.d_q[lane] : 0.0f;
  }
  for (int base = 0; base < S; base += 64) {
    const int s = base + lane;
    const bool valid = s < S;
    const int sc = valid ? s : S - 1;
    const auto raw = raw_at(sc);
    if (nonfinite != nullptr && valid) n_bad += (finite_probe(raw) != 0.0f) ? 1u : 0u;
    const float z0 = zr[sc];
    const float z1 = (sc + 1 < S) ? zr[sc + 1] : z0;
    const SampleTerms t = sample_terms(raw_sigma(raw), noise_at(sc), noise_std, z0, z1, sc == S - 1, rd_norm);
    const float w = transmittance_step(t.alpha, t.one_m_alpha, valid, s, carry).w;
    on_sample(s, valid, w, raw);
    s_d += w * z0;
    s_a += w;
    if (k0 > 0) dex_chunk(thres, m_lane, k0, t.sigma, valid, base, lane, first_idx, found);
    if constexpr (kQuant) {
      if (q_n > 0) {
        const double c = wave_scan_add(static_cast<double>(w)) + q_carry;   // C_s (w is 0 past the ray's end)
        const double cprev = wave_shift_up1(c, q_carry);                     // C_{s-1}
        q_carry = wave_last(c);
        for (int k = 0; k < q_n; ++k) {
          if ((q_found >> k) & 1ull) continue;
          const double qk = static_cast<double>(read_lane(q_lane, k));
          if (!(q_carry >= qk)) continue;
          const unsigned long long hit = __ballot(valid && (c >= qk));
          // In a ragged last chunk lane 63 sums the same terms as the last valid lane in another order: q_carry may reach q_k by a
          // rounding where no valid C does.  Then the ray has no crossing (the scan's own C decides).
          if (hit == 0ull) continue;
          const int h = __builtin_ctzll(hit);
          const float hz0 = read_lane(z0, h), hz1 = read_lane(z1, h), hw = read_lane(w, h);
          const double hc = read_lane(cprev, h);
          if (lane == k) { q_idx = base + h; q_z0 = hz0; q_z1 = hz1; q_w = hw; q_cprev = hc; }
          q_found |= 1ull << k;
        }
      }
    }
  }
  s_d = wave_sum(s_d); s_a = wave_sum(s_a);
  const RaySums sums{s_d, s_a};
  if (nonfinite != nullptr && __ballot(n_bad != 0u) != 0ull) {   // (wave-uniform branch; never taken on healthy weights)
    const unsigned total = static_cast<unsigned>(wave_sum(static_cast<float>(n_bad)));
    if (lane == 0 && live) atomicAdd(nonfinite, total);
  }
  if (lane == 0 && live) {
    if (depth != nullptr) depth[ray] = s_d;
    if (acc != nullptr) acc[ray] = s_a;
  }
  if constexpr (kQuant) {
    if (lane < q_n && live) {
      if (quant.qdepth != nullptr) {
        float out = zr[S - 1];   // no crossing (acc < q): the ray went through
        if (q_idx >= 0) {
          out = q_z0;
          // fp64 from the fp32 inputs, rounded once; the last sample's interval is the 1e10 one: its value is z[S-1]
          if (quant.interp != 0 && q_idx < S - 1)
            out = static_cast<float>(static_cast<double>(q_z0) + (static_cast<double>(q_z1) - static_cast<double>(q_z0)) *
                                                                     (static_cast<double>(q_lane) - q_cprev) / static_cast<double>(q_w));
        }
        quant.qdepth[static_cast<int64_t>(lane) * n_rays + ray] = out;
      }
      if constexpr (!std::is_same<decltype(quant.on_quantile), NoQuantileHook>::value) quant.on_quantile(lane, q_idx);
    }
  }
  if constexpr (!kFirstHook) {
    if (dex == nullptr) return sums;
  }
  // argmax of an all-zero row is index 0 -> z[0] (volume_rendering_utils.py:54-58)
  if (lane < k0 && live) {
    if (dex != nullptr) dex[static_cast<int64_t>(lane) * n_rays + ray] = zr[first_idx < 0 ? 0 : first_idx];
    if constexpr (kFirstHook) on_first(lane, first_idx);
  }
  if constexpr (Thres::kGroups) {
    for (int kg = 64; kg < n_thres; kg += 64) {   // thresholds 64.. : sigma only
      const int kn = (n_thres - kg) < 64 ? (n_thres - kg) : 64;
      const float m = thres.lane_value(kg, kn, lane);
      int first = -1;
      unsigned long long fnd = 0ull;
      for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        const bool valid = s < S;
        const int sc = valid ? s : S - 1;
        dex_chunk(thres, m, kn, sample_sigma(raw_sigma(raw_at(sc)), noise_at(sc), noise_std), valid, base, lane, first, fnd);
      }
      if (lane < kn && live) {
        if (dex != nullptr) dex[static_cast<int64_t>(kg + lane) * n_rays + ray] = zr[first < 0 ? 0 : first];
        if constexpr (kFirstHook) on_first(kg + lane, first);
      }
    }
  }
  return sums;
}

// The colour client: rgb (with `white` on a white background), disparity and the (N,S) weights map beside forward_ray's depth, acc and
// dex (th: n_thres <= kMaxThres thresholds from the host).  The colour sums ride on the per-sample hook: lane-local over ascending
// chunks, then wave_sum - the order of forward_ray's depth sum.
template <class RawAt, class NoiseAt>
__device__ __forceinline__ void composite_ray(RawAt raw_at, NoiseAt noise_at, const float* __restrict__ zr,
                                              const float* __restrict__ rd3, int64_t ray, int lane, int white, const ThresArgs& th, int n_thres,
                                              int64_t n_rays, int S, float* __restrict__ rgb, float* __restrict__ disp, float* __restrict__ acc,
                                              float* __restrict__ weights, float* __restrict__ depth, float* __restrict__ dex,
                                              unsigned* __restrict__ nonfinite) {
  float s_r = 0.f, s_g = 0.f, s_b = 0.f;
  const RaySums sums = forward_ray(raw_at, noise_at, HostThres{th, n_thres}, zr, rd3, ray, true, lane, n_rays, S, acc, depth, dex,
                                   nonfinite, [&](int s, bool valid, float w, float4 raw) {
                                     if (valid && weights != nullptr) weights[ray * S + s] = w;
                                     s_r += w * sigmoidf_(raw.x);
                                     s_g += w * sigmoidf_(raw.y);
                                     s_b += w * sigmoidf_(raw.z);
                                   });
  s_r = wave_sum(s_r); s_g = wave_sum(s_g); s_b = wave_sum(s_b);
  if (lane == 0) {
    if (white) {
      const float bg = 1.0f - sums.acc;
      s_r += bg; s_g += bg; s_b += bg;
    }
    if (rgb != nullptr) {
      rgb[ray * 3 + 0] = s_r; rgb[ray * 3 + 1] = s_g; rgb[ray * 3 + 2] = s_b;
    }
    if (disp != nullptr) {
      const float q = sums.depth / sums.acc;  // NaN when acc == 0; torch.max propagates it
      disp[ray] = 1.0f / ((q != q) ? q : fmaxf(1e-10f, q));
    }
  }
}

}  // namespace dn
