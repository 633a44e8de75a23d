// The sigma-only compositing of ONE ray by one wave: expected depth, accumulation and the Dex first-crossing depths
// (volume_render_radiance_field, reference nerf/volume_rendering_utils.py:6-70, without its colour sums).  The terms, the fp64
// transmittance scan and the order of every sum are composite_ray's (composite_body.h), so depth / acc / weights / dex carry the
// same bits as dn_volume_render's for the same sigma and depths.  Shared by composite_density_kernel and density_resample_kernel.
#pragma once
#include "composite_body.h"
#include <type_traits>

namespace dn {

struct NoFirstHook {};   // density_ray without the first-crossing hook
struct NoQuantiles {};   // density_ray without the opacity-quantile readout
struct NoQuantileHook {};

// The opacity-quantile readout of density_ray (include/dexnerf_hip_quantile.h): d_q: n_q <= 64 quantiles in DEVICE memory - lane k of
// the wave tracks quantile k; qdepth (Q,N) or NULL; interp 0: z at the crossing sample, 1: the piecewise-linear CDF inversion.
// on_quantile(k, idx) - optional - is called by the lane that holds quantile k with the crossing index i(q_k) (-1: acc < q_k).
template <class OnQuantile = NoQuantileHook>
struct Quantiles {
  const float* d_q;
  int n_q, interp;
  float* qdepth;
  OnQuantile on_quantile;
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

// sample_terms' sigma alone (the Dex passes over threshold groups past the first re-read the column)
__device__ __forceinline__ float density_sigma(float raw_sigma, float noise, float noise_std) {
  float raw = raw_sigma;
  if (noise_std > 0.0f) raw = raw + noise * noise_std;
  return fmaxf(raw, 0.0f);
}

// rfr: the ray's (S,4) raw rows (only .w is read); on_weight(s, w): called once per sample with its compositing weight;
// d_thres: n_thres thresholds in DEVICE memory, any count - lane k of a wave tracks threshold 64 g + k of group g; group 0 rides
// in the compositing pass, every further group is one more pass over the ray's sigma column (L2-resident by then).
// on_first(k, idx) - optional - is called by the lane that holds threshold k with the index of the first sample whose sigma exceeds it
// (-1: none; the Dex depth then falls back to z[0]), for every threshold, whether or not `dex` is given (composite_normals_kernel).
// quant - optional, a Quantiles<> - adds the opacity-quantile depths: C_s, the inclusive prefix sum of the fp32 weights in fp64
// (wave_scan_add per chunk plus a carry), is non-decreasing, so a chunk can hold quantile k's crossing (the first s with C_s >= q_k)
// only if its last C reaches q_k - a wave-uniform test, like the Dex pass's chunk maximum; on a hit the owning lane takes z_i, z_{i+1},
// w_i and C_{i-1} from the hit lane.  No crossing: z[S-1] - the ray went through (NOT the Dex depth's z[0]).  Without it (NoQuantiles)
// none of that code exists: the kernels built on this body before the readout keep their instructions.
template <class OnWeight, class OnFirst = NoFirstHook, class Quant = NoQuantiles>
__device__ __forceinline__ void density_ray(const float4* __restrict__ rfr, const float* __restrict__ zr, const float* __restrict__ rd3,
                                            int64_t ray, bool live, int lane, const float* __restrict__ noise, float noise_std,
                                            const float* __restrict__ d_thres, int n_thres, int64_t n_rays, int S,
                                            float* __restrict__ acc, float* __restrict__ depth, float* __restrict__ dex,
                                            unsigned* __restrict__ nonfinite, OnWeight on_weight, OnFirst on_first = OnFirst{},
                                            Quant quant = Quant{}) {
  constexpr bool kFirstHook = !std::is_same<OnFirst, NoFirstHook>::value;
  constexpr bool kQuant = !std::is_same<Quant, NoQuantiles>::value;
  const float* sig = reinterpret_cast<const float*>(rfr) + 3;   // raw sigma of sample s: sig[4 s]
  unsigned n_bad = 0;
  const float dx = rd3[0], dy = rd3[1], dz = rd3[2];
  const float rd_norm = sqrtf((dx * dx + dy * dy) + dz * dz);
  double carry = 1.0;
  float s_d = 0.f, s_a = 0.f;
  const int k0 = n_thres < 64 ? n_thres : 64;   // thresholds of group 0
  const float m_lane = (lane < k0) ? d_thres[lane] : 0.0f;
  int first_idx = -1;
  unsigned long long found = 0ull;
  // quantile k rides in lane k: its crossing index and, for the linear mode, z_i, z_{i+1}, w_i, C_{i-1} of the crossing sample
  int q_n = 0, q_idx = -1;
  float q_lane = 0.0f, q_z0 = 0.0f, q_z1 = 0.0f, q_w = 0.0f;
  double q_carry = 0.0, q_cprev = 0.0;
  unsigned long long q_found = 0ull;
  if constexpr (kQuant) {
    q_n = quant.n_q < 64 ? quant.n_q : 64;
    q_lane = (lane < q_n) ? quant.d_q[lane] : 0.0f;
  }
  auto noise_at = [&](int sc) { return (noise_std > 0.0f && noise != nullptr) ? noise[ray * S + sc] : 0.0f; };
  // first crossings of one chunk for the 64 thresholds held one per lane in `m` (composite_ray's scheme: found mask + chunk maximum)
  auto dex_chunk = [&](float sigma, bool valid, int base, float m, int kn, int& first, unsigned long long& fnd) {
    float cmax = valid ? sigma : -__builtin_inff();
    cmax = wave_max(cmax);
    const float cmax_u = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, cmax)));
    for (int k = 0; k < kn; ++k) {
      if ((fnd >> k) & 1ull) continue;
      const float mk = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m), k));
      if (!(cmax_u > mk)) continue;
      const unsigned long long hit = __ballot(valid && (sigma > mk));
      if (lane == k) first = base + __builtin_ctzll(hit);
      fnd |= 1ull << k;
    }
  };
  for (int base = 0; base < S; base += 64) {
    const int s = base + lane;
    const bool valid = s < S;
    const int sc = valid ? s : S - 1;
    const float raw = sig[4 * sc];
    if (nonfinite != nullptr && valid) n_bad += ((raw - raw) != 0.0f) ? 1u : 0u;   // x - x: 0 for finite x, NaN otherwise
    const float z0 = zr[sc];
    const float z1 = (sc + 1 < S) ? zr[sc + 1] : z0;
    const SampleTerms t = sample_terms(raw, noise_at(sc), noise_std, z0, z1, sc == S - 1, rd_norm);
    const double f = valid ? static_cast<double>(t.one_m_alpha) : 1.0;
    const double incl = wave_scan_mul(f) * carry;
    const double excl = wave_shift_up1(incl, carry);
    carry = wave_last(incl);
    const float trans = (s == 0) ? 1.0f : static_cast<float>(excl);
    const float w = valid ? t.alpha * trans : 0.0f;
    if (valid) on_weight(s, w);
    s_d += w * z0;
    s_a += w;
    if (k0 > 0) dex_chunk(t.sigma, valid, base, m_lane, k0, first_idx, found);
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
    if (dex == nullptr) return;
  }
  // argmax of an all-zero row is index 0 -> z[0] (volume_rendering_utils.py:54-58)
  if (lane < k0 && live) {
    if (dex != nullptr) dex[static_cast<int64_t>(lane) * n_rays + ray] = zr[first_idx < 0 ? 0 : first_idx];
    if constexpr (kFirstHook) on_first(lane, first_idx);
  }
  for (int kg = 64; kg < n_thres; kg += 64) {   // thresholds 64.. : sigma only
    const int kn = (n_thres - kg) < 64 ? (n_thres - kg) : 64;
    const float m = (lane < kn) ? d_thres[kg + lane] : 0.0f;
    int first = -1;
    unsigned long long fnd = 0ull;
    for (int base = 0; base < S; base += 64) {
      const int s = base + lane;
      const bool valid = s < S;
      const int sc = valid ? s : S - 1;
      dex_chunk(density_sigma(sig[4 * sc], noise_at(sc), noise_std), valid, base, m, kn, first, fnd);
    }
    if (lane < kn && live) {
      if (dex != nullptr) dex[static_cast<int64_t>(kg + lane) * n_rays + ray] = zr[first < 0 ? 0 : first];
      if constexpr (kFirstHook) on_first(kg + lane, first);
    }
  }
}

}  // namespace dn
