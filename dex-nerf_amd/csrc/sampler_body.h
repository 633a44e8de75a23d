// The inverse-CDF sampler's per-ray device code (sample_pdf_2, reference nerf/nerf_helpers.py:262-304, + the coarse / fine depth merge,
// nerf/train_utils.py:163-173): shared by sampler_kernel (rays_sampling.hip: weights from HBM) and density_resample_kernel
// (composite_density.hip: weights formed in the same wave) - one body, so the two produce the same bits.
#pragma once
#include "dn_common.h"
#include "dn_rng.h"

namespace dn {

// Cross-lane hand-off through the wave's OWN LDS rows (one lane writes, another reads): a wave's DS instructions execute in
// order, so no s_barrier is needed - but the compiler must not move the reads above the neighbouring lanes' writes.  The bare
// wave_barrier intrinsic does not order memory for alias analysis; the wavefront-scope fence does (it emits no instruction
// beyond, at most, an s_waitcnt lgkmcnt).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int kSamplerWaves = 4;  // rays per 256-thread block

// ATen multi_row_sum / row_sum / vectorized_inner_sum order for a contiguous fp32 row of length L held
// in LDS.  Lanes 0..7 each own one vector lane; the result is broadcast to the whole wave.
__device__ inline float aten_order_sum(const float* w, int L) {
  const int lane = lane_id();
  const int nvec = L >> 3;
  const int groups = nvec >> 2;
  float part = 0.0f;
  if (lane < 8) {
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
    int ceil_log2 = 0;
    while ((1 << ceil_log2) < groups) ++ceil_log2;
    const int level_power = max(4, ceil_log2 / 4);
    const int level_step = 1 << level_power;
    const int level_mask = level_step - 1;
    int i = 0;
    for (; i + level_step <= groups;) {
      for (int j = 0; j < level_step; ++j, ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[0][k] += w[(i * 4 + k) * 8 + lane];
      }
      for (int j = 1; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc[j][k] += acc[j - 1][k];
          acc[j - 1][k] = 0.0f;
        }
        const int mask = level_mask << (j * level_power);
        if ((i & mask) != 0) break;
      }
    }
    for (; i < groups; ++i) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[0][k] += w[(i * 4 + k) * 8 + lane];
    }
    for (int j = 1; j < 4; ++j) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[0][k] += acc[j][k];
    }
    for (int v = groups * 4; v < nvec; ++v) acc[0][0] += w[v * 8 + lane];
    part = ((acc[0][0] + acc[0][1]) + acc[0][2]) + acc[0][3];
  }
  float total = 0.0f;
  for (int k = nvec * 8; k < L; ++k) total += w[k];
#pragma unroll
  for (int k = 0; k < 8; ++k) total += __shfl(part, k, 64);
  return total;  // identical in every lane
}

// Builds cdf[0..B) in LDS from w[0..B-1) (already +1e-5) ; w is overwritten with the pdf.
__device__ inline void build_cdf(float* w, float* cdf, int B) {
  const int lane = lane_id();
  const int L = B - 1;
  const float s = aten_order_sum(w, L);
  double carry = 0.0;
  if (lane == 0) cdf[0] = 0.0f;
  for (int base = 0; base < L; base += 64) {
    const int i = base + lane;
    const float pdf = (i < L) ? w[i] / s : 0.0f;
    const double inc = wave_scan_add(static_cast<double>(pdf)) + carry;
    if (i < L) cdf[i + 1] = static_cast<float>(inc);
    carry = __shfl(inc, 63, 64);
  }
}

__device__ __forceinline__ float invert_cdf(const float* cdf, const float* bins, int B, float u, int* ind_out) {
  int lo = 0, hi = B;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
  }
  *ind_out = lo;
  const int below = max(lo - 1, 0);
  const int above = min(lo, B - 1);
  const float cb = cdf[below], ca = cdf[above];
  const float bb = bins[below], ba = bins[above];
  float denom = ca - cb;
  if (denom < 1e-5f) denom = 1.0f;
  const float t = (u - cb) / denom;
  return bb + t * (ba - bb);
}

// One ray, one wave, from the point where w[0..B-1) (weights + 1e-5), bins[0..B) and (MODE 1) sbuf[0..B+1) = the coarse depths sit in
// this wave's LDS rows: cdf, the nf inverse-CDF samples, and (MODE 1) z_fine = sort(cat(z_coarse, samples)).
template <int MODE>
__device__ __forceinline__ void sampler_resample(float* w, float* cdf, float* bins, float* sbuf, const float* __restrict__ u, int64_t ray,
                                                 bool live, int B, int nf, float* __restrict__ samples, int64_t* __restrict__ inds,
                                                 float* __restrict__ z_fine, int sort_len, RngRef rng) {
  const int lane = lane_id();
  wave_lds_sync();   // (this wave's own rows: DS instructions of a wave execute in order)
  build_cdf(w, cdf, B);
  wave_lds_sync();
  for (int q = lane; q < nf; q += 64) {
    const float uq = (u != nullptr) ? u[ray * nf + q]
                     : (rng.state != nullptr ? rng_uniform(rng, static_cast<uint64_t>(ray) * nf + q) : linspace_elem(0.0f, 1.0f, nf, q));
    int ind;
    const float s = invert_cdf(cdf, bins, B, uq, &ind);
    if (live) {
      if (samples != nullptr) samples[ray * nf + q] = s;
      if (inds != nullptr) inds[ray * nf + q] = ind;
    }
    if (MODE == 1) sbuf[B + 1 + q] = s;
  }
  if (MODE == 1) {
    const int nc = B + 1;
    const int total = nc + nf;
    // Everything below touches this wave's own LDS rows only: a wave's DS instructions execute in order, so no workgroup
    // barrier is needed between the steps (the round-1 kernel had one per bitonic stage: 36 for 192 depths).
    wave_lds_sync();
    // sort(cat(z_coarse, z_samples)) (train_utils.py:173).  Both halves are usually already ascending - the coarse depths
    // always, the samples whenever u is ascending (deterministic resampling: every validation render) - and then the sort is
    // a MERGE: an element's output slot = its own index + the number of elements of the other half in front of it (coarse
    // depths first on ties), found by binary search.  192 depths: ~7 LDS reads per element instead of 36 compare-exchange
    // stages.  Whether the samples really are ascending is checked on the values (an interpolated sample can land an ulp past
    // its bin edge); anything else takes the bitonic sort, which produces the same multiset in the same order.
    const float* zs = sbuf + nc;
    bool ordered = true;
    for (int q = lane; q < nf; q += 64)
      if (q + 1 < nf && zs[q] > zs[q + 1]) ordered = false;
    for (int i = lane; i < nc; i += 64)
      if (i + 1 < nc && sbuf[i] > sbuf[i + 1]) ordered = false;
    constexpr int kMergeCoarse = 4, kMergeFine = 8;   // merge path: up to 256 coarse + 512 fine depths (values held in registers)
    if (nc <= 64 * kMergeCoarse && nf <= 64 * kMergeFine && __all(ordered)) {
      float vc[kMergeCoarse], vf[kMergeFine];
      int sc[kMergeCoarse], sf[kMergeFine];
#pragma unroll
      for (int e = 0; e < kMergeCoarse; ++e) {        // coarse depth i: samples strictly in front of it
        if (64 * e >= nc) { vc[e] = 0.0f; sc[e] = 0; continue; }   // (wave-uniform: no search for rows that do not exist)
        const int i = lane + 64 * e;
        const float v = sbuf[min(i, nc - 1)];
        int lo = 0, hi = nf;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (zs[mid] < v) lo = mid + 1; else hi = mid; }
        vc[e] = v; sc[e] = i + lo;
      }
#pragma unroll
      for (int e = 0; e < kMergeFine; ++e) {          // sample q: coarse depths in front of it or equal to it
        if (64 * e >= nf) { vf[e] = 0.0f; sf[e] = 0; continue; }
        const int q = lane + 64 * e;
        const float v = zs[min(q, nf - 1)];
        int lo = 0, hi = nc;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (sbuf[mid] <= v) lo = mid + 1; else hi = mid; }
        vf[e] = v; sf[e] = q + lo;
      }
      wave_lds_sync();   // every search has read its operands (one wave, in order): now overwrite in place
#pragma unroll
      for (int e = 0; e < kMergeCoarse; ++e) if (lane + 64 * e < nc) sbuf[sc[e]] = vc[e];
#pragma unroll
      for (int e = 0; e < kMergeFine; ++e) if (lane + 64 * e < nf) sbuf[sf[e]] = vf[e];
      wave_lds_sync();
      if (live)
        for (int i = lane; i < total; i += 64) z_fine[ray * total + i] = sbuf[i];
      return;
    }
    for (int i = total + lane; i < sort_len; i += 64) sbuf[i] = __builtin_inff();
    // bitonic sort of sort_len (power of two) floats by one wave
    for (int k = 2; k <= sort_len; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        wave_lds_sync();
        for (int t = lane; t < (sort_len >> 1); t += 64) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int hi = lo | j;
          const bool up = ((lo & k) == 0);
          const float a = sbuf[lo], b = sbuf[hi];
          if ((a > b) == up) {
            sbuf[lo] = b;
            sbuf[hi] = a;
          }
        }
      }
    }
    wave_lds_sync();
    if (live)
      for (int i = lane; i < total; i += 64) z_fine[ray * total + i] = sbuf[i];
  }
}

}  // namespace dn
