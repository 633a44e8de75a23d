// Coarse depths, standalone positional encoding, inverse-CDF sampler and the coarse+fine depth merge, with
// their backwards.  HBM-bound elementwise / wave-scan kernels (one wave64 per ray for the sampler); compiled
// with -ffp-contract=off so plain mul/add sequences round like ATen's.  (Ray generation and selection:
// ray_select.hip; the loss heads: loss_head.hip.)
#include "dn_common.h"
#include "dn_rng.h"
#include "sampler_body.h"

namespace dn {

// ------------------------------------------------------------------------------------------------
// S3 coarse depths (reference nerf/train_utils.py:111-133)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float coarse_z_at(float near, float far, int nc, int i, int lindisp) {
  const float t = linspace_elem(0.0f, 1.0f, nc, i);
  if (!lindisp) return near * (1.0f - t) + far * t;
  return 1.0f / (1.0f / near * (1.0f - t) + 1.0f / far * t);
}

__global__ void coarse_depths_kernel(const float* __restrict__ rays, int ray_stride, int64_t n_rays, int nc,
                                     int lindisp, const float* __restrict__ t_rand, float* __restrict__ z, RngRef rng) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= n_rays * nc) return;
  const int64_t r = idx / nc;
  const int i = static_cast<int>(idx - r * nc);
  const float near = rays[r * ray_stride + 6];
  const float far = rays[r * ray_stride + 7];
  const float zi = coarse_z_at(near, far, nc, i, lindisp);
  if (t_rand == nullptr && rng.state == nullptr) {
    z[idx] = zi;
    return;
  }
  const float z_last = coarse_z_at(near, far, nc, nc - 1, lindisp);
  const float z_first = coarse_z_at(near, far, nc, 0, lindisp);
  const float upper = (i < nc - 1) ? 0.5f * (coarse_z_at(near, far, nc, i + 1, lindisp) + zi) : z_last;
  const float lower = (i > 0) ? 0.5f * (zi + coarse_z_at(near, far, nc, i - 1, lindisp)) : z_first;
  const float t = (t_rand != nullptr) ? t_rand[idx] : rng_uniform(rng, static_cast<uint64_t>(idx));   // (drawn here: dn_rng.h)
  z[idx] = lower + (upper - lower) * t;
}

// ------------------------------------------------------------------------------------------------
// S5 positional_encoding (reference nerf/nerf_helpers.py:115-159)
// ------------------------------------------------------------------------------------------------
struct FreqArgs {
  float f[32];
};

__global__ void posenc_kernel(const float* __restrict__ x, int64_t n_elems, int dim, int num_fns, int include_input,
                              FreqArgs fr, float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= n_elems) return;
  const int64_t p = idx / dim;
  const int c = static_cast<int>(idx - p * dim);
  const int width = dim * ((include_input ? 1 : 0) + 2 * num_fns);
  float* o = out + p * width;
  const float v = x[idx];
  int base = 0;
  if (include_input) {
    o[c] = v;
    base = dim;
  }
  for (int k = 0; k < num_fns; ++k) {
    const float arg = v * fr.f[k];
    o[base + (2 * k) * dim + c] = sinf(arg);
    o[base + (2 * k + 1) * dim + c] = cosf(arg);
  }
}

// ------------------------------------------------------------------------------------------------
// S7 sample_pdf_2 (reference nerf/nerf_helpers.py:262-304) + searchsorted(side="right")
//   One wave64 per ray.  Bit-exact index recipe:
//     sum  : ATen-CPU association order (8-lane vectors, 4 ILP accumulators, cascade levels);
//     cdf  : fp64 prefix sums rounded to fp32 per element - here a wave-level fp64 scan, which is
//            bit-identical to the sequential one because every partial sum of <=2^6 fp32 pdf values
//            in [2^-24, 1] is exactly representable in fp64 (no rounding happens at all);
//     inds : count of cdf entries <= u (upper bound by binary search over the LDS-resident cdf).
// ------------------------------------------------------------------------------------------------

// mode 0: bins/weights given (dn_sample_pdf).  mode 1: z_coarse/weights_coarse given (dn_fine_depths):
// bins = z_mid, w = weights[1:-1], then z_fine = sort(cat(z_coarse, samples)).
template <int MODE>
__global__ __launch_bounds__(256) void sampler_kernel(const float* __restrict__ bins_or_z, const float* __restrict__ weights,
                                                      const float* __restrict__ u, int64_t n_rays, int B, int nf,
                                                      float* __restrict__ samples, int64_t* __restrict__ inds,
                                                      float* __restrict__ z_fine, int sort_len, RngRef rng) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int64_t ray_raw = static_cast<int64_t>(blockIdx.x) * kSamplerWaves + wave;
  const bool live = ray_raw < n_rays;
  const int64_t ray = live ? ray_raw : (n_rays - 1);
  const int per_wave = 3 * (B + 1) + sort_len;
  float* w = lds + wave * per_wave;   // B-1 used
  float* cdf = w + (B + 1);           // B
  float* bins = cdf + (B + 1);        // B
  float* sbuf = bins + (B + 1);       // sort_len (MODE 1)
  const int L = B - 1;
  if (MODE == 0) {
    for (int i = lane; i < B; i += 64) bins[i] = bins_or_z[ray * B + i];
    for (int i = lane; i < L; i += 64) w[i] = weights[ray * L + i] + 1e-5f;
  } else {
    const int nc = B + 1;
    const float* zc = bins_or_z + ray * nc;
    for (int i = lane; i < B; i += 64) bins[i] = 0.5f * (zc[i + 1] + zc[i]);
    for (int i = lane; i < L; i += 64) w[i] = weights[ray * nc + 1 + i] + 1e-5f;
    for (int i = lane; i < nc; i += 64) sbuf[i] = zc[i];
  }
  sampler_resample<MODE>(w, cdf, bins, sbuf, u, ray, live, B, nf, samples, inds, z_fine, sort_len, rng);
}

// Backward of coarse_depths_kernel w.r.t. the near / far columns of the ray rows: one wave per ray.  The stratified jitter
// z'_i = lower_i + (upper_i - lower_i) t_i is linear in the unjittered depths, coupled to the neighbours through the midpoints:
//   dL/dz_j = g_j ((1 - t_j) (j > 0 ? 1/2 : 1) + t_j (j < nc - 1 ? 1/2 : 1)) + g_{j+1} (1 - t_{j+1}) / 2 + g_{j-1} t_{j-1} / 2,
// then dz_j/dnear = 1 - t, dz_j/dfar = t (linear) or z_j^2 (1 - t) / near^2, z_j^2 t / far^2 (lindisp), t = linspace(0, 1, nc)[j].
// The two sums are lane-local in ascending j, then the fixed butterfly of wave_sum, in fp64: plain stores, bit-reproducible.
__global__ __launch_bounds__(256) void coarse_depths_bwd_kernel(const float* __restrict__ rays, int ray_stride, int64_t n_rays, int nc,
                                                                int lindisp, const float* __restrict__ t_rand,
                                                                const float* __restrict__ g_z, float* __restrict__ g_near_far,
                                                                const float* __restrict__ g_z_b, const float* __restrict__ g_z_c,
                                                                RngRef rng) {
  const int lane = lane_id();
  const int64_t ray = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (ray >= n_rays) return;   // wave-uniform; no block-level sync in this kernel
  const float near = rays[ray * ray_stride + 6];
  const float far = rays[ray * ray_stride + 7];
  const float* tr = (t_rand != nullptr) ? t_rand + ray * nc : nullptr;
  // the upstream gradient of depth i: g_z alone, or (g_z + g_z_b) + g_z_c when the caller hands the terms of a sum separately
  // (dn_render_rays_backward_geom: compositing + network + merge); the jitter as given, or regenerated as coarse_depths_kernel drew it
  auto g = [&](int i) {
    float v = g_z[ray * nc + i];
    if (g_z_b != nullptr) v += g_z_b[ray * nc + i];
    if (g_z_c != nullptr) v += g_z_c[ray * nc + i];
    return v;
  };
  // (a lane forms the terms of depths j - 1, j, j + 1: up to three reads per pointer and, in the RNG form, three Philox draws per
  // depth instead of one - a few hundred multiplies per ray at nc = 64, beside a kernel that is launch-bound; not cached per lane)
  const bool jitter = tr != nullptr || rng.state != nullptr;
  auto t_of = [&](int i) { return tr != nullptr ? tr[i] : rng_uniform(rng, static_cast<uint64_t>(ray) * nc + i); };
  double s_near = 0.0, s_far = 0.0;
  for (int j = lane; j < nc; j += 64) {
    float gz = g(j);
    if (jitter) {
      const float tj = t_of(j);
      gz = gz * ((1.0f - tj) * (j > 0 ? 0.5f : 1.0f) + tj * (j < nc - 1 ? 0.5f : 1.0f));
      if (j + 1 < nc) gz += g(j + 1) * (1.0f - t_of(j + 1)) * 0.5f;
      if (j > 0) gz += g(j - 1) * t_of(j - 1) * 0.5f;
    }
    const float t = linspace_elem(0.0f, 1.0f, nc, j);
    float dn_ = 1.0f - t, df_ = t;
    if (lindisp) {
      const float zj = coarse_z_at(near, far, nc, j, 1);
      dn_ = zj * zj * (1.0f - t) / (near * near);
      df_ = zj * zj * t / (far * far);
    }
    s_near += static_cast<double>(gz) * static_cast<double>(dn_);
    s_far += static_cast<double>(gz) * static_cast<double>(df_);
  }
  s_near = wave_sum(s_near);
  s_far = wave_sum(s_far);
  if (lane == 0) {
    g_near_far[ray * 2 + 0] = static_cast<float>(s_near);
    g_near_far[ray * 2 + 1] = static_cast<float>(s_far);
  }
}

// Backward of the coarse + fine merge z_fine = sort(cat(z_coarse, z_samples)) w.r.t. the coarse depths (the samples are detached, as in
// the reference: train_utils.py:170): g_z_coarse[j] = g_z_fine[p(j)], p(j) = the slot coarse depth j takes in a stable ascending sort
// of the concatenation = (coarse depths in front of it: smaller, or equal with a smaller index) + (samples strictly smaller) - coarse
// entries come first on ties, as in the forward's merge, so z_fine[p(j)] == z_coarse[j] bitwise whichever arm the forward took.  One
// wave per ray on its own LDS rows; a half that is ascending is counted by its index / a binary search, one that is not (a
// non-ascending z_coarse, the samples of a random u) by comparing against every element.  A pure gather: plain stores.
__global__ __launch_bounds__(256) void fine_depths_bwd_kernel(const float* __restrict__ z_coarse, const float* __restrict__ z_samples,
                                                              const float* __restrict__ g_z_fine, int64_t n_rays, int nc, int nf,
                                                              float* __restrict__ g_z_coarse, const float* __restrict__ g_z_fine_b) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int64_t ray = static_cast<int64_t>(blockIdx.x) * kSamplerWaves + wave;
  if (ray >= n_rays) return;   // wave-uniform; the waves share no LDS row and no barrier
  float* zc = lds + wave * (nc + nf);
  float* zs = zc + nc;
  for (int i = lane; i < nc; i += 64) zc[i] = z_coarse[ray * nc + i];
  for (int q = lane; q < nf; q += 64) zs[q] = z_samples[ray * nf + q];
  wave_lds_sync();
  bool c_ordered = true, s_ordered = true;
  for (int i = lane; i + 1 < nc; i += 64)
    if (zc[i] > zc[i + 1]) c_ordered = false;
  for (int q = lane; q + 1 < nf; q += 64)
    if (zs[q] > zs[q + 1]) s_ordered = false;
  const bool c_asc = __all(c_ordered), s_asc = __all(s_ordered);
  const int total = nc + nf;
  for (int j = lane; j < nc; j += 64) {
    const float v = zc[j];
    int p = j;
    if (!c_asc) {
      p = 0;
      for (int k = 0; k < nc; ++k) p += (zc[k] < v || (zc[k] == v && k < j)) ? 1 : 0;
    }
    if (s_asc) {
      int lo = 0, hi = nf;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (zs[mid] < v) lo = mid + 1; else hi = mid; }
      p += lo;
    } else {
      for (int q = 0; q < nf; ++q) p += (zs[q] < v) ? 1 : 0;
    }
    const int64_t at = ray * total + min(p, total - 1);   // (p < nc + nf always; the clamp only keeps a NaN depth's read in bounds)
    g_z_coarse[ray * nc + j] = (g_z_fine_b != nullptr) ? g_z_fine[at] + g_z_fine_b[at] : g_z_fine[at];   // (g_z_fine_b: the second term of a sum)
  }
}

static int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace dn

using namespace dn;

extern "C" int dn_coarse_depths(const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int lindisp,
                                const float* t_rand, float* z_vals, dn_stream_t stream) {
  return dn::coarse_depths_rng(rays, ray_stride, n_rays, num_coarse, lindisp, t_rand, z_vals, nullptr, stream);
}

// dn_coarse_depths; t_rand == NULL with an RNG state: the stratified jitter is drawn in the kernel (dn_rng.h)
int dn::coarse_depths_rng(const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int lindisp,
                                const float* t_rand, float* z_vals, const uint32_t* rng_state, dn_stream_t stream) {
  if (n_rays == 0) return 0;  // empty tensors carry NULL data pointers
  DN_REQUIRE(rays && z_vals && n_rays >= 0 && num_coarse >= 1 && ray_stride >= 8, "dn_coarse_depths: bad arguments");
  const int64_t total = n_rays * num_coarse;
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((total + block - 1) / block);
  hipLaunchKernelGGL(coarse_depths_kernel, dim3(grid), dim3(block), 0, as_stream(stream), rays, ray_stride, n_rays,
                     num_coarse, lindisp, t_rand, z_vals, RngRef{rng_state, kRngStreamJitter});
  return check_launch("dn_coarse_depths");
}

extern "C" int dn_coarse_depths_backward(const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int lindisp,
                                         const float* t_rand, const float* g_z, float* g_near_far, dn_stream_t stream) {
  return dn::coarse_depths_backward_rng(rays, ray_stride, n_rays, num_coarse, lindisp, t_rand, g_z, nullptr, nullptr, g_near_far, nullptr, stream);
}

// dn_coarse_depths_backward; the upstream gradient as up to three terms, (g_z + g_z_b) + g_z_c; t_rand == NULL with an RNG state: the
// jitter coarse_depths_rng drew for this iteration, regenerated in the kernel
int dn::coarse_depths_backward_rng(const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int lindisp, const float* t_rand,
                                   const float* g_z, const float* g_z_b, const float* g_z_c, float* g_near_far, const uint32_t* rng_state,
                                   dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(rays && g_z && g_near_far && n_rays >= 0 && num_coarse >= 1 && ray_stride >= 8, "dn_coarse_depths_backward: bad arguments");
  const unsigned grid = static_cast<unsigned>((n_rays + 3) / 4);
  hipLaunchKernelGGL(coarse_depths_bwd_kernel, dim3(grid), dim3(256), 0, as_stream(stream), rays, ray_stride, n_rays, num_coarse, lindisp,
                     t_rand, g_z, g_near_far, g_z_b, g_z_c, RngRef{rng_state, kRngStreamJitter});
  return check_launch("dn_coarse_depths_backward");
}

namespace dn {
// frequency bands as the reference builds them (nerf_helpers.py:134-149): 2**linspace(0, L-1, L) or
// linspace(1, 2**(L-1), L), fp32.
void fill_freqs(float* f, int num_fns, int log_sampling) {
  for (int k = 0; k < num_fns; ++k) {
    if (log_sampling) {
      f[k] = exp2f(linspace_elem(0.0f, static_cast<float>(num_fns - 1), num_fns, k));
    } else {
      f[k] = linspace_elem(1.0f, exp2f(static_cast<float>(num_fns - 1)), num_fns, k);
    }
  }
}
}  // namespace dn

extern "C" int dn_positional_encoding(const float* x, int64_t n_points, int dim, int num_fns, int include_input,
                                      int log_sampling, float* out, dn_stream_t stream) {
  if (n_points == 0) return 0;
  DN_REQUIRE(x && out && n_points >= 0 && dim >= 1 && num_fns >= 0 && num_fns <= 32,
             "dn_positional_encoding: bad arguments (num_fns must be in [0,32])");
  DN_REQUIRE(include_input || num_fns > 0, "dn_positional_encoding: empty encoding");
  if (n_points == 0) return 0;
  FreqArgs fr;
  fill_freqs(fr.f, num_fns, log_sampling);
  const int64_t total = n_points * dim;
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((total + block - 1) / block);
  hipLaunchKernelGGL(posenc_kernel, dim3(grid), dim3(block), 0, as_stream(stream), x, total, dim, num_fns,
                     include_input, fr, out);
  return check_launch("dn_positional_encoding");
}

extern "C" int dn_sample_pdf(const float* bins, const float* weights, const float* u, int64_t n_rays, int n_bins,
                             int n_samples, float* samples, int64_t* inds, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(bins && weights && samples && n_rays >= 0 && n_samples >= 1, "dn_sample_pdf: bad arguments");
  DN_REQUIRE(n_bins >= 9 && n_bins <= 512, "dn_sample_pdf: n_bins must be in [9, 512] (weights row >= 8 wide)");
  if (n_rays == 0) return 0;
  const size_t lds = static_cast<size_t>(kSamplerWaves) * 3 * (n_bins + 1) * sizeof(float);
  const unsigned grid = static_cast<unsigned>((n_rays + kSamplerWaves - 1) / kSamplerWaves);
  hipLaunchKernelGGL(sampler_kernel<0>, dim3(grid), dim3(256), lds, as_stream(stream), bins, weights, u, n_rays,
                     n_bins, n_samples, samples, inds, static_cast<float*>(nullptr), 0, RngRef{nullptr, 0u});
  return check_launch("dn_sample_pdf");
}

extern "C" int dn_fine_depths(const float* z_coarse, const float* weights, const float* u, int64_t n_rays,
                              int num_coarse, int num_fine, float* z_fine, float* z_samples, dn_stream_t stream) {
  return dn::fine_depths_rng(z_coarse, weights, u, n_rays, num_coarse, num_fine, z_fine, z_samples, nullptr, stream);
}

// dn_fine_depths; u == NULL with an RNG state: the resampling draws are made in the kernel (dn_rng.h), NULL without: deterministic
int dn::fine_depths_rng(const float* z_coarse, const float* weights, const float* u, int64_t n_rays,
                              int num_coarse, int num_fine, float* z_fine, float* z_samples, const uint32_t* rng_state, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(z_coarse && weights && z_fine && n_rays >= 0 && num_fine >= 1, "dn_fine_depths: bad arguments");
  DN_REQUIRE(num_coarse >= 10 && num_coarse <= 512 && num_coarse + num_fine <= 2048,
             "dn_fine_depths: need 10 <= num_coarse <= 512 and num_coarse + num_fine <= 2048");
  if (n_rays == 0) return 0;
  const int B = num_coarse - 1;
  const int sort_len = next_pow2(num_coarse + num_fine);
  const size_t lds = static_cast<size_t>(kSamplerWaves) * (3 * (B + 1) + sort_len) * sizeof(float);
  const unsigned grid = static_cast<unsigned>((n_rays + kSamplerWaves - 1) / kSamplerWaves);
  hipLaunchKernelGGL(sampler_kernel<1>, dim3(grid), dim3(256), lds, as_stream(stream), z_coarse, weights, u, n_rays, B,
                     num_fine, z_samples, static_cast<int64_t*>(nullptr), z_fine, sort_len, RngRef{rng_state, kRngStreamU});
  return check_launch("dn_fine_depths");
}

extern "C" int dn_fine_depths_backward(const float* z_coarse, const float* z_samples, const float* g_z_fine, int64_t n_rays, int num_coarse,
                                       int num_fine, float* g_z_coarse, dn_stream_t stream) {
  return dn::fine_depths_backward_sum(z_coarse, z_samples, g_z_fine, nullptr, n_rays, num_coarse, num_fine, g_z_coarse, stream);
}

// dn_fine_depths_backward; the upstream gradient as g_z_fine + g_z_fine_b (the second term may be NULL)
int dn::fine_depths_backward_sum(const float* z_coarse, const float* z_samples, const float* g_z_fine, const float* g_z_fine_b, int64_t n_rays,
                                 int num_coarse, int num_fine, float* g_z_coarse, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(z_coarse && z_samples && g_z_fine && g_z_coarse && n_rays >= 0, "dn_fine_depths_backward: bad arguments");
  DN_REQUIRE(num_coarse >= 1 && num_coarse <= 512 && num_fine >= 1 && num_coarse + num_fine <= 2048,
             "dn_fine_depths_backward: need 1 <= num_coarse <= 512, num_fine >= 1 and num_coarse + num_fine <= 2048");
  const size_t lds = static_cast<size_t>(kSamplerWaves) * (num_coarse + num_fine) * sizeof(float);   // <= 32 KiB
  const unsigned grid = static_cast<unsigned>((n_rays + kSamplerWaves - 1) / kSamplerWaves);
  hipLaunchKernelGGL(fine_depths_bwd_kernel, dim3(grid), dim3(256), lds, as_stream(stream), z_coarse, z_samples, g_z_fine, n_rays,
                     num_coarse, num_fine, g_z_coarse, g_z_fine_b);
  return check_launch("dn_fine_depths_backward");
}
