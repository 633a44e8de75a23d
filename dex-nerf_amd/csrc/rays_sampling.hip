// Ray generation, coarse depths, standalone positional encoding, inverse-CDF sampler and the
// coarse+fine depth merge.  HBM-bound elementwise / wave-scan kernels (one wave64 per ray for the
// sampler); compiled with -ffp-contract=off so plain mul/add sequences round like ATen's.
#include "dn_common.h"
#include "dn_rng.h"
#include "sampler_body.h"

namespace dn {



// ------------------------------------------------------------------------------------------------
// S1 get_ray_bundle (reference nerf/nerf_helpers.py:67-112)
// ------------------------------------------------------------------------------------------------
struct RayBundleArgs {
  float rinv[9];
  float origin[3];
  float fx, cx, cy;
  int height, width;
};

__global__ void ray_bundle_kernel(RayBundleArgs a, float* __restrict__ ro, float* __restrict__ rd) {
  const int64_t pix = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t total = static_cast<int64_t>(a.height) * a.width;
  if (pix >= total) return;
  const int row = static_cast<int>(pix / a.width);
  const int col = static_cast<int>(pix - static_cast<int64_t>(row) * a.width);
  // dir = [(ii-cx)/fx, (jj-cy)/fx, 1]: fx divides the y term too (nerf_helpers.py:100-101)
  const float d0 = (static_cast<float>(col) - a.cx) / a.fx;
  const float d1 = (static_cast<float>(row) - a.cy) / a.fx;
  const float d2 = 1.0f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // sum over the last dim of dir[None,:] * Rinv  ->  ((p0 + p1) + p2), products rounded first
    const float p0 = d0 * a.rinv[3 * j + 0];
    const float p1 = d1 * a.rinv[3 * j + 1];
    const float p2 = d2 * a.rinv[3 * j + 2];
    rd[pix * 3 + j] = (p0 + p1) + p2;
    ro[pix * 3 + j] = a.origin[j];
  }
}

// Forward-facing NDC warp of one ray (reference nerf/nerf_helpers.py:172-199), op for op (compiled -ffp-contract=off): the body of
// dn_ndc_rays, and of dn_select_rays_draw_ndc, whose rows must equal a plain draw followed by dn_ndc_rays bit for bit.
__device__ __forceinline__ void ndc_warp(double h, double w, double focal, double near_d, const float (&o)[3], const float (&d)[3],
                                         float* __restrict__ ro_out, float* __restrict__ rd_out) {
  const float dx = d[0], dy = d[1], dz = d[2];
  const float near = static_cast<float>(near_d);
  const float t = -(near + o[2]) / dz;
  const float ox = o[0] + t * dx, oy = o[1] + t * dy, oz = o[2] + t * dz;
  // python-float constants are computed in double and then meet fp32 tensors as fp32 scalars
  const float cw = static_cast<float>(-1.0 / (w / (2.0 * focal)));
  const float ch = static_cast<float>(-1.0 / (h / (2.0 * focal)));
  const float two_near = static_cast<float>(2.0 * near_d);
  ro_out[0] = cw * ox / oz;
  ro_out[1] = ch * oy / oz;
  ro_out[2] = 1.0f + two_near / oz;
  rd_out[0] = cw * (dx / dz - ox / oz);
  rd_out[1] = ch * (dy / dz - oy / oz);
  rd_out[2] = -two_near / oz;
}

// Training-ray selection (reference train_dexnerf_rgb.py:229-242 + the packing of train_utils.py:225-250): for each
// chosen pixel build the packed ray row [ro3, rd3, near, far, viewdir3] directly (same arithmetic as
// ray_bundle_kernel for rd; viewdir = rd / ||rd||, train_utils.py:225) and gather the target pixel's RGB.
__global__ void select_rays_kernel(RayBundleArgs a, float near, float far, const int64_t* __restrict__ pix, int64_t n,
                                   const float* __restrict__ image, int channels, float* __restrict__ rays,
                                   float* __restrict__ target) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t px = pix[i];
  const int row = static_cast<int>(px / a.width);
  const int col = static_cast<int>(px - static_cast<int64_t>(row) * a.width);
  const float d0 = (static_cast<float>(col) - a.cx) / a.fx;
  const float d1 = (static_cast<float>(row) - a.cy) / a.fx;
  const float d2 = 1.0f;
  float rd[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float p0 = d0 * a.rinv[3 * j + 0];
    const float p1 = d1 * a.rinv[3 * j + 1];
    const float p2 = d2 * a.rinv[3 * j + 2];
    rd[j] = (p0 + p1) + p2;
  }
  const float nrm = sqrtf((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2]);
  float* r = rays + i * 11;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    r[j] = a.origin[j];
    r[3 + j] = rd[j];
    r[8 + j] = rd[j] / nrm;
  }
  r[6] = near;
  r[7] = far;
  if (target != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) target[i * 3 + c] = image[px * channels + c];
  }
}

// The row of ray i: pixel `px` of the camera record `cam`, target pixel from that view's image `img` (NULL target: none).  The body
// of select_rays_indirect_kernel and select_rays_views_kernel - one sequence of fp32 operations (the unit is compiled with
// -ffp-contract=off), so the rows of the two kernels are bit-identical for the same (view, pixel).
template <bool NDC>
__device__ __forceinline__ void select_ray_row(const float* __restrict__ cam, int height, int width, float near, float far, int64_t px,
                                               const float* __restrict__ img, int channels, float* __restrict__ r, float* __restrict__ tgt,
                                               double focal, double ndc_near) {
  const float fx = cam[12], cx = cam[13], cy = cam[14];
  const int row = static_cast<int>(px / width);
  const int col = static_cast<int>(px - static_cast<int64_t>(row) * width);
  const float d0 = (static_cast<float>(col) - cx) / fx;
  const float d1 = (static_cast<float>(row) - cy) / fx;
  const float d2 = 1.0f;
  float rd[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float p0 = d0 * cam[3 * j + 0];
    const float p1 = d1 * cam[3 * j + 1];
    const float p2 = d2 * cam[3 * j + 2];
    rd[j] = (p0 + p1) + p2;
  }
  const float nrm = sqrtf((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2]);
  if constexpr (NDC) {
    const float o[3] = {cam[9], cam[10], cam[11]};
    ndc_warp(static_cast<double>(height), static_cast<double>(width), focal, ndc_near, o, rd, r, r + 3);
#pragma unroll
    for (int j = 0; j < 3; ++j) r[8 + j] = rd[j] / nrm;
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      r[j] = cam[9 + j];
      r[3 + j] = rd[j];
      r[8 + j] = rd[j] / nrm;
    }
  }
  r[6] = near;
  r[7] = far;
  if (tgt != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) tgt[c] = img[px * channels + c];
  }
}

// The same with the camera chosen on the device: `cams` holds one 16-float record per training view
// [rinv9, origin3, fx, cx, cy, -] and `view` is a device scalar, so a captured HIP graph of the whole training
// iteration can be replayed for any view (host-side camera constants would be frozen into the graph).
// pix == NULL: the pixels are DRAWN here - element i of this iteration's draw without replacement, a keyed permutation of the
// H W pixels (dn_rng.h feistel_permute; reference train_dexnerf_rgb.py:229-236: np.random.choice(H W, n, replace=False)) - from
// the RNG state's NEXT iteration counter, which thread 0 then publishes as the CURRENT one for the rest of the iteration.
// NDC: the origin and direction of every row warped to NDC (ndc_warp with the image's height / width, `focal`, `ndc_near`); the view
// direction (columns 8:11) stays that of the unwarped direction, as in run_one_iter_of_nerf (reference train_utils.py:240-262).
template <bool NDC>
__global__ void select_rays_indirect_kernel(const float* __restrict__ cams, const int* __restrict__ view, int n_views, int height, int width,
                                            float near, float far, const int64_t* __restrict__ pix, int64_t n,
                                            const float* __restrict__ images, int channels, float* __restrict__ rays,
                                            float* __restrict__ target, uint32_t* __restrict__ rng_state, int64_t* __restrict__ pix_out,
                                            double focal, double ndc_near) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  uint32_t iteration = 0;
  if (pix == nullptr) {
    iteration = rng_state[3];
    if (i == 0) rng_state[2] = iteration;   // (nobody in this launch reads word 2)
  }
  if (i >= n) return;
  int v;
  if (view != nullptr) v = *view;
  else {   // the iteration's training view drawn here too (reference: img_idx = np.random.choice(i_train), train_dexnerf_rgb.py:223)
    uint32_t w[4];
    rng_words(rng_state[0], rng_state[1], iteration, kRngStreamView, 0, w);
    v = static_cast<int>(w[0] % static_cast<uint32_t>(n_views));
  }
  int64_t px;
  if (pix != nullptr) px = pix[i];
  else {
    px = feistel_permute(static_cast<uint32_t>(i), static_cast<uint32_t>(height) * static_cast<uint32_t>(width), rng_state[0], rng_state[1], iteration);
    if (pix_out != nullptr) pix_out[i] = px;
  }
  select_ray_row<NDC>(cams + static_cast<int64_t>(v) * 16, height, width, near, far, px,
                      target != nullptr ? images + static_cast<int64_t>(v) * height * width * channels : nullptr, channels, rays + i * 11,
                      target != nullptr ? target + i * 3 : nullptr, focal, ndc_near);
}

// Mixed-camera batches: every ray carries its own view.  pix != NULL: ray i is pixel pix[i] of view view_index[i] (both the caller's
// contract: 0 <= view_index[i] < n_views).  pix == NULL: the (view, pixel) pairs are DRAWN here - element i of the iteration's draw
// is q = feistel_permute(i, V H W), the keyed permutation of select_rays_indirect_kernel over the pixels of ALL views, view = q / (H W),
// pixel = q - view H W - so any prefix is a draw without replacement over (view, pixel) pairs, and with one view it is that kernel's
// draw.  The first kernel of an iteration like it: thread 0 publishes the state's NEXT counter as the CURRENT one.
template <bool NDC>
__global__ void select_rays_views_kernel(const float* __restrict__ cams, const int* __restrict__ view_index, int n_views, int height, int width,
                                         float near, float far, const int64_t* __restrict__ pix, int64_t n, const float* __restrict__ images,
                                         int channels, float* __restrict__ rays, float* __restrict__ target, uint32_t* __restrict__ rng_state,
                                         int64_t* __restrict__ pix_out, int* __restrict__ view_out, double focal, double ndc_near) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  uint32_t iteration = 0;
  if (pix == nullptr) {
    iteration = rng_state[3];
    if (i == 0) rng_state[2] = iteration;   // (nobody in this launch reads word 2)
  }
  if (i >= n) return;
  const uint32_t per_view = static_cast<uint32_t>(height) * static_cast<uint32_t>(width);
  int v;
  int64_t px;
  if (pix != nullptr) {
    v = view_index[i];
    px = pix[i];
  } else {
    const uint32_t q = feistel_permute(static_cast<uint32_t>(i), static_cast<uint32_t>(n_views) * per_view, rng_state[0], rng_state[1], iteration);
    v = static_cast<int>(q / per_view);
    px = q - static_cast<uint32_t>(v) * per_view;
    if (pix_out != nullptr) pix_out[i] = px;
    if (view_out != nullptr) view_out[i] = v;
  }
  select_ray_row<NDC>(cams + static_cast<int64_t>(v) * 16, height, width, near, far, px,
                      target != nullptr ? images + static_cast<int64_t>(v) * height * width * channels : nullptr, channels, rays + i * 11,
                      target != nullptr ? target + i * 3 : nullptr, focal, ndc_near);
}

// Forward-facing NDC warp (reference nerf/nerf_helpers.py:172-199), op for op (compiled -ffp-contract=off).
__global__ void ndc_rays_kernel(double h, double w, double focal, double near_d, const float* __restrict__ ro,
                                const float* __restrict__ rd, int64_t n, float* __restrict__ ro_out,
                                float* __restrict__ rd_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float o[3] = {ro[i * 3 + 0], ro[i * 3 + 1], ro[i * 3 + 2]};
  const float d[3] = {rd[i * 3 + 0], rd[i * 3 + 1], rd[i * 3 + 2]};
  ndc_warp(h, w, focal, near_d, o, d, ro_out + i * 3, rd_out + i * 3);
}

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

// Backward of ray generation w.r.t. the camera: the 16-float record [rinv9, origin3, fx, cx, cy, ndc_focal] of ray_bundle_kernel /
// select_rays*_kernel receives the gradient of the rays' origins, directions and unit view directions (NDC: of the warped origins /
// directions of ndc_warp, the view directions those of the unwarped directions).  Per ray, in fp64 from the fp32 record and the integer
// pixel: d = [(col - cx) / fx, (row - cy) / fx, 1], rd_j = sum_k d_k rinv[3j + k], v = rd / |rd|;
//   NDC: (g_o', g_d') pulled back through the six expressions of ndc_warp and the shift o + t rd to (g_o, g_d); o'_{0,1}, d'_{0,1} are
//        linear in the focal length, so g_focal = (g_o'_0 o'_0 + g_o'_1 o'_1 + g_d'_0 d'_0 + g_d'_1 d'_1) / focal;
//   g_d += (g_v - v (v . g_v)) / |rd|;
//   g_origin += g_o, g_rinv[3j + k] += g_d[j] d_k, e_k = sum_j g_d[j] rinv[3j + k], g_cx -= e_0 / fx, g_cy -= e_1 / fx,
//   g_fx -= (e_0 d_0 + e_1 d_1) / fx.
// The sums are formed in a fixed order: a lane adds its rays (thread index, then strides of the whole grid) in ascending order, the
// lanes of a wave meet in wave_sum's butterfly, the waves of a workgroup through LDS in wave order, and each workgroup stores 16
// doubles; camera_grad_finish_kernel adds those in workgroup order.  The grid is a function of n alone (camera_grad_blocks): plain
// stores, bit-reproducible on any device.
constexpr int kCamGradThreads = 256;
constexpr int kCamGradMaxBlocks = 64;

static int camera_grad_blocks(int64_t n) {
  const int64_t blocks = (n + kCamGradThreads - 1) / kCamGradThreads;
  return static_cast<int>(blocks < kCamGradMaxBlocks ? blocks : kCamGradMaxBlocks);
}

// The camera record in fp64 and the two NDC scales: what every ray of one camera shares.
struct CamGradCamera {
  double rinv[9], origin[3], fx, cx, cy, sx, sy;
};

__device__ __forceinline__ CamGradCamera camera_grad_load(const float* __restrict__ cam, int width, double height_d, double ndc_focal) {
  CamGradCamera c;
#pragma unroll
  for (int k = 0; k < 9; ++k) c.rinv[k] = static_cast<double>(cam[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) c.origin[k] = static_cast<double>(cam[9 + k]);
  c.fx = static_cast<double>(cam[12]);
  c.cx = static_cast<double>(cam[13]);
  c.cy = static_cast<double>(cam[14]);
  c.sx = -1.0 / (static_cast<double>(width) / (2.0 * ndc_focal));
  c.sy = -1.0 / (height_d / (2.0 * ndc_focal));
  return c;
}

// The Jacobian of ray i (pixel px of camera c) applied to its upstream gradients, added to the 16 sums of the record's gradient:
// the one statement of the formulas above, shared by camera_grad_kernel and camera_grad_views_kernel.
__device__ __forceinline__ void camera_grad_ray(const CamGradCamera& c, int width, int64_t px, int64_t i, const float* __restrict__ g_ro,
                                                int ro_stride, const float* __restrict__ g_rd, int rd_stride, const float* __restrict__ g_vd,
                                                int vd_stride, bool ndc, double ndc_focal, double ndc_near, double (&acc)[16]) {
  const double* rinv = c.rinv;
  const double* origin = c.origin;
  const double fx = c.fx, cx = c.cx, cy = c.cy, sx = c.sx, sy = c.sy;
  const int64_t row = px / width;
  const int64_t col = px - row * width;
  const double d[3] = {(static_cast<double>(col) - cx) / fx, (static_cast<double>(row) - cy) / fx, 1.0};
  double rd[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) rd[j] = (d[0] * rinv[3 * j + 0] + d[1] * rinv[3 * j + 1]) + d[2] * rinv[3 * j + 2];
  double go[3] = {0.0, 0.0, 0.0}, gd[3] = {0.0, 0.0, 0.0};
  if (g_ro != nullptr) {
#pragma unroll
    for (int j = 0; j < 3; ++j) go[j] = static_cast<double>(g_ro[i * ro_stride + j]);
  }
  if (g_rd != nullptr) {
#pragma unroll
    for (int j = 0; j < 3; ++j) gd[j] = static_cast<double>(g_rd[i * rd_stride + j]);
  }
  if (ndc) {
    // forward: t = -(near + o_z) / rd_z, p = o + t rd, o' = [sx p0 / p2, sy p1 / p2, 1 + 2 near / p2],
    //          d' = [sx (rd0 / rd2 - p0 / p2), sy (rd1 / rd2 - p1 / p2), -2 near / p2]
    const double t = -(ndc_near + origin[2]) / rd[2];
    const double p[3] = {origin[0] + t * rd[0], origin[1] + t * rd[1], origin[2] + t * rd[2]};
    const double ip = 1.0 / p[2], iz = 1.0 / rd[2];
    const double o0 = sx * p[0] * ip, o1 = sy * p[1] * ip;
    const double w0 = sx * (rd[0] * iz - p[0] * ip), w1 = sy * (rd[1] * iz - p[1] * ip);
    acc[15] += (go[0] * o0 + go[1] * o1 + gd[0] * w0 + gd[1] * w1) / ndc_focal;
    const double a0 = go[0] - gd[0], a1 = go[1] - gd[1];
    double gp[3];
    gp[0] = sx * ip * a0;
    gp[1] = sy * ip * a1;
    gp[2] = -(sx * p[0] * a0 + sy * p[1] * a1) * ip * ip + 2.0 * ndc_near * ip * ip * (gd[2] - go[2]);
    double gr[3];
    gr[0] = sx * iz * gd[0];
    gr[1] = sy * iz * gd[1];
    gr[2] = -(sx * rd[0] * gd[0] + sy * rd[1] * gd[1]) * iz * iz;
    const double gt = gp[0] * rd[0] + gp[1] * rd[1] + gp[2] * rd[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      go[j] = gp[j];
      gd[j] = gr[j] + t * gp[j];
    }
    go[2] -= gt * iz;
    gd[2] -= gt * t * iz;
  }
  if (g_vd != nullptr) {
    const double gv[3] = {static_cast<double>(g_vd[i * vd_stride + 0]), static_cast<double>(g_vd[i * vd_stride + 1]),
                          static_cast<double>(g_vd[i * vd_stride + 2])};
    const double inv_nrm = 1.0 / sqrt((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2]);
    const double v[3] = {rd[0] * inv_nrm, rd[1] * inv_nrm, rd[2] * inv_nrm};
    const double vg = (v[0] * gv[0] + v[1] * gv[1]) + v[2] * gv[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) gd[j] += (gv[j] - v[j] * vg) * inv_nrm;
  }
  double e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) e[k] = (gd[0] * rinv[k] + gd[1] * rinv[3 + k]) + gd[2] * rinv[6 + k];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    acc[9 + j] += go[j];
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[3 * j + k] += gd[j] * d[k];
  }
  acc[12] -= (e[0] * d[0] + e[1] * d[1]) / fx;
  acc[13] -= e[0] / fx;
  acc[14] -= e[1] / fx;
}

// The 16 sums of a workgroup: wave_sum's butterfly, the waves through LDS in wave order, 16 doubles stored.  Every thread of the
// workgroup calls it (it holds a barrier).
__device__ __forceinline__ void camera_grad_block_store(const double (&acc)[16], double* __restrict__ out16) {
  __shared__ double part[kCamGradThreads / 64][16];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane_id() == 0) part[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    double s = part[0][threadIdx.x];
    for (int w = 1; w < kCamGradThreads / 64; ++w) s += part[w][threadIdx.x];
    out16[threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(kCamGradThreads) void camera_grad_kernel(const float* __restrict__ cam, int width, const int64_t* __restrict__ pix,
                                                                      int64_t n, const float* __restrict__ g_ro, int ro_stride,
                                                                      const float* __restrict__ g_rd, int rd_stride,
                                                                      const float* __restrict__ g_vd, int vd_stride, double height_d,
                                                                      double ndc_focal, double ndc_near, double* __restrict__ partials) {
  const CamGradCamera c = camera_grad_load(cam, width, height_d, ndc_focal);
  const bool ndc = ndc_focal > 0.0;
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kCamGradThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kCamGradThreads + threadIdx.x; i < n; i += step) {
    const int64_t px = (pix != nullptr) ? pix[i] : i;
    camera_grad_ray(c, width, px, i, g_ro, ro_stride, g_rd, rd_stride, g_vd, vd_stride, ndc, ndc_focal, ndc_near, acc);
  }
  camera_grad_block_store(acc, partials + static_cast<int64_t>(blockIdx.x) * 16);
}

// Mixed-camera batches: workgroup (b, v) of a (camera_grad_blocks(n), V) grid walks the rays in camera_grad_kernel's order and adds
// those of view v (the others are skipped: the 4-byte view index of every ray is read once per view), then stores its 16 sums at
// partials[(v blocks + b) 16]; camera_grad_finish_kernel, one workgroup per view, adds a view's partials in workgroup order.  The
// order of every sum is a function of (n, V) and the view indices alone: plain stores, bit-reproducible on any device.
__global__ __launch_bounds__(kCamGradThreads) void camera_grad_views_kernel(const float* __restrict__ cams, int width, const int* __restrict__ view_index,
                                                                            const int64_t* __restrict__ pix, int64_t n,
                                                                            const float* __restrict__ g_ro, int ro_stride,
                                                                            const float* __restrict__ g_rd, int rd_stride,
                                                                            const float* __restrict__ g_vd, int vd_stride, double height_d,
                                                                            double ndc_focal, double ndc_near, double* __restrict__ partials) {
  const int view = static_cast<int>(blockIdx.y);
  const CamGradCamera c = camera_grad_load(cams + static_cast<int64_t>(view) * 16, width, height_d, ndc_focal);
  const bool ndc = ndc_focal > 0.0;
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kCamGradThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kCamGradThreads + threadIdx.x; i < n; i += step) {
    if (view_index[i] != view) continue;
    camera_grad_ray(c, width, pix[i], i, g_ro, ro_stride, g_rd, rd_stride, g_vd, vd_stride, ndc, ndc_focal, ndc_near, acc);
  }
  camera_grad_block_store(acc, partials + (static_cast<int64_t>(view) * gridDim.x + blockIdx.x) * 16);
}

// Workgroup v adds the n_blocks partials of record v in workgroup order (dn_camera_grad: one record, one workgroup).
__global__ __launch_bounds__(64) void camera_grad_finish_kernel(const double* __restrict__ partials, int n_blocks, float* __restrict__ g_cam) {
  if (threadIdx.x >= 16) return;
  const double* mine = partials + static_cast<int64_t>(blockIdx.x) * n_blocks * 16;
  double s = 0.0;
  for (int b = 0; b < n_blocks; ++b) s += mine[b * 16 + threadIdx.x];
  g_cam[static_cast<int64_t>(blockIdx.x) * 16 + threadIdx.x] = static_cast<float>(s);
}

static int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace dn

using namespace dn;

extern "C" int dn_ray_bundle(int height, int width, const float* h_rinv9, const float* h_origin3, float fx, float cx,
                             float cy, float* ro, float* rd, dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && h_rinv9 && h_origin3 && ro && rd, "dn_ray_bundle: bad arguments");
  RayBundleArgs a;
  for (int i = 0; i < 9; ++i) a.rinv[i] = h_rinv9[i];
  for (int i = 0; i < 3; ++i) a.origin[i] = h_origin3[i];
  a.fx = fx; a.cx = cx; a.cy = cy; a.height = height; a.width = width;
  const int64_t total = static_cast<int64_t>(height) * width;
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((total + block - 1) / block);
  hipLaunchKernelGGL(ray_bundle_kernel, dim3(grid), dim3(block), 0, as_stream(stream), a, ro, rd);
  return check_launch("dn_ray_bundle");
}

extern "C" int dn_select_rays(int height, int width, const float* h_rinv9, const float* h_origin3, float fx, float cx,
                              float cy, float near, float far, const int64_t* pixel_index, int64_t n_rays,
                              const float* image, int channels, float* rays, float* target, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(height > 0 && width > 0 && h_rinv9 && h_origin3 && pixel_index && rays && n_rays >= 0,
             "dn_select_rays: bad arguments");
  DN_REQUIRE(target == nullptr || (image != nullptr && channels >= 3), "dn_select_rays: target requested without an image of >= 3 channels");
  RayBundleArgs a;
  for (int i = 0; i < 9; ++i) a.rinv[i] = h_rinv9[i];
  for (int i = 0; i < 3; ++i) a.origin[i] = h_origin3[i];
  a.fx = fx; a.cx = cx; a.cy = cy; a.height = height; a.width = width;
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(select_rays_kernel, dim3(grid), dim3(block), 0, as_stream(stream), a, near, far, pixel_index, n_rays,
                     image, channels, rays, target);
  return check_launch("dn_select_rays");
}

extern "C" int dn_select_rays_indirect(int height, int width, const float* cams, const int32_t* view, float near,
                                       float far, const int64_t* pixel_index, int64_t n_rays, const float* images,
                                       int channels, float* rays, float* target, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(height > 0 && width > 0 && cams && view && pixel_index && rays && n_rays >= 0, "dn_select_rays_indirect: bad arguments");
  DN_REQUIRE(target == nullptr || (images != nullptr && channels >= 3), "dn_select_rays_indirect: target requested without images of >= 3 channels");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(select_rays_indirect_kernel<false>, dim3(grid), dim3(block), 0, as_stream(stream), cams, view, 0, height, width, near,
                     far, pixel_index, n_rays, images, channels, rays, target, static_cast<uint32_t*>(nullptr), static_cast<int64_t*>(nullptr),
                     0.0, 0.0);
  return check_launch("dn_select_rays_indirect");
}

extern "C" int dn_select_rays_indirect_ndc(int height, int width, const float* cams, const int32_t* view, float near, float far,
                                           const int64_t* pixel_index, int64_t n_rays, const float* images, int channels, float* rays,
                                           float* target, double focal, double ndc_near, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(height > 0 && width > 0 && cams && view && pixel_index && rays && n_rays >= 0, "dn_select_rays_indirect_ndc: bad arguments");
  DN_REQUIRE(target == nullptr || (images != nullptr && channels >= 3), "dn_select_rays_indirect_ndc: target requested without images of >= 3 channels");
  DN_REQUIRE(std::isfinite(focal) && focal > 0.0 && std::isfinite(ndc_near), "dn_select_rays_indirect_ndc: focal must be positive and finite, the near plane finite");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(select_rays_indirect_kernel<true>, dim3(grid), dim3(block), 0, as_stream(stream), cams, view, 0, height, width, near,
                     far, pixel_index, n_rays, images, channels, rays, target, static_cast<uint32_t*>(nullptr), static_cast<int64_t*>(nullptr),
                     focal, ndc_near);
  return check_launch("dn_select_rays_indirect_ndc");
}

extern "C" size_t dn_camera_grad_scratch_bytes(int64_t n_rays) {
  const int blocks = camera_grad_blocks(n_rays > 0 ? n_rays : 0);
  return static_cast<size_t>(blocks > 0 ? blocks : 1) * 16 * sizeof(double);
}

extern "C" int dn_camera_grad(int height, int width, const float* cam16, const int64_t* pixel_index, int64_t n_rays, const float* g_ro,
                              int ro_stride, const float* g_rd, int rd_stride, const float* g_viewdir, int vd_stride, double ndc_focal,
                              double ndc_near, void* scratch, size_t scratch_bytes, float* g_cam16, dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && n_rays >= 0, "dn_camera_grad: bad arguments (image size, ray count)");
  DN_REQUIRE(cam16 != nullptr && g_cam16 != nullptr, "dn_camera_grad: the camera record and its gradient must be given");
  DN_REQUIRE(g_ro != nullptr || g_rd != nullptr || g_viewdir != nullptr, "dn_camera_grad: no upstream gradient given");
  DN_REQUIRE((g_ro == nullptr || ro_stride >= 3) && (g_rd == nullptr || rd_stride >= 3) && (g_viewdir == nullptr || vd_stride >= 3),
             "dn_camera_grad: the row stride of an upstream gradient must be >= 3 floats");
  DN_REQUIRE(static_cast<int64_t>(height) * width < (1LL << 31), "dn_camera_grad: image too large");
  DN_REQUIRE(pixel_index != nullptr || n_rays <= static_cast<int64_t>(height) * width, "dn_camera_grad: more rays than pixels without a pixel index");
  DN_REQUIRE(std::isfinite(ndc_focal) && ndc_focal >= 0.0 && std::isfinite(ndc_near),
             "dn_camera_grad: ndc_focal must be finite and >= 0 (0: world-space rays), the near plane finite");
  DN_REQUIRE(scratch != nullptr && scratch_bytes >= dn_camera_grad_scratch_bytes(n_rays),
             "dn_camera_grad: scratch smaller than dn_camera_grad_scratch_bytes(n_rays)");
  DN_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 8 == 0, "dn_camera_grad: scratch must be 8-byte aligned");
  const int blocks = camera_grad_blocks(n_rays);
  double* partials = static_cast<double*>(scratch);
  if (blocks > 0) {
    hipLaunchKernelGGL(camera_grad_kernel, dim3(blocks), dim3(kCamGradThreads), 0, as_stream(stream), cam16, width, pixel_index, n_rays, g_ro,
                       ro_stride, g_rd, rd_stride, g_viewdir, vd_stride, static_cast<double>(height), ndc_focal, ndc_near, partials);
    const int rc = check_launch("dn_camera_grad");
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(camera_grad_finish_kernel, dim3(1), dim3(64), 0, as_stream(stream), partials, blocks, g_cam16);   // (no rays: 16 zeros)
  return check_launch("dn_camera_grad");
}

extern "C" int dn_select_rays_draw(int height, int width, const float* cams, const int32_t* view, int n_views, float near, float far,
                                   uint32_t* rng_state, int64_t n_rays, const float* images, int channels, float* rays, float* target,
                                   int64_t* pixel_index_out, dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && cams && (view || n_views >= 1) && rng_state && rays && n_rays >= 1, "dn_select_rays_draw: bad arguments");
  DN_REQUIRE(n_rays <= static_cast<int64_t>(height) * width, "dn_select_rays_draw: more rays than pixels (the draw is without replacement)");
  DN_REQUIRE(static_cast<int64_t>(height) * width < (1LL << 31), "dn_select_rays_draw: image too large");
  DN_REQUIRE(target == nullptr || (images != nullptr && channels >= 3), "dn_select_rays_draw: target requested without images of >= 3 channels");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(select_rays_indirect_kernel<false>, dim3(grid), dim3(block), 0, as_stream(stream), cams, view, n_views, height, width, near,
                     far, static_cast<const int64_t*>(nullptr), n_rays, images, channels, rays, target, rng_state, pixel_index_out, 0.0, 0.0);
  return check_launch("dn_select_rays_draw");
}

extern "C" int dn_select_rays_draw_ndc(int height, int width, const float* cams, const int32_t* view, int n_views, float near, float far,
                                       uint32_t* rng_state, int64_t n_rays, const float* images, int channels, float* rays, float* target,
                                       int64_t* pixel_index_out, double focal, double ndc_near, dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && cams && (view || n_views >= 1) && rng_state && rays && n_rays >= 1, "dn_select_rays_draw_ndc: bad arguments");
  DN_REQUIRE(n_rays <= static_cast<int64_t>(height) * width, "dn_select_rays_draw_ndc: more rays than pixels (the draw is without replacement)");
  DN_REQUIRE(static_cast<int64_t>(height) * width < (1LL << 31), "dn_select_rays_draw_ndc: image too large");
  DN_REQUIRE(target == nullptr || (images != nullptr && channels >= 3), "dn_select_rays_draw_ndc: target requested without images of >= 3 channels");
  DN_REQUIRE(std::isfinite(focal) && focal > 0.0 && std::isfinite(ndc_near), "dn_select_rays_draw_ndc: focal must be positive and finite, the near plane finite");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(select_rays_indirect_kernel<true>, dim3(grid), dim3(block), 0, as_stream(stream), cams, view, n_views, height, width, near,
                     far, static_cast<const int64_t*>(nullptr), n_rays, images, channels, rays, target, rng_state, pixel_index_out, focal,
                     ndc_near);
  return check_launch("dn_select_rays_draw_ndc");
}

extern "C" int dn_select_rays_views(int height, int width, const float* cams, int n_views, const int32_t* view_index, float near, float far,
                                    const int64_t* pixel_index, int64_t n_rays, const float* images, int channels, float* rays, float* target,
                                    double ndc_focal, double ndc_near, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(height > 0 && width > 0 && rays && n_rays >= 0, "dn_select_rays_views: bad arguments (image size, ray count, rows)");
  DN_REQUIRE(cams != nullptr && n_views >= 1, "dn_select_rays_views: the camera records (n_views >= 1) must be given");
  DN_REQUIRE(view_index != nullptr && pixel_index != nullptr, "dn_select_rays_views: view_index and pixel_index must be given");
  DN_REQUIRE(static_cast<int64_t>(n_views) * height * width < (1LL << 31), "dn_select_rays_views: n_views x image too large (V H W must be < 2^31)");
  DN_REQUIRE(target == nullptr || (images != nullptr && channels >= 3), "dn_select_rays_views: target requested without images of >= 3 channels");
  DN_REQUIRE(std::isfinite(ndc_focal) && ndc_focal >= 0.0 && std::isfinite(ndc_near),
             "dn_select_rays_views: ndc_focal must be finite and >= 0 (0: world-space rays), the near plane finite");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  if (ndc_focal > 0.0) {
    hipLaunchKernelGGL(select_rays_views_kernel<true>, dim3(grid), dim3(block), 0, as_stream(stream), cams, view_index, n_views, height, width, near,
                       far, pixel_index, n_rays, images, channels, rays, target, static_cast<uint32_t*>(nullptr), static_cast<int64_t*>(nullptr),
                       static_cast<int*>(nullptr), ndc_focal, ndc_near);
  } else {
    hipLaunchKernelGGL(select_rays_views_kernel<false>, dim3(grid), dim3(block), 0, as_stream(stream), cams, view_index, n_views, height, width, near,
                       far, pixel_index, n_rays, images, channels, rays, target, static_cast<uint32_t*>(nullptr), static_cast<int64_t*>(nullptr),
                       static_cast<int*>(nullptr), 0.0, 0.0);
  }
  return check_launch("dn_select_rays_views");
}

extern "C" int dn_select_rays_draw_views(int height, int width, const float* cams, int n_views, float near, float far, uint32_t* rng_state,
                                         int64_t n_rays, const float* images, int channels, float* rays, float* target,
                                         int64_t* pixel_index_out, int32_t* view_index_out, double ndc_focal, double ndc_near, dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && rng_state && rays, "dn_select_rays_draw_views: bad arguments (image size, RNG state, rows)");
  DN_REQUIRE(cams != nullptr && n_views >= 1, "dn_select_rays_draw_views: the camera records (n_views >= 1) must be given");
  DN_REQUIRE(static_cast<int64_t>(n_views) * height * width < (1LL << 31), "dn_select_rays_draw_views: n_views x image too large (V H W must be < 2^31)");
  DN_REQUIRE(n_rays >= 1 && n_rays <= static_cast<int64_t>(n_views) * height * width,
             "dn_select_rays_draw_views: need 1 <= n_rays <= V H W (the draw is without replacement)");
  DN_REQUIRE(target == nullptr || (images != nullptr && channels >= 3), "dn_select_rays_draw_views: target requested without images of >= 3 channels");
  DN_REQUIRE(std::isfinite(ndc_focal) && ndc_focal >= 0.0 && std::isfinite(ndc_near),
             "dn_select_rays_draw_views: ndc_focal must be finite and >= 0 (0: world-space rays), the near plane finite");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  if (ndc_focal > 0.0) {
    hipLaunchKernelGGL(select_rays_views_kernel<true>, dim3(grid), dim3(block), 0, as_stream(stream), cams, static_cast<const int*>(nullptr), n_views,
                       height, width, near, far, static_cast<const int64_t*>(nullptr), n_rays, images, channels, rays, target, rng_state,
                       pixel_index_out, view_index_out, ndc_focal, ndc_near);
  } else {
    hipLaunchKernelGGL(select_rays_views_kernel<false>, dim3(grid), dim3(block), 0, as_stream(stream), cams, static_cast<const int*>(nullptr), n_views,
                       height, width, near, far, static_cast<const int64_t*>(nullptr), n_rays, images, channels, rays, target, rng_state,
                       pixel_index_out, view_index_out, 0.0, 0.0);
  }
  return check_launch("dn_select_rays_draw_views");
}

extern "C" size_t dn_camera_grad_views_scratch_bytes(int64_t n_rays, int n_views) {
  const int blocks = camera_grad_blocks(n_rays > 0 ? n_rays : 0);
  return static_cast<size_t>(blocks > 0 ? blocks : 1) * static_cast<size_t>(n_views > 0 ? n_views : 1) * 16 * sizeof(double);
}

extern "C" int dn_camera_grad_views(int height, int width, const float* cams, int n_views, const int32_t* view_index, const int64_t* pixel_index,
                                    int64_t n_rays, const float* g_ro, int ro_stride, const float* g_rd, int rd_stride, const float* g_viewdir,
                                    int vd_stride, double ndc_focal, double ndc_near, void* scratch, size_t scratch_bytes, float* g_cams,
                                    dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && n_rays >= 0, "dn_camera_grad_views: bad arguments (image size, ray count)");
  DN_REQUIRE(cams != nullptr && g_cams != nullptr, "dn_camera_grad_views: the camera records and their gradient must be given");
  DN_REQUIRE(n_views >= 1 && n_views <= 65535, "dn_camera_grad_views: n_views must be in [1, 65535]");
  DN_REQUIRE(view_index != nullptr && pixel_index != nullptr, "dn_camera_grad_views: view_index and pixel_index must be given");
  DN_REQUIRE(g_ro != nullptr || g_rd != nullptr || g_viewdir != nullptr, "dn_camera_grad_views: no upstream gradient given");
  DN_REQUIRE((g_ro == nullptr || ro_stride >= 3) && (g_rd == nullptr || rd_stride >= 3) && (g_viewdir == nullptr || vd_stride >= 3),
             "dn_camera_grad_views: the row stride of an upstream gradient must be >= 3 floats");
  DN_REQUIRE(static_cast<int64_t>(n_views) * height * width < (1LL << 31), "dn_camera_grad_views: n_views x image too large (V H W must be < 2^31)");
  DN_REQUIRE(std::isfinite(ndc_focal) && ndc_focal >= 0.0 && std::isfinite(ndc_near),
             "dn_camera_grad_views: ndc_focal must be finite and >= 0 (0: world-space rays), the near plane finite");
  DN_REQUIRE(scratch != nullptr && scratch_bytes >= dn_camera_grad_views_scratch_bytes(n_rays, n_views),
             "dn_camera_grad_views: scratch smaller than dn_camera_grad_views_scratch_bytes(n_rays, n_views)");
  DN_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 8 == 0, "dn_camera_grad_views: scratch must be 8-byte aligned");
  const int blocks = camera_grad_blocks(n_rays);
  double* partials = static_cast<double*>(scratch);
  if (blocks > 0) {
    hipLaunchKernelGGL(camera_grad_views_kernel, dim3(blocks, n_views), dim3(kCamGradThreads), 0, as_stream(stream), cams, width, view_index,
                       pixel_index, n_rays, g_ro, ro_stride, g_rd, rd_stride, g_viewdir, vd_stride, static_cast<double>(height), ndc_focal,
                       ndc_near, partials);
    const int rc = check_launch("dn_camera_grad_views");
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(camera_grad_finish_kernel, dim3(n_views), dim3(64), 0, as_stream(stream), partials, blocks, g_cams);   // (no rays: V x 16 zeros)
  return check_launch("dn_camera_grad_views");
}

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
}  // namespace dn

namespace dn {
__global__ void rng_fill_kernel(const uint32_t* __restrict__ state, uint32_t stream, int64_t n, int normal, float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const RngRef r{state, stream};
  out[i] = normal ? rng_normal(r, static_cast<uint64_t>(i)) : rng_uniform(r, static_cast<uint64_t>(i));
}
}  // namespace dn

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

// ---- S2 ray packing of run_one_iter_of_nerf (nerf/train_utils.py:220-250): (N,3) origins / directions -> the (N, 8 | 11) rows
// [o, d, near, far, d_view / |d_view|] predict_and_render_radiance reads - the reference forms them with a norm, a division, two
// ones_like, two multiplies and a cat (eight launches per image); op for op as those run on the device.
namespace dn {
__global__ void pack_ray_rows_kernel(const float* __restrict__ ro, const float* __restrict__ rd, const float* __restrict__ rd_view,
                                     float near, float far, int64_t n, float* __restrict__ rows) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float* r = rows + i * (rd_view != nullptr ? 11 : 8);
#pragma unroll
  for (int j = 0; j < 3; ++j) { r[j] = ro[i * 3 + j]; r[3 + j] = rd[i * 3 + j]; }
  r[6] = near;
  r[7] = far;
  if (rd_view != nullptr) {
    const float x = rd_view[i * 3], y = rd_view[i * 3 + 1], z = rd_view[i * 3 + 2];
    // the order of torch's device reduction over three elements ((x x + z z) + y y: measured, scripts/rows_diag.py) - this kernel
    // replaces torch ops that ran on the device, and the rows stay bit-identical to them
    const float nrm = sqrtf((x * x + z * z) + y * y);
    r[8] = x / nrm; r[9] = y / nrm; r[10] = z / nrm;
  }
}
}  // namespace dn

extern "C" int dn_pack_ray_rows(const float* rays_o, const float* rays_d, const float* view_d, float near, float far, int64_t n_rays,
                                float* rows, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(rays_o && rays_d && rows && n_rays >= 0, "dn_pack_ray_rows: bad arguments");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(pack_ray_rows_kernel, dim3(grid), dim3(block), 0, as_stream(stream), rays_o, rays_d, view_d, near, far, n_rays, rows);
  return check_launch("dn_pack_ray_rows");
}

extern "C" int dn_ndc_rays(int height, int width, double focal, double near, const float* rays_o, const float* rays_d,
                           int64_t n_rays, float* rays_o_out, float* rays_d_out, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(rays_o && rays_d && rays_o_out && rays_d_out && n_rays >= 0 && height > 0 && width > 0, "dn_ndc_rays: bad arguments");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(ndc_rays_kernel, dim3(grid), dim3(block), 0, as_stream(stream), static_cast<double>(height),
                     static_cast<double>(width), focal, near, rays_o, rays_d, n_rays, rays_o_out, rays_d_out);
  return check_launch("dn_ndc_rays");
}

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
