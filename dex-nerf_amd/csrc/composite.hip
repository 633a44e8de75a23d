// volume_render_radiance_field forward / backward (reference nerf/volume_rendering_utils.py:6-70,
// cumprod_exclusive nerf/nerf_helpers.py:43-64) with the Dex-NeRF fixed-sigma depth readout.
//
// One wave64 per ray, samples laid out lane-contiguous (sample s = 64*chunk + lane) so every wave
// instruction reads one coalesced run of the (ray, sample) row; the transmittance product is a
// wave-level fp64 scan with a carry between 64-sample chunks (ATen's CPU cumprod accumulates in double
// and rounds each prefix to fp32), the Dex readout is a ballot + first-set-bit per threshold.
// HBM-bound: 20 B/sample in (rf float4 + z), (10+K)*4 B/ray out; backward 40 B/sample, its geometry form 44 B/sample + 12 B/ray.
#include "composite_body.h"

namespace dn {

constexpr int kRaysPerBlock = 4;  // 256 threads

__global__ __launch_bounds__(256) void composite_fwd_kernel(
    const float4* __restrict__ rf, const float* __restrict__ z, const float* __restrict__ rd, int rd_stride,
    const float* __restrict__ noise, float noise_std, int white, ThresArgs th, int n_thres, int64_t n_rays, int S,
    float* __restrict__ rgb, float* __restrict__ disp, float* __restrict__ acc, float* __restrict__ weights,
    float* __restrict__ depth, float* __restrict__ dex, unsigned* __restrict__ nonfinite, RngRef rng) {
  const int lane = lane_id();
  const int64_t ray = static_cast<int64_t>(blockIdx.x) * kRaysPerBlock + (threadIdx.x >> 6);
  if (ray >= n_rays) return;  // wave-uniform exit; no block-level sync in this kernel
  const float4* rfr = rf + ray * S;
  composite_ray([&](int sc) { return rfr[sc]; }, DrawnNoise{noise, rng, noise_std, ray, S}, z + ray * S, rd + ray * rd_stride, ray, lane,
                white, th, n_thres, n_rays, S, rgb, disp, acc, weights, depth, dex, nonfinite);
}

// Backward w.r.t. rf (checked against autograd of the reference in fp64):
//   s_i = gC.c_i + gD z_i + gA + gW_i ;  R_i = sum_{k>i} s_k w_k ;  dL/dalpha_i = s_i T_i - R_i / o_i ;
//   dL/dsigma_i = dL/dalpha_i * dist_i * exp(-sigma_i dist_i) ; dL/draw_sigma = [raw+noise > 0] * that ;
//   dL/draw_rgb = w_i * gC * c (1 - c).
//
// GEOM: the geometry form (dn_volume_render_backward_geom) - the same wave, scan and sample_terms, and besides g_rf (now optional)
// the gradients w.r.t. the depths and the direction the intervals dist_i = dz_i |rd| are made of (dz_i = z[i+1] - z[i]; the last
// sample's interval is the constant 1e10):
//   ddist_i = dL/dalpha_i * sigma_i * exp(-sigma_i dist_i)   (0 where raw+noise <= 0)
//   g_z_i   = gD w_i + |rd| (ddist_{i-1} - ddist_i)          (ddist_{-1} = 0; the last sample has no -ddist term)
//   g_rd    = (sum_i ddist_i dz_i) rd / |rd|                 (the last sample included, with dz = 1e10)
// The second loop runs over the chunks in descending order and g_z needs the previous sample's ddist across the chunk boundary:
// ddist is kept per chunk and a third, ascending pass hands lane 63's value on as a carry, as the forward scan does.  Plain stores;
// g_rd is one lane-local sum in chunk order followed by the fixed butterfly of wave_sum: bit-reproducible.  GEOM = false compiles to
// the kernel as it was.
__device__ __forceinline__ float wave_shift_up1(float v, float first) {   // lane l - 1's value (lane 0: `first`)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, first), __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, false));   // wave_shr:1
}

template <int MAXC, bool GEOM>
__global__ __launch_bounds__(256) void composite_bwd_kernel(
    const float4* __restrict__ rf, const float* __restrict__ z, const float* __restrict__ rd, int rd_stride,
    const float* __restrict__ noise, float noise_std, int white, int64_t n_rays, int S, const float* __restrict__ g_rgb,
    const float* __restrict__ g_depth, const float* __restrict__ g_acc, const float* __restrict__ g_disp,
    const float* __restrict__ g_weights, float4* __restrict__ g_rf, RngRef rng, unsigned* __restrict__ absmax_part,
    float* __restrict__ g_z, float* __restrict__ g_rd) {
  const int lane = lane_id();
  const int64_t ray_of_wave = static_cast<int64_t>(blockIdx.x) * kRaysPerBlock + (threadIdx.x >> 6);
  // absmax_part (the 8-bit-saved-tensor training path, api.cpp): this workgroup's largest finite |gradient it stores| goes to
  // absmax_part[blockIdx.x] - what absmax_kernel (mlp_train48.hip) would otherwise read g_rf again for.  Every workgroup writes its
  // word (nothing needs zeroing), so a wave without a ray stays for the workgroup's exchange: it works on the last ray and stores nothing.
  const bool live = ray_of_wave < n_rays;
  if (!live && absmax_part == nullptr) return;
  const int64_t ray = live ? ray_of_wave : n_rays - 1;
  float gmax = 0.0f;
  const float dx = rd[ray * rd_stride + 0], dy = rd[ray * rd_stride + 1], dz = rd[ray * rd_stride + 2];
  const float rd_norm = sqrtf((dx * dx + dy * dy) + dz * dz);
  const float* zr = z + ray * S;
  const float4* rfr = rf + ray * S;
  float gc0 = 0.f, gc1 = 0.f, gc2 = 0.f, gd = 0.f, ga = 0.f;
  if (g_rgb != nullptr) { gc0 = g_rgb[ray * 3]; gc1 = g_rgb[ray * 3 + 1]; gc2 = g_rgb[ray * 3 + 2]; }
  if (g_depth != nullptr) gd = g_depth[ray];
  if (g_acc != nullptr) ga = g_acc[ray];
  if (white) ga -= (gc0 + gc1 + gc2);

  float w_[MAXC], t_[MAXC], om_[MAXC], de_[MAXC], sw_[MAXC], s_[MAXC], c0_[MAXC], c1_[MAXC], c2_[MAXC];
  bool pos_[MAXC];
  // GEOM: dz_i, and sigma_i exp(-sigma_i dist_i) = ddist_i / dalpha_i, which the second loop turns into ddist_i in place
  float dzv_[GEOM ? MAXC : 1], dd_[GEOM ? MAXC : 1];
  double carry = 1.0;
  float sum_d = 0.f, sum_a = 0.f;
  const DrawnNoise noise_at{noise, rng, noise_std, ray, S};
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int base = c * 64;
    const int s = base + lane;
    const bool valid = s < S;
    const int sc = valid ? s : S - 1;
    const float4 raw = rfr[sc];
    const float z0 = zr[sc];
    const float z1 = (sc + 1 < S) ? zr[sc + 1] : z0;
    const SampleTerms t = sample_terms(raw.w, noise_at(sc), noise_std, z0, z1, sc == S - 1, rd_norm);   // (the forward's noise again)
    const auto [trans, w] = transmittance_step(t.alpha, t.one_m_alpha, valid, s, carry);
    c0_[c] = sigmoidf_(raw.x); c1_[c] = sigmoidf_(raw.y); c2_[c] = sigmoidf_(raw.z);
    w_[c] = w; t_[c] = trans; om_[c] = t.one_m_alpha;
    de_[c] = t.dist * expf(-t.sigma * t.dist);  // dalpha/dsigma
    if constexpr (GEOM) {
      dzv_[c] = (sc == S - 1) ? 1e10f : (z1 - z0);
      dd_[c] = t.sigma * expf(-t.sigma * t.dist);   // dalpha/ddist
    }
    pos_[c] = valid && (t.sigma > 0.0f);
    s_[c] = z0;  // z for now; turned into s_i below once gD is final
    sum_d += w * z0;
    sum_a += w;
  }
  if (g_disp != nullptr) {
    // disp = 1 / max(1e-10, depth/acc): only the q > 1e-10 branch has a gradient
    sum_d = wave_sum(sum_d);
    sum_a = wave_sum(sum_a);
    const float q = sum_d / sum_a;
    if (q > 1e-10f) {
      const float gq = -g_disp[ray] / (q * q);
      gd += gq / sum_a;
      ga += -gq * sum_d / (sum_a * sum_a);
    }
  }
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int s = c * 64 + lane;
    float si = (gc0 * c0_[c] + gc1 * c1_[c] + gc2 * c2_[c]) + gd * s_[c] + ga;
    if (g_weights != nullptr && s < S) si += g_weights[ray * S + s];
    s_[c] = si;
    sw_[c] = (s < S) ? si * w_[c] : 0.0f;
  }
  // reverse exclusive scan of s_k w_k over the whole ray
  float tail = 0.0f;  // sum over all later chunks
#pragma unroll
  for (int c = MAXC - 1; c >= 0; --c) {
    const float incl = wave_scan_add(sw_[c]);            // prefix within chunk
    const float total = __shfl(incl, 63, 64);
    const float suffix_excl = (total - incl) + tail;     // sum_{k > i} within chunk + later chunks
    tail += total;
    const int s = c * 64 + lane;
    if constexpr (GEOM) {
      if (s >= S) dd_[c] = 0.0f;
    }
    if (s < S) {
      const float dalpha = s_[c] * t_[c] - suffix_excl / om_[c];
      const float dsig = pos_[c] ? dalpha * de_[c] : 0.0f;
      if constexpr (GEOM) dd_[c] = pos_[c] ? dalpha * dd_[c] : 0.0f;
      float4 g;
      g.x = w_[c] * gc0 * c0_[c] * (1.0f - c0_[c]);
      g.y = w_[c] * gc1 * c1_[c] * (1.0f - c1_[c]);
      g.z = w_[c] * gc2 * c2_[c] * (1.0f - c2_[c]);
      g.w = dsig;
      if (live && (!GEOM || g_rf != nullptr)) {
        g_rf[ray * S + s] = g;
        const float a0 = fabsf(g.x), a1 = fabsf(g.y), a2 = fabsf(g.z), a3 = fabsf(g.w);
        gmax = (a0 < 3.0e38f) ? fmaxf(gmax, a0) : gmax;   // (a non-finite gradient does not set the scale: absmax_kernel's rule)
        gmax = (a1 < 3.0e38f) ? fmaxf(gmax, a1) : gmax;
        gmax = (a2 < 3.0e38f) ? fmaxf(gmax, a2) : gmax;
        gmax = (a3 < 3.0e38f) ? fmaxf(gmax, a3) : gmax;
      }
    }
  }
  if constexpr (GEOM) {
    // third pass, ascending: the previous sample's ddist (lane 63 of the chunk before as the carry)
    float prev_last = 0.0f, rd_sum = 0.0f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int s = c * 64 + lane;
      const float prev = wave_shift_up1(dd_[c], prev_last);
      prev_last = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dd_[c]), 63));
      if (s < S) {
        const float own = (s == S - 1) ? 0.0f : dd_[c];   // the last interval is a constant: no -ddist term
        if (g_z != nullptr) g_z[ray * S + s] = gd * w_[c] + rd_norm * (prev - own);
        rd_sum += dd_[c] * dzv_[c];
      }
    }
    if (g_rd != nullptr) {
      rd_sum = wave_sum(rd_sum);
      if (lane < 3) g_rd[ray * 3 + lane] = rd_sum * (lane == 0 ? dx : (lane == 1 ? dy : dz)) / rd_norm;
    }
  }
  if (absmax_part != nullptr) {   // (workgroup-uniform)
    __shared__ float wave_max[kRaysPerBlock];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, o, 64));
    if (lane == 0) wave_max[threadIdx.x >> 6] = gmax;
    __syncthreads();
    if (threadIdx.x == 0) {
      float r = wave_max[0];
#pragma unroll
      for (int w = 1; w < kRaysPerBlock; ++w) r = fmaxf(r, wave_max[w]);
      absmax_part[blockIdx.x] = __float_as_uint(r);
    }
  }
}

}  // namespace dn

using namespace dn;

extern "C" int dn_volume_render(const float* rf, const float* z, const float* rd, int rd_stride, const float* noise,
                                float noise_std, int white_background, const float* h_m_thres, int n_thres,
                                int64_t n_rays, int n_samples, float* rgb, float* disp, float* acc, float* weights,
                                float* depth, float* dex, dn_stream_t stream) {
  return dn::volume_render_counting(rf, z, rd, rd_stride, noise, noise_std, white_background, h_m_thres, n_thres, n_rays, n_samples,
                                    rgb, disp, acc, weights, depth, dex, nullptr, stream);
}

// dn_volume_render + a count of the non-finite raw radiance-field values it met, added to *nonfinite (device word, may be NULL)
int dn::volume_render_counting(const float* rf, const float* z, const float* rd, int rd_stride, const float* noise,
                               float noise_std, int white_background, const float* h_m_thres, int n_thres,
                               int64_t n_rays, int n_samples, float* rgb, float* disp, float* acc, float* weights,
                               float* depth, float* dex, unsigned* nonfinite, dn_stream_t stream, const uint32_t* rng_state,
                               uint32_t rng_stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(rf && z && rd && n_rays >= 0 && n_samples >= 1 && rd_stride >= 3, "dn_volume_render: bad arguments");
  DN_REQUIRE(n_thres >= 0 && n_thres <= kMaxThres, "dn_volume_render: at most %d Dex thresholds", kMaxThres);
  DN_REQUIRE(n_thres == 0 || (h_m_thres && dex), "dn_volume_render: thresholds given without dex output");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(rf) & 15) == 0, "dn_volume_render: rf must be 16-byte aligned");
  ThresArgs th;
  for (int k = 0; k < kMaxThres; ++k) th.m[k] = (k < n_thres) ? h_m_thres[k] : 0.0f;
  const unsigned grid = static_cast<unsigned>((n_rays + kRaysPerBlock - 1) / kRaysPerBlock);
  hipLaunchKernelGGL(composite_fwd_kernel, dim3(grid), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(rf), z, rd, rd_stride, noise, noise_std, white_background, th,
                     n_thres, n_rays, n_samples, rgb, disp, acc, weights, depth, dex, nonfinite, RngRef{rng_state, rng_stream});
  return check_launch("dn_volume_render");
}

// The one launcher of composite_bwd_kernel (dn_volume_render_backward, dn_volume_render_backward_geom and the backward driver of
// api.cpp; `name`: the entry point, for messages).  g_z / g_rd (the geometry outputs) and absmax_part are optional; GEOM is chosen by
// whether a geometry output is wanted - none: the plain kernel, which needs g_rf.  noise == NULL with an RNG state: the forward's
// density noise regenerated in the kernel.
using CompositeBwdKernel = decltype(&composite_bwd_kernel<1, false>);

static CompositeBwdKernel composite_bwd_instance(int chunks, bool geom) {
  if (chunks <= 1) return geom ? composite_bwd_kernel<1, true> : composite_bwd_kernel<1, false>;
  if (chunks <= 2) return geom ? composite_bwd_kernel<2, true> : composite_bwd_kernel<2, false>;
  if (chunks <= 4) return geom ? composite_bwd_kernel<4, true> : composite_bwd_kernel<4, false>;
  if (chunks <= 8) return geom ? composite_bwd_kernel<8, true> : composite_bwd_kernel<8, false>;
  return geom ? composite_bwd_kernel<16, true> : composite_bwd_kernel<16, false>;
}

int dn::volume_render_backward_rng(const char* name, const float* rf, const float* z, const float* rd, int rd_stride, const float* noise,
                                   float noise_std, int white_background, int64_t n_rays, int n_samples, const float* g_rgb,
                                   const float* g_depth, const float* g_acc, const float* g_disp, const float* g_weights, float* g_rf,
                                   float* g_z, float* g_rd, const uint32_t* rng_state, uint32_t rng_stream, unsigned* absmax_part,
                                   dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(rf && z && rd && (g_rf || g_z || g_rd) && n_rays >= 0 && n_samples >= 1 && rd_stride >= 3, "%s: bad arguments", name);
  DN_REQUIRE(n_samples <= 1024, "%s: at most 1024 samples per ray", name);
  DN_REQUIRE(((reinterpret_cast<uintptr_t>(rf) | reinterpret_cast<uintptr_t>(g_rf)) & 15) == 0, "%s: rf / g_rf must be 16-byte aligned", name);
  const unsigned grid = static_cast<unsigned>((n_rays + kRaysPerBlock - 1) / kRaysPerBlock);
  hipLaunchKernelGGL(composite_bwd_instance((n_samples + 63) / 64, g_z != nullptr || g_rd != nullptr), dim3(grid), dim3(256), 0,
                     as_stream(stream), reinterpret_cast<const float4*>(rf), z, rd, rd_stride, noise, noise_std, white_background, n_rays,
                     n_samples, g_rgb, g_depth, g_acc, g_disp, g_weights, reinterpret_cast<float4*>(g_rf), RngRef{rng_state, rng_stream},
                     absmax_part, g_z, g_rd);
  return check_launch(name);
}

extern "C" int dn_volume_render_backward(const float* rf, const float* z, const float* rd, int rd_stride,
                                         const float* noise, float noise_std, int white_background, int64_t n_rays,
                                         int n_samples, const float* g_rgb, const float* g_depth, const float* g_acc,
                                         const float* g_disp, const float* g_weights, float* g_rf,
                                         dn_stream_t stream) {
  return dn::volume_render_backward_rng("dn_volume_render_backward", rf, z, rd, rd_stride, noise, noise_std, white_background, n_rays, n_samples,
                                        g_rgb, g_depth, g_acc, g_disp, g_weights, g_rf, nullptr, nullptr, nullptr, 0u, nullptr, stream);
}

extern "C" int dn_volume_render_backward_geom(const float* rf, const float* z, const float* rd, int rd_stride, const float* noise,
                                              float noise_std, int white_background, int64_t n_rays, int n_samples,
                                              const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_disp,
                                              const float* g_weights, float* g_rf, float* g_z, float* g_rd, dn_stream_t stream) {
  return dn::volume_render_backward_rng("dn_volume_render_backward_geom", rf, z, rd, rd_stride, noise, noise_std, white_background, n_rays,
                                        n_samples, g_rgb, g_depth, g_acc, g_disp, g_weights, g_rf, g_z, g_rd, nullptr, 0u, nullptr, stream);
}
