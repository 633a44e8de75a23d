// Dex depth layers (include/dexnerf_hip_layers.h): every entry into and exit from {sigma > m} along a ray.
//   composite_layers_kernel    composite_density_kernel without noise (forward_ray without the first-crossing hook: depth, acc and dex
//                              carry dn_composite_density's bits), then one more pass per threshold over the ray's sigma column -
//                              L2-resident by then, as for the threshold groups past 64 - that counts the state changes and keeps
//                              the first 2L of them as bracket records (z_lo, z_hi, s_lo, s_hi) with their first midpoints
//   layers_thresholds_kernel   the thresholds repeated 2L times each: what dn_dex_bisect's kernel reads as ITS thresholds on the
//                              records (N, K*2L) - the step rule does not ask which end of a bracket is deeper, so exits take the
//                              same step as entries
//   dex_layers_finish_kernel   the event depths (K,2L,N) and widths: elementwise, like dex_refine_finish_kernel, and it knows an exit
//                              from an entry by the parity of the event
// One wave64 per ray, four rays per workgroup, like composite_density.hip; plain vector stores, no LDS, no atomics beyond forward_ray's
// non-finite counter, no workgroup waits on another.
//
// The event pass, per 64-sample chunk: ballot `above`; prev = (above << 1) | carry is the state of each lane's previous sample (carry:
// the state of the last sample of the chunk before, false ahead of sample 0); the transitions are (above ^ prev) masked to the lanes
// that hold a sample; their popcount goes to the count; while fewer than 2L events are held the set bits are taken in ascending order
// and lane e keeps the sample index of event e.  Chunk edges:
//   an event at sample 0 of a chunk   bit 0 of prev is the carry, so lane 0's transition compares with sample 63 of the chunk before
//   a ragged last chunk               lanes past S-1 ballot false and are masked out of the transitions: the end of the ray is no event;
//                                     the carry it leaves is never read (it is the last chunk)
//   S = 1                             one chunk, one valid lane, carry false: an entry at 0 or nothing
// Everything of the pass but a lane's own kept index is wave-uniform (ballots, popcounts, the held count): scalar registers.
//
// Memory: per (ray, threshold) the pass re-reads S densities (4 B each, strided 16 B: the .w column) from L2 and stores 2L records of
// 16 B + 4 B and one count; the lanes below 2L re-read two depths and two densities each.
#include "../../include/dexnerf_hip_layers.h"
#include "composite_body.h"

namespace dn {

constexpr int kLayersBlock = 256;

__global__ __launch_bounds__(256) void composite_layers_kernel(const float4* __restrict__ rf, const float* __restrict__ z,
                                                               const float* __restrict__ rd, int rd_stride, const float* __restrict__ d_thres,
                                                               int n_thres, int n_events, int64_t n_rays, int S, float* __restrict__ depth,
                                                               float* __restrict__ acc, float* __restrict__ dex, float4* __restrict__ br,
                                                               float* __restrict__ z_mid, int* __restrict__ count,
                                                               unsigned* __restrict__ nonfinite) {
  const int lane = lane_id();
  const int64_t ray = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (ray >= n_rays) return;  // wave-uniform exit; no block-level sync in this kernel
  const SigmaColumn sig(rf + ray * S);
  const float* zr = z + ray * S;
  forward_ray(sig, TensorNoise{nullptr, 0.0f, ray, S}, DeviceThres{d_thres, dex != nullptr ? n_thres : 0}, zr, rd + ray * rd_stride, ray, true,
              lane, n_rays, S, acc, depth, dex, nonfinite, [](int, bool, float, float) {});
  for (int k = 0; k < n_thres; ++k) {   // wave-uniform
    const float m = d_thres[k];
    unsigned long long carry = 0ull;   // above_{base - 1}
    int total = 0, held = 0;           // wave-uniform: events met, events kept (<= n_events)
    int mine = -1;                     // lane e: the sample index of event e
    for (int base = 0; base < S; base += 64) {
      const int s = base + lane;
      const bool valid = s < S;
      const float v = sig(valid ? s : S - 1);
      const unsigned long long above = __ballot(valid && (v > m));   // NaN is not above, +inf is
      const int left = S - base;
      const unsigned long long lanes = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
      unsigned long long events = (above ^ ((above << 1) | carry)) & lanes;
      carry = above >> 63;
      total += __builtin_popcountll(events);
      while (held < n_events && events != 0ull) {
        if (lane == held) mine = base + __builtin_ctzll(events);
        events &= events - 1ull;
        ++held;
      }
    }
    const int64_t row = ray * n_thres + k;
    if (lane < n_events) {
      float4 r;
      if (mine < 0) {
        r = make_float4(zr[0], zr[0], __builtin_inff(), -__builtin_inff());
      } else {
        const int before = mine > 0 ? mine - 1 : 0;
        // an entry's hi end is the sample of the event, an exit's is the sample before it: the hi end is the one above m
        const int lo = (lane & 1) ? mine : before, hi = (lane & 1) ? before : mine;
        r = make_float4(zr[lo], zr[hi], sig(lo), sig(hi));
      }
      const int64_t rec = row * n_events + lane;
      br[rec] = r;
      z_mid[rec] = r.x + 0.5f * (r.y - r.x);
    }
    if (lane == 0) count[static_cast<int64_t>(k) * n_rays + ray] = total;
  }
}

// out[k * n_events + e] = d_thres[k]
__global__ __launch_bounds__(kLayersBlock) void layers_thresholds_kernel(const float* __restrict__ d_thres, int n_events, int n_out,
                                                                         float* __restrict__ out) {
  const int idx = blockIdx.x * kLayersBlock + threadIdx.x;
  if (idx < n_out) out[idx] = d_thres[idx / n_events];
}

// output idx = (k * 2L + e) * N + ray: the stores are coalesced, the 16-byte record loads K 2L records apart
__global__ __launch_bounds__(kLayersBlock) void dex_layers_finish_kernel(const float4* __restrict__ br, const float* __restrict__ d_thres,
                                                                         int n_thres, int n_events, int interp, int64_t n_rays,
                                                                         float* __restrict__ events, float* __restrict__ width) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kLayersBlock + threadIdx.x;
  const int64_t per_ray = static_cast<int64_t>(n_thres) * n_events;
  if (idx >= n_rays * per_ray) return;
  const int64_t ke = idx / n_rays, ray = idx - ke * n_rays;
  const int k = static_cast<int>(ke / n_events), e = static_cast<int>(ke - static_cast<int64_t>(k) * n_events);
  const float4 r = br[ray * per_ray + ke];   // (z_lo, z_hi, s_lo, s_hi)
  float out, wd;
  if (r.w == -__builtin_inff()) {
    out = __builtin_inff();   // no such event: the ray never gets there
    wd = -1.0f;
  } else if (interp == 0) {
    out = (e & 1) ? r.x : r.y;   // the sample at which the state changes: an entry's hi end, an exit's lo end
    wd = fabsf(r.y - r.x);
  } else if (r.x == r.y) {
    out = r.x;
    wd = 0.0f;
  } else {
    const bool finite = (r.z - r.z == 0.0f) && (r.w - r.w == 0.0f);
    const double m = static_cast<double>(d_thres[k]);
    const double lo = static_cast<double>(r.x), hi = static_cast<double>(r.y), s_lo = static_cast<double>(r.z), s_hi = static_cast<double>(r.w);
    const double t = finite ? (m - s_lo) / (s_hi - s_lo) : 0.5;
    out = static_cast<float>(lo + (hi - lo) * t);   // fp64 from the fp32 inputs, rounded once: dex_refine_finish_kernel's formula
    wd = fabsf(r.y - r.x);
  }
  events[idx] = out;
  if (width != nullptr) width[idx] = wd;
}

int layers_check(const char* who, int n_thres, int n_layers, int64_t n_rays) {
  DN_REQUIRE(n_thres >= 1, "%s: needs at least one threshold", who);
  DN_REQUIRE(n_layers >= 1 && n_layers <= DN_MAX_LAYERS, "%s: need 1 <= n_layers <= %d", who, DN_MAX_LAYERS);
  DN_REQUIRE(n_thres <= DN_MAX_LAYER_RECORDS / (2 * n_layers), "%s: at most %d records per ray (n_thres * 2 n_layers)", who,
             DN_MAX_LAYER_RECORDS);
  DN_REQUIRE(n_rays <= INT64_C(0x7fffffff) / (static_cast<int64_t>(n_thres) * 2 * n_layers),
             "%s: at most 2^31 - 1 records (n_rays * n_thres * 2 n_layers)", who);
  return 0;
}

int composite_layers_counting(const SigmaCompositeArgs& a, int n_layers, float* br, float* z_mid, int* count, dn_stream_t stream) {
  const char* who = "dn_composite_density_layers";
  if (a.n_rays == 0) return 0;   // (before the checks, like dn_composite_density: empty tensors carry NULL data pointers)
  DN_REQUIRE(a.rf && a.z && a.rd && br && z_mid && count && a.n_rays >= 0 && a.n_samples >= 1 && a.rd_stride >= 3, "%s: bad arguments", who);
  DN_REQUIRE(a.n_thres >= 1 && a.d_m_thres, "%s: needs at least one threshold", who);
  if (int rc = layers_check(who, a.n_thres, n_layers, a.n_rays)) return rc;
  DN_REQUIRE(((reinterpret_cast<uintptr_t>(a.rf) | reinterpret_cast<uintptr_t>(br)) & 15) == 0, "%s: rf and br must be 16-byte aligned", who);
  hipLaunchKernelGGL(composite_layers_kernel, dim3(ray_grid(a.n_rays)), dim3(256), 0, as_stream(stream), reinterpret_cast<const float4*>(a.rf),
                     a.z, a.rd, a.rd_stride, a.d_m_thres, a.n_thres, 2 * n_layers, a.n_rays, a.n_samples, a.depth, a.acc, a.dex,
                     reinterpret_cast<float4*>(br), z_mid, count, a.nonfinite);
  return check_launch(who);
}

int layers_thresholds_launch(const float* d_m_thres, int n_thres, int n_layers, float* out, dn_stream_t stream) {
  const int n_out = n_thres * 2 * n_layers;
  hipLaunchKernelGGL(layers_thresholds_kernel, dim3((n_out + kLayersBlock - 1) / kLayersBlock), dim3(kLayersBlock), 0, as_stream(stream),
                     d_m_thres, 2 * n_layers, n_out, out);
  return check_launch("dn_render_rays_depth_layers");
}

int dex_layers_finish_launch(const float* br, const float* d_m_thres, int n_thres, int n_layers, int interp, int64_t n_rays, float* events,
                             float* width, dn_stream_t stream) {
  const char* who = "dn_dex_layers_finish";
  if (n_rays == 0) return 0;
  DN_REQUIRE(br && events && n_rays >= 0, "%s: bad arguments", who);
  DN_REQUIRE(n_thres >= 1 && d_m_thres, "%s: needs at least one threshold", who);
  DN_REQUIRE(interp == 0 || interp == 1, "%s: interp is 0 (sample mode) or 1 (interpolated mode)", who);
  if (int rc = layers_check(who, n_thres, n_layers, n_rays)) return rc;
  DN_REQUIRE((reinterpret_cast<uintptr_t>(br) & 15) == 0, "%s: br must be 16-byte aligned", who);
  const int64_t n_out = n_rays * n_thres * 2 * n_layers;
  hipLaunchKernelGGL(dex_layers_finish_kernel, dim3(static_cast<unsigned>((n_out + kLayersBlock - 1) / kLayersBlock)), dim3(kLayersBlock), 0,
                     as_stream(stream), reinterpret_cast<const float4*>(br), d_m_thres, n_thres, 2 * n_layers, interp, n_rays, events, width);
  return check_launch(who);
}

}  // namespace dn

extern "C" int dn_composite_density_layers(const float* rf, const float* z, const float* rd, int rd_stride, const float* d_m_thres,
                                           int n_thres, int n_layers, int64_t n_rays, int n_samples, float* depth, float* acc, float* dex,
                                           float* br, float* z_mid, int* count, dn_stream_t stream) {
  return dn::composite_layers_counting({rf, z, rd, rd_stride, nullptr, 0.0f, d_m_thres, n_thres, n_rays, n_samples, depth, acc, dex}, n_layers,
                                       br, z_mid, count, stream);
}

extern "C" int dn_dex_layers_finish(const float* br, const float* d_m_thres, int n_thres, int n_layers, int interp, int64_t n_rays,
                                    float* events, float* width, dn_stream_t stream) {
  return dn::dex_layers_finish_launch(br, d_m_thres, n_thres, n_layers, interp, n_rays, events, width, stream);
}
