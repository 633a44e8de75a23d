// The bisection of the Dex first-crossing brackets (include/dexnerf_hip_refine.h): composite_brackets_kernel (composite_density.hip)
// leaves one record (z_lo, z_hi, s_lo, s_hi) per (ray, threshold) and the first midpoints; the density network evaluates the midpoints
// (dn_run_network on rays + z_mid with samples_per_ray = K), and
//   dex_bisect_kernel         one step on every record: the half of the bracket that still holds the crossing, and the next midpoint
//   dex_refine_finish_kernel  the refined depth - the linear interpolation of the last bracket in fp64, rounded once - and its width
// Both are elementwise, one thread per record, 16-byte record loads and stores, plain vector stores, no atomics; the grids are
// functions of N K alone.
//
// Memory: HBM / L2-bound and small - per record the step reads 16 B (record) + 16 B (network row, .w used) + 4 B (threshold, cached)
// and writes 16 B + 4 B; the finish reads 16 B and writes 4 or 8 B.  For a 400 x 400 image and one threshold that is 8 MB per step:
// a few microseconds beside the network launch whose rows it reads.
#include "../../include/dexnerf_hip_refine.h"
#include "dn_common.h"

namespace dn {

constexpr int kRefineBlock = 256;

// record idx = ray * K + k
__global__ __launch_bounds__(kRefineBlock) void dex_bisect_kernel(float4* __restrict__ br, const float4* __restrict__ rf_mid,
                                                                  const float* __restrict__ d_thres, int n_thres, int64_t n_records,
                                                                  float* __restrict__ z_mid) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kRefineBlock + threadIdx.x;
  if (idx >= n_records) return;
  float4 r = br[idx];   // (z_lo, z_hi, s_lo, s_hi)
  if (r.x != r.y) {     // a record with z_lo == z_hi is never changed: the first-sample crossing, "none", two equal depths
    const float m = d_thres[idx % n_thres];
    const float zm = r.x + 0.5f * (r.y - r.x);   // the midpoint the network was run at
    const float s = rf_mid[idx].w;
    if (s > m) { r.y = zm; r.w = s; }
    else { r.x = zm; r.z = s; }   // NaN included: NaN never crosses
    br[idx] = r;
  }
  z_mid[idx] = r.x + 0.5f * (r.y - r.x);
}

// output idx = k * N + ray: the stores are coalesced, the 16-byte record loads K records apart
__global__ __launch_bounds__(kRefineBlock) void dex_refine_finish_kernel(const float4* __restrict__ br, const float* __restrict__ d_thres,
                                                                         int n_thres, int64_t n_rays, float* __restrict__ refined,
                                                                         float* __restrict__ width) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kRefineBlock + threadIdx.x;
  if (idx >= n_rays * n_thres) return;
  const int64_t k = idx / n_rays, ray = idx - k * n_rays;
  const float4 r = br[ray * n_thres + k];
  float out = r.x, wd = 0.0f;
  if (r.w == -__builtin_inff()) {
    wd = -1.0f;   // no crossing: z_0, the Dex fallback
  } else if (r.x != r.y) {
    const bool finite = (r.z - r.z == 0.0f) && (r.w - r.w == 0.0f);
    const double m = static_cast<double>(d_thres[k]);
    const double lo = static_cast<double>(r.x), hi = static_cast<double>(r.y), s_lo = static_cast<double>(r.z), s_hi = static_cast<double>(r.w);
    const double t = finite ? (m - s_lo) / (s_hi - s_lo) : 0.5;
    out = static_cast<float>(lo + (hi - lo) * t);   // fp64 from the fp32 inputs, rounded once
    wd = r.y - r.x;
  }
  refined[idx] = out;
  if (width != nullptr) width[idx] = wd;
}

static unsigned record_grid(int64_t n_records) { return static_cast<unsigned>((n_records + kRefineBlock - 1) / kRefineBlock); }

// N K <= 2^31 - 1 records: the grid of one thread per record stays far inside the launch limits, and N K 4 floats is what the
// network's output buffer holds anyway
static bool records_fit(int64_t n_rays, int n_thres) { return n_rays <= INT64_C(0x7fffffff) / n_thres; }

int dex_bisect_launch(float* br, const float* rf_mid, const float* d_m_thres, int n_thres, int64_t n_rays, float* z_mid, dn_stream_t stream) {
  const char* who = "dn_dex_bisect";
  if (n_rays == 0) return 0;   // (before the checks: empty tensors carry NULL data pointers)
  DN_REQUIRE(br && rf_mid && z_mid && n_rays >= 0, "%s: bad arguments", who);
  DN_REQUIRE(n_thres >= 1 && d_m_thres, "%s: needs at least one threshold", who);
  DN_REQUIRE(records_fit(n_rays, n_thres), "%s: at most 2^31 - 1 records (n_rays * n_thres)", who);
  DN_REQUIRE(((reinterpret_cast<uintptr_t>(br) | reinterpret_cast<uintptr_t>(rf_mid)) & 15) == 0, "%s: br and rf_mid must be 16-byte aligned", who);
  const int64_t n_records = n_rays * n_thres;
  hipLaunchKernelGGL(dex_bisect_kernel, dim3(record_grid(n_records)), dim3(kRefineBlock), 0, as_stream(stream), reinterpret_cast<float4*>(br),
                     reinterpret_cast<const float4*>(rf_mid), d_m_thres, n_thres, n_records, z_mid);
  return check_launch(who);
}

int dex_refine_finish_launch(const float* br, const float* d_m_thres, int n_thres, int64_t n_rays, float* refined, float* width,
                             dn_stream_t stream) {
  const char* who = "dn_dex_refine_finish";
  if (n_rays == 0) return 0;
  DN_REQUIRE(br && refined && n_rays >= 0, "%s: bad arguments", who);
  DN_REQUIRE(n_thres >= 1 && d_m_thres, "%s: needs at least one threshold", who);
  DN_REQUIRE(records_fit(n_rays, n_thres), "%s: at most 2^31 - 1 records (n_rays * n_thres)", who);
  DN_REQUIRE((reinterpret_cast<uintptr_t>(br) & 15) == 0, "%s: br must be 16-byte aligned", who);
  hipLaunchKernelGGL(dex_refine_finish_kernel, dim3(record_grid(n_rays * n_thres)), dim3(kRefineBlock), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(br), d_m_thres, n_thres, n_rays, refined, width);
  return check_launch(who);
}

}  // namespace dn

extern "C" int dn_dex_bisect(float* br, const float* rf_mid, const float* d_m_thres, int n_thres, int64_t n_rays, float* z_mid,
                             dn_stream_t stream) {
  return dn::dex_bisect_launch(br, rf_mid, d_m_thres, n_thres, n_rays, z_mid, stream);
}

extern "C" int dn_dex_refine_finish(const float* br, const float* d_m_thres, int n_thres, int64_t n_rays, float* refined, float* width,
                                    dn_stream_t stream) {
  return dn::dex_refine_finish_launch(br, d_m_thres, n_thres, n_rays, refined, width, stream);
}
