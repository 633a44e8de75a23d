// An occupancy grid kept live beside training networks (include/dexnerf_hip_live.h): one jittered point per cell, a decayed running
// maximum of the density found there, and the bit grid of it.
//
//   cell_points_kernel   one thread per cell: Philox on (seed, iteration, kRngStreamCell, c), three uniforms, the point of the cell.
//                        A thread stores its row's 3 floats; a wave's 64 rows are 768 consecutive bytes
//   ema_update_kernel    one LANE per cell: the density column(s), the ema load and the ema store are each one coalesced access of
//                        the wave (256 consecutive bytes at stride 1; every fourth dword of 1 KB on dn_run_network's rows).  The
//                        64-lane ballot of the predicate IS the two 32-bit words of the wave's 64 cells - a wave starts at a multiple
//                        of 64 cells, so no other wave shares a word with it - and lanes 0 and 32 store one word each.  Lanes past
//                        the last cell load nothing and contribute 0.  No LDS, no scratch memory.
//
// The dilation of the raw words is occupancy.hip's (occupancy_grid.h): the one copy dn_occupancy_build runs.  No workgroup waits on
// another, no atomics, plain vector stores: the output is a function of the input.
#include "../../include/dexnerf_hip_live.h"
#include "dn_rng.h"
#include "occupancy_grid.h"

namespace dn {
namespace live {

constexpr int kThreads = 256;
static_assert(kThreads % kWave == 0, "a wave starts at a multiple of 64 cells");
static_assert(DN_OCC_MAX_AXIS_CELLS <= (1 << 24), "(float)i must be exact");

struct Lattice {
  float b0[3], h[3];
  int cy, cz;
};

__global__ __launch_bounds__(kThreads) void cell_points_kernel(Lattice g, int64_t c0, int64_t n, uint32_t* __restrict__ rng_state,
                                                               float* __restrict__ pts) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  // the first slab draws from nxt and hands it on as cur (nobody in that launch reads word 2); a later slab reads cur
  const uint32_t iteration = c0 == 0 ? rng_state[3] : rng_state[2];
  if (c0 == 0 && e == 0) rng_state[2] = iteration;
  if (e >= n) return;
  const int64_t c = c0 + e;
  const int k = static_cast<int>(c % g.cz);
  const int j = static_cast<int>((c / g.cz) % g.cy);
  const int i = static_cast<int>(c / (static_cast<int64_t>(g.cz) * g.cy));
  uint32_t w[4];
  rng_words(rng_state[0], rng_state[1], iteration, kRngStreamCell, static_cast<uint64_t>(c), w);
  float* row = pts + e * 3;
  row[0] = g.b0[0] + (static_cast<float>(i) + rng_to_uniform(w[0])) * g.h[0];
  row[1] = g.b0[1] + (static_cast<float>(j) + rng_to_uniform(w[1])) * g.h[1];
  row[2] = g.b0[2] + (static_cast<float>(k) + rng_to_uniform(w[2])) * g.h[2];
}

__device__ __forceinline__ bool finite_bits(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ float max_of(float a, float b) { return b > a ? b : a; }

template <bool TWO>
__global__ __launch_bounds__(kThreads) void ema_update_kernel(const float* __restrict__ sa, int64_t stride_a, const float* __restrict__ sb,
                                                              int64_t stride_b, int64_t n, float decay, float level,
                                                              float* __restrict__ ema, unsigned* __restrict__ words,
                                                              uint32_t* __restrict__ rng_state) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (c == 0) rng_state[3] = rng_state[2] + 1u;   // (nobody in this launch reads word 3)
  bool raw = false;
  if (c < n) {
    float s = sa[c * stride_a];
    bool hot = !finite_bits(s);
    if (TWO) {
      const float b = sb[c * stride_b];
      hot = hot || !finite_bits(b);
      s = max_of(s, b);
    }
    const float d = ema[c] * decay;
    const float e = hot ? d : max_of(d, s);
    ema[c] = e;
    raw = hot || e > level;
  }
  // every lane of the wave arrives here: the ballot's bit l is lane l's predicate, 0 for a lane past the last cell
  const unsigned long long mask = __ballot(raw);
  if (words != nullptr && c < n) {
    const int lane = threadIdx.x & (kWave - 1);
    if (lane == 0) words[c >> 5] = static_cast<unsigned>(mask);
    if (lane == 32) words[c >> 5] = static_cast<unsigned>(mask >> 32);
  }
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
bool is_finite(float x) { return x - x == 0.0f; }

}  // namespace live
}  // namespace dn

using namespace dn;
using namespace dn::live;

extern "C" int dn_occupancy_cell_points(int cx, int cy, int cz, float x0, float y0, float z0, float hx, float hy, float hz, int64_t c0,
                                        int64_t n, unsigned* rng_state, float* pts, dn_stream_t stream) {
  const char* who = "dn_occupancy_cell_points";
  occ::Cells g;
  DN_REQUIRE(rng_state && pts, "%s: null rng record or points", who);
  DN_REQUIRE(occ::cells_of(cx, cy, cz, g), "%s: cells %d x %d x %d: each axis needs 1 .. %d cells, their product at most %d", who, cx, cy, cz,
             DN_OCC_MAX_AXIS_CELLS, DN_OCC_MAX_CELLS);
  DN_REQUIRE(is_finite(x0) && is_finite(y0) && is_finite(z0), "%s: the lower bounds must be finite", who);
  DN_REQUIRE(is_finite(hx) && is_finite(hy) && is_finite(hz) && hx > 0.0f && hy > 0.0f && hz > 0.0f,
             "%s: the cell sizes (b1 - b0) / cells must be finite and > 0", who);
  DN_REQUIRE(c0 >= 0 && n >= 1 && c0 <= g.n && n <= g.n - c0, "%s: the cell range [%lld, %lld + %lld) must be non-empty and inside the %lld cells",
             who, static_cast<long long>(c0), static_cast<long long>(c0), static_cast<long long>(n), static_cast<long long>(g.n));
  DN_REQUIRE(aligned4(rng_state) && aligned4(pts), "%s: pointers must be 4-byte aligned", who);
  const Lattice l{{x0, y0, z0}, {hx, hy, hz}, cy, cz};
  const unsigned blocks = static_cast<unsigned>((n + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(cell_points_kernel, dim3(blocks), dim3(kThreads), 0, as_stream(stream), l, c0, n, rng_state, pts);
  return check_launch(who);
}

extern "C" size_t dn_occupancy_ema_workspace_bytes(int cx, int cy, int cz, int dilate) {
  occ::Cells g;
  if (!occ::cells_of(cx, cy, cz, g) || dilate < 0 || dilate > DN_OCC_MAX_DILATE) return 0;
  return sizeof(unsigned) * static_cast<size_t>(occ::words_of(g));
}

extern "C" int dn_occupancy_ema_update(const float* sigma_a, int stride_a, const float* sigma_b, int stride_b, int cx, int cy, int cz,
                                       float decay, float level, int write_bits, int dilate, float* ema, unsigned* bits, unsigned* scratch,
                                       unsigned* rng_state, dn_stream_t stream) {
  const char* who = "dn_occupancy_ema_update";
  occ::Cells g;
  DN_REQUIRE(sigma_a, "%s: null first density column", who);
  DN_REQUIRE(ema && rng_state, "%s: null ema or rng record", who);
  DN_REQUIRE(stride_a >= 1 && (sigma_b == nullptr || stride_b >= 1), "%s: the strides must be >= 1", who);
  DN_REQUIRE(occ::cells_of(cx, cy, cz, g), "%s: cells %d x %d x %d: each axis needs 1 .. %d cells, their product at most %d", who, cx, cy, cz,
             DN_OCC_MAX_AXIS_CELLS, DN_OCC_MAX_CELLS);
  DN_REQUIRE(decay > 0.0f && decay <= 1.0f, "%s: decay must be in (0, 1] (got %g)", who, static_cast<double>(decay));
  DN_REQUIRE(is_finite(level) && level >= 0.0f, "%s: level must be finite and >= 0 (got %g)", who, static_cast<double>(level));
  DN_REQUIRE(dilate >= 0 && dilate <= DN_OCC_MAX_DILATE, "%s: dilate must be 0 .. %d (got %d)", who, DN_OCC_MAX_DILATE, dilate);
  DN_REQUIRE(!write_bits || bits, "%s: write_bits needs the bits", who);
  DN_REQUIRE(!write_bits || dilate == 0 || scratch, "%s: write_bits with dilate > 0 needs the scratch words", who);
  DN_REQUIRE(!write_bits || dilate == 0 || scratch != bits, "%s: the scratch words must not be the grid's", who);
  DN_REQUIRE(aligned4(sigma_a) && aligned4(sigma_b) && aligned4(ema) && aligned4(bits) && aligned4(scratch) && aligned4(rng_state),
             "%s: pointers must be 4-byte aligned", who);
  hipStream_t s = as_stream(stream);
  const unsigned blocks = static_cast<unsigned>((g.n + kThreads - 1) / kThreads);
  unsigned* words = !write_bits ? nullptr : (dilate > 0 ? scratch : bits);
  const int64_t sta = stride_a, stb = stride_b;
  if (sigma_b) hipLaunchKernelGGL(ema_update_kernel<true>, dim3(blocks), dim3(kThreads), 0, s, sigma_a, sta, sigma_b, stb, g.n, decay, level, ema, words, rng_state);
  else hipLaunchKernelGGL(ema_update_kernel<false>, dim3(blocks), dim3(kThreads), 0, s, sigma_a, sta, sigma_b, stb, g.n, decay, level, ema, words, rng_state);
  if (write_bits && dilate > 0) occ::launch_dilate(scratch, g, dilate, 0, bits, s);
  return check_launch(who);
}
