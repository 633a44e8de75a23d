// The occupied span of a ray in an occupancy bit grid (include/dexnerf_hip_span.h): the rewrite of a ray row's near / far that lets the
// render after it place its samples where the grid has set cells.
//
//   ray_spans_kernel   one thread per ray: the row's 8 floats loaded once, the slab clip against the grid's box, then a cell-by-cell
//                      walk (the next boundary of each axis recomputed from the integer cell, never accumulated) that reads the cells'
//                      bit words through the cache - a 128^3 grid is 256 KB - and keeps the entry of the first set cell, the exit of
//                      the last one and their count.  The walk is divergent by nature: a wave runs as long as its longest ray.
//
// No LDS, no atomics, no workgroup waits on another; plain vector stores; only columns 6 and 7 of a hit row are written, and only
// with `apply`: the output is a function of the input.
#include "../../include/dexnerf_hip_span.h"
#include "dn_common.h"

namespace dn {
namespace span {

constexpr int kThreads = 256;
static_assert(DN_OCC_MAX_AXIS_CELLS <= (1 << 24), "(float)cells and (float)(i + 1) must be exact");

struct Grid {
  float b0[3], s[3];
  int cells[3];
};

__device__ __forceinline__ float max_of(float a, float b) { return b > a ? b : a; }
__device__ __forceinline__ float min_of(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ bool finite_bits(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(kThreads) void ray_spans_kernel(float* __restrict__ rays, int64_t ray_stride, int64_t n_rays,
                                                             const unsigned* __restrict__ bits, Grid g, float pad_cells, int apply,
                                                             float* __restrict__ span, int* __restrict__ visits) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (r >= n_rays) return;
  float* row = rays + r * ray_stride;
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = row[c];
  const float near = v[6], far = v[7];
  bool miss = false;
#pragma unroll
  for (int c = 0; c < 8; ++c) miss = miss || !finite_bits(v[c]);

  // per-axis arrays indexed by compile-time constants only: the walk picks its axis with selects, since a run-time index into a
  // register array would go through scratch
  float o[3], d[3], inv[3], tn[3];
  int i[3], step[3];
  float t_in = near, t_out = far;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = (v[a] - g.b0[a]) * g.s[a];
    d[a] = v[3 + a] * g.s[a];
    const float c = static_cast<float>(g.cells[a]);
    if (d[a] == 0.0f) {
      miss = miss || !(o[a] >= 0.0f && o[a] < c);
      inv[a] = 0.0f;   // never read: the axis is never stepped along
    } else {
      inv[a] = 1.0f / d[a];
      const float ta = (0.0f - o[a]) * inv[a], tb = (c - o[a]) * inv[a];
      const bool fwd = ta <= tb;
      t_in = max_of(t_in, fwd ? ta : tb);
      t_out = min_of(t_out, fwd ? tb : ta);
    }
  }
  miss = miss || !(t_in < t_out);

  int count = 0;
  float lo = 0.0f, hi = 0.0f;
  if (!miss) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float c = static_cast<float>(g.cells[a]);
      const float p = o[a] + d[a] * t_in;
      const int cell = static_cast<int>(min_of(max_of(floorf(p), 0.0f), c - 1.0f));
      i[a] = min(max(cell, 0), g.cells[a] - 1);   // (a no-op unless p is NaN)
      step[a] = d[a] > 0.0f ? 1 : (d[a] < 0.0f ? -1 : 0);
      tn[a] = d[a] == 0.0f ? __builtin_inff() : (static_cast<float>(i[a] + (d[a] > 0.0f ? 1 : 0)) - o[a]) * inv[a];
    }
    float t_cur = t_in;
    const int64_t most = static_cast<int64_t>(g.cells[0]) + g.cells[1] + g.cells[2] + 1;
    for (int64_t it = 0; it < most; ++it) {
      const bool use1 = tn[1] < tn[0];
      const float t01 = use1 ? tn[1] : tn[0];
      const bool use2 = tn[2] < t01;
      const float tn_a = use2 ? tn[2] : t01;
      const float t_exit = min_of(tn_a, t_out);
      const int64_t cell = (static_cast<int64_t>(i[0]) * g.cells[1] + i[1]) * g.cells[2] + i[2];
      if ((bits[cell >> 5] >> (cell & 31)) & 1u) {
        if (count == 0) lo = t_cur;
        hi = t_exit;
        ++count;
      }
      if (!(tn_a < t_out)) break;
      // step along the chosen axis: selects, not a run-time index
      bool left;
      if (use2) {
        i[2] += step[2];
        left = i[2] < 0 || i[2] >= g.cells[2];
        tn[2] = (static_cast<float>(i[2] + (d[2] > 0.0f ? 1 : 0)) - o[2]) * inv[2];
      } else if (use1) {
        i[1] += step[1];
        left = i[1] < 0 || i[1] >= g.cells[1];
        tn[1] = (static_cast<float>(i[1] + (d[1] > 0.0f ? 1 : 0)) - o[1]) * inv[1];
      } else {
        i[0] += step[0];
        left = i[0] < 0 || i[0] >= g.cells[0];
        tn[0] = (static_cast<float>(i[0] + (d[0] > 0.0f ? 1 : 0)) - o[0]) * inv[0];
      }
      if (left) break;
      t_cur = tn_a;
    }
  }

  float s0 = near, s1 = far;   // a miss: the row's own bits
  if (count > 0) {
    const float pad = pad_cells / max_of(max_of(fabsf(d[0]), fabsf(d[1])), fabsf(d[2]));
    s0 = max_of(near, lo - pad);
    s1 = min_of(far, hi + pad);
    if (apply) {
      row[6] = s0;
      row[7] = s1;
    }
  }
  if (span) {
    span[2 * r] = s0;
    span[2 * r + 1] = s1;
  }
  if (visits) visits[r] = count;
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
bool is_finite(float x) { return x - x == 0.0f; }

}  // namespace span
}  // namespace dn

using namespace dn;
using namespace dn::span;

extern "C" int dn_occupancy_ray_spans(float* rays, int ray_stride, int64_t n_rays, const unsigned* bits, int cx, int cy, int cz, float x0,
                                      float y0, float z0, float x1, float y1, float z1, float sx, float sy, float sz, float pad_cells,
                                      int apply, float* span, int* visits, dn_stream_t stream) {
  const char* who = "dn_occupancy_ray_spans";
  DN_REQUIRE(rays && bits, "%s: null rays or bits", who);
  DN_REQUIRE(ray_stride >= 8, "%s: ray_stride must be >= 8", who);
  DN_REQUIRE(n_rays >= 0 && n_rays <= DN_OCC_MAX_SAMPLES, "%s: n_rays must be 0 .. %d (got %lld)", who, DN_OCC_MAX_SAMPLES,
             static_cast<long long>(n_rays));
  // (dn_occupancy_words is 0 for exactly the cells the occupancy entry points refuse)
  DN_REQUIRE(dn_occupancy_words(cx, cy, cz) > 0, "%s: cells %d x %d x %d: each axis needs 1 .. %d cells, their product at most %d", who, cx, cy,
             cz, DN_OCC_MAX_AXIS_CELLS, DN_OCC_MAX_CELLS);
  DN_REQUIRE(is_finite(x0) && is_finite(y0) && is_finite(z0) && is_finite(x1) && is_finite(y1) && is_finite(z1) && x1 > x0 && y1 > y0 && z1 > z0,
             "%s: bounds must be finite with x1 > x0, y1 > y0, z1 > z0", who);
  DN_REQUIRE(is_finite(sx) && is_finite(sy) && is_finite(sz) && sx > 0.0f && sy > 0.0f && sz > 0.0f,
             "%s: the scales cells / (b1 - b0) must be finite and > 0", who);
  DN_REQUIRE(is_finite(pad_cells) && pad_cells >= 0.0f, "%s: pad_cells must be finite and >= 0", who);
  DN_REQUIRE(span || apply, "%s: without `apply` the span output is required", who);
  DN_REQUIRE(aligned4(rays) && aligned4(bits) && aligned4(span) && aligned4(visits), "%s: pointers must be 4-byte aligned", who);
  if (n_rays == 0) return 0;
  const Grid g{{x0, y0, z0}, {sx, sy, sz}, {cx, cy, cz}};
  const unsigned blocks = static_cast<unsigned>((n_rays + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(ray_spans_kernel, dim3(blocks), dim3(kThreads), 0, as_stream(stream), rays, static_cast<int64_t>(ray_stride), n_rays, bits,
                     g, pad_cells, apply ? 1 : 0, span, visits);
  return check_launch(who);
}
