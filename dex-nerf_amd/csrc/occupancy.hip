// An occupancy bit grid of the density field and the compaction of ray samples against it (include/dexnerf_hip_occupancy.h): the
// pieces of a depth-only render that runs the network only on the samples whose cell is occupied.
//
//   raw_bits_kernel        one thread per 32-cell word: a cell's bit is set iff one of its 8 corners is non-finite or > level
//   dilate_kernel          one thread per word: the OR of the raw bits over the Chebyshev neighbourhood; a (di,dj) row of it is a run of
//                          at most 17 consecutive bits of the raw words, tested with one or two word loads
//   classify_kernel        one thread per 4 consecutive ray samples: keep flag (0 / -1) into slot[], the workgroup's kept count
//   scan_totals_kernel     scan_row (scan_blocks.h) on one row; the top level is one workgroup and writes the record
//   scan_slots_kernel      slot[p] = rank of p among the kept samples: the scan inside the workgroup plus the two scanned levels above
//   emit_kernel            pts[slot[p]] = ro + rd * z, the bits classify_kernel judged; <true> also dirs[slot[p]] = columns 8..10 of the
//                          sample's ray row, in the same launch (include/dexnerf_hip_cull.h)
//   gather_rows_kernel     dst[p][c] = src[slot[p]][c] or fill_c for c < width, as 32-bit words; a thread owns 4 consecutive dst rows, so
//                          kept rows are read in ascending order; rows of 16 aligned bytes move as one dwordx4 load and store; optionally
//                          the workgroup's count of non-finite values.  dn_occupancy_gather is its width 1 on column 3 of 4-float rows
//   sum_partials_kernel    one workgroup: the sum of those counts, in a fixed order
//
// No workgroup waits on another, no atomics, plain vector stores: the output is a function of the input.  Memory: the sample kernels
// touch about 40 B per sample (z twice, slot written twice and read three times, 12 B per kept point, one 16-byte line share of rf).
#include "../../include/dexnerf_hip_cull.h"
#include "occupancy_grid.h"
#include "scan_blocks.h"

namespace dn {
namespace occ {

constexpr int kThreads = kScanThreads;
constexpr int kPerThread = kScanPerThread;
constexpr int64_t kMaxCells = DN_OCC_MAX_CELLS;
constexpr int64_t kMaxSamples = DN_OCC_MAX_SAMPLES;
static_assert(kMaxSamples <= static_cast<int64_t>(kScanElems) * kScanElems * kScanElems && kMaxSamples < (int64_t{1} << 31), "limits");
static_assert(DN_OCC_MAX_AXIS_CELLS <= (1 << 24), "(float)cells must be exact");

__device__ __forceinline__ bool hot(float x, float level) {
  const bool finite = (__builtin_bit_cast(unsigned, x) & 0x7F800000u) != 0x7F800000u;
  return !finite || x > level;
}

// ---- build ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void raw_bits_kernel(const float* __restrict__ f, int64_t fs, Cells g, float level, int accumulate,
                                                            int64_t n_words, unsigned* __restrict__ out) {
  const int64_t w = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (w >= n_words) return;
  const int64_t c0 = w * 32;
  int k = static_cast<int>(c0 % g.cz);
  int j = static_cast<int>((c0 / g.cz) % g.cy);
  int i = static_cast<int>(c0 / (static_cast<int64_t>(g.cz) * g.cy));
  const int64_t vz = g.cz + 1, vy = g.cy + 1;
  unsigned v = 0;
  for (int b = 0; b < 32 && c0 + b < g.n; ++b) {
    const int64_t base = (static_cast<int64_t>(i) * vy + j) * vz + k;
    bool any = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) any |= hot(f[(base + ((c >> 2) & 1) * vy * vz + ((c >> 1) & 1) * vz + (c & 1)) * fs], level);
    v |= static_cast<unsigned>(any) << b;
    if (++k == g.cz) {
      k = 0;
      if (++j == g.cy) { j = 0; ++i; }
    }
  }
  out[w] = accumulate ? (out[w] | v) : v;
}

// any bit of the cells a .. b (a <= b < a + 32) set
__device__ __forceinline__ bool any_in_run(const unsigned* __restrict__ raw, int64_t a, int64_t b) {
  const int64_t wa = a >> 5, wb = b >> 5;
  const unsigned from = ~0u << (a & 31), upto = ~0u >> (31 - (b & 31));
  if (wa == wb) return (raw[wa] & from & upto) != 0u;
  return ((raw[wa] & from) | (raw[wb] & upto)) != 0u;
}

__global__ __launch_bounds__(kThreads) void dilate_kernel(const unsigned* __restrict__ raw, Cells g, int d, int accumulate, int64_t n_words,
                                                          unsigned* __restrict__ out) {
  const int64_t w = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (w >= n_words) return;
  const int64_t c0 = w * 32;
  int k = static_cast<int>(c0 % g.cz);
  int j = static_cast<int>((c0 / g.cz) % g.cy);
  int i = static_cast<int>(c0 / (static_cast<int64_t>(g.cz) * g.cy));
  unsigned v = 0;
  for (int b = 0; b < 32 && c0 + b < g.n; ++b) {
    const int k0 = max(k - d, 0), k1 = min(k + d, g.cz - 1);
    bool any = false;
    for (int ii = max(i - d, 0); ii <= min(i + d, g.cx - 1) && !any; ++ii)
      for (int jj = max(j - d, 0); jj <= min(j + d, g.cy - 1) && !any; ++jj) {
        const int64_t row = (static_cast<int64_t>(ii) * g.cy + jj) * g.cz;
        any = any_in_run(raw, row + k0, row + k1);
      }
    v |= static_cast<unsigned>(any) << b;
    if (++k == g.cz) {
      k = 0;
      if (++j == g.cy) { j = 0; ++i; }
    }
  }
  out[w] = accumulate ? (out[w] | v) : v;
}

// ---- samples --------------------------------------------------------------------------------------------------------------------
struct Samples {
  const float* rays;
  int64_t ray_stride;
  const float* z;
  int64_t n;   // P
  int s;       // samples per ray
};

// x = ro + rd * z: multiply, then add (the unit is compiled with -ffp-contract=off)
__device__ __forceinline__ void point_of(const Samples& a, int64_t p, float (&x)[3]) {
  const float* row = a.rays + (p / a.s) * a.ray_stride;
  const float z = a.z[p];
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = row[c] + row[3 + c] * z;
}

struct Box {
  float b0[3], s[3];
  int cells[3];
};

__device__ __forceinline__ bool kept(const float (&x)[3], const Box& box, const unsigned* __restrict__ bits) {
  float t[3];
  bool in = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    t[c] = (x[c] - box.b0[c]) * box.s[c];
    in = in && t[c] >= 0.0f && t[c] < static_cast<float>(box.cells[c]);
  }
  if (!in) return false;
  const int64_t cell = (static_cast<int64_t>(static_cast<int>(t[0])) * box.cells[1] + static_cast<int>(t[1])) * box.cells[2] + static_cast<int>(t[2]);
  return (bits[cell >> 5] >> (cell & 31)) & 1u;
}

__global__ __launch_bounds__(kThreads) void classify_kernel(Samples a, Box box, const unsigned* __restrict__ bits, int* __restrict__ slot,
                                                            unsigned* __restrict__ tot0) {
  __shared__ unsigned lds[4];
  const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kScanElems + threadIdx.x * kPerThread;
  unsigned n = 0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int64_t p = e0 + q;
    if (p < a.n) {
      float x[3];
      point_of(a, p, x);
      const bool keep = kept(x, box, bits);
      slot[p] = keep ? 0 : -1;
      n += keep;
    }
  }
  unsigned all;
  block_scan_exclusive(n, lds, all);
  if (threadIdx.x == 0) tot0[blockIdx.x] = all;
}

// record: the top level (one workgroup) alone - {n_kept, P, 0, 0}
__global__ __launch_bounds__(kThreads) void scan_totals_kernel(unsigned* __restrict__ a, unsigned n, unsigned* __restrict__ up, unsigned n_samples,
                                                               int top) {
  __shared__ unsigned lds[4];
  scan_row(a, n, up, lds);
  if (top && threadIdx.x == 0) { up[1] = n_samples; up[2] = 0u; up[3] = 0u; }
}

__global__ __launch_bounds__(kThreads) void scan_slots_kernel(int64_t n, const unsigned* __restrict__ tot0, const unsigned* __restrict__ tot1,
                                                              int* __restrict__ slot) {
  __shared__ unsigned lds[4];
  const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kScanElems + threadIdx.x * kPerThread;
  int f[kPerThread];
  unsigned mine = 0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    f[q] = e0 + q < n ? slot[e0 + q] : -1;
    mine += f[q] == 0;
  }
  unsigned all;
  unsigned run = tot0[blockIdx.x] + tot1[blockIdx.x / kScanElems] + block_scan_exclusive(mine, lds, all);
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    if (e0 + q < n && f[q] == 0) slot[e0 + q] = static_cast<int>(run++);
  }
}

template <bool DIRS>
__global__ __launch_bounds__(kThreads) void emit_kernel(Samples a, const int* __restrict__ slot, int64_t max_points, float* __restrict__ pts,
                                                        float* __restrict__ dirs) {
  const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kScanElems + threadIdx.x * kPerThread;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int64_t p = e0 + q;
    if (p >= a.n) continue;
    const int64_t s = slot[p];
    if (s < 0 || s >= max_points) continue;
    float x[3];
    point_of(a, p, x);
    float* row = pts + s * 3;
    row[0] = x[0]; row[1] = x[1]; row[2] = x[2];
    if (DIRS) {
      const float* ray = a.rays + (p / a.s) * a.ray_stride;
      float* d = dirs + s * 3;
      d[0] = ray[8]; d[1] = ray[9]; d[2] = ray[10];
    }
  }
}

struct Fills {
  unsigned v[DN_CULL_MAX_WIDTH];
};

// W: the row width; VEC: rows of 16 aligned bytes on both sides (W == 4, both strides 4).  Words, not floats: a copy of bits.
template <int W, bool VEC, bool COUNT>
__global__ __launch_bounds__(kThreads) void gather_rows_kernel(const int* __restrict__ slot, const unsigned* __restrict__ src, int64_t src_stride,
                                                               int64_t n_rows, int64_t n, Fills fill, unsigned* __restrict__ dst,
                                                               int64_t dst_stride, unsigned* __restrict__ partial) {
  static_assert(!VEC || W == 4, "a 16-byte row is four words");
  __shared__ unsigned lds[4];
  const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kScanElems + threadIdx.x * kPerThread;
  unsigned bad = 0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int64_t p = e0 + q;
    if (p >= n) continue;
    const int64_t s = slot[p];
    unsigned v[W];
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = fill.v[c];
    if (s >= 0 && s < n_rows) {
      if constexpr (VEC) {
        const uint4 r = *reinterpret_cast<const uint4*>(src + s * 4);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
      } else {
#pragma unroll
        for (int c = 0; c < W; ++c) v[c] = src[s * src_stride + c];
      }
      if (COUNT) {
#pragma unroll
        for (int c = 0; c < W; ++c) bad += (v[c] & 0x7F800000u) == 0x7F800000u;
      }
    }
    if constexpr (VEC) {
      *reinterpret_cast<uint4*>(dst + p * 4) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int c = 0; c < W; ++c) dst[p * dst_stride + c] = v[c];
    }
  }
  if (COUNT) {
    unsigned all;
    block_scan_exclusive(bad, lds, all);
    if (threadIdx.x == 0) partial[blockIdx.x] = all;
  }
}

__global__ __launch_bounds__(kThreads) void sum_partials_kernel(const unsigned* __restrict__ partial, unsigned n, unsigned* __restrict__ record) {
  __shared__ unsigned lds[4];
  unsigned mine = 0;
  for (unsigned e = threadIdx.x; e < n; e += kThreads) mine += partial[e];
  unsigned all;
  block_scan_exclusive(mine, lds, all);
  if (threadIdx.x == 0) record[2] = all;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// false: cells the entry points refuse
bool cells_of(int cx, int cy, int cz, Cells& g) {
  if (cx < 1 || cy < 1 || cz < 1 || cx > DN_OCC_MAX_AXIS_CELLS || cy > DN_OCC_MAX_AXIS_CELLS || cz > DN_OCC_MAX_AXIS_CELLS) return false;
  const int64_t cxy = static_cast<int64_t>(cx) * cy;
  if (cxy > kMaxCells || cxy * cz > kMaxCells) return false;
  g = Cells{cx, cy, cz, cxy * cz};
  return true;
}
int64_t words_of(const Cells& g) { return (g.n + 31) / 32; }
unsigned blocks_for(int64_t n, int per_block) { return static_cast<unsigned>((n + per_block - 1) / per_block); }

void launch_dilate(const unsigned* raw, const Cells& g, int d, int accumulate, unsigned* out, hipStream_t s) {
  const int64_t n_words = words_of(g);
  hipLaunchKernelGGL(dilate_kernel, dim3(blocks_for(n_words, kThreads)), dim3(kThreads), 0, s, raw, g, d, accumulate, n_words, out);
}

struct Layout {
  int64_t n;              // P
  unsigned n0, n1;        // totals at scan level 0 and 1
  size_t tot0, tot1, bytes;
};

// false: sizes the entry points refuse
bool layout_of(int64_t n_rays, int n_samples, Layout& l) {
  if (n_rays < 1 || n_samples < 1 || n_samples > DN_OCC_MAX_SAMPLES_PER_RAY || n_rays > kMaxSamples) return false;
  l.n = n_rays * n_samples;
  if (l.n > kMaxSamples) return false;
  l.n0 = blocks_for(l.n, kScanElems);
  l.n1 = blocks_for(l.n0, kScanElems);
  l.tot0 = 0;
  l.tot1 = up256(sizeof(unsigned) * l.n0);
  l.bytes = l.tot1 + up256(sizeof(unsigned) * l.n1);
  return true;
}

int samples_check(const char* who, const float* rays, int ray_stride, const float* z, int64_t n_rays, int n_samples, Layout& l) {
  DN_REQUIRE(rays && z, "%s: null rays or depths", who);
  DN_REQUIRE(ray_stride >= 8, "%s: ray_stride must be >= 8", who);
  DN_REQUIRE(layout_of(n_rays, n_samples, l), "%s: needs n_rays >= 1, n_samples in 1 .. %d and n_rays * n_samples <= %lld (got %lld x %d)", who,
             DN_OCC_MAX_SAMPLES_PER_RAY, static_cast<long long>(kMaxSamples), static_cast<long long>(n_rays), n_samples);
  return 0;
}

bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }
bool is_finite(float x) { return x - x == 0.0f; }

template <int W, bool VEC>
void launch_gather_rows(bool count, unsigned blocks, hipStream_t s, const int* slot, const unsigned* src, int64_t src_stride, int64_t n_rows,
                        int64_t n, const Fills& fill, unsigned* dst, int64_t dst_stride, unsigned* partial) {
  if (count)
    hipLaunchKernelGGL((gather_rows_kernel<W, VEC, true>), dim3(blocks), dim3(kThreads), 0, s, slot, src, src_stride, n_rows, n, fill, dst, dst_stride,
                       partial);
  else
    hipLaunchKernelGGL((gather_rows_kernel<W, VEC, false>), dim3(blocks), dim3(kThreads), 0, s, slot, src, src_stride, n_rows, n, fill, dst, dst_stride,
                       partial);
}

// Both emit entry points.  with_dirs: dn_occupancy_compact_emit_dirs - the ray rows carry the view direction, and both outputs are wanted.
int emit(const char* who, const float* rays, int ray_stride, const float* z, int64_t n_rays, int n_samples, const int* slot, int64_t max_points,
         float* pts, float* dirs, bool with_dirs, dn_stream_t stream) {
  Layout l;
  if (int rc = samples_check(who, rays, ray_stride, z, n_rays, n_samples, l)) return rc;
  if (with_dirs) {
    DN_REQUIRE(ray_stride >= 11, "%s: ray_stride must be >= 11: the view direction is columns 8..10 of a ray row (got %d)", who, ray_stride);
    DN_REQUIRE(aligned(rays, 4) && aligned(z, 4), "%s: rays and depths must be 4-byte aligned", who);
  }
  DN_REQUIRE(slot && aligned(slot, 4), "%s: null or unaligned slots", who);
  DN_REQUIRE(max_points >= 0, "%s: negative capacity", who);
  if (with_dirs) {
    DN_REQUIRE(max_points == 0 || (pts && dirs && aligned(pts, 4) && aligned(dirs, 4)), "%s: a capacity without both of its outputs", who);
    DN_REQUIRE(max_points == 0 || pts != dirs, "%s: the points and the directions must not be one buffer", who);
  } else {
    DN_REQUIRE(max_points == 0 || (pts && aligned(pts, 4)), "%s: a capacity without its output", who);
  }
  if (max_points == 0) return 0;
  const Samples a{rays, ray_stride, z, l.n, n_samples};
  if (with_dirs) hipLaunchKernelGGL(emit_kernel<true>, dim3(l.n0), dim3(kThreads), 0, as_stream(stream), a, slot, max_points, pts, dirs);
  else hipLaunchKernelGGL(emit_kernel<false>, dim3(l.n0), dim3(kThreads), 0, as_stream(stream), a, slot, max_points, pts, static_cast<float*>(nullptr));
  return check_launch(who);
}

// Both gather entry points.  dst_name and src_name: what the entry point calls its destination and its source in a refusal.
int gather_rows(const char* who, const char* dst_name, const char* src_name, const int* slot, const float* src, int src_stride, int64_t n_rows,
                int64_t n_points, int width, const float (&fills)[DN_CULL_MAX_WIDTH], float* dst, int dst_stride, void* workspace,
                unsigned* d_record, dn_stream_t stream) {
  DN_REQUIRE(slot && dst && aligned(slot, 4) && aligned(dst, 4), "%s: null or unaligned slots or %s", who, dst_name);
  DN_REQUIRE(n_points >= 1 && n_points <= kMaxSamples, "%s: n_points must be 1 .. %lld (got %lld)", who, static_cast<long long>(kMaxSamples),
             static_cast<long long>(n_points));
  DN_REQUIRE(n_rows >= 0 && n_rows <= n_points, "%s: n_rows must be 0 .. n_points", who);
  DN_REQUIRE(width >= 1 && width <= DN_CULL_MAX_WIDTH, "%s: width must be 1 .. %d (got %d)", who, DN_CULL_MAX_WIDTH, width);
  DN_REQUIRE(src_stride >= width && dst_stride >= width, "%s: the strides (%d, %d floats) must be at least the width %d", who, src_stride,
             dst_stride, width);
  DN_REQUIRE(n_rows == 0 || (src && aligned(src, 4)), "%s: rows without %s", who, src_name);
  DN_REQUIRE((workspace == nullptr) == (d_record == nullptr), "%s: the count needs both the workspace and the record", who);
  DN_REQUIRE(aligned(workspace, 256) && aligned(d_record, 4), "%s: workspace must be 256-byte aligned, the record 4-byte aligned", who);
  const unsigned blocks = blocks_for(n_points, kScanElems);
  hipStream_t s = as_stream(stream);
  Fills fill;
  for (int c = 0; c < DN_CULL_MAX_WIDTH; ++c) fill.v[c] = __builtin_bit_cast(unsigned, fills[c]);
  const unsigned* from = reinterpret_cast<const unsigned*>(src);
  unsigned* to = reinterpret_cast<unsigned*>(dst);
  unsigned* partial = static_cast<unsigned*>(workspace);   // the level-0 totals of the count: dead once the slots are written
  const bool count = d_record != nullptr;
  // (n_rows == 0 reads no source row: a NULL source passes as 16-byte aligned, and the vector kernel then only stores)
  const bool vec = width == 4 && src_stride == 4 && dst_stride == 4 && aligned(src, 16) && aligned(dst, 16);
  const int64_t ss = src_stride, ds = dst_stride;
  if (vec) launch_gather_rows<4, true>(count, blocks, s, slot, from, ss, n_rows, n_points, fill, to, ds, partial);
  else if (width == 4) launch_gather_rows<4, false>(count, blocks, s, slot, from, ss, n_rows, n_points, fill, to, ds, partial);
  else if (width == 3) launch_gather_rows<3, false>(count, blocks, s, slot, from, ss, n_rows, n_points, fill, to, ds, partial);
  else if (width == 2) launch_gather_rows<2, false>(count, blocks, s, slot, from, ss, n_rows, n_points, fill, to, ds, partial);
  else launch_gather_rows<1, false>(count, blocks, s, slot, from, ss, n_rows, n_points, fill, to, ds, partial);
  if (count) hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(kThreads), 0, s, partial, blocks, d_record);
  return check_launch(who);
}

}  // namespace occ
}  // namespace dn

using namespace dn;
using namespace dn::occ;

extern "C" int64_t dn_occupancy_words(int cx, int cy, int cz) {
  Cells g;
  return cells_of(cx, cy, cz, g) ? words_of(g) : 0;
}

extern "C" int dn_occupancy_build(const float* field, int field_stride, int cx, int cy, int cz, float level, int dilate, int accumulate,
                                  unsigned* scratch, unsigned* bits, dn_stream_t stream) {
  Cells g;
  DN_REQUIRE(field && bits, "dn_occupancy_build: null field or bits");
  DN_REQUIRE(field_stride >= 1, "dn_occupancy_build: field_stride must be >= 1");
  DN_REQUIRE(cells_of(cx, cy, cz, g), "dn_occupancy_build: cells %d x %d x %d: each axis needs 1 .. %d cells, their product at most %lld", cx, cy,
             cz, DN_OCC_MAX_AXIS_CELLS, static_cast<long long>(kMaxCells));
  DN_REQUIRE(dilate >= 0 && dilate <= DN_OCC_MAX_DILATE, "dn_occupancy_build: dilate must be 0 .. %d (got %d)", DN_OCC_MAX_DILATE, dilate);
  DN_REQUIRE(dilate == 0 || scratch, "dn_occupancy_build: dilate > 0 needs the scratch words");
  DN_REQUIRE(aligned(bits, 4) && aligned(scratch, 4) && aligned(field, 4), "dn_occupancy_build: pointers must be 4-byte aligned");
  DN_REQUIRE(dilate == 0 || scratch != bits, "dn_occupancy_build: the scratch words must not be the grid's");
  const int64_t n_words = words_of(g);
  const unsigned blocks = blocks_for(n_words, kThreads);
  hipStream_t s = as_stream(stream);
  const int acc = accumulate ? 1 : 0;
  if (dilate == 0) {
    hipLaunchKernelGGL(raw_bits_kernel, dim3(blocks), dim3(kThreads), 0, s, field, static_cast<int64_t>(field_stride), g, level, acc, n_words, bits);
  } else {
    hipLaunchKernelGGL(raw_bits_kernel, dim3(blocks), dim3(kThreads), 0, s, field, static_cast<int64_t>(field_stride), g, level, 0, n_words, scratch);
    launch_dilate(scratch, g, dilate, acc, bits, s);
  }
  return check_launch("dn_occupancy_build");
}

extern "C" size_t dn_occupancy_compact_workspace_bytes(int64_t n_rays, int n_samples) {
  Layout l;
  return layout_of(n_rays, n_samples, l) ? l.bytes : 0;
}

extern "C" int dn_occupancy_compact_count(const float* rays, int ray_stride, const float* z, int64_t n_rays, int n_samples, const unsigned* bits,
                                          int cx, int cy, int cz, float x0, float y0, float z0, float x1, float y1, float z1, float sx, float sy,
                                          float sz, void* workspace, int* slot, unsigned* d_record, dn_stream_t stream) {
  const char* who = "dn_occupancy_compact_count";
  Layout l;
  Cells g;
  if (int rc = samples_check(who, rays, ray_stride, z, n_rays, n_samples, l)) return rc;
  DN_REQUIRE(bits && workspace && slot && d_record, "%s: null bits, workspace, slots or record", who);
  DN_REQUIRE(cells_of(cx, cy, cz, g), "%s: cells %d x %d x %d: each axis needs 1 .. %d cells, their product at most %lld", who, cx, cy, cz,
             DN_OCC_MAX_AXIS_CELLS, static_cast<long long>(kMaxCells));
  DN_REQUIRE(is_finite(x0) && is_finite(y0) && is_finite(z0) && is_finite(x1) && is_finite(y1) && is_finite(z1) && x1 > x0 && y1 > y0 && z1 > z0,
             "%s: bounds must be finite with x1 > x0, y1 > y0, z1 > z0", who);
  DN_REQUIRE(is_finite(sx) && is_finite(sy) && is_finite(sz) && sx > 0.0f && sy > 0.0f && sz > 0.0f, "%s: the scales cells / (b1 - b0) must be finite and > 0",
             who);
  DN_REQUIRE(aligned(workspace, 256), "%s: workspace must be 256-byte aligned", who);
  DN_REQUIRE(aligned(slot, 4) && aligned(d_record, 4) && aligned(bits, 4), "%s: slots, record and bits must be 4-byte aligned", who);
  char* ws = static_cast<char*>(workspace);
  unsigned* t0 = reinterpret_cast<unsigned*>(ws + l.tot0);
  unsigned* t1 = reinterpret_cast<unsigned*>(ws + l.tot1);
  const Samples a{rays, ray_stride, z, l.n, n_samples};
  const Box box{{x0, y0, z0}, {sx, sy, sz}, {cx, cy, cz}};
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(classify_kernel, dim3(l.n0), dim3(kThreads), 0, s, a, box, bits, slot, t0);
  hipLaunchKernelGGL(scan_totals_kernel, dim3(l.n1), dim3(kThreads), 0, s, t0, l.n0, t1, 0u, 0);
  hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(kThreads), 0, s, t1, l.n1, d_record, static_cast<unsigned>(l.n), 1);
  hipLaunchKernelGGL(scan_slots_kernel, dim3(l.n0), dim3(kThreads), 0, s, l.n, t0, t1, slot);
  return check_launch(who);
}

extern "C" int dn_occupancy_compact_emit(const float* rays, int ray_stride, const float* z, int64_t n_rays, int n_samples, const int* slot,
                                         int64_t max_points, float* pts, dn_stream_t stream) {
  return emit("dn_occupancy_compact_emit", rays, ray_stride, z, n_rays, n_samples, slot, max_points, pts, nullptr, false, stream);
}

extern "C" int dn_occupancy_gather(const int* slot, const float* net_out, int64_t n_rows, int64_t n_points, float* rf, void* workspace,
                                   unsigned* d_record, dn_stream_t stream) {
  // column 3 of 4-float rows on both sides (a NULL stays NULL: the refusals are judged on the pointers the caller gave)
  return gather_rows("dn_occupancy_gather", "rf", "the network's output", slot, net_out ? net_out + 3 : nullptr, 4, n_rows, n_points, 1,
                     {DN_OCC_FILL, 0.0f, 0.0f, 0.0f}, rf ? rf + 3 : nullptr, 4, workspace, d_record, stream);
}

// ---- include/dexnerf_hip_cull.h -----------------------------------------------------------------------------------------------------
extern "C" int dn_occupancy_compact_emit_dirs(const float* rays, int ray_stride, const float* z, int64_t n_rays, int n_samples, const int* slot,
                                              int64_t max_points, float* pts, float* dirs, dn_stream_t stream) {
  return emit("dn_occupancy_compact_emit_dirs", rays, ray_stride, z, n_rays, n_samples, slot, max_points, pts, dirs, true, stream);
}

extern "C" int dn_occupancy_gather_rows(const int* slot, const float* src, int src_stride, int64_t n_rows, int64_t n_points, int width,
                                        float fill0, float fill1, float fill2, float fill3, float* dst, int dst_stride, void* workspace,
                                        unsigned* d_record, dn_stream_t stream) {
  return gather_rows("dn_occupancy_gather_rows", "destination", "their source", slot, src, src_stride, n_rows, n_points, width,
                     {fill0, fill1, fill2, fill3}, dst, dst_stride, workspace, d_record, stream);
}
