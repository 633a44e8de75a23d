// The Dex threshold surface of a sampled density field as an indexed triangle mesh (include/dexnerf_hip_mesh.h): marching tetrahedra
// on the six Kuhn tetrahedra of every grid cell, in a fixed order - classify, count, exclusive scan, emit.
//
//   classify_kernel        one thread per grid vertex, a wave on 64 consecutive k of one (i,j) column: the 8 corners of the vertex's
//                          cell give its 7-bit owned-edge mask, the triangle count of the cell (0..12) and its own non-finite flag,
//                          packed into one 16-bit word per vertex (mask | count << 8 | nonfinite << 15)
//   block_totals_kernel    the three sums (edge vertices, triangles, non-finite samples) of every 1024 words
//   scan_totals_kernel     exclusive scan of 1024 totals per workgroup, in place, and their sums one level up; the top level is one
//                          workgroup and writes the counts record
//   scan_elements_kernel   the per-vertex and per-cell exclusive prefixes (first mesh vertex of a grid vertex, first triangle of a cell):
//                          the scan inside a workgroup's 1024 words plus the two scanned levels above it
//   emit_vertices_kernel   one thread per grid vertex: its owned edges' vertices, fp64 from the fp32 inputs, rounded once
//   emit_triangles_kernel  one thread per cell: an edge's vertex is base[owner] + popcount(mask[owner] & ((1 << slot) - 1))
//
// No workgroup waits on another (the scan is the multi-launch kind), no atomics (the non-finite count is a third scanned sum), plain
// vector stores, every sum in a fixed order: the output is a function of the field.  The grid of every launch is a function of
// (nx, ny, nz) alone (an emit launch whose capacity is 0 is left out).
//
// Memory: HBM-bound.  classify reads 4 B per sample once (the other seven corners of a cell are its neighbours' samples: cache
// hits) and writes 2 B; the scan passes read 2 B twice and write 8 B; emit reads 2 B per vertex and touches the field and the prefixes
// only at surface cells.
#include "../../include/dexnerf_hip_mesh.h"
#include "scan_blocks.h"

namespace dn {
namespace iso {

constexpr int kThreads = kScanThreads;
constexpr int kPerThread = kScanPerThread;
constexpr int kScanBlock = DN_ISO_SCAN_BLOCK;   // elements per workgroup at every scan level
static_assert(kScanBlock == kScanElems && kScanBlock == kThreads * kPerThread, "a workgroup scans 256 x 4 elements (scan_blocks.h)");
constexpr int64_t kMaxVertices = DN_ISO_MAX_GRID_VERTICES;
// the top scan level is one workgroup; 7 mesh vertices per grid vertex stay inside int32
static_assert(kMaxVertices <= static_cast<int64_t>(kScanBlock) * kScanBlock * kScanBlock && 7 * kMaxVertices < (int64_t{1} << 31), "limits");

// ---- the Kuhn tetrahedra and their cases ----------------------------------------------------------------------------------------
// A cell corner is its code 4dx + 2dy + dz.  Tetrahedron p (the axis permutations in lexicographic order) has the corners
// 0, c1 = bit(p1), c2 = c1 | bit(p2), 7; packed three bits per tetrahedron.
constexpr int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
constexpr int axis_bit(int a) { return 4 >> a; }
constexpr unsigned pack_corners(int which) {
  unsigned r = 0;
  for (int p = 0; p < 6; ++p) {
    const int c1 = axis_bit(kPerm[p][0]);
    r |= static_cast<unsigned>(which == 1 ? c1 : (c1 | axis_bit(kPerm[p][1]))) << (3 * p);
  }
  return r;
}
constexpr unsigned kTetC1 = pack_corners(1), kTetC2 = pack_corners(2);

// Entry (p, m), m = the inside bits of the tetrahedron's corners 0..3: up to four edge references of 6 bits each (owner corner code |
// slot << 3) in the order of the header's rule - three for a triangle, q0..q3 for the quad -, the triangle count in bits 24..25 and
// the swap of the last two indices in bit 26.  The swap is found here, at compile time, on the unit cube with the vertices at the
// edge midpoints (coordinates doubled, so integers): the sign of ((v1 - v0) x (v2 - v0)) . (outside centroid - inside centroid) does
// not depend on where on its edge a vertex sits, nor on the (increasing) grid coordinates.
struct CaseTable {
  unsigned e[6 * 16];
};
constexpr CaseTable make_cases() {
  CaseTable t{};
  for (int p = 0; p < 6; ++p) {
    const int c1 = axis_bit(kPerm[p][0]);
    const int code[4] = {0, c1, c1 | axis_bit(kPerm[p][1]), 7};
    for (int m = 1; m < 15; ++m) {
      int in[4] = {}, out[4] = {}, ni = 0, no = 0;
      for (int c = 0; c < 4; ++c) {
        if ((m >> c) & 1) in[ni++] = c; else out[no++] = c;
      }
      int ea[4] = {}, eb[4] = {}, ne = 3;
      if (ni == 1) {
        for (int q = 0; q < 3; ++q) { ea[q] = in[0]; eb[q] = out[q]; }
      } else if (ni == 3) {
        for (int q = 0; q < 3; ++q) { ea[q] = in[q]; eb[q] = out[0]; }
      } else {
        ea[0] = in[0]; eb[0] = out[0];
        ea[1] = in[0]; eb[1] = out[1];
        ea[2] = in[1]; eb[2] = out[1];
        ea[3] = in[1]; eb[3] = out[0];
        ne = 4;
      }
      long pos[4][3] = {}, dir[3] = {};
      for (int d = 0; d < 3; ++d) {
        for (int q = 0; q < ne; ++q) pos[q][d] = ((code[ea[q]] >> (2 - d)) & 1) + ((code[eb[q]] >> (2 - d)) & 1);
        for (int q = 0; q < no; ++q) dir[d] += ni * ((code[out[q]] >> (2 - d)) & 1);
        for (int q = 0; q < ni; ++q) dir[d] -= no * ((code[in[q]] >> (2 - d)) & 1);
      }
      const long u[3] = {pos[1][0] - pos[0][0], pos[1][1] - pos[0][1], pos[1][2] - pos[0][2]};
      const long w[3] = {pos[2][0] - pos[0][0], pos[2][1] - pos[0][1], pos[2][2] - pos[0][2]};
      const long dot = (u[1] * w[2] - u[2] * w[1]) * dir[0] + (u[2] * w[0] - u[0] * w[2]) * dir[1] + (u[0] * w[1] - u[1] * w[0]) * dir[2];
      unsigned bits = static_cast<unsigned>(ne - 2) << 24 | (dot < 0 ? 1u << 26 : 0u);
      for (int q = 0; q < ne; ++q) {
        const int lo = ea[q] < eb[q] ? ea[q] : eb[q], hi = ea[q] < eb[q] ? eb[q] : ea[q];
        bits |= static_cast<unsigned>(code[lo] | (code[hi] - code[lo] - 1) << 3) << (6 * q);
      }
      t.e[p * 16 + m] = bits;
    }
  }
  return t;
}
__constant__ CaseTable kCases = make_cases();

// ---- shared device pieces -------------------------------------------------------------------------------------------------------
struct Grid {
  int nx, ny, nz;
  unsigned nchunk;   // 64-sample chunks per column
};

// One thread per grid vertex; wave w of the launch takes chunk w % nchunk of column w / nchunk, its lanes 64 consecutive k.
__device__ __forceinline__ bool vertex_of_thread(const Grid& g, int& i, int& j, int& k) {
  const unsigned wave = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
  const unsigned col = wave / g.nchunk, chunk = wave - col * g.nchunk;
  if (col >= static_cast<unsigned>(g.nx) * static_cast<unsigned>(g.ny)) return false;
  i = static_cast<int>(col / static_cast<unsigned>(g.ny));
  j = static_cast<int>(col - static_cast<unsigned>(i) * static_cast<unsigned>(g.ny));
  k = static_cast<int>(chunk * kWave) + lane_id();
  return k < g.nz;
}

__device__ __forceinline__ int64_t corner_offset(const Grid& g, unsigned code) {
  return static_cast<int64_t>((code >> 2) & 1) * g.ny * g.nz + static_cast<int64_t>((code >> 1) & 1) * g.nz + (code & 1);
}

// bit c of `fin` / `ins`: corner c of the cell at (i,j,k) is in the grid and finite / inside
__device__ __forceinline__ void corner_bits(const float* __restrict__ f, int64_t fs, const Grid& g, int i, int j, int k, int64_t v, float level,
                                            unsigned& fin, unsigned& ins) {
  const bool hx = i + 1 < g.nx, hy = j + 1 < g.ny, hz = k + 1 < g.nz;
  fin = ins = 0;
#pragma unroll
  for (unsigned c = 0; c < 8; ++c) {
    const bool there = (!(c & 4) || hx) && (!(c & 2) || hy) && (!(c & 1) || hz);
    if (there) {
      const float x = f[(v + corner_offset(g, c)) * fs];
      const bool finite = (__builtin_bit_cast(unsigned, x) & 0x7F800000u) != 0x7F800000u;
      fin |= static_cast<unsigned>(finite) << c;
      ins |= static_cast<unsigned>(finite && x > level) << c;
    }
  }
}

// the inside bits of tetrahedron p's corners 0..3; 0 ("emits nothing") if one of them is not finite
__device__ __forceinline__ unsigned tet_case(unsigned fin, unsigned ins, int p) {
  const unsigned c1 = (kTetC1 >> (3 * p)) & 7, c2 = (kTetC2 >> (3 * p)) & 7;
  if (!(fin & (fin >> c1) & (fin >> c2) & (fin >> 7) & 1)) return 0;
  return (ins & 1) | ((ins >> c1) & 1) << 1 | ((ins >> c2) & 1) << 2 | ((ins >> 7) & 1) << 3;
}

__device__ __forceinline__ unsigned edges_of(unsigned word) { return __popc(word & 0x7Fu); }
__device__ __forceinline__ unsigned triangles_of(unsigned word) { return (word >> 8) & 0xFu; }

// the four class words of thread t of workgroup b (elements b * 1024 + 4t ..), 0 past the end
__device__ __forceinline__ void load_words(const uint16_t* __restrict__ cls, int64_t n, int64_t e0, unsigned (&w)[kPerThread]) {
  if (e0 + kPerThread <= n) {
    const uint2 r = *reinterpret_cast<const uint2*>(cls + e0);
    w[0] = r.x & 0xFFFFu; w[1] = r.x >> 16; w[2] = r.y & 0xFFFFu; w[3] = r.y >> 16;
  } else {
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) w[q] = e0 + q < n ? cls[e0 + q] : 0u;
  }
}

// ---- kernels --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void classify_kernel(const float* __restrict__ f, int64_t fs, Grid g, float level,
                                                            uint16_t* __restrict__ cls) {
  int i, j, k;
  if (!vertex_of_thread(g, i, j, k)) return;
  const int64_t v = (static_cast<int64_t>(i) * g.ny + j) * g.nz + k;
  unsigned fin, ins;
  corner_bits(f, fs, g, i, j, k, v, level, fin, ins);
  // slot c - 1: both ends finite (a corner outside the grid counts as not finite) and exactly one inside
  const unsigned own = (fin & 1) ? 0x7Fu : 0u, flip = (ins & 1) ? 0x7Fu : 0u;
  const unsigned mask = (fin >> 1) & own & ((ins >> 1) ^ flip);
  unsigned tris = 0;
  if (i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz) {
#pragma unroll
    for (int p = 0; p < 6; ++p) tris += (kCases.e[p * 16 + tet_case(fin, ins, p)] >> 24) & 3u;
  }
  cls[v] = static_cast<uint16_t>(mask | tris << 8 | ((fin & 1) ? 0u : 0x8000u));
}

__global__ __launch_bounds__(kThreads) void block_totals_kernel(const uint16_t* __restrict__ cls, int64_t n, unsigned* __restrict__ tot_v,
                                                                unsigned* __restrict__ tot_t, unsigned* __restrict__ tot_n) {
  __shared__ unsigned lds[3][4];
  unsigned w[kPerThread];
  load_words(cls, n, static_cast<int64_t>(blockIdx.x) * kScanBlock + threadIdx.x * kPerThread, w);
  unsigned sv = 0, st = 0, sn = 0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) { sv += edges_of(w[q]); st += triangles_of(w[q]); sn += w[q] >> 15; }
  unsigned av, at, an;
  block_scan_exclusive(sv, lds[0], av);
  block_scan_exclusive(st, lds[1], at);
  block_scan_exclusive(sn, lds[2], an);
  if (threadIdx.x == 0) { tot_v[blockIdx.x] = av; tot_t[blockIdx.x] = at; tot_n[blockIdx.x] = an; }
}

// (scan_row of scan_blocks.h: a row's exclusive prefix inside every block of 1024, in place, and the blocks' sums one level up)
__global__ __launch_bounds__(kThreads) void scan_totals_kernel(unsigned* __restrict__ a_v, unsigned* __restrict__ a_t, unsigned* __restrict__ a_n,
                                                               unsigned n, unsigned* __restrict__ up_v, unsigned* __restrict__ up_t,
                                                               unsigned* __restrict__ up_n, unsigned* __restrict__ reserved) {
  __shared__ unsigned lds[3][4];
  scan_row(a_v, n, up_v, lds[0]);
  scan_row(a_t, n, up_t, lds[1]);
  scan_row(a_n, n, up_n, lds[2]);
  if (reserved && blockIdx.x == 0 && threadIdx.x == 0) *reserved = 0u;
}

// tot: the level-0 totals scanned inside their blocks of 1024; up: the scanned level-1 totals - their sum is the prefix of workgroup b
__global__ __launch_bounds__(kThreads) void scan_elements_kernel(const uint16_t* __restrict__ cls, int64_t n, const unsigned* __restrict__ tot_v,
                                                                 const unsigned* __restrict__ tot_t, const unsigned* __restrict__ up_v,
                                                                 const unsigned* __restrict__ up_t, unsigned* __restrict__ vbase,
                                                                 unsigned* __restrict__ tbase) {
  __shared__ unsigned lds[2][4];
  const int64_t e0 = static_cast<int64_t>(blockIdx.x) * kScanBlock + threadIdx.x * kPerThread;
  unsigned w[kPerThread];
  load_words(cls, n, e0, w);
  unsigned sv = 0, st = 0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) { sv += edges_of(w[q]); st += triangles_of(w[q]); }
  unsigned all;
  unsigned rv = tot_v[blockIdx.x] + up_v[blockIdx.x / kScanBlock] + block_scan_exclusive(sv, lds[0], all);
  unsigned rt = tot_t[blockIdx.x] + up_t[blockIdx.x / kScanBlock] + block_scan_exclusive(st, lds[1], all);
  unsigned ov[kPerThread], ot[kPerThread];
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    ov[q] = rv; ot[q] = rt;
    rv += edges_of(w[q]); rt += triangles_of(w[q]);
  }
  if (e0 + kPerThread <= n) {
    *reinterpret_cast<uint4*>(vbase + e0) = make_uint4(ov[0], ov[1], ov[2], ov[3]);
    *reinterpret_cast<uint4*>(tbase + e0) = make_uint4(ot[0], ot[1], ot[2], ot[3]);
  } else {
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
      if (e0 + q < n) { vbase[e0 + q] = ov[q]; tbase[e0 + q] = ot[q]; }
    }
  }
}

__global__ __launch_bounds__(kThreads) void emit_vertices_kernel(const float* __restrict__ f, int64_t fs, const float* __restrict__ xs,
                                                                 const float* __restrict__ ys, const float* __restrict__ zs, Grid g, float level,
                                                                 const uint16_t* __restrict__ cls, const unsigned* __restrict__ vbase,
                                                                 int64_t max_vertices, float* __restrict__ out) {
  int i, j, k;
  if (!vertex_of_thread(g, i, j, k)) return;
  const int64_t v = (static_cast<int64_t>(i) * g.ny + j) * g.nz + k;
  const unsigned mask = cls[v] & 0x7Fu;
  if (!mask) return;
  const int64_t base = vbase[v];
  if (base >= max_vertices) return;
  const double fa = f[v * fs], lv = level;
  // a set slot's far end is in the grid, so the clamped loads below read the far coordinate wherever it is used
  const double ax = xs[i], ay = ys[j], az = zs[k];
  const double bx = xs[min(i + 1, g.nx - 1)], by = ys[min(j + 1, g.ny - 1)], bz = zs[min(k + 1, g.nz - 1)];
#pragma unroll
  for (unsigned s = 0; s < 7; ++s) {
    if (!((mask >> s) & 1)) continue;
    const unsigned c = s + 1;
    const int64_t idx = base + __popc(mask & ((1u << s) - 1u));
    if (idx >= max_vertices) continue;
    const double fb = f[(v + corner_offset(g, c)) * fs];
    const double t = (lv - fa) / (fb - fa);
    float* row = out + idx * 3;
    row[0] = static_cast<float>(ax + (((c & 4) ? bx : ax) - ax) * t);
    row[1] = static_cast<float>(ay + (((c & 2) ? by : ay) - ay) * t);
    row[2] = static_cast<float>(az + (((c & 1) ? bz : az) - az) * t);
  }
}

__global__ __launch_bounds__(kThreads) void emit_triangles_kernel(const float* __restrict__ f, int64_t fs, Grid g, float level,
                                                                  const uint16_t* __restrict__ cls, const unsigned* __restrict__ vbase,
                                                                  const unsigned* __restrict__ tbase, int64_t max_triangles,
                                                                  int* __restrict__ out) {
  int i, j, k;
  if (!vertex_of_thread(g, i, j, k)) return;
  if (i + 1 >= g.nx || j + 1 >= g.ny || k + 1 >= g.nz) return;
  const int64_t v = (static_cast<int64_t>(i) * g.ny + j) * g.nz + k;
  if (!triangles_of(cls[v])) return;
  int64_t t = tbase[v];
  if (t >= max_triangles) return;
  unsigned fin, ins;
  corner_bits(f, fs, g, i, j, k, v, level, fin, ins);
  for (int p = 0; p < 6; ++p) {
    const unsigned e = kCases.e[p * 16 + tet_case(fin, ins, p)];
    const unsigned ntri = (e >> 24) & 3u;
    if (!ntri) continue;
    auto vertex = [&](int q) {
      const unsigned r = (e >> (6 * q)) & 63u;
      const int64_t owner = v + corner_offset(g, r & 7u);
      return static_cast<int>(vbase[owner] + __popc(cls[owner] & ((1u << (r >> 3)) - 1u)));
    };
    const bool swap = (e >> 26) & 1u;
    const int q0 = vertex(0), q1 = vertex(1), q2 = vertex(2);
    if (t < max_triangles) {
      int* row = out + t * 3;
      row[0] = q0; row[1] = swap ? q2 : q1; row[2] = swap ? q1 : q2;
    }
    ++t;
    if (ntri == 2) {
      const int q3 = vertex(3);
      if (t < max_triangles) {
        int* row = out + t * 3;
        row[0] = q0; row[1] = swap ? q3 : q2; row[2] = swap ? q2 : q3;
      }
      ++t;
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct Layout {
  int64_t nv;
  unsigned n0, n1;                                  // totals at scan level 0 and 1
  size_t cls, vbase, tbase, tot0, tot1, bytes;      // byte offsets of the regions; tot0 / tot1 hold three rows of row0 / row1 words
  size_t row0, row1;
};

// false: a grid the entry points refuse
bool layout_of(int nx, int ny, int nz, Layout& l) {
  if (nx < 2 || ny < 2 || nz < 2) return false;
  const int64_t nxy = static_cast<int64_t>(nx) * ny;
  if (nxy > kMaxVertices) return false;
  l.nv = nxy * nz;
  if (l.nv > kMaxVertices) return false;
  if (12 * (static_cast<int64_t>(nx - 1) * (ny - 1) * (nz - 1)) >= (int64_t{1} << 31)) return false;
  l.n0 = static_cast<unsigned>((l.nv + kScanBlock - 1) / kScanBlock);
  l.n1 = (l.n0 + kScanBlock - 1) / kScanBlock;
  if (l.n1 > static_cast<unsigned>(kScanBlock)) return false;
  l.row0 = up256(sizeof(unsigned) * l.n0) / sizeof(unsigned);
  l.row1 = up256(sizeof(unsigned) * l.n1) / sizeof(unsigned);
  l.cls = 0;
  l.vbase = l.cls + up256(sizeof(uint16_t) * static_cast<size_t>(l.nv));
  l.tbase = l.vbase + up256(sizeof(unsigned) * static_cast<size_t>(l.nv));
  l.tot0 = l.tbase + up256(sizeof(unsigned) * static_cast<size_t>(l.nv));
  l.tot1 = l.tot0 + 3 * sizeof(unsigned) * l.row0;
  l.bytes = l.tot1 + 3 * sizeof(unsigned) * l.row1;
  return true;
}

int common_check(const char* who, const float* field, int field_stride, const float* xs, const float* ys, const float* zs, int nx, int ny,
                 int nz, const void* workspace, Layout& l) {
  DN_REQUIRE(field && xs && ys && zs && workspace, "%s: null field, coordinates or workspace", who);
  DN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: every axis needs at least 2 coordinates, got %d x %d x %d", who, nx, ny, nz);
  DN_REQUIRE(field_stride >= 1, "%s: field_stride must be >= 1", who);
  DN_REQUIRE(layout_of(nx, ny, nz, l), "%s: grid %d x %d x %d is past the maximum (nx*ny*nz <= %lld and 12 * cells < 2^31)", who, nx, ny,
             nz, static_cast<long long>(kMaxVertices));
  DN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  return 0;
}

Grid grid_of(int nx, int ny, int nz) { return Grid{nx, ny, nz, static_cast<unsigned>((nz + kWave - 1) / kWave)}; }
// workgroups of the one-thread-per-grid-vertex launches: four waves each, a wave per (column, chunk)
unsigned vertex_blocks(const Grid& g) {
  const int64_t waves = static_cast<int64_t>(g.nx) * g.ny * g.nchunk;   // <= nx*ny*nz
  return static_cast<unsigned>((waves + kThreads / kWave - 1) / (kThreads / kWave));
}

}  // namespace iso
}  // namespace dn

using namespace dn;
using namespace dn::iso;

extern "C" size_t dn_isosurface_workspace_bytes(int nx, int ny, int nz) {
  Layout l;
  return layout_of(nx, ny, nz, l) ? l.bytes : 0;
}

extern "C" int dn_isosurface_count(const float* field, int field_stride, const float* xs, const float* ys, const float* zs, int nx, int ny,
                                   int nz, float level, void* workspace, unsigned* d_counts, dn_stream_t stream) {
  Layout l;
  if (int rc = common_check("dn_isosurface_count", field, field_stride, xs, ys, zs, nx, ny, nz, workspace, l)) return rc;
  DN_REQUIRE(d_counts, "dn_isosurface_count: null counts record");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(d_counts) & 3) == 0, "dn_isosurface_count: counts record must be 4-byte aligned");
  char* ws = static_cast<char*>(workspace);
  uint16_t* cls = reinterpret_cast<uint16_t*>(ws + l.cls);
  unsigned* vbase = reinterpret_cast<unsigned*>(ws + l.vbase);
  unsigned* tbase = reinterpret_cast<unsigned*>(ws + l.tbase);
  unsigned* t0 = reinterpret_cast<unsigned*>(ws + l.tot0);
  unsigned* t1 = reinterpret_cast<unsigned*>(ws + l.tot1);
  const Grid g = grid_of(nx, ny, nz);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(classify_kernel, dim3(vertex_blocks(g)), dim3(kThreads), 0, s, field, static_cast<int64_t>(field_stride), g, level, cls);
  hipLaunchKernelGGL(block_totals_kernel, dim3(l.n0), dim3(kThreads), 0, s, cls, l.nv, t0, t0 + l.row0, t0 + 2 * l.row0);
  hipLaunchKernelGGL(scan_totals_kernel, dim3(l.n1), dim3(kThreads), 0, s, t0, t0 + l.row0, t0 + 2 * l.row0, l.n0, t1, t1 + l.row1,
                     t1 + 2 * l.row1, static_cast<unsigned*>(nullptr));
  hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(kThreads), 0, s, t1, t1 + l.row1, t1 + 2 * l.row1, l.n1, d_counts, d_counts + 1,
                     d_counts + 2, d_counts + 3);
  hipLaunchKernelGGL(scan_elements_kernel, dim3(l.n0), dim3(kThreads), 0, s, cls, l.nv, t0, t0 + l.row0, t1, t1 + l.row1, vbase, tbase);
  return check_launch("dn_isosurface_count");
}

extern "C" int dn_isosurface_emit(const float* field, int field_stride, const float* xs, const float* ys, const float* zs, int nx, int ny,
                                  int nz, float level, const void* workspace, int64_t max_vertices, int64_t max_triangles, float* vertices,
                                  int* triangles, dn_stream_t stream) {
  Layout l;
  if (int rc = common_check("dn_isosurface_emit", field, field_stride, xs, ys, zs, nx, ny, nz, workspace, l)) return rc;
  DN_REQUIRE(max_vertices >= 0 && max_triangles >= 0, "dn_isosurface_emit: negative capacity");
  DN_REQUIRE((max_vertices == 0 || vertices) && (max_triangles == 0 || triangles), "dn_isosurface_emit: a capacity without its output");
  const char* ws = static_cast<const char*>(workspace);
  const uint16_t* cls = reinterpret_cast<const uint16_t*>(ws + l.cls);
  const unsigned* vbase = reinterpret_cast<const unsigned*>(ws + l.vbase);
  const unsigned* tbase = reinterpret_cast<const unsigned*>(ws + l.tbase);
  const Grid g = grid_of(nx, ny, nz);
  hipStream_t s = as_stream(stream);
  if (max_vertices > 0)
    hipLaunchKernelGGL(emit_vertices_kernel, dim3(vertex_blocks(g)), dim3(kThreads), 0, s, field, static_cast<int64_t>(field_stride), xs, ys, zs, g,
                       level, cls, vbase, max_vertices, vertices);
  if (max_triangles > 0)
    hipLaunchKernelGGL(emit_triangles_kernel, dim3(vertex_blocks(g)), dim3(kThreads), 0, s, field, static_cast<int64_t>(field_stride), g, level, cls,
                       vbase, tbase, max_triangles, triangles);
  return check_launch("dn_isosurface_emit");
}
