// Input gradients of the fused network: dL/d(points), dL/d(view directions) and - for the ray-rows form - dL/d(ray rows), dL/d(depths).
//
// dn_mlp_backward_data leaves dL/d(pre-activation) of every stage in the `grads` records.  The encodings enter the network in
// layer1, in every wide trunk layer (skip connections) and in layers_dir.0, so for a tile of 32 points per wave
//     g_enc_xyz[64 x 32] = layer1.weight^T . g_layer1 + sum_{i wide} layers_xyz[i].weight[:, W:W+DX]^T . g_trunk_i
//     g_enc_dir[32 x 32] = layers_dir.0.weight[:, W:W+DD]^T . g_dirout
// on MFMA with fp32 accumulation: the B operand is the saved gradient piece exactly as it lies in the record (column = lane =
// point), the A operand a small pre-packed transposed stream of those weight blocks (dn_mlp_pack_input_grad).  Row m of output
// tile mt is chosen so that the accumulator registers of a lane in half h are the encoding slots u = 16 mt + r of ITS half
// (pe_slot_col, the forward's own slot order; padding slots are zero rows): the Jacobian of the positional encoding
//     dx_d = g[d] + sum_k f_k (cos(f_k x_d) g[3 + 6k + d] - sin(f_k x_d) g[6 + 6k + d])
// is then formed in registers, sin / cos recomputed from the fp32 inputs, and the two halves' partial sums meet in one cross-lane
// add.  A second small launch (one wave per ray, fixed summation order) reduces the per-point results to the ray rows.
// Plain stores, no atomics: the result is a pure function of the inputs.
//
// Memory traffic is what the kernel costs: a point reads its three or four gradient slots once and writes 24 B (d_pts + d_viewdir).  Bytes per
// point at D8/W256 with view directions: layer1 + one wide layer + layers_dir.0 = 256 + 256 + 128 values = 1280 B (16-bit saves)
// or 2560 B (fp32), + 16..28 B of inputs, + 24 B out; 4 x 128 nets: 128 + 64 values = 384 B / 768 B.  The transposed stream
// (72 KiB / 144 KiB at D8/W256) is read once per workgroup into LDS, or through L2 when a deep net's stream exceeds LDS.
// The MFMA work is ~6 % of the forward's.  Measured (profiles/input_grad_time.md, both launches, 4096 x 192 points at D8/W256):
// 3.8 TB/s with 16-bit saves, 2.9 TB/s in fp32 - 60 % / 46 % of the 6.29 TB/s copy rate; 150 VGPRs at L_xyz = 10 keep a CU at one
// workgroup (two waves per SIMD), which is what stands between it and the copy rate.
#include "mlp_internal.h"

namespace dn {

constexpr int kIgMaxStages = 32;       // layer1 + at most D - 2 <= 30 wide trunk layers
constexpr int kIgWaves = 8;            // waves per workgroup, one 32-point tile each per pass (16 waves would cap a wave at 128 VGPRs: the L = 10 Jacobian spills)
constexpr int kIgLdsBudget = 160 * 1024;

struct IgLayout {
  int n_x;                             // xyz stages: layer1, then the wide trunk layers in ascending order
  int src[kIgMaxStages];               // index into the weight pointer list
  int ld[kIgMaxStages];                // in_features of that weight
  int col0[kIgMaxStages];              // first column of its xyz-encoding block
  int gslot[kIgMaxStages];             // first piece of the stage's gradient in a `grads` record
  int kh;                              // pieces of a W-wide hidden vector
  int dir_piece0, dir_pieces;          // layers_dir.0 stage: one 32-row tile, kh / 2 pieces (0 without view directions)
  int dir_src, dir_ld, dir_col0, gslot_dirout;
  int grad_pieces;
  int total_pieces;
  int LX, LD;
};

static void build_input_grad_layout(const dn_mlp_desc& d, int precision, IgLayout* out) {
  TrainLayout t;
  build_train_layout(d, precision, &t);
  const int W = d.hidden_size, D = d.num_layers;
  const int DX = 3 + 6 * d.num_encoding_fn_xyz, DD = 3 + 6 * d.num_encoding_fn_dir;
  IgLayout& g = *out;
  g = IgLayout{};
  g.kh = t.kh; g.grad_pieces = t.grad_pieces; g.LX = d.num_encoding_fn_xyz; g.LD = d.num_encoding_fn_dir;
  int n = 0;
  g.src[n] = 0; g.ld[n] = DX; g.col0[n] = 0; g.gslot[n] = t.gslot_layer1; ++n;
  for (int i = 1; i < D - 1; ++i) {
    if (i % d.skip_connect_every != 0) continue;   // (the wide layers of build_layout)
    g.src[n] = 1 + i; g.ld[n] = W + DX; g.col0[n] = W; g.gslot[n] = t.gslot_trunk0 + i * t.kh; ++n;
  }
  g.n_x = n;
  g.dir_piece0 = n * 2 * t.kh;
  g.dir_pieces = d.use_viewdirs ? t.kh / 2 : 0;
  g.dir_src = D; g.dir_ld = W + DD; g.dir_col0 = W; g.gslot_dirout = t.gslot_dirout;
  g.total_pieces = g.dir_piece0 + g.dir_pieces;
}

// ---- pack: nn.Linear weights -> transposed A pieces ----------------------------------------------------------
// Piece (stage s, output tile mt, k): lane (m, hh) element e = W_s[kout][col0 + pe_slot_col(L, h_m, 16 mt + r_m)], where
// kout = the feature piece k holds for (hh, e) in a gradient record and (h_m, r_m) = the lane half / accumulator register that
// receives row m of the tile (the inverse of acc_row).
template <int BF16>
__global__ void pack_input_grad_kernel(IgLayout g, PackPtrs ptrs, char* __restrict__ packed) {
  using P = Prec<BF16>;
  const long long n_elems = static_cast<long long>(g.total_pieces) * 64 * P::EPP;
  for (long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; idx < n_elems;
       idx += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int e = static_cast<int>(idx % P::EPP);
    const int lane = static_cast<int>((idx / P::EPP) % 64);
    const int piece = static_cast<int>(idx / (P::EPP * 64));
    const int m = lane & 31, hh = lane >> 5;
    const int h_m = (m >> 2) & 1, r_m = (m & 3) + 4 * (m >> 3);
    int k, pc, ld, col0;
    const float* w;
    if (piece < g.dir_piece0) {
      const int s = piece / (2 * g.kh), rel = piece % (2 * g.kh);
      k = rel % g.kh;
      pc = pe_slot_col(g.LX, h_m, 16 * (rel / g.kh) + r_m);
      w = ptrs.w[g.src[s]]; ld = g.ld[s]; col0 = g.col0[s];
    } else {
      k = piece - g.dir_piece0;
      pc = pe_slot_col(g.LD, h_m, r_m);
      w = ptrs.w[g.dir_src]; ld = g.dir_ld; col0 = g.dir_col0;
    }
    const int kout = (k / P::PPT) * 32 + acc_row((k % P::PPT) * P::EPP + e, hh);
    const float v = (pc >= 0) ? w[static_cast<long long>(kout) * ld + col0 + pc] : 0.0f;
    reinterpret_cast<typename P::Elem*>(packed)[idx] = static_cast<typename P::Elem>(v);
  }
}

struct IgParams {
  const char* stream;      // transposed pieces (dn_mlp_pack_input_grad)
  int stream_bytes;
  int in_lds;              // the stream fits LDS: every workgroup copies it once
  const char* grads;       // [tile32][grad_pieces][64][16 B]
  int grad_pieces;
  int n_x, kh;
  int gslot[kIgMaxStages];
  int gslot_dirout, dir_piece0, use_viewdirs;
  int mode;                // 0: rays + z, 1: pts (+ viewdirs)
  const float* rays;
  int ray_stride;
  const float* z;
  const float* pts;
  const float* viewdirs;
  long long n_points;
  int S;
  long long n_tiles32, n_wg_tiles;
  float* d_pts;            // (P,3)
  float* d_vd;             // (P,3) per point, or NULL
  float fx[16];
  float fd[8];
};

// Jacobian of one lane-half's encoding slots: g[u] = dL/d(slot u) (pe_slot_col order), x = the fp32 input.
template <int NF>
__device__ __forceinline__ void pe_jacobian(const float* g, const float (&x)[3], const float* freqs, int h, float (&dx)[3]) {
  dx[0] = dx[1] = dx[2] = 0.0f;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const float fr = h ? freqs[NF + f] : freqs[f];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float sv, cv;
      sincosf(x[c] * fr, &sv, &cv);   // the forward's argument: the fp32 product
      dx[c] += fr * (cv * g[6 * f + c] - sv * g[6 * f + 3 + c]);
    }
  }
  // identity slots: half 0 owns x, y; half 1 owns z
  if (h) dx[2] += g[6 * NF];
  else { dx[0] += g[6 * NF]; dx[1] += g[6 * NF + 1]; }
}

// v(lane) + v(lane ^ 32).  (Through ds_bpermute: with v_permlane32_swap of a value with itself hipcc folded the two results into
// one where only one lane half's sum is stored - the other half's partial was lost.)
__device__ __forceinline__ float add_other_half(float v) { return v + __shfl_xor(v, 32, 64); }

template <int BF16, int LX>
__global__ __launch_bounds__(kIgWaves * 64) void mlp_input_grad_kernel(IgParams p) {
  using P = Prec<BF16>;
  using BPiece = typename P::BPiece;
  constexpr int LD = 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, j = lane & 31;

  if (p.in_lds) {
    for (int off = threadIdx.x * 16; off < p.stream_bytes; off += kIgWaves * 64 * 16)
      *reinterpret_cast<f32x4*>(smem + off) = *reinterpret_cast<const f32x4*>(p.stream + off);
    __syncthreads();
  }
  const char* abase = (p.in_lds ? static_cast<const char*>(smem) : p.stream) + lane * 16;
  const int kh = p.kh;

  for (long long tile = blockIdx.x; tile < p.n_wg_tiles; tile += gridDim.x) {
    const long long tile32 = tile * kIgWaves + wave;
    if (tile32 >= p.n_tiles32) continue;   // (no barrier inside the loop)
    const char* gtile = p.grads + (tile32 * p.grad_pieces * 64 + lane) * 16;

    // ---- this lane's point: lanes j and j + 32 share point tile32 * 32 + j ----
    const long long pt_raw = tile32 * 32 + j;
    const bool live = pt_raw < p.n_points;
    const long long pt = live ? pt_raw : p.n_points - 1;   // padding lanes recompute a valid point and store nothing
    float x[3], vd[3] = {0.0f, 0.0f, 0.0f};
    if (p.mode == 0) {
      const float* r = p.rays + (pt / p.S) * p.ray_stride;
      const float zz = p.z[pt];
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = r[c] + r[3 + c] * zz;   // plain mul then add, as the forward forms it
      if (p.use_viewdirs) {
#pragma unroll
        for (int c = 0; c < 3; ++c) vd[c] = r[8 + c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = p.pts[pt * 3 + c];
      if (p.use_viewdirs) {
#pragma unroll
        for (int c = 0; c < 3; ++c) vd[c] = p.viewdirs[(pt / p.S) * 3 + c];
      }
    }

    // ---- encoded gradient of the xyz panel: two 32-row tiles, every stage accumulates into them ----
    f32x16 acc0 = {}, acc1 = {};
    for (int s = 0; s < p.n_x; ++s) {
      const char* b = gtile + static_cast<long long>(p.gslot[s]) * kPieceBytes;
      const char* a0 = abase + static_cast<long long>(s) * 2 * kh * kPieceBytes;
      const char* a1 = a0 + static_cast<long long>(kh) * kPieceBytes;
      for (int k0 = 0; k0 < kh; k0 += 8) {   // (kh is a multiple of 8: eight record pieces in flight per pass)
        BPiece bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) bv[u] = *reinterpret_cast<const BPiece*>(b + (k0 + u) * kPieceBytes);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          acc0 = mma_piece<BF16>(acc0, *reinterpret_cast<const f32x4*>(a0 + (k0 + u) * kPieceBytes), bv[u]);
          acc1 = mma_piece<BF16>(acc1, *reinterpret_cast<const f32x4*>(a1 + (k0 + u) * kPieceBytes), bv[u]);
        }
      }
    }
    float g[32];
#pragma unroll
    for (int r = 0; r < 16; ++r) { g[r] = acc0[r]; g[16 + r] = acc1[r]; }
    float dx[3];
    pe_jacobian<LX / 2>(g, x, p.fx, h, dx);
#pragma unroll
    for (int c = 0; c < 3; ++c) dx[c] = add_other_half(dx[c]);
    if (live && h == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p.d_pts[pt * 3 + c] = dx[c];
    }

    // ---- view direction ----
    if (p.use_viewdirs) {
      f32x16 accd = {};
      const char* b = gtile + static_cast<long long>(p.gslot_dirout) * kPieceBytes;
      const char* a = abase + static_cast<long long>(p.dir_piece0) * kPieceBytes;
      for (int k0 = 0; k0 < kh / 2; k0 += 4) {
        BPiece bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) bv[u] = *reinterpret_cast<const BPiece*>(b + (k0 + u) * kPieceBytes);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          accd = mma_piece<BF16>(accd, *reinterpret_cast<const f32x4*>(a + (k0 + u) * kPieceBytes), bv[u]);
      }
      float gd[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) gd[r] = accd[r];
      float dv[3];
      pe_jacobian<LD / 2>(gd, vd, p.fd, h, dv);
#pragma unroll
      for (int c = 0; c < 3; ++c) dv[c] = add_other_half(dv[c]);
      if (live && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.d_vd[pt * 3 + c] = dv[c];
      }
    }
  }
}

// ---- per-ray reduction: one wave per ray, lanes stride over the samples, then the butterfly of wave_sum -------------
//   d_ro = sum_s d_pts, d_rd = sum_s z_s d_pts, d_viewdir = sum_s d_viewdir_s, d_z_s = rd . d_pts_s; near / far (and any further
//   column of a row) get 0.  Points form (rays == NULL): only d_viewdirs (N,3).
__global__ __launch_bounds__(256) void input_grad_rays_kernel(const float* __restrict__ d_pts, const float* __restrict__ d_vd,
                                                              const float* __restrict__ rays, int ray_stride,
                                                              const float* __restrict__ z, long long n_rays, int S,
                                                              float* __restrict__ d_rays, float* __restrict__ d_z,
                                                              float* __restrict__ d_viewdirs) {
  const int lane = threadIdx.x & 63;
  const long long ray = static_cast<long long>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (ray >= n_rays) return;
  float rd[3] = {0.0f, 0.0f, 0.0f};
  if (rays) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rd[c] = rays[ray * ray_stride + 3 + c];
  }
  float a_ro[3] = {0.0f, 0.0f, 0.0f}, a_rd[3] = {0.0f, 0.0f, 0.0f}, a_vd[3] = {0.0f, 0.0f, 0.0f};
  for (int s = lane; s < S; s += 64) {
    const long long pt = ray * S + s;
    if (rays) {
      const float zz = z[pt];
      float dp[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { dp[c] = d_pts[pt * 3 + c]; a_ro[c] += dp[c]; a_rd[c] += zz * dp[c]; }
      d_z[pt] = rd[0] * dp[0] + rd[1] * dp[1] + rd[2] * dp[2];
    }
    if (d_vd) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a_vd[c] += d_vd[pt * 3 + c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { a_ro[c] = wave_sum(a_ro[c]); a_rd[c] = wave_sum(a_rd[c]); a_vd[c] = wave_sum(a_vd[c]); }
  if (rays) {
    // lane c writes column c of the row
    for (int c = lane; c < ray_stride; c += 64) {
      float v = 0.0f;
      if (c < 3) v = c == 0 ? a_ro[0] : c == 1 ? a_ro[1] : a_ro[2];
      else if (c < 6) v = c == 3 ? a_rd[0] : c == 4 ? a_rd[1] : a_rd[2];
      else if (d_vd && c >= 8 && c < 11) v = c == 8 ? a_vd[0] : c == 9 ? a_vd[1] : a_vd[2];
      d_rays[ray * ray_stride + c] = v;
    }
  } else if (lane < 3) {
    d_viewdirs[ray * 3 + lane] = lane == 0 ? a_vd[0] : lane == 1 ? a_vd[1] : a_vd[2];
  }
}

template <int BF16, int LX>
static int launch_input_grad(IgParams p, hipStream_t stream) {
  auto kern = mlp_input_grad_kernel<BF16, LX>;
  p.n_tiles32 = (p.n_points + 31) / 32;
  p.n_wg_tiles = (p.n_tiles32 + kIgWaves - 1) / kIgWaves;
  p.in_lds = p.stream_bytes <= kIgLdsBudget;
  const size_t lds = p.in_lds ? static_cast<size_t>(p.stream_bytes) : 0;
  if (lds > 64 * 1024) {
    if (int rc = ensure_big_lds(reinterpret_cast<const void*>(kern))) return rc;
  }
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(persistent_grid(p.n_wg_tiles))), dim3(kIgWaves * 64), lds, stream, p);
  return check_launch("mlp_input_grad");
}

// descriptor / precision checks shared by the entry points: the 32-point record layout (fp32, or bf16 with 16-bit saves)
static int validate_input_grad(const dn_mlp_desc* desc, int precision, const char* who) {
  if (!desc) { set_error("%s: NULL descriptor", who); return DN_E_INVAL; }
  if (precision == DN_PREC_F16 || precision == DN_PREC_BF16_S8) {
    set_error("%s: input gradients exist for DN_PREC_F32 and DN_PREC_BF16 with 16-bit saved tensors (fp16 is a render-only mode; "
              "the 8-bit-saved 48-point layout is not covered)", who);
    return DN_E_UNSUPPORTED;
  }
  if (int rc = validate_desc(desc, precision)) return rc;
  if (!train_lxyz_supported(*desc)) {
    set_error("%s: training kernels are built for L_xyz in {6, 10} (got %d)", who, desc->num_encoding_fn_xyz);
    return DN_E_UNSUPPORTED;
  }
  return 0;
}

static size_t input_grad_workspace(const dn_mlp_desc& d, int64_t n_points, int ray_form) {
  const size_t per = static_cast<size_t>(n_points) * 3 * sizeof(float);
  const size_t per_pad = (per + 255) / 256 * 256;
  return per_pad * ((ray_form ? 1 : 0) + (d.use_viewdirs ? 1 : 0));
}

// The first launch of dn_mlp_backward_input alone: the per-point d_pts (P,3) - and d_viewdir (P,3) with view directions - from the
// gradient records, the points given as pts (+ viewdirs) or formed from rays + z.  Arguments already judged by the caller.
static int point_input_grads(const dn_mlp_desc* desc, int precision, const void* packed_ig, const void* grads, const float* pts,
                             const float* viewdirs, const float* rays, int ray_stride, const float* z_vals, int64_t n_points,
                             int samples_per_ray, float* d_pts, float* d_vd, dn_stream_t stream) {
  IgLayout g;
  build_input_grad_layout(*desc, precision, &g);
  FwdParams fp;
  int rc;
  if ((rc = setup_params(desc, precision, packed_ig, &fp))) return rc;   // (for the frequency tables)
  const bool vdirs = desc->use_viewdirs != 0;
  IgParams p{};
  p.stream = static_cast<const char*>(packed_ig);
  p.stream_bytes = g.total_pieces * kPieceBytes;
  p.grads = static_cast<const char*>(grads);
  p.grad_pieces = g.grad_pieces;
  p.n_x = g.n_x; p.kh = g.kh;
  for (int s = 0; s < g.n_x; ++s) p.gslot[s] = g.gslot[s];
  p.gslot_dirout = g.gslot_dirout; p.dir_piece0 = g.dir_piece0; p.use_viewdirs = vdirs;
  p.mode = pts == nullptr ? 0 : 1;
  p.rays = rays; p.ray_stride = ray_stride; p.z = z_vals; p.pts = pts; p.viewdirs = viewdirs;
  p.n_points = n_points; p.S = samples_per_ray;
  p.d_pts = d_pts;
  p.d_vd = vdirs ? d_vd : nullptr;
  for (int i = 0; i < 16; ++i) p.fx[i] = fp.fx[i];
  for (int i = 0; i < 8; ++i) p.fd[i] = fp.fd[i];

  const bool bf = precision == DN_PREC_BF16;
  const int LX = desc->num_encoding_fn_xyz;
  if (bf && LX == 10) return launch_input_grad<1, 10>(p, as_stream(stream));
  if (bf) return launch_input_grad<1, 6>(p, as_stream(stream));
  if (LX == 10) return launch_input_grad<0, 10>(p, as_stream(stream));
  return launch_input_grad<0, 6>(p, as_stream(stream));
}

// api.cpp (dn_render_rays_normals): the descriptor / precision rule of the input gradient, and the per-point d_pts (P,3) of a
// no-view-direction network from rays + z into the caller's buffer - no per-ray reduction, no workspace
int input_grad_check(const dn_mlp_desc* desc, int precision, const char* who) { return validate_input_grad(desc, precision, who); }

int input_grad_points_from_rays(const dn_mlp_desc* desc, int precision, const void* packed_ig, const void* grads, const float* rays,
                                int ray_stride, const float* z_vals, int64_t n_rays, int samples_per_ray, float* d_pts, dn_stream_t stream) {
  int rc = validate_input_grad(desc, precision, "input_grad_points_from_rays");
  if (rc) return rc;
  DN_REQUIRE(!desc->use_viewdirs && packed_ig && grads && rays && z_vals && d_pts && n_rays >= 0 && samples_per_ray >= 1 && ray_stride >= 8,
             "input_grad_points_from_rays: bad arguments");
  DN_REQUIRE(((reinterpret_cast<uintptr_t>(packed_ig) | reinterpret_cast<uintptr_t>(grads)) & 15) == 0,
             "input_grad_points_from_rays: buffers must be 16-byte aligned");
  if (n_rays == 0) return 0;
  return point_input_grads(desc, precision, packed_ig, grads, nullptr, nullptr, rays, ray_stride, z_vals, n_rays * samples_per_ray,
                           samples_per_ray, d_pts, nullptr, stream);
}

}  // namespace dn

using namespace dn;

extern "C" size_t dn_mlp_input_grad_packed_bytes(const dn_mlp_desc* desc, int precision) {
  if (validate_input_grad(desc, precision, "dn_mlp_input_grad_packed_bytes")) return 0;
  IgLayout g;
  build_input_grad_layout(*desc, precision, &g);
  return static_cast<size_t>(g.total_pieces) * kPieceBytes;
}

extern "C" int dn_mlp_pack_input_grad(const dn_mlp_desc* desc, int precision, const float* const* h_weights, void* packed,
                                      dn_stream_t stream) {
  int rc = validate_input_grad(desc, precision, "dn_mlp_pack_input_grad");
  if (rc) return rc;
  DN_REQUIRE(h_weights && packed, "dn_mlp_pack_input_grad: NULL pointer");
  PackPtrs ptrs;
  if ((rc = collect_pack_ptrs("dn_mlp_pack_input_grad", *desc, h_weights, nullptr, &ptrs))) return rc;
  IgLayout g;
  build_input_grad_layout(*desc, precision, &g);
  if (precision == DN_PREC_BF16)
    hipLaunchKernelGGL(pack_input_grad_kernel<1>, dim3(256), dim3(256), 0, as_stream(stream), g, ptrs, static_cast<char*>(packed));
  else
    hipLaunchKernelGGL(pack_input_grad_kernel<0>, dim3(256), dim3(256), 0, as_stream(stream), g, ptrs, static_cast<char*>(packed));
  return check_launch("dn_mlp_pack_input_grad");
}

extern "C" size_t dn_mlp_backward_input_workspace_bytes(const dn_mlp_desc* desc, int64_t n_points, int ray_form) {
  if (!desc || n_points < 0) return 0;
  return input_grad_workspace(*desc, n_points, ray_form);
}

extern "C" int dn_mlp_backward_input(const dn_mlp_desc* desc, int precision, const void* packed_ig, const void* grads,
                                     const float* pts, const float* viewdirs, const float* rays, int ray_stride,
                                     const float* z_vals, int64_t n_rays, int samples_per_ray, float* d_pts, float* d_viewdirs,
                                     float* d_rays, float* d_z, void* workspace, size_t workspace_bytes, dn_stream_t stream) {
  int rc = validate_input_grad(desc, precision, "dn_mlp_backward_input");
  if (rc) return rc;
  DN_REQUIRE(packed_ig && grads && n_rays >= 0 && samples_per_ray >= 1, "dn_mlp_backward_input: bad arguments");
  DN_REQUIRE(((reinterpret_cast<uintptr_t>(packed_ig) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
             "dn_mlp_backward_input: buffers must be 16-byte aligned");
  const bool ray_form = pts == nullptr;
  const bool vdirs = desc->use_viewdirs != 0;
  if (ray_form) {
    DN_REQUIRE(rays && z_vals && d_rays && d_z, "dn_mlp_backward_input: need pts + d_pts, or rays + z_vals + d_rays + d_z");
    DN_REQUIRE(ray_stride >= (vdirs ? 11 : 8), "dn_mlp_backward_input: ray_stride too small");
  } else {
    DN_REQUIRE(d_pts, "dn_mlp_backward_input: d_pts is NULL");
    DN_REQUIRE(!vdirs || (viewdirs && d_viewdirs), "dn_mlp_backward_input: viewdirs and d_viewdirs required with use_viewdirs");
  }
  const int64_t n_points = n_rays * samples_per_ray;
  const size_t need = input_grad_workspace(*desc, n_points, ray_form ? 1 : 0);
  DN_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "dn_mlp_backward_input: workspace too small (%zu bytes needed)", need);
  if (n_points == 0) return 0;

  const size_t per_pad = (static_cast<size_t>(n_points) * 3 * sizeof(float) + 255) / 256 * 256;
  char* ws = static_cast<char*>(workspace);
  float* pt_grads = ray_form ? reinterpret_cast<float*>(ws) : d_pts;
  float* vd_grads = vdirs ? reinterpret_cast<float*>(ws + (ray_form ? per_pad : 0)) : nullptr;
  if ((rc = point_input_grads(desc, precision, packed_ig, grads, pts, viewdirs, rays, ray_stride, z_vals, n_points, samples_per_ray, pt_grads,
                              vd_grads, stream)))
    return rc;
  if (!ray_form && !vdirs) return 0;
  const unsigned blocks = static_cast<unsigned>((n_rays + 3) / 4);
  hipLaunchKernelGGL(input_grad_rays_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), pt_grads, vd_grads, ray_form ? rays : nullptr,
                     ray_stride, z_vals, static_cast<long long>(n_rays), samples_per_ray, d_rays, d_z, d_viewdirs);
  return check_launch("mlp_input_grad_rays");
}
