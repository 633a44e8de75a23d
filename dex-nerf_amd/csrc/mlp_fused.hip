// Host side of the 32-point forward kernel (mlp_fused_kernel.h; its instances are compiled in mlp_fused_*.hip): the weight pack
// kernel, the dispatch over the instance list (and the hand-off to the 48-point family), and the extern "C" entry points.
#include "mlp_fused_kernel.h"
#include "mlp_internal.h"
#include "mlp_geo48.h"

namespace dn {

DN_FWD32_INSTANCES(DN_FWD32_EXTERN)

// ---- pack kernel: nn.Linear tensors -> bias tiles + MFMA-A piece stream ---------------------------------

// DENS = 1 (dn_mlp_pack_density): L is the layout of the no-view-direction net of the same trunk and the last stage's source is
// fc_alpha - its one row becomes row 3 of the 4-row head, rows 0-2 and their biases are +0
template <int BF16, int DENS = 0>
__global__ void pack_kernel(NetLayout L, PackPtrs ptrs, char* __restrict__ packed) {
  using P = Prec<BF16>;
  // bias tiles
  const int n_bias = L.total_bias_tiles * 32;
  float* bias_out = reinterpret_cast<float*>(packed);
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < L.bias_bytes / 4; idx += gridDim.x * blockDim.x) {
    float v = 0.0f;
    if (idx < n_bias) {
      const int tile = idx / 32, hh = (idx % 32) / 16, r = idx % 16, s = pack_stage_of_bias_tile(L, tile);
      int src;
      const int n = pack_src_row<32>(L.st[s], tile - L.st[s].bias0, acc_row(r, hh), DENS && s == L.n_stages - 1, &src);
      if (n >= 0) v = ptrs.b[src][n];
    }
    bias_out[idx] = v;
  }
  // weight pieces
  char* wout = packed + L.bias_bytes;
  const long long n_elems = static_cast<long long>(L.total_pieces) * 64 * P::EPP;
  for (long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; idx < n_elems;
       idx += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int e = static_cast<int>(idx % P::EPP);
    const int lane = static_cast<int>((idx / P::EPP) % 64);
    const int piece = static_cast<int>(idx / (P::EPP * 64));
    const int i = lane & 31, hh = lane >> 5;
    float v = 0.0f;
    const int s = pack_stage_of_piece(L, piece);
    const StageDesc& st = L.st[s];
    const int rel = piece - st.piece0;
    if (st.transposed) {
      // backward-data stage: A[row][k] = W[k][row0 + row]; k runs over the forward layer's outputs in accumulator
      // order (hidden pieces) and then over one optional "custom" piece (half hh, element e -> k = hh*EPP + e)
      if (rel < st.n_tiles * st.pieces_per_tile) {
        const int ts = rel / st.pieces_per_tile;
        const int k = rel % st.pieces_per_tile;
        const int kh = st.hidden_in / (2 * P::EPP);
        const int row = ts * 32 + i;
        if (row < st.n_real) {
          if (k < kh) {
            const int kout = (k / P::PPT) * 32 + acc_row((k % P::PPT) * P::EPP + e, hh);
            v = ptrs.w[st.src][static_cast<long long>(kout) * st.ld + st.col_hidden0 + row];
          } else {
            const int kc = hh * P::EPP + e;
            if (kc < st.custom_k) {
              const int srcw = st.src2 >= 0 ? st.src2 : st.src;
              v = ptrs.w[srcw][static_cast<long long>(kc) * st.ld + st.col_hidden0 + row];
            }
          }
        }
      }
    } else if (rel < st.n_tiles * st.pieces_per_tile) {
      const int ts = rel / st.pieces_per_tile;
      const int k = rel % st.pieces_per_tile;
      const int kh = st.hidden_in / (2 * P::EPP);  // hidden pieces
      int col;
      if (k < kh) {
        const int nt_in = k / P::PPT;
        const int r = (k % P::PPT) * P::EPP + e;
        col = st.col_hidden0 + nt_in * 32 + acc_row(r, hh);
      } else {
        const int u = (k - kh) * P::EPP + e;
        const int pc = pe_slot_col(st.pe_kind == 1 ? L.LX : L.LD, hh, u);
        col = (pc >= 0) ? st.col_pe0 + pc : -1;
      }
      int src;
      const int n = pack_src_row<32>(st, ts, i, DENS && s == L.n_stages - 1, &src);
      if (col >= 0 && n >= 0) v = ptrs.w[src][static_cast<long long>(n) * st.ld + col];
    }
    reinterpret_cast<typename P::Elem*>(wout)[idx] = static_cast<typename P::Elem>(v);
  }
}

template <int W, int LX, int LD, int BF16, int PT, int SAVE>
static int launch_forward(FwdParams p, hipStream_t stream) {
  auto kern = mlp_forward_kernel<W, LX, LD, BF16, PT, SAVE>;
  constexpr int WAVES = waves_of<BF16, PT>();
  constexpr int PTS_PER_WG = WAVES * 32 * PT;
  constexpr int KXP = kXyzPanel / (2 * Prec<BF16>::EPP);
  p.n_tiles = (p.n_points + PTS_PER_WG - 1) / PTS_PER_WG;
  constexpr int KDP = round_up(3 + 6 * LD, 16) / (2 * Prec<BF16>::EPP);
  const size_t lds = kRingBytes + p.bias_bytes + WAVES * (kInRows * 32 * PT * sizeof(float) + PT * (KXP + KDP) * kPieceBytes);
  if (int rc = ensure_big_lds(reinterpret_cast<const void*>(kern))) return rc;
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(persistent_grid(p.n_tiles))), dim3(WAVES * 64), lds, stream, p);
  return check_launch("mlp_forward");
}

int dispatch_forward(const dn_mlp_desc& d, int precision, FwdParams& p, hipStream_t stream, const CompParams* comp, int* composited,
                     unsigned* tile_counter) {
  const bool bf = precision == DN_PREC_BF16;
  const bool hf = precision == DN_PREC_F16;
  // bf16 geometry: PT=1 (8 waves x 32 points, two waves per SIMD) measured fastest (1327 vs 1277 TFLOP/s for
  // PT=2 = 4 waves x 64 points, one wave per SIMD)
  // bf16 / fp16 inference from rays / points: the 48-points-per-wave geometry (mlp_fused48.hip) when the net fits it;
  // DEXNERF_BF16_GEOM=32 keeps the 32-point kernels (same results up to bf16 accumulation order and the cosine's phase form)
  const char* region48 = p.packed + core_stream_bytes(p.bias_bytes, p.total_pieces);
  if ((bf || hf) && !read_switches().geom32 && p.act == nullptr && p.mode != 2 && p.n_points < (1LL << 31) - 1024 && g48_supported(d, precision))
    return launch_forward48(d, precision, p, region48, stream, comp, composited, tile_counter);
  if (p.act != nullptr && hf) { set_error("mlp_forward(train): fp16 is a render-only mode"); return DN_E_UNSUPPORTED; }
  if (p.act != nullptr && p.save8) {   // training forward with 8-bit saved units: a kernel of the 48-point geometry (mlp_fused48.hip)
    if (!bf || p.mode == 2 || !g48_train_supported(d) || p.n_points >= (1LL << 31) - 1024) {
      set_error("mlp_forward(train, 8-bit saved tensors): bf16 arithmetic, rays / points input, W in {128, 256}, L_xyz in {6, 10}, a depth the 48-point kernel holds in LDS");
      return DN_E_UNSUPPORTED;
    }
    return launch_forward48(d, precision, p, region48, stream);
  }
  // one instance per row of DN_FWD32_INSTANCES (mlp_fused_kernel.h): training forward (bf16 / fp32) of the L_xyz in {10, 6} nets
  // (L_xyz = 6: the forward-facing nets of the reference's LLFF configs; the saved xyz panel's slots past 3 + 6 L are zeros), fp16
  // render kernels of the L_xyz = 10 nets, bf16 / fp32 inference
  const int prec_arg = bf ? 1 : hf ? 2 : 0;
  const int save = p.act != nullptr ? 1 : 0;
#define DN_CASE(W_, LX_, F_, SAVE_)                                                            \
  if (d.hidden_size == W_ && d.num_encoding_fn_xyz == LX_ && prec_arg == F_ && save == SAVE_) \
    return launch_forward<W_, LX_, 4, F_, 1, SAVE_>(p, stream);
  DN_FWD32_INSTANCES(DN_CASE)
#undef DN_CASE
  if (save) {
    set_error("mlp_forward(train): no kernel instance for W=%d L_xyz=%d", d.hidden_size, d.num_encoding_fn_xyz);
    return DN_E_UNSUPPORTED;
  }
  if (hf) {
    set_error("mlp_forward(fp16): no kernel instance for W=%d L_xyz=%d", d.hidden_size, d.num_encoding_fn_xyz);
    return DN_E_UNSUPPORTED;
  }
  set_error("mlp_forward: no kernel instance for W=%d L_xyz=%d", d.hidden_size, d.num_encoding_fn_xyz);
  return DN_E_UNSUPPORTED;
}

int setup_params(const dn_mlp_desc* desc, int precision, const void* packed, FwdParams* p) {
  int rc = validate_desc(desc, precision);
  if (rc) return rc;
  NetLayout L;
  build_layout(*desc, precision, &L);
  *p = FwdParams{};
  p->packed = static_cast<const char*>(packed);
  p->bias_bytes = L.bias_bytes;
  p->total_pieces = L.total_pieces;
  p->D = desc->num_layers;
  p->skip_mask = L.skip_mask;
  p->use_viewdirs = desc->use_viewdirs;
  fill_freqs(p->fx, desc->num_encoding_fn_xyz, desc->log_sampling_xyz);
  if (desc->use_viewdirs) fill_freqs(p->fd, desc->num_encoding_fn_dir, desc->log_sampling_dir);
  return 0;
}

int launch_pack(const NetLayout& L, const PackPtrs& ptrs, void* packed, int precision, hipStream_t stream, bool density) {
  with_prec<true>(precision, [&](auto f) {
    constexpr int F = decltype(f)::value;
    auto kern = density ? pack_kernel<F, 1> : pack_kernel<F, 0>;
    hipLaunchKernelGGL(kern, dim3(512), dim3(256), 0, stream, L, ptrs, static_cast<char*>(packed));
  });
  return check_launch(density ? "mlp_pack_density" : "mlp_pack");
}

}  // namespace dn

using namespace dn;

extern "C" size_t dn_mlp_packed_bytes(const dn_mlp_desc* desc, int precision) {
  if (validate_desc(desc, precision)) return 0;
  NetLayout L;
  build_layout(*desc, precision, &L);
  return core_stream_bytes(L.bias_bytes, L.total_pieces) + (g48_supported(*desc, precision) ? g48_region_bytes(*desc) : 0);
}

extern "C" int dn_fp16_range_guard(const dn_mlp_desc* desc) {
  if (validate_desc(desc, DN_PREC_F16)) return 0;
  // 1 when an fp16 launch of this network reports EVERY hidden activation that leaves fp16's range (FwdParams::range_flag).
  // DEXNERF_BF16_GEOM in its wider reading: set to ANYTHING answers 0, although only 32 moves the dispatch (Switches)
  const Switches sw = read_switches();
  return (!sw.runtime_shape && !sw.geom_set && g48_supported(*desc, DN_PREC_F16) && g48_shape(*desc).range_guard_complete()) ? 1 : 0;
}

extern "C" int dn_mlp_pack(const dn_mlp_desc* desc, int precision, const float* const* h_weights,
                           const float* const* h_biases, void* packed, dn_stream_t stream) {
  return dn_mlp_pack_parts(desc, precision, h_weights, h_biases, packed, DN_PACK_ALL, stream);
}

extern "C" int dn_mlp_pack_parts(const dn_mlp_desc* desc, int precision, const float* const* h_weights,
                                 const float* const* h_biases, void* packed, int parts, dn_stream_t stream) {
  int rc = validate_desc(desc, precision);
  if (rc) return rc;
  DN_REQUIRE(h_weights && h_biases && packed, "dn_mlp_pack: NULL pointer");
  DN_REQUIRE(parts != 0 && (parts & ~DN_PACK_ALL) == 0, "dn_mlp_pack_parts: parts must be a non-empty mask of DN_PACK_CORE | DN_PACK_G48");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, "dn_mlp_pack: packed buffer must be 16-byte aligned");
  NetLayout L;
  build_layout(*desc, precision, &L);
  PackPtrs ptrs;
  if ((rc = collect_pack_ptrs("dn_mlp_pack", *desc, h_weights, h_biases, &ptrs))) return rc;
  if (parts & DN_PACK_CORE) rc = launch_pack(L, ptrs, packed, precision, as_stream(stream));
  if (rc == 0 && (parts & DN_PACK_G48) && g48_supported(*desc, precision))
    rc = launch_pack48(*desc, precision, ptrs, static_cast<char*>(packed) + core_stream_bytes(L.bias_bytes, L.total_pieces), as_stream(stream));
  return rc;
}

// ---- the density sub-network of a view-direction net: its trunk + fc_alpha as row 3 of a 4-row head (models.py:239-249) ----
extern "C" int dn_mlp_density_desc(const dn_mlp_desc* full, dn_mlp_desc* out) {
  DN_REQUIRE(full && out, "dn_mlp_density_desc: NULL descriptor");
  *out = *full;
  out->use_viewdirs = 0;
  return 0;
}

extern "C" size_t dn_mlp_density_packed_bytes(const dn_mlp_desc* full, int precision) {
  dn_mlp_desc d;
  if (dn_mlp_density_desc(full, &d) || validate_desc(full, precision)) return 0;
  return dn_mlp_packed_bytes(&d, precision);
}

extern "C" int dn_mlp_pack_density(const dn_mlp_desc* full, int precision, const float* const* h_weights,
                                   const float* const* h_biases, void* packed, dn_stream_t stream) {
  int rc = validate_desc(full, precision);
  if (rc) return rc;
  if (!full->use_viewdirs) return dn_mlp_pack(full, precision, h_weights, h_biases, packed, stream);   // already its own density net
  DN_REQUIRE(h_weights && h_biases && packed, "dn_mlp_pack_density: NULL pointer");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, "dn_mlp_pack_density: packed buffer must be 16-byte aligned");
  dn_mlp_desc d;
  dn_mlp_density_desc(full, &d);
  NetLayout L;
  build_layout(d, precision, &L);
  const int D = full->num_layers;
  PackPtrs ptrs;
  if ((rc = collect_pack_ptrs("dn_mlp_pack_density", *full, h_weights, h_biases, &ptrs, D))) return rc;   // layer1 + the trunk
  DN_REQUIRE(h_weights[D + 1] && h_biases[D + 1], "dn_mlp_pack_density: fc_alpha is NULL");
  ptrs.w[D] = h_weights[D + 1];   // the head stage's source: fc_alpha (pack_kernel, DENS)
  ptrs.b[D] = h_biases[D + 1];
  rc = launch_pack(L, ptrs, packed, precision, as_stream(stream), true);
  if (rc == 0 && g48_supported(d, precision))
    rc = launch_pack48(d, precision, ptrs, static_cast<char*>(packed) + core_stream_bytes(L.bias_bytes, L.total_pieces), as_stream(stream), true);
  return rc;
}

extern "C" int dn_run_network(const dn_mlp_desc* desc, int precision, const void* packed, const float* pts,
                              const float* viewdirs, const float* rays, int ray_stride, const float* z_vals,
                              int64_t n_rays, int samples_per_ray, float* out, dn_stream_t stream) {
  return dn::run_network_flagged(desc, precision, packed, pts, viewdirs, rays, ray_stride, z_vals, n_rays, samples_per_ray, out,
                                 nullptr, stream);
}

// dn_run_network + the fp16 range flag of the 48-point kernel (FwdParams::range_flag; ignored by every other kernel)
int dn::run_network_flagged(const dn_mlp_desc* desc, int precision, const void* packed, const float* pts,
                            const float* viewdirs, const float* rays, int ray_stride, const float* z_vals,
                            int64_t n_rays, int samples_per_ray, float* out, unsigned* range_flag, dn_stream_t stream,
                            const CompParams* comp, int* composited, unsigned* tile_counter) {
  if (composited) *composited = 0;
  FwdParams p;
  int rc = setup_params(desc, precision, packed, &p);
  if (rc) return rc;
  if (n_rays == 0) return 0;
  DN_REQUIRE(packed && out && n_rays >= 0 && samples_per_ray >= 1, "dn_run_network: bad arguments");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "dn_run_network: out must be 16-byte aligned");
  if ((rc = set_point_inputs("dn_run_network", *desc, pts, viewdirs, rays, ray_stride, z_vals, n_rays, samples_per_ray, &p))) return rc;
  p.out = out;
  p.range_flag = range_flag;
  if (p.n_points == 0) return 0;
  return dispatch_forward(*desc, precision, p, as_stream(stream), comp, composited, tile_counter);
}

extern "C" int dn_mlp_forward_encoded(const dn_mlp_desc* desc, int precision, const void* packed, const float* x,
                                      int64_t n_rows, float* out, dn_stream_t stream) {
  FwdParams p;
  int rc = setup_params(desc, precision, packed, &p);
  if (rc) return rc;
  if (n_rows == 0) return 0;
  DN_REQUIRE(packed && x && out && n_rows >= 0, "dn_mlp_forward_encoded: bad arguments");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "dn_mlp_forward_encoded: out must be 16-byte aligned");
  p.mode = 2; p.enc = x;
  p.enc_ld = (3 + 6 * desc->num_encoding_fn_xyz) + (desc->use_viewdirs ? 3 + 6 * desc->num_encoding_fn_dir : 0);
  p.n_points = n_rows; p.S = 1; p.out = out;
  if (n_rows == 0) return 0;
  return dispatch_forward(*desc, precision, p, as_stream(stream));
}
