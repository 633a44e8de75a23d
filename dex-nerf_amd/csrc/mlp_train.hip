// Training kernels of the fused network path: the backward-data (dL/dX) chain and the native->plain unpack.
//
// The training forward is mlp_forward_kernel<..., SAVE=true> (mlp_fused_kernel.h): it keeps every stage's output
// pieces and a 128-bit ReLU mask word per lane per stage.  The backward chain below is the same register-resident
// MFMA chain run on the TRANSPOSED weight stream: for 32 points per wave,
//     dX^T[K x 32] = W^T[K x N] . dY^T[N x 32],   dY = dX_next (.) relu'(Y)
// so the gradient tile produced by one stage's MFMAs is (after masking) the B operand of the next stage, exactly
// like the activations in the forward.  Every masked gradient dL/d(pre-activation) is written out once in the
// wave-native piece layout; dW/db are formed from those and the saved activations by the weight-gradient kernels of
// mlp_wgrad.hip (bf16 MFMA, or exact-fp32 MFMA in the parity mode).
// In practice bound by the HBM write stream of the stored gradients (3.6 KiB/point at D8/W256), not by the MFMAs.
#include "mlp_internal.h"
#include "mlp_geo48.h"
#include <atomic>
#include <cmath>

namespace dn {

struct BwdParams {
  const char* packed;      // backward (transposed) piece stream, no bias region
  int total_pieces;
  int D;
  int use_viewdirs;
  const float* g_out;      // (P,4) dL/d[r,g,b,sigma] of the raw radiance field
  const char* masks;       // ReLU mask words from the training forward
  int mask_words;
  long long n_points;
  long long n_tiles;
  char* grads;             // [tile32][grad_pieces][64][16 B]
  int grad_pieces;
  int gslot_dirout, gslot_feat, gslot_trunk0, gslot_layer1, gslot_out;
  // Read by nobody.  The struct's size places the launch's hidden arguments (block counts) in the kernel-argument segment, so without
  // these four bytes one s_load offset of every mlp_backward_kernel instance changes; delete it with the next change that moves an
  // instruction of that kernel anyway.
  float unused_tail;
};

// dn_set_s8_grad_scale: gradient scale of the 8-bit saved tensors.  Process-wide, not per thread: PyTorch runs the backward of a
// step on its autograd thread, and the backward-data kernel (which multiplies) and the weight-gradient kernel (which divides)
// must see the value the caller set on its own thread.
static std::atomic<float> g_s8_grad_scale{0.0f};   // 0: per launch, from the largest upstream gradient (safe for any loss reduction / scaling)

constexpr int kBwdWaveLds = 6 * kPieceBytes;  // per wave: 2 output-gradient slots + 4 mask-word slots (1 KiB each)

template <int W, int BF16>
__global__ __launch_bounds__((waves_of<BF16, 1>() * 64), (BF16 ? 2 : 1)) void mlp_backward_kernel(BwdParams p) {
  using P = Prec<BF16>;
  using BPiece = typename P::BPiece;
  constexpr int PT = 1;
  constexpr int NT = W / 32;
  constexpr int KH = NT * P::PPT;
  constexpr int WAVES = waves_of<BF16, 1>();

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5;
  const int j = lane & 31;
  // per-wave staging: the output gradient rows of the NEXT tile and the ReLU mask words two stages ahead arrive by
  // LDS-DMA; no VGPR-destination global load exists in the tile loop (a wait on one would also wait for every older
  // store - HBM latency - and for the weight DMAs)
  char* wbuf = smem + kRingBytes + wave * kBwdWaveLds;
  const unsigned wbuf_addr = static_cast<unsigned>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)wbuf));
  const int n_masks = p.mask_words;          // stage q < n_masks applies mask word n_masks-1-q; stage n_masks: none

  auto issue_gout = [&](long long tile, int slot) {
    long long pt = (tile * WAVES + wave) * 32 + j;
    if (pt >= p.n_points) pt = p.n_points - 1;  // clamped lanes recompute a valid point; their stores hit padding tiles
    dma16_lanes(p.g_out + pt * 4, wbuf_addr + slot * kPieceBytes);
  };
  auto issue_mask = [&](long long tile, int q) {  // mask word of stage q of `tile` -> slot q & 3
    const char* src = p.masks + (((tile * WAVES + wave) * p.mask_words + (n_masks - 1 - q)) * 64 + lane) * 16;
    dma16_lanes(src, wbuf_addr + (2 + (q & 3)) * kPieceBytes);
  };

  Pipe<WAVES> pipe;
  pipe.ring = ring;
  pipe.ring_addr = static_cast<unsigned>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)ring));
  pipe.lane16 = lane * 16;
  pipe.wsrc = p.packed;
  pipe.total_bytes = static_cast<unsigned>(p.total_pieces) * kPieceBytes;
  pipe.q_issue = 0;
  pipe.slot_wr = 0;
  pipe.wave = wave;
  issue_gout(blockIdx.x, 0);
  issue_mask(blockIdx.x, 0);
  if (n_masks > 1) issue_mask(blockIdx.x, 1);
#pragma unroll
  for (int ph = 0; ph < kRingPhases - 1; ++ph) pipe.issue_phase();
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  pipe.slot_nxt = 0;
  pipe.rd_cur = ring + lane * 16;
  pipe.rd_nxt = ring + lane * 16;
#pragma unroll
  for (int e = 0; e < PipeGeo32::PREFETCH; ++e) pipe.af[e] = *reinterpret_cast<const f32x4*>(pipe.rd_nxt + e * kPieceBytes);

  int g_slot = 0;
  for (long long tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
    const long long tile32 = tile * WAVES + wave;
    const long long nxt = tile + gridDim.x;
    const f32x4 g = *reinterpret_cast<const f32x4*>(wbuf + g_slot * kPieceBytes + lane * 16);
    const char* grad_tile = uniform_ptr(p.grads + tile32 * p.grad_pieces * kPieceBytes);
    auto store_grad = [&](int slot, const BPiece& v) {
      store16_uniform(grad_tile + static_cast<long long>(slot) * kPieceBytes, pipe.lane16, v);
    };
    // Start of stage q: fetch this stage's mask word from its LDS slot, then stage what will be needed two stages on
    // (same tile, or the first two stages / the output gradient of the next tile) into the slot just read or one idle
    // for two stages.  The LDS read is complete (lgkmcnt(0)) before a DMA may overwrite the slot.
    auto stage_begin = [&](int q) {
      uint4 mw = make_uint4(~0u, ~0u, ~0u, ~0u);
      if (q < n_masks) mw = *reinterpret_cast<const uint4*>(wbuf + (2 + (q & 3)) * kPieceBytes + lane * 16);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const int r = q + 2;
      if (r < n_masks) issue_mask(tile, r);
      else if (r > n_masks && nxt < p.n_tiles) {   // r == n_masks + 1 / + 2: stages 0 / 1 of the next tile
        const int r2 = r - (n_masks + 1);
        if (r2 < n_masks) issue_mask(nxt, r2);
        if (r2 == 0) issue_gout(nxt, g_slot ^ 1);
      }
      return mw;
    };

    // masked gradient tile -> next stage's B pieces + one store per piece
    auto emit_grad = [&](auto nt_c, const f32x16& acc_in, const uint4& mw, BPiece* bout, int gslot) {
      constexpr int nt = decltype(nt_c)::value;
      if constexpr (BF16) {
        // convert first, then mask the PACKED pairs: dword j of the tile's two pieces holds registers 2j / 2j+1, whose
        // mask bits sit at (j + 8*(nt&1)) and 16 + that (relu_mask_bit): (bits & 0x00010001) * 0xFFFF = the AND mask
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const unsigned word = nt / 2 == 0 ? mw.x : nt / 2 == 1 ? mw.y : nt / 2 == 2 ? mw.z : mw.w;
        static_for<P::PPT>([&](auto s_c) {
          constexpr int s = decltype(s_c)::value;
          u32x4 bits = __builtin_bit_cast(u32x4, make_piece<BF16, false, s>(acc_in));
#pragma unroll
          for (int d = 0; d < 4; ++d) bits[d] &= ((word >> (s * 4 + d + 8 * (nt & 1))) & 0x00010001u) * 0xFFFFu;
          const BPiece piece = __builtin_bit_cast(BPiece, bits);
          bout[nt * P::PPT + s] = piece;
          store_grad(gslot + nt * P::PPT + s, piece);
        });
      } else {
        f32x16 acc = acc_in;
        const unsigned words[4] = {mw.x, mw.y, mw.z, mw.w};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool on = (words[relu_mask_bit(nt, r) / 32] >> (relu_mask_bit(nt, r) % 32)) & 1u;
          acc[r] = on ? acc[r] : 0.0f;
        }
        static_for<P::PPT>([&](auto s_c) {
          constexpr int s = decltype(s_c)::value;
          const BPiece piece = make_piece<BF16, false, s>(acc);
          bout[nt * P::PPT + s] = piece;
          store_grad(gslot + nt * P::PPT + s, piece);
        });
      }
    };

    BPiece ba[PT][KH], bb[PT][KH];
    BPiece none[PT][1];
    auto no_pe = [&](int, int) { return BPiece{}; };
    int q = 0;  // stage counter of this tile
    if (p.use_viewdirs) {
      // custom input pieces: element (half 0, e) carries k = e
      BPiece crgb{}, calpha{};
      if (h == 0) {
        if constexpr (BF16) {
          crgb[0] = static_cast<__bf16>(g[0]); crgb[1] = static_cast<__bf16>(g[1]); crgb[2] = static_cast<__bf16>(g[2]);
          calpha[0] = static_cast<__bf16>(g[3]);
        } else {
          crgb[0] = g[0]; crgb[1] = g[1]; crgb[2] = g[2];
          calpha[0] = g[3];
        }
      }
      store_grad(p.gslot_out, crgb);        // for dW(fc_rgb)
      store_grad(p.gslot_out + 1, calpha);  // for dW(fc_alpha)
      // ---- d g = fc_rgb^T d rgb, masked by relu'(layers_dir.0 out) ----
      uint4 mw = stage_begin(q++);
      auto c_rgb = [&](int, int) { return crgb; };
      run_stage<BF16, PT, NT / 2, 0, 1, 0, false>(pipe, none, c_rgb, nullptr, [&](auto nt_c, auto, const f32x16& acc) {
        emit_grad(nt_c, acc, mw, ba[0], p.gslot_dirout);
      });
      // ---- d feat = layers_dir.0[:, :W]^T d dirpre, masked by relu'(fc_feat out) ----
      constexpr int P1 = (NT / 2) % kPhasePieces;
      mw = stage_begin(q++);
      run_stage<BF16, PT, NT, KH / 2, 0, P1, false>(pipe, ba, no_pe, nullptr, [&](auto nt_c, auto, const f32x16& acc) {
        emit_grad(nt_c, acc, mw, bb[0], p.gslot_feat);
      });
      // ---- d h = fc_feat^T d featpre + fc_alpha^T d alpha, masked by relu'(layers_xyz[D-2] out) ----
      constexpr int P2 = (P1 + NT * (KH / 2)) % kPhasePieces;
      mw = stage_begin(q++);
      auto c_alpha = [&](int, int) { return calpha; };
      run_stage<BF16, PT, NT, KH, 1, P2, false>(pipe, bb, c_alpha, nullptr, [&](auto nt_c, auto, const f32x16& acc) {
        emit_grad(nt_c, acc, mw, ba[0], p.gslot_trunk0 + (p.D - 2) * KH);
      });
    } else {
      // ---- d h = fc_out^T d out, masked by relu'(layers_xyz[D-2] out) ----
      BPiece cout{};
      if (h == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if constexpr (BF16) cout[c] = static_cast<__bf16>(g[c]); else cout[c] = g[c];
        }
      }
      store_grad(p.gslot_out, cout);  // for dW(fc_out)
      const uint4 mw = stage_begin(q++);
      auto c_out = [&](int, int) { return cout; };
      run_stage<BF16, PT, NT, 0, 1, 0, false>(pipe, none, c_out, nullptr, [&](auto nt_c, auto, const f32x16& acc) {
        emit_grad(nt_c, acc, mw, ba[0], p.gslot_trunk0 + (p.D - 2) * KH);
      });
    }
    // ---- trunk, i = D-2 .. 0:  d x_i = layers_xyz[i][:, :W]^T d pre_i, masked by relu'(x_i) (x_0 = layer1 out: the
    //      last stage has no mask word - stage_begin hands back all ones).  The gradient sets ping-pong between `ba`
    //      and `bb`.  Positions: both head variants leave the same offset mod 16 per precision/W.
    constexpr int PV = ((NT / 2) + NT * (KH / 2) + NT * (KH + 1)) % kPhasePieces;  // viewdirs head
    constexpr int PN = NT % kPhasePieces;                                            // fc_out head
    auto trunk = [&](auto pos_c) {
      constexpr int POS = decltype(pos_c)::value;
      auto layer = [&](int i, const BPiece (&bin)[PT][KH], BPiece (&bout)[PT][KH]) __attribute__((always_inline)) {
        const uint4 mw = stage_begin(q++);
        const int gslot = i > 0 ? p.gslot_trunk0 + (i - 1) * KH : p.gslot_layer1;
        run_stage<BF16, PT, NT, KH, 0, POS, false>(pipe, bin, no_pe, nullptr, [&](auto nt_c, auto, const f32x16& acc) {
          emit_grad(nt_c, acc, mw, bout[0], gslot);
        });
      };
      int i = p.D - 2;
      for (; i >= 1; i -= 2) {
        layer(i, ba, bb);
        layer(i - 1, bb, ba);
      }
      if (i == 0) layer(0, ba, bb);
      if constexpr (POS % kPhasePieces != 0) pipe.template skip<POS, kPhasePieces - POS>();
    };
    static_assert((NT * KH) % kPhasePieces == 0, "trunk stages must preserve the phase offset");
    if (p.use_viewdirs) trunk(std::integral_constant<int, PV>{});
    else trunk(std::integral_constant<int, PN>{});
    g_slot ^= 1;
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

// ---- native piece layout -> plain (P, width) fp32 rows -------------------------------------------------------
// kind 0: hidden vector (feature = 32*(q/PPT) + acc_row(...)); kind 1/2: xyz / dir positional encoding.
template <int BF16>
__global__ void unpack_kernel(const char* __restrict__ native, int pieces_per_tile, int slot0, int n_pieces, int kind,
                              int L, long long n_points, float* __restrict__ out, int ld_out, int col0) {
  using P = Prec<BF16>;
  const long long total = ((n_points + 31) / 32) * n_pieces * 64 * P::EPP;
  for (long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int e = static_cast<int>(idx % P::EPP);
    const int lane = static_cast<int>((idx / P::EPP) % 64);
    const int q = static_cast<int>((idx / (P::EPP * 64)) % n_pieces);
    const long long tile32 = idx / (static_cast<long long>(P::EPP) * 64 * n_pieces);
    const int j = lane & 31, hh = lane >> 5;
    const long long pt = tile32 * 32 + j;
    if (pt >= n_points) continue;
    int col;
    if (kind == 0) col = (q / P::PPT) * 32 + acc_row((q % P::PPT) * P::EPP + e, hh);
    else col = pe_slot_col(L, hh, q * P::EPP + e);
    if (col < 0) continue;
    const char* src = native + ((tile32 * pieces_per_tile + slot0 + q) * 64 + lane) * 16;
    float v;
    if constexpr (BF16) v = static_cast<float>(reinterpret_cast<const __bf16*>(src)[e]);
    else v = reinterpret_cast<const float*>(src)[e];
    out[pt * ld_out + col0 + col] = v;
  }
}

template <int W, int BF16>
static int launch_backward(BwdParams p, hipStream_t stream) {
  auto kern = mlp_backward_kernel<W, BF16>;
  constexpr int WAVES = waves_of<BF16, 1>();
  p.n_tiles = (p.n_points + WAVES * 32 - 1) / (WAVES * 32);
  if (int rc = ensure_big_lds(reinterpret_cast<const void*>(kern))) return rc;
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(persistent_grid(p.n_tiles))), dim3(WAVES * 64), kRingBytes + WAVES * kBwdWaveLds, stream, p);
  return check_launch("mlp_backward");
}

static long long padded_tiles(long long n_points, int precision) {
  // both training kernels process whole workgroup tiles; buffers are sized for the padded tile count
  const int per_wg = 32 * (precision != DN_PREC_F32 ? 8 : 4);
  return (n_points + per_wg - 1) / per_wg * (per_wg / 32);
}

}  // namespace dn

using namespace dn;

extern "C" int dn_mlp_train_sizes(const dn_mlp_desc* desc, int precision, int64_t n_points, size_t* act_bytes,
                                  size_t* mask_bytes, size_t* grad_bytes) {
  const bool s8 = split_precision(&precision);
  int rc = validate_desc(desc, precision);
  if (rc) return rc;
  DN_REQUIRE(precision != DN_PREC_F16, "training kernels exist for fp32 and bf16 (fp16 is a render-only mode)");
  DN_REQUIRE(n_points >= 0 && act_bytes && mask_bytes && grad_bytes, "dn_mlp_train_sizes: bad arguments");
  if (!train_lxyz_supported(*desc)) {
    set_error("dn_mlp_train_sizes: training kernels are built for L_xyz in {6, 10} (got %d)", desc->num_encoding_fn_xyz);
    return DN_E_UNSUPPORTED;
  }
  if (s8) {   // s8-48 layout (mlp_geo48.h): units per 16-point group, two groups per 32-point record, whole 384-point tiles
    if (!g48_train_supported(*desc)) {
      set_error("dn_mlp_train_sizes: the 8-bit-saved-tensor training kernels run the 48-point geometry (W in {128, 256}, L_xyz in {6, 10}, a depth whose bias rows fit its LDS); train this network with DN_PREC_BF16");
      return DN_E_UNSUPPORTED;
    }
    TrainLayout48 t8;
    build_train_layout48(*desc, &t8);
    const size_t records = static_cast<size_t>(g48_padded_records(n_points));
    *act_bytes = records * 2 * t8.act_units * kPieceBytes;
    *mask_bytes = static_cast<size_t>(g48_mask_wave_tiles(n_points)) * t8.mask_stages * 2 * kPieceBytes;
    *grad_bytes = records * 2 * t8.grad_units * kPieceBytes + kS8BlockBytes;   // + the statistics / scale record (mlp_geo48.h)
    return 0;
  }
  TrainLayout t;
  build_train_layout(*desc, precision, &t);
  const size_t tiles = static_cast<size_t>(padded_tiles(n_points, precision));
  *act_bytes = tiles * t.act_pieces * kPieceBytes;
  *mask_bytes = tiles * t.mask_words * kPieceBytes;
  *grad_bytes = tiles * t.grad_pieces * kPieceBytes;
  return 0;
}

extern "C" size_t dn_mlp_backward_packed_bytes(const dn_mlp_desc* desc, int precision) {
  if (precision == DN_PREC_BF16_S8) {   // the 48-point chain's stream
    if (validate_desc(desc, DN_PREC_BF16) || !g48_train_supported(*desc)) return 0;
    NetLayout L48;
    build_backward_layout48(*desc, &L48);
    return static_cast<size_t>(L48.total_pieces) * kPieceBytes;
  }
  if (validate_desc(desc, precision)) return 0;
  NetLayout L;
  build_backward_layout(*desc, precision, &L);
  return static_cast<size_t>(L.total_pieces) * kPieceBytes;
}

extern "C" int dn_mlp_pack_backward(const dn_mlp_desc* desc, int precision, const float* const* h_weights, void* packed,
                                    dn_stream_t stream) {
  const bool s8 = split_precision(&precision);
  int rc = validate_desc(desc, precision);
  if (rc) return rc;
  DN_REQUIRE(h_weights && packed, "dn_mlp_pack_backward: NULL pointer");
  PackPtrs ptrs;
  if ((rc = collect_pack_ptrs("dn_mlp_pack_backward", *desc, h_weights, nullptr, &ptrs))) return rc;
  if (s8) {
    DN_REQUIRE(g48_train_supported(*desc), "dn_mlp_pack_backward: no 8-bit-saved-tensor training kernels for this network");
    return launch_pack48_backward(*desc, ptrs, static_cast<char*>(packed), as_stream(stream));
  }
  NetLayout L;
  build_backward_layout(*desc, precision, &L);
  return launch_pack(L, ptrs, packed, precision, as_stream(stream));
}

// Both streams a DN_PREC_BF16_S8 training step reads - the 48-point forward stream (inside `packed`, behind the core one) and the
// transposed backward stream - for TWO networks of one architecture (the coarse and the fine net), in two launches instead of four.
extern "C" int dn_mlp_pack_train_pair(const dn_mlp_desc* desc, const float* const* h_weights_a, const float* const* h_biases_a,
                                      void* packed_a, void* packed_bwd_a, const float* const* h_weights_b,
                                      const float* const* h_biases_b, void* packed_b, void* packed_bwd_b, dn_stream_t stream) {
  int rc = validate_desc(desc, DN_PREC_BF16);
  if (rc) return rc;
  DN_REQUIRE(g48_train_supported(*desc), "dn_mlp_pack_train_pair: no 8-bit-saved-tensor training kernels for this network");
  DN_REQUIRE(h_weights_a && h_biases_a && packed_a && packed_bwd_a && h_weights_b && h_biases_b && packed_b && packed_bwd_b,
             "dn_mlp_pack_train_pair: NULL pointer");
  PackPtrs a, b;
  if ((rc = collect_pack_ptrs("dn_mlp_pack_train_pair", *desc, h_weights_a, h_biases_a, &a))) return rc;
  if ((rc = collect_pack_ptrs("dn_mlp_pack_train_pair", *desc, h_weights_b, h_biases_b, &b))) return rc;
  NetLayout L;
  build_layout(*desc, DN_PREC_BF16, &L);   // the 48-point region starts behind the core stream
  const size_t core = core_stream_bytes(L.bias_bytes, L.total_pieces);
  if ((rc = launch_pack48(*desc, DN_PREC_BF16, a, static_cast<char*>(packed_a) + core, as_stream(stream), false, &b, static_cast<char*>(packed_b) + core))) return rc;
  return launch_pack48_backward(*desc, a, static_cast<char*>(packed_bwd_a), as_stream(stream), &b, static_cast<char*>(packed_bwd_b));
}

extern "C" int dn_run_network_train(const dn_mlp_desc* desc, int precision, const void* packed, const float* pts,
                                    const float* viewdirs, const float* rays, int ray_stride, const float* z_vals,
                                    int64_t n_rays, int samples_per_ray, float* out, void* act, void* masks,
                                    dn_stream_t stream) {
  const bool s8 = split_precision(&precision);
  FwdParams p;
  int rc = setup_params(desc, precision, packed, &p);
  if (rc) return rc;
  DN_REQUIRE(packed && out && act && masks && n_rays >= 0 && samples_per_ray >= 1, "dn_run_network_train: bad arguments");
  DN_REQUIRE(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(act) | reinterpret_cast<uintptr_t>(masks)) & 15) == 0,
             "dn_run_network_train: buffers must be 16-byte aligned");
  if ((rc = set_point_inputs("dn_run_network_train", *desc, pts, viewdirs, rays, ray_stride, z_vals, n_rays, samples_per_ray, &p))) return rc;
  p.out = out;
  p.act = static_cast<char*>(act);
  p.masks = static_cast<char*>(masks);
  if (s8) {   // the 48-point training forward: slots / strides in units of the s8-48 layout
    DN_REQUIRE(g48_train_supported(*desc), "dn_run_network_train: no 8-bit-saved-tensor training kernels for this network (see dn_mlp_train_sizes)");
    TrainLayout48 t8;
    build_train_layout48(*desc, &t8);
    p.act_pieces = t8.act_units; p.mask_words = t8.mask_stages;
    copy_act_slots(t8, &p);
    p.save8 = 1;
  } else {
    TrainLayout t;
    build_train_layout(*desc, precision, &t);
    p.act_pieces = t.act_pieces; p.mask_words = t.mask_words;
    copy_act_slots(t, &p);
  }
  if (p.n_points == 0) return 0;
  return dispatch_forward(*desc, precision, p, as_stream(stream));
}

extern "C" int dn_mlp_backward_data(const dn_mlp_desc* desc, int precision, const void* packed_bwd, const float* g_out,
                                    const void* masks, int64_t n_points, void* grads, dn_stream_t stream) {
  return dn::mlp_backward_data_partials(desc, precision, packed_bwd, g_out, masks, n_points, grads, nullptr, 0, stream);
}

bool dn::s8_scale_is_per_launch() { return g_s8_grad_scale.load() == 0.0f; }

int dn::mlp_backward_data_partials(const dn_mlp_desc* desc, int precision, const void* packed_bwd, const float* g_out, const void* masks,
                                   int64_t n_points, void* grads, const unsigned* partials, int n_partials, dn_stream_t stream) {
  const bool s8 = split_precision(&precision);
  int rc = validate_desc(desc, precision);
  if (rc) return rc;
  DN_REQUIRE(precision != DN_PREC_F16, "dn_mlp_backward_data: fp16 is a render-only mode");
  DN_REQUIRE(packed_bwd && g_out && masks && grads && n_points >= 0, "dn_mlp_backward_data: bad arguments");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(g_out) & 15) == 0, "dn_mlp_backward_data: g_out must be 16-byte aligned");
  if (n_points == 0) return 0;
  if (s8) {   // the 48-point chain (mlp_train48.hip)
    DN_REQUIRE(g48_train_supported(*desc), "dn_mlp_backward_data: no 8-bit-saved-tensor training kernels for this network (see dn_mlp_train_sizes)");
    DN_REQUIRE(n_points < (1LL << 31) - 1024, "dn_mlp_backward_data (8-bit saved tensors): at most 2^31 - 1024 points per call");
    return backward48_entry(desc, packed_bwd, g_out, masks, n_points, grads, g_s8_grad_scale.load(), as_stream(stream), partials, n_partials);
  }
  NetLayout L;
  build_backward_layout(*desc, precision, &L);
  TrainLayout t;
  build_train_layout(*desc, precision, &t);
  BwdParams p{};
  p.packed = static_cast<const char*>(packed_bwd);
  p.total_pieces = L.total_pieces;
  p.D = desc->num_layers;
  p.use_viewdirs = desc->use_viewdirs;
  p.g_out = g_out;
  p.masks = static_cast<const char*>(masks);
  p.mask_words = t.mask_words;
  p.n_points = n_points;
  p.grads = static_cast<char*>(grads);
  p.grad_pieces = t.grad_pieces;
  copy_grad_slots(t, &p);
  const bool bf = precision == DN_PREC_BF16;
  if (desc->hidden_size == 256) return bf ? launch_backward<256, true>(p, as_stream(stream)) : launch_backward<256, false>(p, as_stream(stream));
  if (desc->hidden_size == 128) return bf ? launch_backward<128, true>(p, as_stream(stream)) : launch_backward<128, false>(p, as_stream(stream));
  set_error("dn_mlp_backward_data: no kernel instance for W=%d", desc->hidden_size);
  return DN_E_UNSUPPORTED;
}

extern "C" int dn_mlp_unpack(const dn_mlp_desc* desc, int precision, int which, const void* native, int64_t n_points,
                             int slot, int width, int kind, float* out, int ld_out, int col0, dn_stream_t stream) {
  if (precision == DN_PREC_BF16_S8) {   // the 8-bit units of the 48-point training kernels (kind 3: the custom output-gradient unit)
    int rc8 = validate_desc(desc, DN_PREC_BF16);
    if (rc8) return rc8;
    DN_REQUIRE(native && out && n_points >= 0 && width > 0 && ld_out >= col0 + 1 && (which == 0 || which == 1) && kind >= 0 && kind <= 3 &&
               g48_train_supported(*desc), "dn_mlp_unpack (8-bit layout): bad arguments");
    if (n_points == 0) return 0;
    return unpack48_entry(desc, which, native, n_points, slot, width, kind, out, ld_out, col0, as_stream(stream));
  }
  int rc = validate_desc(desc, precision);
  if (rc) return rc;
  DN_REQUIRE(native && out && n_points >= 0 && width > 0 && ld_out >= col0 + 1 && (which == 0 || which == 1) && kind >= 0 && kind <= 2,
             "dn_mlp_unpack: bad arguments");
  if (n_points == 0) return 0;
  TrainLayout t;
  build_train_layout(*desc, precision, &t);
  const int per_tile = which == 0 ? t.act_pieces : t.grad_pieces;
  const int n_pieces = (kind == 0) ? width / t.kpp : (kind == 1 ? t.kxp : t.kdp);
  const int L = kind == 1 ? desc->num_encoding_fn_xyz : desc->num_encoding_fn_dir;
  DN_REQUIRE(slot >= 0 && slot + n_pieces <= per_tile, "dn_mlp_unpack: slot range outside the tile");
  if (precision == DN_PREC_BF16)
    hipLaunchKernelGGL(unpack_kernel<true>, dim3(2048), dim3(256), 0, as_stream(stream), static_cast<const char*>(native),
                       per_tile, slot, n_pieces, kind, L, n_points, out, ld_out, col0);
  else
    hipLaunchKernelGGL(unpack_kernel<false>, dim3(2048), dim3(256), 0, as_stream(stream), static_cast<const char*>(native),
                       per_tile, slot, n_pieces, kind, L, n_points, out, ld_out, col0);
  return check_launch("dn_mlp_unpack");
}

extern "C" int dn_set_s8_grad_scale(float scale) {
  int e = 0;
  DN_REQUIRE(scale == 0.0f || (scale > 0.0f && std::isfinite(scale) && std::frexp(scale, &e) == 0.5f),
             "dn_set_s8_grad_scale: the scale must be a power of two (the scaling and its inverse are then exact), or 0 = chosen per launch from the largest upstream gradient");
  g_s8_grad_scale.store(scale);
  return 0;
}
