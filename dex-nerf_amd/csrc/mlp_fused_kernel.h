// Fused positional-encoding + FlexibleNeRFModel forward for gfx950 (reference run_network,
// nerf/train_utils.py:72-89; positional_encoding nerf/nerf_helpers.py:115-159; FlexibleNeRFModel.forward
// nerf/models.py:233-256).
//
// Design (see mlp_layout.h and DESIGN.md):
//   * persistent workgroups (one per CU); each wave64 owns 32 sample points and walks them through the
//     whole network with the activations resident in registers: the 32x32 accumulator tile of layer l
//     (rows = features, column = lane = point) is fed back as the B operand of layer l+1, so no
//     activation ever touches LDS or HBM;
//   * weights arrive as a linear stream of 1 KiB MFMA-A pieces, LDS-DMA'd (global_load_lds_dwordx4) from
//     L2 into a 5-slot x 16 KiB LDS ring shared by the waves of the workgroup; one counted
//     `s_waitcnt vmcnt(N)` + one raw `s_barrier` per 16 pieces; the next phase is always fully landed, two more are
//     in flight;
//   * positional encodings are computed in registers straight into B-fragment layout (the reference
//     materialises a (P,90) tensor and recomputes the direction encoding per sample);
//   * bf16 / fp16 modes: v_mfma_f32_32x32x16_{bf16,f16}, 8 waves x 32 points per workgroup, 2 waves / SIMD;
//     fp32 mode: v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains), 4 waves x 32 points, 1 wave / SIMD.
// MFMA-bound: 1,186,816 FLOP per point (D8/W256) against 16 B written per point.  SAVE = 1 is the bf16 / fp32 training forward:
// the same chain also streams every stage's output pieces (non-temporal, scalar-base stores) and ReLU mask words to HBM.  (The
// training forward with 8-bit saved tensors is a 48-point kernel: mlp_fused48*.hip.)
//
// This header holds the kernel template and, below it, the one list of its instances: the units mlp_fused_*.hip instantiate their
// rows of it, mlp_fused.hip (host side: packing, dispatch, entry points) declares all rows extern and dispatches over them.
#pragma once
#include "mlp_device.h"

namespace dn {

// SAVE = training forward: every stage's output pieces (and both encodings) are also written to `p.act` in the
// wave-native piece layout, plus one 128-bit ReLU mask word per lane per masked stage to `p.masks`.
template <int W, int LX, int LD, int BF16, int PT, int SAVE>   // SAVE: 0 inference, 1 training forward (bf16 / fp32 pieces)
__global__ __launch_bounds__((waves_of<BF16, PT>() * 64), ((BF16 && PT == 1) ? 2 : 1)) void mlp_forward_kernel(FwdParams p) {
  using P = Prec<BF16>;
  using BPiece = typename P::BPiece;
  constexpr int NT = W / 32;
  constexpr int KH = NT * P::PPT;                      // hidden pieces of a W-wide input
  constexpr int KXP = kXyzPanel / (2 * P::EPP);                 // PE xyz pieces (fixed 64-wide panel)
  static_assert(3 + 6 * LX <= kXyzPanel, "xyz encoding wider than its K panel");
  constexpr int KDP = round_up(3 + 6 * LD, 16) / (2 * P::EPP);  // PE dir pieces
  constexpr int WAVES = waves_of<BF16, PT>();
  constexpr int PTS_PER_WAVE = 32 * PT;
  constexpr int PTS_PER_WG = PTS_PER_WAVE * WAVES;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  char* bias_lds = smem + kRingBytes;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5;
  const int j = lane & 31;
  // per-wave input staging rows (PTS_PER_WAVE floats each): 0-2 origin / point, 3-5 direction, 6 depth, 7-9 view dir
  float* inbuf = reinterpret_cast<float*>(smem + kRingBytes + p.bias_bytes) + wave * (kInRows * PTS_PER_WAVE);
  // per-wave copy of the xyz-encoding B pieces (re-read at layer1 and at the skip layers instead of pinning
  // registers for the whole trunk)
  char* pex = smem + kRingBytes + p.bias_bytes + WAVES * kInRows * PTS_PER_WAVE * 4 +
              wave * (PT * (KXP + KDP) * kPieceBytes) + lane * 16;
  char* ped = pex + PT * KXP * kPieceBytes;  // the view-direction encoding pieces, used once near the end of the tile

  // Stage the inputs of a tile by LDS-DMA (4 B per lane, per-lane source address): no VGPR-destination load is
  // ever in flight next to the weight DMAs, so the compiler never drains the pipeline with vmcnt(0).
  // Lane l (< PTS_PER_WAVE) stages point l of this wave's PTS_PER_WAVE points.
  auto issue_inputs = [&](long long tile) {
    long long pt = tile * PTS_PER_WG + wave * PTS_PER_WAVE + lane;
    if (pt >= p.n_points) pt = p.n_points - 1;
    auto dma = [&](const float* src, int row) {
      if (lane < PTS_PER_WAVE)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(inbuf + row * PTS_PER_WAVE), 4, 0, 0);
    };
    if (p.mode == 0) {
      const float* r = p.rays + (pt / p.S) * p.ray_stride;
#pragma unroll
      for (int c = 0; c < 6; ++c) dma(r + c, c);
      dma(p.z + pt, 6);
      if (p.use_viewdirs) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dma(r + 8 + c, 7 + c);
      }
    } else if (p.mode == 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dma(p.pts + pt * 3 + c, c);
      if (p.use_viewdirs) {
        const float* v = p.viewdirs + (pt / p.S) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) dma(v + c, 7 + c);
      }
    }
  };

  // biases -> LDS once per workgroup (fp32, pre-permuted [tile][half][16])
  {
    const f32x4* g = reinterpret_cast<const f32x4*>(p.packed);
    f32x4* l = reinterpret_cast<f32x4*>(bias_lds);
    for (int i = threadIdx.x; i < p.bias_bytes / 16; i += WAVES * 64) l[i] = g[i];
  }
  issue_inputs(blockIdx.x);

  Pipe<WAVES> pipe;
  pipe.ring = ring;
  pipe.ring_addr = static_cast<unsigned>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)ring));
  pipe.lane16 = lane * 16;
  pipe.wsrc = p.packed + p.bias_bytes;
  pipe.total_bytes = static_cast<unsigned>(p.total_pieces) * kPieceBytes;
  pipe.q_issue = 0;
  pipe.slot_wr = 0;
  pipe.wave = wave;
#pragma unroll
  for (int ph = 0; ph < kRingPhases - 1; ++ph) pipe.issue_phase();
  // one-time full drain: biases, first inputs and the first five phases are resident
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  pipe.slot_nxt = 0;
  pipe.rd_cur = ring + lane * 16;
  pipe.rd_nxt = ring + lane * 16;  // phase_begin() of phase 0 turns this into rd_cur
#pragma unroll
  for (int e = 0; e < PipeGeo32::PREFETCH; ++e)
    pipe.af[e] = *reinterpret_cast<const f32x4*>(pipe.rd_nxt + e * kPieceBytes);

  const char* bias_half = bias_lds + h * 64;

  for (long long tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
    // ---- inputs: lanes j and j+32 share the points {t*32 + j} of this wave ----
    // Everything a lane derives from its inputs (both encodings) goes to LDS here, so no VGPR is carried across
    // the trunk: spilled carries would be reloaded with vmcnt(0) waits that drain the weight pipeline.
    if (p.mode != 2) {
      // staged by this wave's own DMAs one tile ago; VMEM ops retire in order, so every counted wait since then
      // (>= 70 phases, each leaving at most 6/12 younger ops outstanding) has covered them
      float in[PT][10];
#pragma unroll
      for (int t = 0; t < PT; ++t)
#pragma unroll
        for (int c = 0; c < 10; ++c) in[t][c] = inbuf[c * PTS_PER_WAVE + t * 32 + j];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const long long nxt = tile + gridDim.x;
      if (nxt < p.n_tiles) issue_inputs(nxt);
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        float x[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)  // plain mul then add (train_utils.py:136)
          x[c] = (p.mode == 0) ? in[t][c] + in[t][3 + c] * in[t][6] : in[t][c];
        BPiece bx[KXP];
        encode_pieces<BF16, LX, KXP>(x, p.fx, h, bx);
#pragma unroll
        for (int k = 0; k < KXP; ++k) *reinterpret_cast<BPiece*>(pex + (t * KXP + k) * kPieceBytes) = bx[k];
        if (p.use_viewdirs) {
          float vdir[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) vdir[c] = in[t][7 + c];
          BPiece bd[KDP];
          encode_pieces<BF16, LD, KDP>(vdir, p.fd, h, bd);
#pragma unroll
          for (int k = 0; k < KDP; ++k) *reinterpret_cast<BPiece*>(ped + (t * KDP + k) * kPieceBytes) = bd[k];
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        long long pt = tile * PTS_PER_WG + wave * PTS_PER_WAVE + j + t * 32;
        if (pt >= p.n_points) pt = p.n_points - 1;
        BPiece bx[KXP];
        gather_pieces<BF16, LX, KXP>(p.enc + pt * p.enc_ld, h, bx);
        BPiece bd[KDP];
        if (p.use_viewdirs) gather_pieces<BF16, LD, KDP>(p.enc + pt * p.enc_ld + (3 + 6 * LX), h, bd);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int k = 0; k < KXP; ++k) *reinterpret_cast<BPiece*>(pex + (t * KXP + k) * kPieceBytes) = bx[k];
        if (p.use_viewdirs) {
#pragma unroll
          for (int k = 0; k < KDP; ++k) *reinterpret_cast<BPiece*>(ped + (t * KDP + k) * kPieceBytes) = bd[k];
        }
      }
    }
    auto pe_xyz = [&](int t, int k) { return *reinterpret_cast<const BPiece*>(pex + (t * KXP + k) * kPieceBytes); };
    auto no_pe = [&](int, int) { return BPiece{}; };
    // training forward: where this wave's 32-point tile t keeps its saved pieces / mask words
    // this wave's saved-activation record(s) and mask words of the tile: wave-uniform bases, lane offset = lane * 16
    const char* act_tile[PT];
    const char* mask_tile_base[PT];
    if constexpr (SAVE) {
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        const long long tile32 = (tile * WAVES + wave) * PT + t;
        act_tile[t] = uniform_ptr(p.act + tile32 * p.act_pieces * kPieceBytes);
        mask_tile_base[t] = uniform_ptr(p.masks + tile32 * p.mask_words * kPieceBytes);
      }
    }
    auto save_piece = [&](int t, int slot, const BPiece& v) {
      store16_uniform(act_tile[t] + static_cast<long long>(slot) * kPieceBytes, pipe.lane16, v);
    };
    // (the piece arrays are passed by reference to their array type and indexed with compile-time constants only: a
    // decayed pointer sends the whole register-resident activation set to scratch memory in the fp32 instances)
    auto save_pieces = [&](auto nt_c, int t, int slot0, const auto& pieces) {
      if constexpr (SAVE) {
        constexpr int nt = decltype(nt_c)::value;
        static_for<P::PPT>([&](auto s_c) {
          constexpr int s2 = decltype(s_c)::value;
          save_piece(t, slot0 + nt * P::PPT + s2, pieces[nt * P::PPT + s2]);
        });
      }
    };
    unsigned maskw[PT][4];
    auto mask_clear = [&]() {
#pragma unroll
      for (int t = 0; t < PT; ++t) { maskw[t][0] = 0u; maskw[t][1] = 0u; maskw[t][2] = 0u; maskw[t][3] = 0u; }
    };
    // ReLU mask bits of output tile nt (layout: relu_mask_bit).  16-bit modes read them off the packed ReLU outputs
    // (non-zero <=> pre-activation > 0 in the arithmetic the kernel actually ran): one v_pk_min_u16 + one shift-or per
    // dword instead of compare + select + or per element with sixteen bit constants held in VGPRs.
    auto mask_tile = [&](auto nt_c, int t, const f32x16& acc, const auto& pieces) {
      if constexpr (SAVE) {
        constexpr int nt = decltype(nt_c)::value;
        if constexpr (BF16) {
          typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
          typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
          const u16x8 one = {1, 1, 1, 1, 1, 1, 1, 1};
          static_for<2>([&](auto s_c) {
            constexpr int s2 = decltype(s_c)::value;
            const u32x4 m = __builtin_bit_cast(u32x4, __builtin_elementwise_min(__builtin_bit_cast(u16x8, pieces[nt * 2 + s2]), one));
#pragma unroll
            for (int d = 0; d < 4; ++d) maskw[t][nt / 2] |= m[d] << (s2 * 4 + d + 8 * (nt & 1));
          });
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            maskw[t][relu_mask_bit(nt, r) / 32] |= (acc[r] > 0.0f) ? (1u << (relu_mask_bit(nt, r) % 32)) : 0u;
        }
      }
    };
    auto mask_store = [&](int word) {
      if constexpr (SAVE) {
#pragma unroll
        for (int t = 0; t < PT; ++t) {
          const uint4 v = make_uint4(maskw[t][0], maskw[t][1], maskw[t][2], maskw[t][3]);
          store16_uniform(mask_tile_base[t] + static_cast<long long>(word) * kPieceBytes, pipe.lane16, v);
        }
      }
    };
    if constexpr (SAVE) {
#pragma unroll
      for (int t = 0; t < PT; ++t) {
#pragma unroll
        for (int k = 0; k < KXP; ++k) save_piece(t, p.slot_xyz + k, pe_xyz(t, k));
        if (p.use_viewdirs) {
#pragma unroll
          for (int k = 0; k < KDP; ++k)
            save_piece(t, p.slot_dir + k, *reinterpret_cast<const BPiece*>(ped + (t * KDP + k) * kPieceBytes));
        }
      }
    }

    BPiece ba[PT][KH], bb[PT][KH];
    BPiece none[PT][1];
    int bias_tile = 0;
    // One trunk layer: layers_xyz[i] on (cat(x, xyz) when it is a skip layer) -> W, ReLU (models.py:239-246)
    // always_inline: left as a call (hipcc does that for the large fp32 instances) the register-resident activation sets
    // would have to live in scratch memory to be passed by reference
    auto trunk_layer = [&](int i, const BPiece (&bin)[PT][KH], BPiece (&bout)[PT][KH]) __attribute__((always_inline)) {
      auto emit = [&](auto nt_c, auto t_c, const f32x16& acc) {
        constexpr int t = decltype(t_c)::value;
        emit_pieces<BF16, true, decltype(nt_c)::value>(acc, bout[t]);
        save_pieces(nt_c, t, p.slot_trunk0 + i * KH, bout[t]);
        mask_tile(nt_c, t, acc, bout[t]);
      };
      mask_clear();
      if ((p.skip_mask >> i) & 1u)
        run_stage<BF16, PT, NT, KH, KXP, 0>(pipe, bin, pe_xyz, bias_half + bias_tile * 128, emit);
      else
        run_stage<BF16, PT, NT, KH, 0, 0>(pipe, bin, no_pe, bias_half + bias_tile * 128, emit);
      mask_store(i);
      bias_tile += NT;
    };
    // ---- layer1: xyz encoding -> W, no activation (models.py:238) ----
    run_stage<BF16, PT, NT, 0, KXP, 0>(pipe, none, pe_xyz, bias_half, [&](auto nt_c, auto t_c, const f32x16& acc) {
      constexpr int t = decltype(t_c)::value;
      emit_pieces<BF16, false, decltype(nt_c)::value>(acc, ba[t]);
      save_pieces(nt_c, t, p.slot_layer1, ba[t]);
    });
    bias_tile += NT;
    // ---- trunk, two layers per iteration so the activations ping-pong between two register sets ----
    int i = 0;
    for (; i + 1 < p.D - 1; i += 2) {
      trunk_layer(i, ba, bb);
      trunk_layer(i + 1, bb, ba);
    }
    if (i < p.D - 1) {
      trunk_layer(i, ba, bb);
#pragma unroll
      for (int t = 0; t < PT; ++t)
#pragma unroll
        for (int k = 0; k < KH; ++k) ba[t][k] = bb[t][k];
    }
    float out4[PT][4];
    if (p.use_viewdirs) {
      // ---- fc_alpha (extra tile, streamed first) + fc_feat with ReLU (models.py:248-249) ----
      constexpr int POS_A = 0;
      run_stage<BF16, PT, 1, KH, 0, POS_A>(pipe, ba, no_pe, bias_half + bias_tile * 128,
                                            [&](auto, auto t_c, const f32x16& acc) {
                                              out4[decltype(t_c)::value][3] = acc[0];  // row 0: lanes 0..31, reg 0
                                            });
      constexpr int POS_F = (POS_A + KH) % kPhasePieces;
      mask_clear();
      run_stage<BF16, PT, NT, KH, 0, POS_F>(pipe, ba, no_pe, bias_half + (bias_tile + 1) * 128,
                                             [&](auto nt_c, auto t_c, const f32x16& acc) {
                                               constexpr int t = decltype(t_c)::value;
                                               emit_pieces<BF16, true, decltype(nt_c)::value>(acc, bb[t]);
                                               save_pieces(nt_c, t, p.slot_feat, bb[t]);
                                               mask_tile(nt_c, t, acc, bb[t]);
                                             });
      mask_store(p.D - 1);
      bias_tile += NT + 1;
      // ---- layers_dir[0] on cat(feat, view) -> W/2, ReLU (models.py:250-252) ----
      constexpr int POS_D = (POS_F + NT * KH) % kPhasePieces;
      BPiece bg[PT][KH / 2];
      auto pe_dir = [&](int t, int k) { return *reinterpret_cast<const BPiece*>(ped + (t * KDP + k) * kPieceBytes); };
      mask_clear();
      run_stage<BF16, PT, NT / 2, KH, KDP, POS_D>(pipe, bb, pe_dir, bias_half + bias_tile * 128,
                                                   [&](auto nt_c, auto t_c, const f32x16& acc) {
                                                     constexpr int t = decltype(t_c)::value;
                                                     emit_pieces<BF16, true, decltype(nt_c)::value>(acc, bg[t]);
                                                     save_pieces(nt_c, t, p.slot_dirout, bg[t]);
                                                     mask_tile(nt_c, t, acc, bg[t]);
                                                   });
      mask_store(p.D);
      bias_tile += NT / 2;
      // ---- fc_rgb (models.py:253) ----
      constexpr int POS_R = (POS_D + (NT / 2) * (KH + KDP)) % kPhasePieces;
      run_stage<BF16, PT, 1, KH / 2, 0, POS_R>(pipe, bg, no_pe, bias_half + bias_tile * 128,
                                                [&](auto, auto t_c, const f32x16& acc) {
                                                  constexpr int t = decltype(t_c)::value;
                                                  out4[t][0] = acc[0]; out4[t][1] = acc[1]; out4[t][2] = acc[2];
                                                });
      static_assert((POS_R + KH / 2) % kPhasePieces == 0, "tail must end on a phase boundary");
    } else {
      // ---- fc_out (models.py:256); the stream is padded to a whole phase after it ----
      run_stage<BF16, PT, 1, KH, 0, 0>(pipe, ba, no_pe, bias_half + bias_tile * 128,
                                        [&](auto, auto t_c, const f32x16& acc) {
                                          constexpr int t = decltype(t_c)::value;
                                          out4[t][0] = acc[0]; out4[t][1] = acc[1]; out4[t][2] = acc[2]; out4[t][3] = acc[3];
                                        });
      if constexpr (KH % kPhasePieces != 0) pipe.template skip<KH % kPhasePieces, kPhasePieces - KH % kPhasePieces>();
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      const long long pt = tile * PTS_PER_WG + wave * PTS_PER_WAVE + j + t * 32;
      if (pt < p.n_points && h == 0) {
        f32x4 o;
        o[0] = out4[t][0]; o[1] = out4[t][1]; o[2] = out4[t][2]; o[3] = out4[t][3];
        __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(p.out + pt * 4));  // write-once stream: keep it out of the weight stream's L2
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

// ---- the instances: one row each, X(W, L_xyz, precision, SAVE) -------------------------------------------------------------
// precision is the kernel's BF16 argument: 0 fp32, 1 bf16, 2 fp16 (render-only: no SAVE rows).  Every instance has L_dir = 4, PT = 1.
// One sub-list per translation unit (mlp_fused_<unit>.hip), grouped by measured compile time so that the units build side by side
// (an fp32 W = 256 instance takes three to five times as long as any other: HISTORY.md section 11);
// DN_FWD32_INSTANCES is the whole family.
#define DN_FWD32_FP32_TRAIN_W256(X) X(256, 10, 0, 1) X(256, 6, 0, 1)
#define DN_FWD32_FP32_W256(X) X(256, 10, 0, 0) X(256, 6, 0, 0)
#define DN_FWD32_FP32_W128(X) X(128, 10, 0, 1) X(128, 6, 0, 1) X(128, 10, 0, 0) X(128, 6, 0, 0)
#define DN_FWD32_BF16_TRAIN(X) X(256, 10, 1, 1) X(128, 10, 1, 1) X(256, 6, 1, 1) X(128, 6, 1, 1)
#define DN_FWD32_BF16(X) \
  X(256, 10, 1, 0) X(128, 10, 1, 0) X(256, 6, 1, 0) X(128, 6, 1, 0) /* bf16 inference */ \
  X(256, 10, 2, 0) X(128, 10, 2, 0)                                 /* fp16 render: the L_xyz = 10 nets */
#define DN_FWD32_INSTANCES(X) \
  DN_FWD32_FP32_TRAIN_W256(X) DN_FWD32_FP32_W256(X) DN_FWD32_FP32_W128(X) DN_FWD32_BF16_TRAIN(X) DN_FWD32_BF16(X)

#define DN_FWD32_INSTANTIATE(W, LX, F, SAVE) template __global__ void mlp_forward_kernel<W, LX, 4, F, 1, SAVE>(FwdParams);
#define DN_FWD32_EXTERN(W, LX, F, SAVE) extern DN_FWD32_INSTANTIATE(W, LX, F, SAVE)

}  // namespace dn
