// Developer microbenchmark: the fused network kernel's weight pipeline (Pipe<8>: LDS-DMA ring, counted waits, one
// barrier per 16 pieces, A-fragment FIFO) driving two wave geometries on synthetic data, to price a geometry before
// the real kernel is rewritten for it:
//   mode 0: 8 waves x 32 points, v_mfma_f32_32x32x16_bf16, one MFMA per A piece    (the shipped bf16 geometry)
//   mode 1: 8 waves x 48 points, v_mfma_f32_16x16x32_bf16, three MFMAs per A piece (two activation sets = 192 VGPRs)
// Both run 10 "layers" of 256 -> 256 with ReLU + bf16 conversion between them, activations ping-ponging between two
// register sets exactly as in mlp_fused.hip; no encodings, no heads, no HBM output besides a checksum.
//   build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I dex-nerf_amd/csrc scripts/micro/mfma_geometry.hip -o mfma_geometry
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mlp_device.h"

using namespace dn;

constexpr int kLayers = 10;
constexpr int kLayerPieces = 128;  // 256 x 256 bf16 = 128 KiB
constexpr int kStreamPieces = kLayers * kLayerPieces;

template <int MODE>
__global__ __launch_bounds__(512, 2) void geo_kernel(const char* wstream, int passes, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  Pipe<8> pipe;
  pipe.ring = ring;
  pipe.ring_addr = static_cast<unsigned>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)ring));
  pipe.lane16 = lane * 16;
  pipe.wsrc = wstream;
  pipe.total_bytes = static_cast<unsigned>(kStreamPieces) * kPieceBytes;
  pipe.q_issue = 0;
  pipe.slot_wr = 0;
  pipe.wave = wave;
#pragma unroll
  for (int ph = 0; ph < kRingPhases - 1; ++ph) pipe.issue_phase();
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  pipe.slot_nxt = 0;
  pipe.rd_cur = ring + lane * 16;
  pipe.rd_nxt = ring + lane * 16;
#pragma unroll
  for (int e = 0; e < PipeGeo32::PREFETCH; ++e) pipe.af[e] = *reinterpret_cast<const f32x4*>(pipe.rd_nxt + e * kPieceBytes);

  float check = 0.0f;
  if constexpr (MODE == 0) {
    bf16x8 ba[1][16], bb[1][16];
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) ba[0][k][e] = static_cast<__bf16>(0.1f * ((lane * 7 + k * 3 + e) % 13) - 0.6f);
    auto no_pe = [&](int, int) { return bf16x8{}; };
    auto layer = [&](const bf16x8 (&bin)[1][16], bf16x8 (&bout)[1][16]) __attribute__((always_inline)) {
      run_stage<1, 1, 8, 16, 0, 0, false>(pipe, bin, no_pe, nullptr, [&](auto nt_c, auto, const f32x16& acc) {
        emit_pieces<1, true, decltype(nt_c)::value>(acc, bout[0]);
      });
    };
    for (int pass = 0; pass < passes; ++pass) {
      if (pass) {  // a fresh "tile": realistic magnitudes in every pass (MFMA power depends on the data)
#pragma unroll
        for (int k = 0; k < 16; ++k) check += static_cast<float>(ba[0][k][0]);
#pragma unroll
        for (int k = 0; k < 16; ++k)
#pragma unroll
          for (int e = 0; e < 8; ++e) ba[0][k][e] = static_cast<__bf16>(0.1f * ((lane * 7 + k * 3 + e + pass) % 13) - 0.6f);
      }
      for (int l = 0; l < kLayers; l += 2) {
        layer(ba, bb);
        layer(bb, ba);
      }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) check += static_cast<float>(ba[0][k][0]);
  } else {
    constexpr int PT = 3, NT = 16, KH = 8;
    bf16x8 ba[PT][KH], bb[PT][KH];
#pragma unroll
    for (int t = 0; t < PT; ++t)
#pragma unroll
      for (int k = 0; k < KH; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) ba[t][k][e] = static_cast<__bf16>(0.1f * ((lane * 7 + k * 3 + e + t) % 13) - 0.6f);
    auto layer = [&](const bf16x8 (&bin)[PT][KH], bf16x8 (&bout)[PT][KH]) __attribute__((always_inline)) {
      static_for<NT>([&](auto nt_c) {
        constexpr int nt = decltype(nt_c)::value;
        f32x4 acc[PT];
#pragma unroll
        for (int t = 0; t < PT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        static_for<KH>([&](auto k_c) {
          constexpr int k = decltype(k_c)::value;
          constexpr int pos = nt * KH + k;
          if constexpr (pos % kPhasePieces == 0) pipe.phase_begin();
          if constexpr (pos % kPhasePieces == kPhasePieces / 2) pipe.mid_phase();
          const bf16x8 a = __builtin_bit_cast(bf16x8, pipe.af[pos % PipeGeo32::PREFETCH]);
          static_for<PT>([&](auto t_c) {
            constexpr int t = decltype(t_c)::value;
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bin[t][k], acc[t], 0, 0, 0);
          });
          pipe.template prefetch<pos>();
          __builtin_amdgcn_sched_group_barrier(0x008, PT, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
        // two 16-row output tiles make one 32-deep B piece of the next layer: tile nt fills elements (nt & 1) * 4 .. + 3
        static_for<PT>([&](auto t_c) {
          constexpr int t = decltype(t_c)::value;
          typedef short s16x4 __attribute__((ext_vector_type(4)));
          typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
          bf16x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = static_cast<__bf16>(acc[t][e]);
          s16x4 bits = __builtin_bit_cast(s16x4, v);
          const s16x4 zero = {0, 0, 0, 0};
          bits = __builtin_elementwise_max(bits, zero);
          v = __builtin_bit_cast(bf16x4, bits);
#pragma unroll
          for (int e = 0; e < 4; ++e) bout[t][nt / 2][(nt & 1) * 4 + e] = v[e];
        });
      });
    };
    for (int pass = 0; pass < passes; ++pass) {
      if (pass) {
#pragma unroll
        for (int t = 0; t < PT; ++t)
#pragma unroll
          for (int k = 0; k < KH; ++k) {
            check += static_cast<float>(ba[t][k][0]);
#pragma unroll
            for (int e = 0; e < 8; ++e) ba[t][k][e] = static_cast<__bf16>(0.1f * ((lane * 7 + k * 3 + e + t + pass) % 13) - 0.6f);
          }
      }
      for (int l = 0; l < kLayers; l += 2) {
        layer(ba, bb);
        layer(bb, ba);
      }
    }
#pragma unroll
    for (int t = 0; t < PT; ++t)
#pragma unroll
      for (int k = 0; k < KH; ++k) check += static_cast<float>(ba[t][k][0]);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  out[blockIdx.x * 512 + threadIdx.x] = check;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int MODE>
static int run(const char* d_w, float* d_out, int passes, int grid) {
  auto kern = geo_kernel<MODE>;
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kRingBytes));
  hipEvent_t a, b;
  CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  const double flop_per_piece = (MODE == 0) ? 2.0 * 32 * 16 * 32 : 2.0 * 16 * 32 * 48;
  for (int rep = 0; rep < 4; ++rep) {
    CK(hipEventRecord(a, 0));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), kRingBytes, 0, d_w, passes, d_out);
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, a, b));
    const double flop = flop_per_piece * kStreamPieces * 8.0 * grid * passes;
    float hc[64];
    CK(hipMemcpy(hc, d_out, sizeof(hc), hipMemcpyDeviceToHost));
    printf("mode %d (%s)  passes=%d  %.2f ms  %.1f TFLOP/s  points/pass/WG=%d  check(lane 0, 5, 37)=%.4g %.4g %.4g\n", MODE,
           MODE == 0 ? "8 waves x 32 pts, 32x32x16" : "8 waves x 48 pts, 16x16x32", passes, ms, flop / ms / 1e9, MODE == 0 ? 256 : 384,
           hc[0] / passes, hc[5] / passes, hc[37] / passes);
    fflush(stdout);
  }
  return 0;
}

int main(int argc, char** argv) {
  const int passes = argc > 1 ? atoi(argv[1]) : 400;
  const int only = argc > 2 ? atoi(argv[2]) : -1;
  int dev = 0, cus = 256;
  CK(hipGetDevice(&dev));
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const size_t bytes = static_cast<size_t>(kStreamPieces) * kPieceBytes;
  std::vector<unsigned short> h(bytes / 2);
  unsigned s = 12345u;
  for (auto& v : h) {  // bf16 weights ~ uniform(-0.15, 0.15): keeps the ReLU chain O(1)
    s = s * 1664525u + 1013904223u;
    const float f = (static_cast<float>(s >> 8) / 16777216.0f - 0.5f) * 0.3f;
    unsigned u; memcpy(&u, &f, 4);
    v = static_cast<unsigned short>(u >> 16);
  }
  char* d_w; float* d_out;
  CK(hipMalloc(&d_w, bytes));
  CK(hipMemcpy(d_w, h.data(), bytes, hipMemcpyHostToDevice));
  CK(hipMalloc(&d_out, sizeof(float) * cus * 512));
  if (only != 1 && run<0>(d_w, d_out, passes, cus)) return 1;
  if (only != 0 && run<1>(d_w, d_out, passes, cus)) return 1;
  if (only < 0 && run<0>(d_w, d_out, passes, cus)) return 1;
  return 0;
}
