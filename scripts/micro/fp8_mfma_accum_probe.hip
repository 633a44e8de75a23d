// Probe (gfx950): how exactly does ONE v_mfma_f32_32x32x64_f8f6f4 (A = e5m2, B = e4m3, no scaling, C = 0 but in 2b - the form the 8-bit
// weight-gradient kernel issues, csrc/mlp_wgrad.hip consume_pair_s8) add its 64 products?  Every product of an e5m2 and an e4m3
// value is exact in fp32, so against float64 on the decoded operands only the instruction's internal summation shows.
//   1. small integers (every partial sum exact): checks the operand / result maps used here - must print 0;
//   2. one large product + one product 2^-k below it: where the small one stops counting; 2b. the same with the large value in C;
//   3. the figure: max |D - ref| / sum |a b| over random operands with widely spread magnitudes - every finite e5m2 byte and every
//      finite e4m3 byte equally likely (products over 48 binades) - and, for comparison, over operands with a narrow spread
//      (normal deviates, half of the e5m2 ones zero: what a ReLU network's gradients and activations look like).
// Lane l holds row (A) / column (B) l & 31, K block l >> 5: 32 K slots in 8 dwords, the same slot order in A and B - all a
// contraction needs.  D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
// Build: hipcc --offload-arch=gfx950 -O3 scripts/micro/fp8_mfma_accum_probe.hip -o exp_libs/fp8_mfma_accum_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(64) void probe(const int* __restrict__ a, const int* __restrict__ b, float c, float* __restrict__ d) {
  const long long at = static_cast<long long>(blockIdx.x) * 64 + threadIdx.x;
  i32x8 av, bv;
#pragma unroll
  for (int t = 0; t < 8; ++t) { av[t] = a[at * 8 + t]; bv[t] = b[at * 8 + t]; }
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = c;
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 1 /* A: e5m2 */, 0 /* B: e4m3 */, 0, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) d[at * 16 + r] = acc[r];
}

static double dec_e5m2(uint8_t v) {
  const int e = (v >> 2) & 31, m = v & 3;
  const double mag = e == 0 ? std::ldexp(m / 4.0, -14) : std::ldexp(1.0 + m / 4.0, e - 15);
  return (v & 0x80) ? -mag : mag;
}
static double dec_e4m3(uint8_t v) {
  const int e = (v >> 3) & 15, m = v & 7;
  const double mag = e == 0 ? std::ldexp(m / 8.0, -6) : std::ldexp(1.0 + m / 8.0, e - 7);
  return (v & 0x80) ? -mag : mag;
}
// nearest finite encoding (ties to even) by search: host only, tiny tables
template <class Dec> static uint8_t encode(double x, Dec dec, int top) {
  uint8_t best = 0;
  double err = INFINITY;
  for (int v = 0; v <= top; ++v) {
    const double e = std::fabs(dec(static_cast<uint8_t>(v)) - std::fabs(x));
    if (e < err || (e == err && (v & 1) == 0)) { err = e; best = static_cast<uint8_t>(v); }
  }
  return x < 0 ? best | 0x80 : best;
}

struct Result { double err_over_s, err_over_max; };

// A, B: [blocks][64 lanes][32 bytes]; returns the worst |D - ref| / S and |D - ref| / max |term| over all blocks and elements
static Result run(const std::vector<uint8_t>& A, const std::vector<uint8_t>& B, int blocks, std::vector<float>* keep = nullptr, float c = 0.0f) {
  int *d_a, *d_b;
  float* d_d;
  const size_t bytes = static_cast<size_t>(blocks) * 64 * 32;
  hipMalloc(&d_a, bytes); hipMalloc(&d_b, bytes); hipMalloc(&d_d, static_cast<size_t>(blocks) * 64 * 16 * 4);
  hipMemcpy(d_a, A.data(), bytes, hipMemcpyHostToDevice);
  hipMemcpy(d_b, B.data(), bytes, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(probe, dim3(blocks), dim3(64), 0, 0, d_a, d_b, c, d_d);
  std::vector<float> D(static_cast<size_t>(blocks) * 64 * 16);
  if (hipMemcpy(D.data(), d_d, D.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("HIP error\n"); std::exit(2); }
  hipFree(d_a); hipFree(d_b); hipFree(d_d);
  Result res{0.0, 0.0};
  for (int blk = 0; blk < blocks; ++blk)
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 16; ++r) {
        const int j = lane & 31, i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        double ref = c, s = std::fabs(c), big = std::fabs(c);
        for (int hh = 0; hh < 2; ++hh)
          for (int t = 0; t < 32; ++t) {
            const double p = dec_e5m2(A[(static_cast<size_t>(blk) * 64 + i + 32 * hh) * 32 + t]) *
                             dec_e4m3(B[(static_cast<size_t>(blk) * 64 + j + 32 * hh) * 32 + t]);
            ref += p; s += std::fabs(p); big = std::fmax(big, std::fabs(p));
          }
        const double err = std::fabs(static_cast<double>(D[(static_cast<size_t>(blk) * 64 + lane) * 16 + r]) - ref);
        if (s > 0.0) { res.err_over_s = std::fmax(res.err_over_s, err / s); res.err_over_max = std::fmax(res.err_over_max, err / big); }
        else if (err != 0.0) res.err_over_s = INFINITY;
      }
  if (keep) *keep = D;
  return res;
}

int main() {
  std::mt19937 gen(20260101u);
  // 1. small integers
  {
    const int blocks = 4;
    std::vector<uint8_t> A(blocks * 64 * 32), B(A.size());
    for (auto& v : A) v = encode(static_cast<double>(static_cast<int>(gen() % 7) - 3), dec_e5m2, 0x7B);
    for (auto& v : B) v = encode(static_cast<double>(static_cast<int>(gen() % 9) - 4), dec_e4m3, 0x7E);
    const Result r = run(A, B, blocks);
    printf("1. small integers: max |D - ref| / S = %.3e (must be 0: the operand and result maps)\n", r.err_over_s);
  }
  // 2. big + small: row i < 15: a_small = +1.75 * 2^-i, rows 16 .. 30: -1.75 * 2^-(i - 16); column j: b_small = 1.875 * 2^-(j % 7)
  {
    std::vector<uint8_t> A(64 * 32, 0), B(64 * 32, 0);
    for (int i = 0; i < 32; ++i) {
      const int k1 = i % 16;
      if (k1 > 14) continue;
      A[i * 32 + 0] = encode(1.75, dec_e5m2, 0x7B);
      A[i * 32 + 1] = encode((i < 16 ? 1.0 : -1.0) * std::ldexp(1.75, -k1), dec_e5m2, 0x7B);
    }
    for (int j = 0; j < 32; ++j) {
      B[j * 32 + 0] = encode(1.875, dec_e4m3, 0x7E);
      B[j * 32 + 1] = encode(std::ldexp(1.875, -(j % 7)), dec_e4m3, 0x7E);
    }
    std::vector<float> D;
    run(A, B, 1, &D);
    printf("2. 1.75 x 1.875 + (+-1.75 x 1.875) 2^-k: (D - big) / small, for the + and the - small product\n");
    for (int k = 0; k <= 20; ++k) {
      const int k1 = k < 14 ? k : 14, k2 = k - k1;
      double got[2];
      for (int sgn = 0; sgn < 2; ++sgn) {
        const int i = k1 + 16 * sgn, j = k2;
        int lane = -1, reg = -1;
        for (int l = 0; l < 64; ++l)
          for (int r = 0; r < 16; ++r)
            if ((l & 31) == j && (r & 3) + 8 * (r >> 2) + 4 * (l >> 5) == i) { lane = l; reg = r; }
        const double big = 1.75 * 1.875, small = (sgn ? -1.0 : 1.0) * std::ldexp(big, -k);
        got[sgn] = (static_cast<double>(D[lane * 16 + reg]) - big) / small;
      }
      printf("   k = %2d: %.6f  %.6f\n", k, got[0], got[1]);
    }
  }
  // 2b. the same with the large value in the accumulator: C = 1.75 * 1.875 in every element, ONE product 2^-k below it
  {
    std::vector<uint8_t> A(64 * 32, 0), B(64 * 32, 0);
    for (int i = 0; i < 32; ++i) {
      const int k1 = i % 16;
      if (k1 > 14) continue;
      A[i * 32 + 1] = encode((i < 16 ? 1.0 : -1.0) * std::ldexp(1.75, -k1), dec_e5m2, 0x7B);
    }
    for (int j = 0; j < 32; ++j) B[j * 32 + 1] = encode(std::ldexp(1.875, -(j % 7)), dec_e4m3, 0x7E);
    std::vector<float> D;
    const float c = 1.75f * 1.875f;
    run(A, B, 1, &D, c);
    printf("2b. C = 1.75 x 1.875, one product (+-1.75 x 1.875) 2^-k: (D - C) / product\n");
    for (int k = 0; k <= 20; ++k) {
      const int k1 = k < 14 ? k : 14, k2 = k - k1;
      double got[2];
      for (int sgn = 0; sgn < 2; ++sgn) {
        const int i = k1 + 16 * sgn, j = k2;
        int lane = -1, reg = -1;
        for (int l = 0; l < 64; ++l)
          for (int r = 0; r < 16; ++r)
            if ((l & 31) == j && (r & 3) + 8 * (r >> 2) + 4 * (l >> 5) == i) { lane = l; reg = r; }
        const double small = (sgn ? -1.0 : 1.0) * std::ldexp(static_cast<double>(c), -k);
        got[sgn] = (static_cast<double>(D[lane * 16 + reg]) - c) / small;
      }
      printf("   k = %2d: %.6f  %.6f\n", k, got[0], got[1]);
    }
  }
  // 3. random operands
  const int blocks = 1024;
  std::vector<uint8_t> A(static_cast<size_t>(blocks) * 64 * 32), B(A.size());
  {
    for (auto& v : A) { v = static_cast<uint8_t>(gen() % 0x7C); if (gen() & 1) v |= 0x80; }
    for (auto& v : B) { v = static_cast<uint8_t>(gen() % 0x7F); if (gen() & 1) v |= 0x80; }
    const Result r = run(A, B, blocks);
    printf("3. wide spread (every finite byte equally likely), %d MFMAs: max |D - ref| / S = %.3e, / max |term| = %.3e\n", blocks, r.err_over_s,
           r.err_over_max);
  }
  {
    std::normal_distribution<double> normal(0.0, 1.0);
    for (auto& v : A) v = (gen() & 1) ? encode(6.5 * normal(gen), dec_e5m2, 0x7B) : 0;
    for (auto& v : B) v = encode(std::fmax(normal(gen), 0.0), dec_e4m3, 0x7E);
    const Result r = run(A, B, blocks);
    printf("   narrow spread (normal deviates, ReLU-like zeros), %d MFMAs: max |D - ref| / S = %.3e, / max |term| = %.3e\n", blocks, r.err_over_s,
           r.err_over_max);
  }
  return 0;
}
