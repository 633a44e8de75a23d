// bf16 / fp16 inference forward in the 48-points-per-wave geometry (see mlp_geo48.h): fused positional encoding +
// FlexibleNeRFModel forward (reference run_network, nerf/train_utils.py:72-89; positional_encoding
// nerf/nerf_helpers.py:115-159; FlexibleNeRFModel.forward nerf/models.py:233-256), same design as mlp_fused.hip -
// persistent workgroups, register-resident activation chain, LDS-DMA weight ring (Pipe<8>) - on
// v_mfma_f32_16x16x32_bf16: lane l of a wave holds point (l & 15) of each of its three 16-point groups and lane group
// g = l >> 4 holds rows 4g..4g+3 of every 16-row accumulator tile, which is k-block g of the next layer's B operand.
// Every A fragment read from LDS feeds three MFMAs: 384 points per pass of the weight stream instead of 256.
// A-fragment FIFO of 2 pieces here (4 in the 32-point kernels): a piece lasts three MFMAs = 48 cycles, and the 256-VGPR
// budget of two waves per SIMD is spent on the two 96-register activation sets
#include "mlp_fused48_kernel.h"

namespace dn {

// host code and the pack kernels only: every row of the instance list (mlp_fused48_kernel.h) is compiled in a unit of its own kind
// (mlp_fused48_*.hip) and declared here
DN_FWD48_INSTANCES(DN_FWD48_EXTERN)
// mlp_fused48_density.hip: the same template under another name (declared here, defined there)
template <int W, int F, int DC, unsigned MASKC, int VIEWC, int SAVE, int OVLP, int COMP>
__global__ __launch_bounds__(kG48Waves * 64, 2) void mlp_forward_density48_kernel(FwdParams p, G48Params q);
#define DN_FWD48_DENSITY_EXTERN(W, F, DC, MASKC, VIEWC, SAVE, OVLP, COMP) \
  extern template __global__ void mlp_forward_density48_kernel<W, F, DC, MASKC, VIEWC, SAVE, OVLP, COMP>(FwdParams, G48Params);
DN_FWD48_DENSITY(DN_FWD48_DENSITY_EXTERN)

// ---- pack: nn.Linear tensors -> bias rows + encoding tables + 16x32 A pieces -----------------------------------
// DENS = 1 (dn_mlp_pack_density): the no-view-direction layout with fc_alpha as the last stage's source - row 3 of the head
template <int F, int DENS = 0>
__device__ __forceinline__ void pack48_body(const NetLayout& L, const PackPtrs& ptrs, const G48Tables& tabs, char* __restrict__ region);

template <int F, int DENS = 0>
__global__ void pack48_kernel(NetLayout L, PackPtrs ptrs, G48Tables tabs, char* __restrict__ region) {
  pack48_body<F, DENS>(L, ptrs, tabs, region);
}

// two networks of one architecture (the coarse and the fine net of a training step) in one launch: blockIdx.y picks the net
template <int F>
__global__ void pack48_pair_kernel(NetLayout L, PackPtrs ptrs_a, PackPtrs ptrs_b, G48Tables tabs, char* __restrict__ region_a,
                                   char* __restrict__ region_b) {
  if (blockIdx.y == 0) pack48_body<F>(L, ptrs_a, tabs, region_a);
  else pack48_body<F>(L, ptrs_b, tabs, region_b);
}

template <int F, int DENS>
__device__ __forceinline__ void pack48_body(const NetLayout& L, const PackPtrs& ptrs, const G48Tables& tabs, char* __restrict__ region) {
  using Elem = typename Prec<F>::Elem;
  const int n_rows = L.total_bias_tiles * 16;
  float* bias_out = reinterpret_cast<float*>(region);
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < L.bias_bytes / 4; idx += gridDim.x * blockDim.x) {
    float v = 0.0f;
    if (idx < n_rows) {
      const int tile = idx / 16, s = pack_stage_of_bias_tile(L, tile);
      int src;
      const int n = pack_src_row<16>(L.st[s], tile - L.st[s].bias0, idx % 16, DENS && s == L.n_stages - 1, &src);
      if (n >= 0) v = ptrs.b[src][n];
    }
    bias_out[idx] = v;
  }
  // encoding tables: [4][16] xyz entries of 16 B, then (at byte 1024) [4][8] dir entries: (frequency, phase, identity, sine)
  f32x4* tab = reinterpret_cast<f32x4*>(region + L.bias_bytes);
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < kG48TableBytes / 16; idx += gridDim.x * blockDim.x) {
    const int kind_pe = idx < 64 ? 1 : 2;
    const int gg = idx < 64 ? idx / 16 : (idx - 64) / 8, u = idx < 64 ? idx % 16 : (idx - 64) % 8;
    const int c = g48_pe_col(kind_pe, gg, u, kind_pe == 1 ? L.LX : L.LD);
    f32x4 entry = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c >= 0 && c < 3) entry[2] = 1.0f;
    else if (c >= 3) {
      const int qq = c - 3, f = qq / 6, r = qq % 6;
      entry[0] = (kind_pe == 1 ? tabs.fx[f] : tabs.fd[f]) * 0.15915494309189535f;   // revolutions per unit (pe_value)
      entry[1] = r < 3 ? 0.0f : 0.25f;
      entry[3] = 1.0f;
    }
    tab[idx] = entry;
  }
  // pieces
  Elem* wout = reinterpret_cast<Elem*>(region + L.bias_bytes + kG48TableBytes);
  const long long n_elems = static_cast<long long>(L.total_pieces) * 64 * 8;
  for (long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; idx < n_elems;
       idx += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int e = static_cast<int>(idx % 8);
    const int lane = static_cast<int>((idx / 8) % 64);
    const int piece = static_cast<int>(idx / 512);
    const int i = lane & 15, gg = lane >> 4;
    float v = 0.0f;
    const int s = pack_stage_of_piece(L, piece);
    const StageDesc& st = L.st[s];
    const int rel = piece - st.piece0;
    if (rel < st.n_tiles * st.pieces_per_tile) {
      const int ts = rel / st.pieces_per_tile;
      const int k = rel % st.pieces_per_tile;
      const int kh = st.hidden_in / 32;
      int col;
      if (k < kh) {
        col = st.col_hidden0 + g48_hidden_col(k, gg, e);
      } else {
        const int pc = g48_pe_col(st.pe_kind, gg, (k - kh) * 8 + e, st.pe_kind == 1 ? L.LX : L.LD);
        col = pc >= 0 ? st.col_pe0 + pc : -1;
      }
      int src;
      const int n = pack_src_row<16>(st, ts, i, DENS && s == L.n_stages - 1, &src);
      if (col >= 0 && n >= 0) v = ptrs.w[src][static_cast<long long>(n) * st.ld + col];
    }
    wout[idx] = static_cast<Elem>(v);
  }
}

static G48Tables g48_tables(const dn_mlp_desc& d) {
  G48Tables tabs{};
  fill_freqs(tabs.fx, d.num_encoding_fn_xyz, d.log_sampling_xyz);
  if (d.use_viewdirs) fill_freqs(tabs.fd, d.num_encoding_fn_dir, d.log_sampling_dir);
  tabs.LX = d.num_encoding_fn_xyz; tabs.LD = d.num_encoding_fn_dir;
  return tabs;
}

int launch_pack48(const dn_mlp_desc& d, int precision, const PackPtrs& a, char* region_a, hipStream_t stream, bool density,
                  const PackPtrs* b, char* region_b) {
  NetLayout L;
  build_layout48(d, &L);
  const G48Tables tabs = g48_tables(d);
  const dim3 blocks(pack48_blocks(L), b ? 2 : 1);
  if (b) {
    static_assert(sizeof(NetLayout) + 2 * sizeof(PackPtrs) + sizeof(G48Tables) + 16 <= 4096, "kernel arguments of the pair pack");
    hipLaunchKernelGGL(pack48_pair_kernel<1>, blocks, dim3(256), 0, stream, L, a, *b, tabs, region_a, region_b);
    return check_launch("mlp_pack48_pair");
  }
  with_prec<false>(precision, [&](auto f) {
    constexpr int F = decltype(f)::value;
    auto kern = density ? pack48_kernel<F, 1> : pack48_kernel<F, 0>;
    hipLaunchKernelGGL(kern, blocks, dim3(256), 0, stream, L, a, tabs, region_a);
  });
  return check_launch(density ? "mlp_pack48_density" : "mlp_pack48");
}

#ifdef DN_TILE_STAMP
// Diagnostic build only (scripts/tile_stamps.py): the per-workgroup stamp records of the last kTileStampLaunches forward launches, in a
// device buffer of their own that no kernel reads; dn_tile_stamp_read copies them out.  Not part of the library's interface.
static unsigned long long* g_tile_stamps = nullptr;
static long long g_tile_stamp_launches = 0;
constexpr size_t kTileStampLaunchWords = static_cast<size_t>(kTileStampMaxWgs) * kTileStampWords;
static unsigned long long* tile_stamp_slot(long long grid) {
  if (grid > kTileStampMaxWgs) return nullptr;
  if (g_tile_stamps == nullptr) {
    const size_t bytes = kTileStampLaunches * kTileStampLaunchWords * sizeof(unsigned long long);
    if (hipMalloc(reinterpret_cast<void**>(&g_tile_stamps), bytes) != hipSuccess) { g_tile_stamps = nullptr; return nullptr; }
    if (hipMemset(g_tile_stamps, 0, bytes) != hipSuccess) return nullptr;
  }
  return g_tile_stamps + static_cast<size_t>(g_tile_stamp_launches++ % kTileStampLaunches) * kTileStampLaunchWords;
}
}  // namespace dn
// dst: kTileStampLaunches * kTileStampMaxWgs * kTileStampWords 64-bit words; launch i (counted from 0) is in slot i % kTileStampLaunches.
// Returns the number of launches stamped so far, or -1.
extern "C" __attribute__((visibility("default"))) long long dn_tile_stamp_read(unsigned long long* dst) {
  using namespace dn;
  if (g_tile_stamps == nullptr || hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(dst, g_tile_stamps, kTileStampLaunches * kTileStampLaunchWords * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return g_tile_stamp_launches;
}
namespace dn {
#endif

// In-kernel compositing is OFF unless DEXNERF_FUSED_COMPOSITE=1 (Switches::fused_composite).  It is bit-identical to the two-kernel path and
// takes the raw radiance field out of HBM (fine launch of the headline configuration: see HISTORY.md section 4.7f for the PMC bytes),
// but it costs time: a ray is composited by ONE wave with its SIMD to itself - exponentials, divisions and an fp64 scan as one
// dependency chain - where the standalone kernel hides that latency behind eight waves per SIMD; measured +3 % on a D8/W256
// render and +26 % on the as-shipped 4 x 128 nets.  The network kernels are not byte-bound, so the bytes saved buy nothing back.
int launch_forward48(const dn_mlp_desc& d, int precision, const FwdParams& p_in, const char* region, hipStream_t stream,
                     const CompParams* comp, int* composited, unsigned* tile_counter) {
  if (composited) *composited = 0;
  NetLayout L;
  build_layout48(d, &L);
  FwdParams p = p_in;
  G48Params q{};
  q.base = region; q.bias_bytes = L.bias_bytes; q.total_pieces = L.total_pieces;
  size_t lds = g48_lds_bytes(L);
  if (lds > 160 * 1024) { set_error("mlp_forward48: %zu bytes of LDS", lds); return DN_E_UNSUPPORTED; }
  const int cus = device_cus();
  const G48Pick pick = g48_pick(d, precision, p, comp, cus, read_switches());
  if (pick.refusal) { set_error("%s", pick.refusal); return DN_E_UNSUPPORTED; }
  const G48Key& k = pick.key;
  const int tile_points = k.SAVE == 3 ? 256 : kG48PointsPerWg;   // two point groups per wave: 256-point tiles
  p.n_tiles = (p.n_points + tile_points - 1) / tile_points;
  if (k.OVLP == 1) lds += static_cast<size_t>(kG48Waves) * 3 * kG48PointsPerWave * sizeof(float);   // a third set of view-direction rows
  if (g48_claims(k) && lds + kG48ClaimBytes <= 160 * 1024) {   // (the claim words: always there for these instances, read or not)
    lds += kG48ClaimBytes;
    q.tile_counter = tile_counter;
  }
  if (k.COMP) {
    q.comp = *comp;
    if (composited) *composited = 1;
  }
  auto launch = [&](auto kern) -> int {
    if (int rc = ensure_big_lds(reinterpret_cast<const void*>(kern))) return rc;
#ifdef DN_TILE_STAMP
    q.stamp = tile_stamp_slot(persistent_grid(p.n_tiles, cus));
#endif
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(persistent_grid(p.n_tiles, cus))), dim3(kG48Waves * 64), lds, stream, p, q);
    return check_launch("mlp_forward48");
  };
#define DN_CASE(KERNEL, W, F, DC, MASKC, VIEWC, SAVE, OVLP, COMP) \
  if (k == G48Key{W, F, DC, MASKC, VIEWC, SAVE, OVLP, COMP}) return launch(KERNEL<W, F, DC, MASKC, VIEWC, SAVE, OVLP, COMP>);
#define DN_CASE_FWD(...) DN_CASE(mlp_forward48_kernel, __VA_ARGS__)
#define DN_CASE_DENSITY(...) DN_CASE(mlp_forward_density48_kernel, __VA_ARGS__)
  if (pick.density) { DN_FWD48_DENSITY(DN_CASE_DENSITY) }
  else { DN_FWD48_INSTANCES(DN_CASE_FWD) }
#undef DN_CASE_DENSITY
#undef DN_CASE_FWD
#undef DN_CASE
  set_error("mlp_forward48: the picked instance is not in the list");   // (tests/test_g48_pick.py: cannot happen)
  return DN_E_UNSUPPORTED;
}

}  // namespace dn
