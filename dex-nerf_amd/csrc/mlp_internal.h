// Host-side helpers shared between mlp_fused.hip (packing, forward dispatch, inference entry points; the forward kernel itself is
// mlp_fused_kernel.h, compiled in mlp_fused_*.hip), mlp_train.hip (training forward / backward-data entry points) and mlp_wgrad.hip
// (weight gradients) - and the walk every weight-pack kernel makes over a NetLayout.  Each rule here has this one home.
#pragma once
#include "mlp_device.h"
#include <type_traits>

namespace dn {

struct PackPtrs {
  const float* w[kMaxStages];
  const float* b[kMaxStages];
};

// ---- the pack kernels' walk (pack_kernel, pack48_body, pack48_backward_body) ---------------------------------------------------
// stage that holds piece `piece` / bias tile `tile` of a stream
__device__ __forceinline__ int pack_stage_of_piece(const NetLayout& L, int piece) {
  int s = 0;
  while (s + 1 < L.n_stages && L.st[s + 1].piece0 <= piece) ++s;
  return s;
}
__device__ __forceinline__ int pack_stage_of_bias_tile(const NetLayout& L, int tile) {
  int s = 0;
  while (s + 1 < L.n_stages && L.st[s + 1].bias0 <= tile) ++s;
  return s;
}
// Where output row i of tile ts (tiles of ROWS rows) of forward stage st comes from: parameter *src and the row of it that is
// returned, or -1 for a zero row.  A stage with a second source keeps that source's one row in row 0 of its first tile (fc_alpha
// in front of fc_feat); dens_head (dn_mlp_pack_density, last stage): the source's one row is row 3 of the 4-row head.
template <int ROWS>
__device__ __forceinline__ int pack_src_row(const StageDesc& st, int ts, int i, bool dens_head, int* src) {
  *src = st.src;
  if (st.src2 >= 0) {
    if (ts == 0) { *src = st.src2; return i == 0 ? 0 : -1; }
    --ts;
  } else if (dens_head) {
    return ts * ROWS + i == 3 ? 0 : -1;
  }
  const int n = ts * ROWS + i;
  return n < st.n_real ? n : -1;
}

// ---- packing, host --------------------------------------------------------------------------------------------------------
// The parameter pointers of a pack call (`who`: the entry point, for its messages).  h_biases == NULL: a stream without bias
// tiles, whose b[] is never read.  n_params < 0: every parameter of the network.
inline int collect_pack_ptrs(const char* who, const dn_mlp_desc& d, const float* const* h_weights, const float* const* h_biases,
                             PackPtrs* ptrs, int n_params = -1) {
  if (n_params < 0) n_params = d.num_layers + (d.use_viewdirs ? 4 : 1);
  *ptrs = PackPtrs{};
  for (int i = 0; i < n_params; ++i) {
    DN_REQUIRE(h_weights[i] && (!h_biases || h_biases[i]), "%s: parameter %d is NULL", who, i);
    ptrs->w[i] = h_weights[i];
    ptrs->b[i] = h_biases ? h_biases[i] : h_weights[i];
  }
  return 0;
}
// bytes of the core (32-point) stream of a packed buffer = offset of its 48-point region (mlp_geo48.h)
inline size_t core_stream_bytes(int bias_bytes, int total_pieces) {
  return static_cast<size_t>(bias_bytes) + static_cast<size_t>(total_pieces) * kPieceBytes;
}
// f(std::integral_constant<int, F>) with the Prec<F> code of a DN_PREC_* value: 1 bf16, 2 fp16, 0 fp32 (WITH_F32 = false: the
// 16-bit-only families, where everything but fp16 is bf16)
template <bool WITH_F32, class Fn>
inline void with_prec(int precision, Fn&& f) {
  if (precision == DN_PREC_F16) return f(std::integral_constant<int, 2>{});
  if constexpr (WITH_F32) {
    if (precision != DN_PREC_BF16) return f(std::integral_constant<int, 0>{});
  }
  return f(std::integral_constant<int, 1>{});
}

// ---- entry points ---------------------------------------------------------------------------------------------------------
// DN_PREC_BF16_S8 is bf16 arithmetic with 8-bit saved tensors: leaves the arithmetic precision in *precision, returns the other half
inline bool split_precision(int* precision) {
  const bool s8 = *precision == DN_PREC_BF16_S8;
  if (s8) *precision = DN_PREC_BF16;
  return s8;
}
// the points-or-rays block of a forward call (`who`: the entry point, for its messages)
inline int set_point_inputs(const char* who, const dn_mlp_desc& d, const float* pts, const float* viewdirs, const float* rays,
                            int ray_stride, const float* z_vals, int64_t n_rays, int samples_per_ray, FwdParams* p) {
  if (pts != nullptr) {
    DN_REQUIRE(!d.use_viewdirs || viewdirs, "%s: viewdirs required with use_viewdirs", who);
    p->mode = 1; p->pts = pts; p->viewdirs = viewdirs;
  } else {
    DN_REQUIRE(rays && z_vals, "%s: need pts, or rays + z_vals", who);
    DN_REQUIRE(ray_stride >= (d.use_viewdirs ? 11 : 8), "%s: ray_stride too small", who);
    p->mode = 0; p->rays = rays; p->ray_stride = ray_stride; p->z = z_vals;
  }
  p->n_points = n_rays * samples_per_ray;
  p->S = samples_per_ray;
  return 0;
}
// saved-activation slots of TrainLayout / TrainLayout48 -> FwdParams; gradient slots -> BwdParams / Bwd48Params
template <class Layout>
inline void copy_act_slots(const Layout& t, FwdParams* p) {
  p->slot_xyz = t.slot_xyz; p->slot_dir = t.slot_dir; p->slot_layer1 = t.slot_layer1; p->slot_trunk0 = t.slot_trunk0;
  p->slot_feat = t.slot_feat; p->slot_dirout = t.slot_dirout;
}
template <class Layout, class Params>
inline void copy_grad_slots(const Layout& t, Params* p) {
  p->gslot_dirout = t.gslot_dirout; p->gslot_feat = t.gslot_feat; p->gslot_trunk0 = t.gslot_trunk0; p->gslot_layer1 = t.gslot_layer1;
  p->gslot_out = t.gslot_out;
}
// workgroups of a persistent launch: one per tile up to one per compute unit
inline long long persistent_grid(long long n_tiles, int cus = device_cus()) { return n_tiles < cus ? n_tiles : cus; }

int setup_params(const dn_mlp_desc* desc, int precision, const void* packed, FwdParams* p);
struct CompParams;
// tile_counter: a zeroed device word of the caller's for the instances that claim their tiles (mlp_geo48.h G48Params); NULL = fixed stride
int dispatch_forward(const dn_mlp_desc& d, int precision, FwdParams& p, hipStream_t stream, const CompParams* comp = nullptr, int* composited = nullptr,
                     unsigned* tile_counter = nullptr);
int launch_pack(const NetLayout& L, const PackPtrs& ptrs, void* packed, int precision, hipStream_t stream, bool density = false);
void fill_freqs(float* f, int num_fns, int log_sampling);  // rays_sampling.hip

}  // namespace dn
