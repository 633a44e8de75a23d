// The coarse-to-fine positional encoding of BARF (Lin et al. 2021, eq. 14) around the unchanged network kernels.
//   a_k = (1 - cos(pi * clamp(p L - k, 0, 1))) / 2 ,  p = clamp((it - start) / (end - start), 0, 1)
// A per-band amplitude on the encoding is a per-column scale of the weights that multiply it, W (a * enc) = (W diag(a)) enc, so:
//   anneal_amp_kernel      the table, from the iteration counter ON THE DEVICE (a replayed graph follows it)
//   anneal_weights_kernel  fp32 copies of the layers that read an encoding, band columns times a: what the pack kernels then read
//   anneal_grads_kernel    dL/dW = (dL/dW_eff) diag(a), in place on the band columns of the weight gradients
// Elementwise, a few hundred KiB per network at most: launch-bound.  Plain vector stores, no atomics, no host reads.
#include <cmath>

#include "../../include/dexnerf_hip_anneal.h"
#include "dn_common.h"
#include "mlp_layout.h"

namespace dn {

constexpr int kAnnealMaxBands = 32;
constexpr int kAnnealMaxLayers = 64;   // per network layer1 + the wide trunk layers (at most D - 2 = 30) + layers_dir.0; two networks

__global__ __launch_bounds__(64) void anneal_amp_kernel(const uint32_t* __restrict__ rng_state, double iteration, double start, double end,
                                                        int l_xyz, int l_dir, int anneal_dir, float* __restrict__ amp) {
  const int t = threadIdx.x;
  if (t >= l_xyz + l_dir) return;
  const double it = rng_state != nullptr ? static_cast<double>(rng_state[3]) : iteration;
  double p;
  if (end > start) {
    p = (it - start) / (end - start);
    p = p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p);
  } else {
    p = it >= start ? 1.0 : 0.0;
  }
  const bool dir = t >= l_xyz;
  const int k = dir ? t - l_xyz : t;
  const double x = p * static_cast<double>(dir ? l_dir : l_xyz) - static_cast<double>(k);
  float a;
  if (dir && !anneal_dir) a = 1.0f;
  else if (x <= 0.0) a = 0.0f;      // the clamped ends by branch: exact +0 and exact 1
  else if (x >= 1.0) a = 1.0f;
  else a = static_cast<float>(0.5 * (1.0 - cos(3.14159265358979323846 * x)));
  amp[t] = a;
}

// one layer that reads an encoding: an (rows, ld) row-major matrix whose columns [col_pe0, ld) are the encoding block
struct AnnealLayer {
  const float* src;
  float* dst;
  int32_t rows, ld, col_pe0, amp0;   // amp0: first amplitude of the block's encoding in the table
};
struct AnnealTable {
  int32_t n;
  AnnealLayer layer[kAnnealMaxLayers];
};

// blockIdx.y = layer, element e of its matrix = row * ld + col
__global__ __launch_bounds__(256) void anneal_weights_kernel(AnnealTable tab, const float* __restrict__ amp) {
  const AnnealLayer L = tab.layer[blockIdx.y];
  const int total = L.rows * L.ld;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = e % L.ld - L.col_pe0;
  const float w = L.src[e];
  L.dst[e] = c >= 3 ? w * amp[L.amp0 + (c - 3) / 6] : w;
}

// blockIdx.y = layer, element e of its band columns = row * n_band + j
__global__ __launch_bounds__(256) void anneal_grads_kernel(AnnealTable tab, const float* __restrict__ amp) {
  const AnnealLayer L = tab.layer[blockIdx.y];
  const int n_band = L.ld - L.col_pe0 - 3;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= L.rows * n_band) return;
  const int row = e / n_band, j = e - row * n_band;
  float* g = L.dst + static_cast<int64_t>(row) * L.ld + L.col_pe0 + 3 + j;
  const float a = amp[L.amp0 + j / 6];
  *g = a == 0.0f ? 0.0f : *g * a;
}

// the layers of `d` that read an encoding, from the pointer lists in the reference parameter order, appended to `tab`; `what`: the entry
// point, for messages
static int append_anneal_layers(const char* what, const dn_mlp_desc& d, const float* const* h_src, float* const* h_dst, AnnealTable* tab) {
  const int W = d.hidden_size, D = d.num_layers;
  const int DX = 3 + 6 * d.num_encoding_fn_xyz, DD = 3 + 6 * d.num_encoding_fn_dir;
  auto add = [&](int idx, int rows, int ld, int col_pe0, int amp0) -> bool {
    const float* src = h_src ? h_src[idx] : nullptr;
    float* dst = h_dst[idx];
    if ((h_src && !src) || !dst || tab->n >= kAnnealMaxLayers) return false;
    AnnealLayer& L = tab->layer[tab->n++];
    L.src = src; L.dst = dst; L.rows = rows; L.ld = ld; L.col_pe0 = col_pe0; L.amp0 = amp0;
    return true;
  };
  bool ok = add(0, W, DX, 0, 0);
  for (int i = 1; ok && i < D - 1; ++i)
    if (i % d.skip_connect_every == 0) ok = add(1 + i, W, W + DX, W, 0);   // the wide layers (build_layout's skip_mask)
  if (ok && d.use_viewdirs) ok = add(D, W / 2, W + DD, W, d.num_encoding_fn_xyz);
  if (!ok) {
    set_error("%s: a NULL pointer in the list of a layer that reads an encoding", what);
    return DN_E_INVAL;
  }
  return 0;
}

}  // namespace dn

using namespace dn;

extern "C" int dn_encoding_anneal_amplitudes(const uint32_t* rng_state, int64_t iteration, double start, double end, int l_xyz, int l_dir,
                                             int anneal_dir, float* amp, dn_stream_t stream) {
  DN_REQUIRE(amp != nullptr, "dn_encoding_anneal_amplitudes: amp must be given");
  DN_REQUIRE(l_xyz >= 1 && l_xyz <= kAnnealMaxBands && l_dir >= 0 && l_dir <= kAnnealMaxBands,
             "dn_encoding_anneal_amplitudes: l_xyz in 1..32, l_dir in 0..32 (got %d, %d)", l_xyz, l_dir);
  DN_REQUIRE(std::isfinite(start) && std::isfinite(end) && start >= 0.0 && end >= start,
             "dn_encoding_anneal_amplitudes: start and end are finite iterations with 0 <= start <= end (got %g, %g)", start, end);
  DN_REQUIRE(rng_state != nullptr || iteration >= 0, "dn_encoding_anneal_amplitudes: without an RNG state the iteration must be >= 0");
  hipLaunchKernelGGL(anneal_amp_kernel, dim3(1), dim3(64), 0, as_stream(stream), rng_state, static_cast<double>(iteration), start, end, l_xyz,
                     l_dir, anneal_dir, amp);
  return check_launch("dn_encoding_anneal_amplitudes");
}

// grid: x over the largest layer's elements, y over the layers
static int launch_scale_weights(const char* what, const AnnealTable& tab, const float* amp, dn_stream_t stream) {
  int most = 0;
  for (int i = 0; i < tab.n; ++i) {
    if (tab.layer[i].src == tab.layer[i].dst) {
      set_error("%s: a scaled copy is the weight itself", what);
      return DN_E_INVAL;
    }
    most = tab.layer[i].rows * tab.layer[i].ld > most ? tab.layer[i].rows * tab.layer[i].ld : most;
  }
  hipLaunchKernelGGL(anneal_weights_kernel, dim3((most + 255) / 256, tab.n), dim3(256), 0, as_stream(stream), tab, amp);
  return check_launch(what);
}

static int launch_scale_grads(const char* what, const AnnealTable& tab, const float* amp, dn_stream_t stream) {
  // the widest band block: layer1 / the wide layers (W rows of 6 L_xyz) or layers_dir.0 (W / 2 rows of 6 L_dir)
  int most = 0;
  for (int i = 0; i < tab.n; ++i) {
    const int n = tab.layer[i].rows * (tab.layer[i].ld - tab.layer[i].col_pe0 - 3);
    most = n > most ? n : most;
  }
  hipLaunchKernelGGL(anneal_grads_kernel, dim3((most + 255) / 256, tab.n), dim3(256), 0, as_stream(stream), tab, amp);
  return check_launch(what);
}

static bool same_encodings(const dn_mlp_desc& a, const dn_mlp_desc& b) {
  return a.num_encoding_fn_xyz == b.num_encoding_fn_xyz && a.use_viewdirs == b.use_viewdirs &&
         (!a.use_viewdirs || a.num_encoding_fn_dir == b.num_encoding_fn_dir);
}

extern "C" int dn_encoding_anneal_scale_weights(const dn_mlp_desc* desc, const float* const* h_weights, const float* amp, float* const* h_scaled,
                                                dn_stream_t stream) {
  const char* what = "dn_encoding_anneal_scale_weights";
  int rc = validate_desc(desc, DN_PREC_F32);
  if (rc) return rc;
  DN_REQUIRE(h_weights && amp && h_scaled, "%s: h_weights, amp and h_scaled must be given", what);
  AnnealTable tab;
  tab.n = 0;
  rc = append_anneal_layers(what, *desc, h_weights, h_scaled, &tab);
  if (rc) return rc;
  return launch_scale_weights(what, tab, amp, stream);
}

extern "C" int dn_encoding_anneal_scale_weights_pair(const dn_mlp_desc* desc_a, const float* const* h_weights_a, float* const* h_scaled_a,
                                                     const dn_mlp_desc* desc_b, const float* const* h_weights_b, float* const* h_scaled_b,
                                                     const float* amp, dn_stream_t stream) {
  const char* what = "dn_encoding_anneal_scale_weights_pair";
  int rc = validate_desc(desc_a, DN_PREC_F32);
  if (rc) return rc;
  rc = validate_desc(desc_b, DN_PREC_F32);
  if (rc) return rc;
  DN_REQUIRE(h_weights_a && h_scaled_a && h_weights_b && h_scaled_b && amp, "%s: the four pointer lists and amp must be given", what);
  DN_REQUIRE(same_encodings(*desc_a, *desc_b), "%s: the two networks read one amplitude table: they must agree on L_xyz / L_dir", what);
  AnnealTable tab;
  tab.n = 0;
  rc = append_anneal_layers(what, *desc_a, h_weights_a, h_scaled_a, &tab);
  if (rc) return rc;
  rc = append_anneal_layers(what, *desc_b, h_weights_b, h_scaled_b, &tab);
  if (rc) return rc;
  return launch_scale_weights(what, tab, amp, stream);
}

extern "C" int dn_encoding_anneal_scale_grads(const dn_mlp_desc* desc, const float* amp, float* const* h_dW, dn_stream_t stream) {
  const char* what = "dn_encoding_anneal_scale_grads";
  int rc = validate_desc(desc, DN_PREC_F32);
  if (rc) return rc;
  DN_REQUIRE(amp && h_dW, "%s: amp and h_dW must be given", what);
  AnnealTable tab;
  tab.n = 0;
  rc = append_anneal_layers(what, *desc, nullptr, h_dW, &tab);
  if (rc) return rc;
  return launch_scale_grads(what, tab, amp, stream);
}

extern "C" int dn_encoding_anneal_scale_grads_pair(const dn_mlp_desc* desc_a, float* const* h_dW_a, const dn_mlp_desc* desc_b,
                                                   float* const* h_dW_b, const float* amp, dn_stream_t stream) {
  const char* what = "dn_encoding_anneal_scale_grads_pair";
  int rc = validate_desc(desc_a, DN_PREC_F32);
  if (rc) return rc;
  rc = validate_desc(desc_b, DN_PREC_F32);
  if (rc) return rc;
  DN_REQUIRE(h_dW_a && h_dW_b && amp, "%s: both pointer lists and amp must be given", what);
  DN_REQUIRE(same_encodings(*desc_a, *desc_b), "%s: the two networks read one amplitude table: they must agree on L_xyz / L_dir", what);
  AnnealTable tab;
  tab.n = 0;
  rc = append_anneal_layers(what, *desc_a, nullptr, h_dW_a, &tab);
  if (rc) return rc;
  rc = append_anneal_layers(what, *desc_b, nullptr, h_dW_b, &tab);
  if (rc) return rc;
  return launch_scale_grads(what, tab, amp, stream);
}
