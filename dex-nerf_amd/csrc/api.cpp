// Library-level entry points: error string, ABI version, and the fused predict_and_render_radiance
// forward (reference nerf/train_utils.py:92-202) sequenced on one stream from the per-stage kernels.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/dexnerf_hip_ext.h"
#include "../../include/dexnerf_hip_normals.h"
#include "../../include/dexnerf_hip_quantile.h"
#include "../../include/dexnerf_hip_layers.h"
#include "../../include/dexnerf_hip_refine.h"
#include "dn_common.h"
#include "composite_body.h"
#include "dn_rng.h"
#include "mlp_layout.h"

namespace dn {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int ensure_big_lds(const void* kernel) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  static thread_local std::vector<std::pair<const void*, int>> done;
  for (const auto& kd : done)
    if (kd.first == kernel && kd.second == dev) return 0;
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) { set_error("hipFuncSetAttribute(device %d): %s", dev, hipGetErrorString(e)); return -static_cast<int>(e); }
  done.emplace_back(kernel, dev);
  return 0;
}

int device_cus() {
  constexpr int kMaxDev = 64;
  static thread_local int cache[kMaxDev] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return 256;
  if (cache[dev] == 0) {
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    cache[dev] = cus;
  }
  return cache[dev];
}

static size_t align256(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

// Every workspace is a run of regions, each rounded up to 256 bytes; a NULL base carves nothing and only counts (the *_bytes answers)
struct Carver {
  void* base;
  size_t off = 0;
  void* take(size_t bytes) {
    void* p = base ? static_cast<void*>(static_cast<char*>(base) + off) : nullptr;
    off += align256(bytes);
    return p;
  }
  float* floats(size_t count) { return static_cast<float*>(take(count * sizeof(float))); }
};

struct Workspace {
  float *z_c, *rf_c, *w_c, *z_f, *rf_f, *g_rf;
  float *br, *z_mid, *rf_mid;   // dn_render_rays_depth_refined: the bracket records (N,K,4), their midpoints (N,K), the network's rows there
  float* thres_rep;             // dn_render_rays_depth_layers: the thresholds repeated 2L times each (its records are (N, K*2L, 4))
  unsigned* absmax_part;   // training: one word per workgroup of the compositing backward (largest |gradient| it stored)
  unsigned* status;   // the last 256 bytes: word 0 = non-finite raw radiance-field values met by this call's compositing
  size_t bytes;
};
// kDepth: dn_render_rays_depth's and the normal render's - depths and raw rows only, the coarse weights stay inside
// density_resample_kernel (no w_c region); kTrain: the render's regions, then g_rf and absmax_part
enum WorkspaceKind { kRender, kTrain, kDepth };
// Words of the status block (zeroed by the one hipMemsetAsync at the top of a render call): 0 and 1 are what Python reads and sums
// (non-finite count, fp16 range flag).  dn_render_rays hands two more to its network launches as tile counters (mlp_geo48.h
// G48Params::tile_counter), 64 bytes apart: the coarse launch's and the fine launch's.  The depth, quantile and normal renders run the
// density instances, which do not claim tiles: they pass none.
constexpr int kStatusTilesCoarse = 16, kStatusTilesFine = 32;

// k_refine > 0 (kDepth): the refined render's three regions for k_refine thresholds, between the passes' regions and the status block;
// rep: the layers render's repeated thresholds behind them (it has k_refine = K*2L records per ray)
static Workspace carve(void* base, int64_t n, int nc, int nf, WorkspaceKind kind = kRender, int k_refine = 0, bool rep = false) {
  Workspace w{};
  Carver c{base};
  const size_t rays = static_cast<size_t>(n);
  w.z_c = c.floats(rays * nc);
  w.rf_c = c.floats(rays * nc * 4);
  if (kind != kDepth) w.w_c = c.floats(rays * nc);
  if (nf > 0) {
    w.z_f = c.floats(rays * (nc + nf));
    w.rf_f = c.floats(rays * (nc + nf) * 4);
  }
  if (kind == kTrain) {
    w.g_rf = c.floats(rays * (nc + nf) * 4);   // d loss / d raw radiance field, one network at a time
    w.absmax_part = static_cast<unsigned*>(c.take(static_cast<size_t>((n + 3) / 4) * sizeof(unsigned)));
  }
  if (k_refine > 0) {
    w.br = c.floats(rays * k_refine * 4);
    w.z_mid = c.floats(rays * k_refine);
    w.rf_mid = c.floats(rays * k_refine * 4);
    if (rep) w.thres_rep = c.floats(static_cast<size_t>(k_refine));
  }
  w.status = static_cast<unsigned*>(c.take(256));
  w.bytes = c.off;
  return w;
}

// the distortion regulariser inside the render backward (dn_render_rays_backward_reg): one network at a time, the launches are
// stream-ordered.  The coarse weights need no room: the training forward left them in Workspace::w_c.
struct RegWorkspace {
  float *weights, *g_weights;   // (N, num_coarse + num_fine): the fine network's sample weights; dn_distortion_loss's gradient of either network
  double* ray_loss;             // (N)
  size_t bytes;
};

static RegWorkspace carve_reg(void* base, int64_t n, int nc, int nf) {
  RegWorkspace w{};
  Carver c{base};
  const size_t samples = static_cast<size_t>(n) * (nc + nf);
  w.weights = c.floats(samples);
  w.g_weights = c.floats(samples);
  w.ray_loss = static_cast<double*>(c.take(static_cast<size_t>(n) * sizeof(double)));
  w.bytes = c.off;
  return w;
}

// ---- what the density renders (depth, quantile depth, normals) share: refusals, the status block, the passes before the last ----------
// The refusals every density render makes before any GPU work, under the entry point's name; `extras`: whether the entry point's own
// required pointers are there (they belong to its "bad arguments").  The "thresholds given without ..." line differs: it follows in
// the caller.
static int check_density_render(const char* who, const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine,
                                const void* packed_fine, const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int num_fine,
                                int n_thres, const void* workspace, bool extras = true) {
  DN_REQUIRE(desc_coarse && packed_coarse && extras && rays && workspace && n_rays >= 0, "%s: bad arguments", who);
  DN_REQUIRE(num_coarse >= 1 && num_fine >= 0 && ray_stride >= 8, "%s: bad sample counts / ray stride", who);
  DN_REQUIRE(num_fine == 0 || (desc_fine && packed_fine), "%s: fine pass requested without a fine net", who);
  DN_REQUIRE(n_thres >= 0, "%s: negative threshold count", who);
  DN_REQUIRE(!desc_coarse->use_viewdirs && (num_fine == 0 || !desc_fine->use_viewdirs),
             "%s: takes density sub-networks (dn_mlp_density_desc / dn_mlp_pack_density): use_viewdirs must be 0", who);
  DN_REQUIRE(num_fine == 0 || (num_coarse >= 10 && num_coarse <= 512 && num_coarse + num_fine <= 2048),
             "%s: need 10 <= num_coarse <= 512 and num_coarse + num_fine <= 2048", who);
  DN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  return 0;
}

static int zero_status(const char* who, unsigned* status, dn_stream_t stream) {
  hipError_t e = hipMemsetAsync(status, 0, 256, as_stream(stream));
  if (e != hipSuccess) { set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(e)); return -static_cast<int>(e); }
  return 0;
}

// The passes before the last one, into a kDepth workspace: the coarse depths and, with a fine pass, the coarse density network and its
// compositing fused with the resampling (w.z_f; depth_c / acc_c).  Without a fine pass the coarse network IS the last pass: the caller's.
static int density_coarse_pass(const dn_mlp_desc* desc_coarse, const void* packed_coarse, int precision, const float* rays, int ray_stride,
                               int64_t n_rays, int num_coarse, int num_fine, int lindisp, float noise_std, const float* t_rand,
                               const float* noise_c, const float* u, float* depth_c, float* acc_c, const Workspace& w, dn_stream_t stream) {
  int rc;
  if ((rc = dn_coarse_depths(rays, ray_stride, n_rays, num_coarse, lindisp, t_rand, w.z_c, stream))) return rc;
  if (num_fine == 0) return 0;
  if ((rc = run_network_flagged(desc_coarse, precision, packed_coarse, nullptr, nullptr, rays, ray_stride, w.z_c, n_rays, num_coarse, w.rf_c,
                                w.status + 1, stream)))
    return rc;
  return density_resample_counting(w.rf_c, w.z_c, rays + 3, ray_stride, noise_c, noise_std, u, n_rays, num_coarse, num_fine, depth_c, acc_c,
                                   w.z_f, w.status, stream);
}

}  // namespace dn

using namespace dn;

extern "C" int dn_abi_version(void) { return DN_ABI_VERSION; }

extern "C" const char* dn_last_error(void) { return g_err; }

extern "C" size_t dn_render_workspace_bytes(int64_t n_rays, int num_coarse, int num_fine) {
  if (n_rays < 0 || num_coarse < 1 || num_fine < 0) return 0;
  return carve(nullptr, n_rays, num_coarse, num_fine).bytes;
}

extern "C" int dn_render_rays(const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine,
                              const void* packed_fine, int precision, const float* rays, int ray_stride,
                              int64_t n_rays, int num_coarse, int num_fine, int lindisp, float noise_std,
                              int white_background, const float* h_m_thres, int n_thres, const float* t_rand,
                              const float* noise_c, const float* u, const float* noise_f, float* rgb_c,
                              float* depth_c, float* acc_c, float* rgb_f, float* depth_f, float* acc_f, float* dex_f,
                              void* workspace, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(desc_coarse && packed_coarse && rays && workspace && n_rays >= 0, "dn_render_rays: bad arguments");
  DN_REQUIRE(num_fine == 0 || (desc_fine && packed_fine), "dn_render_rays: fine pass requested without a fine net");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "dn_render_rays: workspace must be 256-byte aligned");
  Workspace w = carve(workspace, n_rays, num_coarse, num_fine);
  int rc;
  if ((rc = zero_status("dn_render_rays", w.status, stream))) return rc;
  if ((rc = dn_coarse_depths(rays, ray_stride, n_rays, num_coarse, lindisp, t_rand, w.z_c, stream))) return rc;
  const bool fine = num_fine > 0;
  DN_REQUIRE(n_thres >= 0 && n_thres <= kMaxThres, "dn_render_rays: at most %d Dex thresholds", kMaxThres);
  // Without density noise the network launch may composite its own rays (the 48-point fixed-shape instances, samples per ray
  // dividing their 384-point tile: the raw radiance field then never goes to HBM); it says whether it did.
  auto comp_for = [&](float* rgb, float* acc, float* weights, float* depth, float* dex, int k) {
    CompParams c{};
    c.rgb = rgb; c.acc = acc; c.weights = weights; c.depth = depth; c.dex = dex; c.disp = nullptr;
    c.nonfinite = w.status; c.n_rays = n_rays; c.n_thres = k; c.white = white_background;
    for (int i = 0; i < kMaxThres; ++i) c.th.m[i] = (i < k) ? h_m_thres[i] : 0.0f;
    return c;
  };
  const bool may_fuse = !(noise_std > 0.0f);
  int done = 0;
  // Dex depths come from the fine pass (train_utils.py:199-201); coarse-only renders report the coarse ones.
  {
    const CompParams c = comp_for(rgb_c, acc_c, w.w_c, depth_c, fine ? nullptr : dex_f, fine ? 0 : n_thres);
    if ((rc = run_network_flagged(desc_coarse, precision, packed_coarse, nullptr, nullptr, rays, ray_stride, w.z_c, n_rays,
                                  num_coarse, w.rf_c, w.status + 1, stream, (may_fuse && rgb_c) ? &c : nullptr, &done,
                                  w.status + kStatusTilesCoarse)))
      return rc;
  }
  if (!done && (rc = volume_render_counting(w.rf_c, w.z_c, rays + 3, ray_stride, noise_c, noise_std, white_background, h_m_thres,
                                            fine ? 0 : n_thres, n_rays, num_coarse, rgb_c, nullptr, acc_c, w.w_c, depth_c,
                                            fine ? nullptr : dex_f, w.status, stream)))
    return rc;
  if (!fine) return 0;
  if ((rc = dn_fine_depths(w.z_c, w.w_c, u, n_rays, num_coarse, num_fine, w.z_f, nullptr, stream))) return rc;
  {
    const CompParams c = comp_for(rgb_f, acc_f, nullptr, depth_f, dex_f, n_thres);
    if ((rc = run_network_flagged(desc_fine, precision, packed_fine, nullptr, nullptr, rays, ray_stride, w.z_f, n_rays,
                                  num_coarse + num_fine, w.rf_f, w.status + 1, stream, (may_fuse && rgb_f) ? &c : nullptr, &done,
                                  w.status + kStatusTilesFine)))
      return rc;
  }
  if (done) return 0;
  return volume_render_counting(w.rf_f, w.z_f, rays + 3, ray_stride, noise_f, noise_std, white_background, h_m_thres, n_thres,
                                n_rays, num_coarse + num_fine, rgb_f, nullptr, acc_f, nullptr, depth_f, dex_f, w.status, stream);
}

// ---- the depth-only render: density sub-networks + sigma-only compositing (depth, acc, Dex depths; no colour) -----------------
extern "C" size_t dn_render_depth_workspace_bytes(int64_t n_rays, int num_coarse, int num_fine) {
  if (n_rays < 0 || num_coarse < 1 || num_fine < 0) return 0;
  return carve(nullptr, n_rays, num_coarse, num_fine, kDepth).bytes;
}

// what dn_render_rays_depth_refined adds to the driver below (include/dexnerf_hip_refine.h)
struct RefineArgs {
  int steps;
  float *refined, *width;
};

// what dn_render_rays_depth_layers adds to the driver below (include/dexnerf_hip_layers.h); steps -1: sample mode
struct LayersArgs {
  int n_layers, steps;
  float* events;
  int* count;
  float* width;
};

// the one driver of dn_render_rays_depth, dn_render_rays_depth_quantiles, dn_render_rays_depth_refined and dn_render_rays_depth_layers
// (`who`: the entry point, for messages): with n_quant > 0 the last pass is composited by composite_quantile_kernel, with `refine` by
// composite_brackets_kernel, with `layers` by composite_layers_kernel, otherwise by composite_density_kernel - the launches are the same
// in number; `refine` and `layers` then add their bisection steps and the finish
static int render_rays_depth_impl(const char* who, const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine,
                                  const void* packed_fine, int precision, const float* rays, int ray_stride, int64_t n_rays,
                                  int num_coarse, int num_fine, int lindisp, float noise_std, const float* d_m_thres, int n_thres,
                                  const float* t_rand, const float* noise_c, const float* u, const float* noise_f, float* depth_c,
                                  float* acc_c, float* depth_f, float* acc_f, float* dex_f, const float* d_quantiles, int n_quant,
                                  int interp, float* qdepth, void* workspace, dn_stream_t stream, const RefineArgs* refine = nullptr,
                                  const LayersArgs* layers = nullptr) {
  // every argument is judged before any GPU work
  int rc;
  if ((rc = check_density_render(who, desc_coarse, packed_coarse, desc_fine, packed_fine, rays, ray_stride, n_rays, num_coarse, num_fine, n_thres,
                                 workspace, (!refine || refine->refined) && (!layers || (layers->events && layers->count)))))
    return rc;
  DN_REQUIRE(n_thres == 0 || (d_m_thres && dex_f), "%s: thresholds given without dex output", who);
  if ((rc = quantile_args_check(who, d_quantiles, n_quant, interp, qdepth))) return rc;
  if (refine) {
    DN_REQUIRE(n_thres >= 1, "%s: needs at least one threshold", who);
    DN_REQUIRE(refine->steps >= 0 && refine->steps <= DN_MAX_REFINE_STEPS, "%s: need 0 <= refine_steps <= %d", who, DN_MAX_REFINE_STEPS);
    DN_REQUIRE(noise_std == 0.0f, "%s: the brackets are those of the raw density: noise_std must be 0", who);
    DN_REQUIRE(n_rays <= INT64_C(0x7fffffff) / n_thres, "%s: at most 2^31 - 1 records (n_rays * n_thres)", who);
  }
  if (layers) {
    if ((rc = layers_check(who, n_thres, layers->n_layers, n_rays))) return rc;
    DN_REQUIRE(layers->steps >= -1 && layers->steps <= DN_MAX_REFINE_STEPS, "%s: need -1 <= refine_steps <= %d", who, DN_MAX_REFINE_STEPS);
    DN_REQUIRE(noise_std == 0.0f, "%s: the events are those of the raw density: noise_std must be 0", who);
  }
  if ((rc = validate_desc(desc_coarse, precision))) return rc;
  if (num_fine > 0 && (rc = validate_desc(desc_fine, precision))) return rc;
  if (n_rays == 0) return 0;
  const int n_records = layers ? n_thres * 2 * layers->n_layers : n_thres;   // per ray
  const Workspace w = carve(workspace, n_rays, num_coarse, num_fine, kDepth, (refine || layers) ? n_records : 0, layers != nullptr);
  if ((rc = zero_status(who, w.status, stream))) return rc;
  if ((rc = density_coarse_pass(desc_coarse, packed_coarse, precision, rays, ray_stride, n_rays, num_coarse, num_fine, lindisp, noise_std, t_rand,
                                noise_c, u, depth_c, acc_c, w, stream)))
    return rc;
  // the last pass: the fine one, or the coarse one of a coarse-only render - the Dex depths are its (train_utils.py:199-201)
  const bool fine = num_fine > 0;
  const int samples = num_coarse + num_fine;
  const float* z_last = fine ? w.z_f : w.z_c;
  float* rf_last = fine ? w.rf_f : w.rf_c;
  if ((rc = run_network_flagged(fine ? desc_fine : desc_coarse, precision, fine ? packed_fine : packed_coarse, nullptr, nullptr, rays, ray_stride,
                                z_last, n_rays, samples, rf_last, w.status + 1, stream)))
    return rc;
  const SigmaCompositeArgs last{rf_last, z_last, rays + 3, ray_stride, fine ? noise_f : noise_c, noise_std, d_m_thres, n_thres, n_rays, samples,
                                fine ? depth_f : depth_c, fine ? acc_f : acc_c, dex_f, w.status, d_quantiles, n_quant, interp, qdepth};
  if (layers) {
    // the events of the last pass, then per step the last pass's network at the midpoints (K*2L "samples" per ray, the same range word)
    // and dn_dex_bisect's kernel on the thresholds repeated 2L times each; the finish reads the records alone
    if ((rc = composite_layers_counting(last, layers->n_layers, w.br, w.z_mid, layers->count, stream))) return rc;
    if (layers->steps > 0 && (rc = layers_thresholds_launch(d_m_thres, n_thres, layers->n_layers, w.thres_rep, stream))) return rc;
    for (int step = 0; step < layers->steps; ++step) {
      if ((rc = run_network_flagged(fine ? desc_fine : desc_coarse, precision, fine ? packed_fine : packed_coarse, nullptr, nullptr, rays,
                                    ray_stride, w.z_mid, n_rays, n_records, w.rf_mid, w.status + 1, stream)))
        return rc;
      if ((rc = dex_bisect_launch(w.br, w.rf_mid, w.thres_rep, n_records, n_rays, w.z_mid, stream))) return rc;
    }
    return dex_layers_finish_launch(w.br, d_m_thres, n_thres, layers->n_layers, layers->steps >= 0, n_rays, layers->events, layers->width,
                                    stream);
  }
  if (!refine) return n_quant > 0 ? composite_quantile_counting(last, stream) : composite_density_counting(last, stream);
  // the brackets of the last pass, then per step the last pass's network at the midpoints (K "samples" per ray, the same range word:
  // the guarded-fp16 policy covers these launches) and the bisection; the finish reads the records alone
  if ((rc = composite_brackets_counting(last, w.br, w.z_mid, stream))) return rc;
  for (int step = 0; step < refine->steps; ++step) {
    if ((rc = run_network_flagged(fine ? desc_fine : desc_coarse, precision, fine ? packed_fine : packed_coarse, nullptr, nullptr, rays, ray_stride,
                                  w.z_mid, n_rays, n_thres, w.rf_mid, w.status + 1, stream)))
      return rc;
    if ((rc = dex_bisect_launch(w.br, w.rf_mid, d_m_thres, n_thres, n_rays, w.z_mid, stream))) return rc;
  }
  return dex_refine_finish_launch(w.br, d_m_thres, n_thres, n_rays, refine->refined, refine->width, stream);
}

extern "C" size_t dn_render_depth_refined_workspace_bytes(int64_t n_rays, int num_coarse, int num_fine, int n_thres) {
  if (n_rays < 0 || num_coarse < 1 || num_fine < 0 || n_thres < 1 || (n_rays > 0 && n_rays > INT64_C(0x7fffffff) / n_thres)) return 0;
  return carve(nullptr, n_rays, num_coarse, num_fine, kDepth, n_thres).bytes;
}

extern "C" int dn_render_rays_depth_refined(const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine,
                                            const void* packed_fine, int precision, const float* rays, int ray_stride, int64_t n_rays,
                                            int num_coarse, int num_fine, int lindisp, float noise_std, const float* d_m_thres,
                                            int n_thres, const float* t_rand, const float* noise_c, const float* u, const float* noise_f,
                                            float* depth_c, float* acc_c, float* depth_f, float* acc_f, float* dex_f, int refine_steps,
                                            float* refined, float* width, void* workspace, dn_stream_t stream) {
  const RefineArgs refine{refine_steps, refined, width};
  return render_rays_depth_impl("dn_render_rays_depth_refined", desc_coarse, packed_coarse, desc_fine, packed_fine, precision, rays, ray_stride,
                                n_rays, num_coarse, num_fine, lindisp, noise_std, d_m_thres, n_thres, t_rand, noise_c, u, noise_f, depth_c,
                                acc_c, depth_f, acc_f, dex_f, nullptr, 0, 0, nullptr, workspace, stream, &refine);
}

extern "C" size_t dn_render_depth_layers_workspace_bytes(int64_t n_rays, int num_coarse, int num_fine, int n_thres, int n_layers) {
  if (n_rays < 0 || num_coarse < 1 || num_fine < 0 || n_thres < 1 || n_layers < 1 || n_layers > DN_MAX_LAYERS ||
      n_thres > DN_MAX_LAYER_RECORDS / (2 * n_layers) || n_rays > INT64_C(0x7fffffff) / (static_cast<int64_t>(n_thres) * 2 * n_layers))
    return 0;
  return carve(nullptr, n_rays, num_coarse, num_fine, kDepth, n_thres * 2 * n_layers, true).bytes;
}

extern "C" int dn_render_rays_depth_layers(const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine,
                                           const void* packed_fine, int precision, const float* rays, int ray_stride, int64_t n_rays,
                                           int num_coarse, int num_fine, int lindisp, float noise_std, const float* d_m_thres, int n_thres,
                                           const float* t_rand, const float* noise_c, const float* u, const float* noise_f, float* depth_c,
                                           float* acc_c, float* depth_f, float* acc_f, float* dex_f, int n_layers, int refine_steps,
                                           float* events, int* count, float* width, void* workspace, dn_stream_t stream) {
  const LayersArgs layers{n_layers, refine_steps, events, count, width};
  return render_rays_depth_impl("dn_render_rays_depth_layers", desc_coarse, packed_coarse, desc_fine, packed_fine, precision, rays, ray_stride,
                                n_rays, num_coarse, num_fine, lindisp, noise_std, d_m_thres, n_thres, t_rand, noise_c, u, noise_f, depth_c,
                                acc_c, depth_f, acc_f, dex_f, nullptr, 0, 0, nullptr, workspace, stream, nullptr, &layers);
}

extern "C" int dn_render_rays_depth(const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine,
                                    const void* packed_fine, int precision, const float* rays, int ray_stride, int64_t n_rays,
                                    int num_coarse, int num_fine, int lindisp, float noise_std, const float* d_m_thres, int n_thres,
                                    const float* t_rand, const float* noise_c, const float* u, const float* noise_f, float* depth_c,
                                    float* acc_c, float* depth_f, float* acc_f, float* dex_f, void* workspace, dn_stream_t stream) {
  return render_rays_depth_impl("dn_render_rays_depth", desc_coarse, packed_coarse, desc_fine, packed_fine, precision, rays, ray_stride, n_rays,
                                num_coarse, num_fine, lindisp, noise_std, d_m_thres, n_thres, t_rand, noise_c, u, noise_f, depth_c, acc_c,
                                depth_f, acc_f, dex_f, nullptr, 0, 0, nullptr, workspace, stream);
}

// the depth-only render with the opacity-quantile depths of its last pass (include/dexnerf_hip_quantile.h)
extern "C" int dn_render_rays_depth_quantiles(const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine,
                                              const void* packed_fine, int precision, const float* rays, int ray_stride, int64_t n_rays,
                                              int num_coarse, int num_fine, int lindisp, float noise_std, const float* d_m_thres,
                                              int n_thres, const float* t_rand, const float* noise_c, const float* u, const float* noise_f,
                                              float* depth_c, float* acc_c, float* depth_f, float* acc_f, float* dex_f,
                                              const float* d_quantiles, int n_quant, int interp, float* qdepth, void* workspace,
                                              dn_stream_t stream) {
  return render_rays_depth_impl("dn_render_rays_depth_quantiles", desc_coarse, packed_coarse, desc_fine, packed_fine, precision, rays, ray_stride,
                                n_rays, num_coarse, num_fine, lindisp, noise_std, d_m_thres, n_thres, t_rand, noise_c, u, noise_f, depth_c,
                                acc_c, depth_f, acc_f, dex_f, d_quantiles, n_quant, interp, qdepth, workspace, stream);
}

// ---- the normal render (include/dexnerf_hip_normals.h): dn_render_rays_depth with the last pass differentiated ---------------------
namespace dn {
// the kDepth regions, then what the differentiated pass keeps: the training forward's saved tensors, the gradient records, the seed
// and the per-point gradient
struct NormalsWorkspace {
  Workspace d;
  void *act, *masks, *grads;
  float *g_out, *g_pts;
  size_t bytes;   // 0: the differentiated network's descriptor / precision is not covered
};

static NormalsWorkspace carve_normals(void* base, const dn_mlp_desc* desc_last, int precision, int64_t n, int nc, int nf) {
  NormalsWorkspace w{};
  w.d = carve(base, n, nc, nf, kDepth);
  const int64_t points = n * (nc + nf);
  size_t act = 0, masks = 0, grads = 0;
  if (dn_mlp_train_sizes(desc_last, precision, points, &act, &masks, &grads)) return w;
  Carver c{base, w.d.bytes};
  w.act = c.take(act); w.masks = c.take(masks); w.grads = c.take(grads);
  w.g_out = c.floats(static_cast<size_t>(points) * 4);
  w.g_pts = c.floats(static_cast<size_t>(points) * 3);
  w.bytes = c.off;
  return w;
}
}  // namespace dn

extern "C" size_t dn_render_normals_workspace_bytes(const dn_mlp_desc* desc_coarse, const dn_mlp_desc* desc_fine, int precision,
                                                    int64_t n_rays, int num_coarse, int num_fine) {
  if (!desc_coarse || n_rays < 0 || num_coarse < 1 || num_fine < 0 || (num_fine > 0 && !desc_fine)) return 0;
  const dn_mlp_desc* last = num_fine > 0 ? desc_fine : desc_coarse;
  if (desc_coarse->use_viewdirs || last->use_viewdirs || validate_desc(desc_coarse, precision) ||
      input_grad_check(last, precision, "dn_render_normals_workspace_bytes"))
    return 0;
  return carve_normals(nullptr, last, precision, n_rays, num_coarse, num_fine).bytes;
}

extern "C" int dn_render_rays_normals(const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine,
                                      const void* packed_fine, const void* packed_bwd, const void* packed_ig, int precision,
                                      const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int num_fine, int lindisp,
                                      float noise_std, const float* d_m_thres, int n_thres, const float* t_rand, const float* noise_c,
                                      const float* u, const float* noise_f, float* depth_c, float* acc_c, float* depth, float* acc,
                                      float* dex, float* normal, float* dex_normal, void* workspace, size_t workspace_bytes,
                                      dn_stream_t stream) {
  // every argument is judged before any GPU work
  const char* who = "dn_render_rays_normals";
  int rc;
  if ((rc = check_density_render(who, desc_coarse, packed_coarse, desc_fine, packed_fine, rays, ray_stride, n_rays, num_coarse, num_fine, n_thres,
                                 workspace, packed_bwd && packed_ig)))
    return rc;
  DN_REQUIRE(n_thres == 0 || (d_m_thres && (dex || dex_normal)), "dn_render_rays_normals: thresholds given without dex or dex_normal output");
  DN_REQUIRE(((reinterpret_cast<uintptr_t>(packed_bwd) | reinterpret_cast<uintptr_t>(packed_ig)) & 15) == 0,
             "dn_render_rays_normals: the backward and input-gradient streams must be 16-byte aligned");
  const bool fine = num_fine > 0;
  const dn_mlp_desc* last = fine ? desc_fine : desc_coarse;
  if ((rc = input_grad_check(last, precision, who))) return rc;   // F32, or BF16 with 16-bit saves; L_xyz in {6, 10}
  if (fine && (rc = validate_desc(desc_coarse, precision))) return rc;
  const NormalsWorkspace w = carve_normals(workspace, last, precision, n_rays, num_coarse, num_fine);
  DN_REQUIRE(w.bytes != 0 && workspace_bytes >= w.bytes, "dn_render_rays_normals: workspace too small (%zu bytes needed)", w.bytes);
  if (n_rays == 0) return 0;
  if ((rc = zero_status(who, w.d.status, stream))) return rc;
  if ((rc = density_coarse_pass(desc_coarse, packed_coarse, precision, rays, ray_stride, n_rays, num_coarse, num_fine, lindisp, noise_std, t_rand,
                                noise_c, u, depth_c, acc_c, w.d, stream)))
    return rc;
  const int samples = num_coarse + num_fine;
  const float* z_last = fine ? w.d.z_f : w.d.z_c;
  float* rf_last = fine ? w.d.rf_f : w.d.rf_c;
  // the differentiated pass: training forward (saves kept), seed, backward-data chain, per-point input gradient, compositing
  if ((rc = dn_run_network_train(last, precision, fine ? packed_fine : packed_coarse, nullptr, nullptr, rays, ray_stride, z_last, n_rays,
                                 samples, rf_last, w.act, w.masks, stream)))
    return rc;
  const int64_t points = n_rays * samples;
  if ((rc = density_seed(w.g_out, points, stream))) return rc;
  if ((rc = dn_mlp_backward_data(last, precision, packed_bwd, w.g_out, w.masks, points, w.grads, stream))) return rc;
  if ((rc = input_grad_points_from_rays(last, precision, packed_ig, w.grads, rays, ray_stride, z_last, n_rays, samples, w.g_pts, stream))) return rc;
  SigmaCompositeArgs c{rf_last, z_last, rays + 3, ray_stride, fine ? noise_f : noise_c, noise_std, d_m_thres, n_thres, n_rays, samples, depth, acc,
                       dex, w.d.status};
  c.g_pts = w.g_pts; c.normal = normal; c.dex_normal = dex_normal;
  return composite_normals_counting(c, stream);
}

// ---- predict_and_render_radiance under autograd (reference nerf/train_utils.py:92-202 + loss.backward(),
// train_dexnerf_rgb.py:278): one call forward, one call backward -------------------------------------------------------
extern "C" size_t dn_render_train_workspace_bytes(int64_t n_rays, int num_coarse, int num_fine) {
  if (n_rays < 0 || num_coarse < 1 || num_fine < 0) return 0;
  return carve(nullptr, n_rays, num_coarse, num_fine, kTrain).bytes;
}

extern "C" int dn_render_rays_train(const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine,
                                    const void* packed_fine, int precision, const float* rays, int ray_stride,
                                    int64_t n_rays, int num_coarse, int num_fine, int lindisp, float noise_std,
                                    int white_background, const float* h_m_thres, int n_thres, const float* t_rand,
                                    const float* noise_c, const float* u, const float* noise_f, float* rgb_c,
                                    float* depth_c, float* acc_c, float* rgb_f, float* depth_f, float* acc_f, float* dex_f,
                                    void* workspace, void* act_c, void* masks_c, void* act_f, void* masks_f,
                                    const uint32_t* rng_state, int perturb, dn_stream_t stream) {
  if (n_rays == 0) return 0;   // (before any check, as ever: empty tensors carry NULL data pointers)
  return dn_render_rays_train_geom(desc_coarse, packed_coarse, desc_fine, packed_fine, precision, rays, ray_stride, n_rays, num_coarse, num_fine,
                                   lindisp, noise_std, white_background, h_m_thres, n_thres, t_rand, noise_c, u, noise_f, rgb_c, depth_c, acc_c,
                                   rgb_f, depth_f, acc_f, dex_f, workspace, act_c, masks_c, act_f, masks_f, rng_state, perturb, nullptr, stream);
}

// dn_render_rays_train + z_samples (N, num_fine): the resamples the merge backward needs (dn_fine_depths_backward), caller-owned, may
// be NULL.  Outputs and workspace layout are dn_render_rays_train's.
extern "C" int dn_render_rays_train_geom(const dn_mlp_desc* desc_coarse, const void* packed_coarse, const dn_mlp_desc* desc_fine,
                                         const void* packed_fine, int precision, const float* rays, int ray_stride,
                                         int64_t n_rays, int num_coarse, int num_fine, int lindisp, float noise_std,
                                         int white_background, const float* h_m_thres, int n_thres, const float* t_rand,
                                         const float* noise_c, const float* u, const float* noise_f, float* rgb_c,
                                         float* depth_c, float* acc_c, float* rgb_f, float* depth_f, float* acc_f, float* dex_f,
                                         void* workspace, void* act_c, void* masks_c, void* act_f, void* masks_f,
                                         const uint32_t* rng_state, int perturb, float* z_samples, dn_stream_t stream) {
  DN_REQUIRE(desc_coarse && packed_coarse && rays && workspace && act_c && masks_c && n_rays >= 0, "dn_render_rays_train: bad arguments");
  DN_REQUIRE(num_fine == 0 || (desc_fine && packed_fine && act_f && masks_f), "dn_render_rays_train: fine pass requested without a fine net / its buffers");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "dn_render_rays_train: workspace must be 256-byte aligned");
  if (n_rays == 0) return 0;
  Workspace w = carve(workspace, n_rays, num_coarse, num_fine, kTrain);
  int rc;
  // a NULL draw with an RNG state: drawn in the kernels (dn_rng.h) - jitter / resampling u only when `perturb`, density noise
  // whenever noise_std > 0; explicit draws win (parity tests inject the reference's)
  const uint32_t* rng_perturb = perturb ? rng_state : nullptr;
  if ((rc = coarse_depths_rng(rays, ray_stride, n_rays, num_coarse, lindisp, t_rand, w.z_c, rng_perturb, stream))) return rc;
  if ((rc = dn_run_network_train(desc_coarse, precision, packed_coarse, nullptr, nullptr, rays, ray_stride, w.z_c, n_rays,
                                 num_coarse, w.rf_c, act_c, masks_c, stream)))
    return rc;
  const bool fine = num_fine > 0;
  if ((rc = volume_render_counting(w.rf_c, w.z_c, rays + 3, ray_stride, noise_c, noise_std, white_background, h_m_thres,
                                   fine ? 0 : n_thres, n_rays, num_coarse, rgb_c, nullptr, acc_c, w.w_c, depth_c,
                                   fine ? nullptr : dex_f, nullptr, stream, rng_state, kRngStreamNoiseCoarse)))
    return rc;
  if (!fine) return 0;
  if ((rc = fine_depths_rng(w.z_c, w.w_c, u, n_rays, num_coarse, num_fine, w.z_f, z_samples, rng_perturb, stream))) return rc;
  if ((rc = dn_run_network_train(desc_fine, precision, packed_fine, nullptr, nullptr, rays, ray_stride, w.z_f, n_rays,
                                 num_coarse + num_fine, w.rf_f, act_f, masks_f, stream)))
    return rc;
  return volume_render_counting(w.rf_f, w.z_f, rays + 3, ray_stride, noise_f, noise_std, white_background, h_m_thres, n_thres,
                                n_rays, num_coarse + num_fine, rgb_f, nullptr, acc_f, nullptr, depth_f, dex_f, nullptr, stream,
                                rng_state, kRngStreamNoiseFine);
}

// ---- the backward of dn_render_rays_train_geom with the ray gradient (pose / ray optimisation on the fused step) -----------------
namespace dn {
struct GeomWorkspace {
  float *g_z_f, *g_rd_f, *d_rays_f, *d_z_f;   // fine pass: compositing geometry, network input gradients
  float *g_z_c, *g_rd_c, *d_rays_c, *d_z_c;   // coarse pass
  float *gathered, *g_near_far;               // the merge's gather into the coarse depths; the near / far columns
  void* input_grad;                           // dn_mlp_backward_input's workspace, one network at a time
  size_t input_grad_bytes, bytes;
};

static GeomWorkspace carve_geom(void* base, const dn_mlp_desc* desc_c, const dn_mlp_desc* desc_f, int64_t n, int stride, int nc, int nf) {
  GeomWorkspace w{};
  Carver c{base};
  const size_t rays = static_cast<size_t>(n);
  if (nf > 0) {
    w.g_z_f = c.floats(rays * (nc + nf)); w.g_rd_f = c.floats(rays * 3); w.d_rays_f = c.floats(rays * stride); w.d_z_f = c.floats(rays * (nc + nf));
    w.gathered = c.floats(rays * nc);
  }
  w.g_z_c = c.floats(rays * nc); w.g_rd_c = c.floats(rays * 3); w.d_rays_c = c.floats(rays * stride); w.d_z_c = c.floats(rays * nc);
  w.g_near_far = c.floats(rays * 2);
  w.input_grad_bytes = dn_mlp_backward_input_workspace_bytes(desc_c, n * nc, 1);
  if (nf > 0) {
    const size_t fine = dn_mlp_backward_input_workspace_bytes(desc_f, n * (nc + nf), 1);
    if (fine > w.input_grad_bytes) w.input_grad_bytes = fine;
  }
  w.input_grad = c.take(w.input_grad_bytes);
  w.bytes = c.off;
  return w;
}

// The one backward of dn_render_rays_train / dn_render_rays_train_geom: the body of dn_render_rays_backward_ws, dn_render_rays_backward
// and dn_render_rays_backward_geom, which judge their own arguments, fill this struct and call it (n_rays > 0).
struct BackwardNet {   // what one network brings
  const dn_mlp_desc* desc;
  const void *packed_bwd, *packed_ig;   // packed_ig: the input-gradient stream, geometry only
  const float *noise, *g_rgb, *g_depth, *g_acc;
  const void *act, *masks;
  void* grads;
  float* const *h_dW, *const *h_db;
  float dist_weight = 0.0f;   // the weight of the network's distortion term (dn_render_rays_backward_reg); 0: none
};

struct RenderBackwardArgs {
  BackwardNet coarse, fine;
  int precision, ray_stride, num_coarse, num_fine, white_background;
  const float* rays;
  int64_t n_rays;
  float noise_std;
  void *workspace, *wg_scratch;
  size_t wg_scratch_bytes;
  int nets;     // bit 0 coarse, bit 1 fine; the geometry route: 3
  bool wgrad;   // weight gradients wanted (the geometry route with frozen networks: not)
  const uint32_t* rng_state;
  dn_stream_t stream;
  // the ray gradient, when d_rays is given: geom_workspace as carve_geom lays it out
  float* d_rays;
  void* geom_workspace;
  int lindisp, perturb;
  const float *t_rand, *z_samples;
  // the distortion regulariser, for a network whose dist_weight is non-zero: reg_workspace as carve_reg lays it out
  void* reg_workspace;
  float* reg2;   // [mean L_ray coarse, mean L_ray fine]
};

static int render_rays_backward(const RenderBackwardArgs& a) {
  const bool geom = a.d_rays != nullptr, fine = a.num_fine > 0;
  const int64_t n_rays = a.n_rays;
  const int nc = a.num_coarse, nf = a.num_fine;
  const Workspace w = carve(a.workspace, n_rays, nc, nf, kTrain);
  const GeomWorkspace g = geom ? carve_geom(a.geom_workspace, a.coarse.desc, a.fine.desc, n_rays, a.ray_stride, nc, nf) : GeomWorkspace{};
  const RegWorkspace reg = carve_reg(a.reg_workspace, n_rays, nc, nf);
  int rc;
  // both networks, one architecture: the two backward-data chains first, then ONE weight-gradient launch for the layers of both
  // (dn_mlp_weight_grad_pair) - a caller that wants the fine half finished early (its all-reduce under the coarse half) asks for
  // the networks one at a time
  const bool pair_wgrad = a.wgrad && a.nets == 3 && fine && a.coarse.desc && a.fine.desc &&
                          std::memcmp(a.coarse.desc, a.fine.desc, sizeof(dn_mlp_desc)) == 0 &&
                          weight_grad_pair_fits(*a.fine.desc);   // (both networks' layers in one batch: two D <= 12 networks)
  auto half = [&](const BackwardNet& net, const float* rf, const float* z, int samples, uint32_t noise_stream, float* g_z, float* g_rd,
                  float* d_rays_net, float* d_z, const float* kept_weights, float* reg_word) -> int {
    // the distortion term: the network's sample weights (as the forward kept them, or composited again - the same kernel, rows and
    // noise stream, so the same bits), dn_distortion_loss, and its gradient as the compositing backward's upstream g_weights
    const float* g_weights = nullptr;
    if (net.dist_weight != 0.0f) {
      const float* weights = kept_weights;
      if (weights == nullptr) {
        if ((rc = volume_render_counting(rf, z, a.rays + 3, a.ray_stride, net.noise, a.noise_std, a.white_background, nullptr, 0, n_rays, samples,
                                         nullptr, nullptr, nullptr, reg.weights, nullptr, nullptr, nullptr, a.stream, a.rng_state, noise_stream)))
          return rc;
        weights = reg.weights;
      }
      if ((rc = dn_distortion_loss(weights, z, a.rays + 6, a.ray_stride, n_rays, samples, net.dist_weight / static_cast<float>(n_rays),
                                   reg.g_weights, nullptr, 0, reg.ray_loss, reg_word, a.stream)))
        return rc;
      g_weights = reg.g_weights;
    }
    // 8-bit saved tensors with the per-launch gradient scale: the compositing backward leaves the largest |gradient| of each of its
    // workgroups behind, and the network backward reduces those words itself - no pass over g_rf in between (a few thousand words at
    // most: beyond that the separate reduction kernel is the cheaper one)
    const int64_t n_parts = (n_rays + 3) / 4;
    // (DEXNERF_S8_ABSMAX_KERNEL=1, read per call: the separate reduction kernel regardless - the A/B of tests/test_hip_parity.py)
    unsigned* parts = (a.precision == DN_PREC_BF16_S8 && s8_scale_is_per_launch() && n_parts <= 4096 && std::getenv("DEXNERF_S8_ABSMAX_KERNEL") == nullptr)
                          ? w.absmax_part : nullptr;
    if ((rc = volume_render_backward_rng(geom ? "dn_volume_render_backward_geom" : "dn_volume_render_backward", rf, z, a.rays + 3, a.ray_stride,
                                         net.noise, a.noise_std, a.white_background, n_rays, samples, net.g_rgb, net.g_depth, net.g_acc, nullptr,
                                         g_weights, w.g_rf, g_z, g_rd, a.rng_state, noise_stream, parts, a.stream)))
      return rc;
    const int64_t n_points = n_rays * samples;
    if ((rc = mlp_backward_data_partials(net.desc, a.precision, net.packed_bwd, w.g_rf, net.masks, n_points, net.grads, parts,
                                         static_cast<int>(parts ? n_parts : 0), a.stream)))
      return rc;
    if (geom && (rc = dn_mlp_backward_input(net.desc, a.precision, net.packed_ig, net.grads, nullptr, nullptr, a.rays, a.ray_stride, z, n_rays,
                                            samples, nullptr, nullptr, d_rays_net, d_z, g.input_grad, g.input_grad_bytes, a.stream)))
      return rc;
    if (!a.wgrad || pair_wgrad) return 0;   // none wanted, or both networks' weight gradients follow in one launch
    // (one network at a time: the launches are stream-ordered, so the scratch is free again when the second one starts)
    return dn_mlp_weight_grad_all_ws(net.desc, a.precision, net.act, net.grads, n_points, net.h_dW, net.h_db, a.wg_scratch, a.wg_scratch_bytes,
                                     a.stream);
  };
  // the fine network first: autograd's order too (its graph node is the younger one), and the half a data-parallel caller
  // wants finished first so that its all-reduce overlaps the coarse half; its depth gradient feeds the coarse depths through the merge
  if ((a.nets & 2) && fine && (rc = half(a.fine, w.rf_f, w.z_f, nc + nf, kRngStreamNoiseFine, g.g_z_f, g.g_rd_f, g.d_rays_f, g.d_z_f, nullptr,
                                            a.reg2 ? a.reg2 + 1 : nullptr)))
    return rc;
  if ((a.nets & 1) && (rc = half(a.coarse, w.rf_c, w.z_c, nc, kRngStreamNoiseCoarse, g.g_z_c, g.g_rd_c, g.d_rays_c, g.d_z_c, w.w_c, a.reg2))) return rc;
  if (pair_wgrad &&
      (rc = dn_mlp_weight_grad_pair_ws(a.fine.desc, a.precision, a.fine.act, a.fine.grads, n_rays * (nc + nf), a.fine.h_dW, a.fine.h_db,
                                       a.coarse.act, a.coarse.grads, n_rays * nc, a.coarse.h_dW, a.coarse.h_db, a.wg_scratch,
                                       a.wg_scratch_bytes, a.stream)))
    return rc;
  if (!geom) return 0;
  // g_z_fine = g_z + d_z, gathered into the coarse depths; g_z_coarse = (g_z + d_z) + gathered -> near / far; then the rows
  if (fine && (rc = fine_depths_backward_sum(w.z_c, a.z_samples, g.g_z_f, g.d_z_f, n_rays, nc, nf, g.gathered, a.stream))) return rc;
  if ((rc = coarse_depths_backward_rng(a.rays, a.ray_stride, n_rays, nc, a.lindisp, a.t_rand, g.g_z_c, g.d_z_c, fine ? g.gathered : nullptr,
                                       g.g_near_far, a.perturb ? a.rng_state : nullptr, a.stream)))
    return rc;
  return combine_ray_grads(g.d_rays_c, fine ? g.d_rays_f : nullptr, g.g_rd_c, fine ? g.g_rd_f : nullptr, g.g_near_far, n_rays, a.ray_stride,
                           a.d_rays, a.stream);
}
}  // namespace dn

// dn_render_rays_backward_ws and dn_render_rays_backward_reg (`name`: the entry point, for messages; without the regulariser: weights 0)
static int render_rays_backward_entry(const char* name, const dn_mlp_desc* desc_coarse, const void* packed_bwd_coarse,
                                      const dn_mlp_desc* desc_fine, const void* packed_bwd_fine, int precision,
                                      const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int num_fine,
                                      float noise_std, int white_background, const float* noise_c, const float* noise_f,
                                      const float* g_rgb_c, const float* g_depth_c, const float* g_acc_c,
                                      const float* g_rgb_f, const float* g_depth_f, const float* g_acc_f, void* workspace,
                                      const void* act_c, const void* masks_c, void* grads_c, const void* act_f,
                                      const void* masks_f, void* grads_f, float* const* h_dW_c, float* const* h_db_c,
                                      float* const* h_dW_f, float* const* h_db_f, int nets, const uint32_t* rng_state,
                                      void* wg_scratch, size_t wg_scratch_bytes, float dist_weight_c, float dist_weight_f,
                                      void* reg_workspace, size_t reg_workspace_bytes, float* reg2, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  // every argument is judged before any GPU work
  DN_REQUIRE(rays && workspace && n_rays >= 0 && (nets & ~3) == 0 && (wg_scratch != nullptr || wg_scratch_bytes == 0), "%s: bad arguments", name);
  DN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "%s: workspace must be 256-byte aligned", name);
  DN_REQUIRE(std::isfinite(dist_weight_c) && std::isfinite(dist_weight_f) && dist_weight_c >= 0.0f && dist_weight_f >= 0.0f,
             "%s: the distortion weights must be finite and >= 0", name);
  if (num_fine <= 0 || !(nets & 2)) dist_weight_f = 0.0f;   // (a network outside this call brings no term)
  if (!(nets & 1)) dist_weight_c = 0.0f;
  if (dist_weight_c != 0.0f || dist_weight_f != 0.0f) {
    DN_REQUIRE(num_coarse >= 1 && num_fine >= 0 && ray_stride >= 8, "%s: bad sample counts / ray stride", name);
    DN_REQUIRE((dist_weight_f != 0.0f ? num_coarse + num_fine : num_coarse) <= 1024, "%s: the distortion term takes at most 1024 samples per ray", name);
    DN_REQUIRE(reg_workspace && reg2, "%s: a non-zero distortion weight needs reg_workspace and reg2", name);
    DN_REQUIRE((reinterpret_cast<uintptr_t>(reg_workspace) & 255) == 0, "%s: reg_workspace must be 256-byte aligned", name);
    const size_t need = carve_reg(nullptr, n_rays, num_coarse, num_fine).bytes;
    DN_REQUIRE(reg_workspace_bytes >= need, "%s: reg_workspace too small (%zu bytes needed)", name, need);
  }
  RenderBackwardArgs a{};
  a.coarse = BackwardNet{desc_coarse, packed_bwd_coarse, nullptr, noise_c, g_rgb_c, g_depth_c, g_acc_c, act_c, masks_c, grads_c, h_dW_c, h_db_c};
  a.fine = BackwardNet{desc_fine, packed_bwd_fine, nullptr, noise_f, g_rgb_f, g_depth_f, g_acc_f, act_f, masks_f, grads_f, h_dW_f, h_db_f};
  auto complete = [](const BackwardNet& n) { return n.desc && n.packed_bwd && n.act && n.masks && n.grads && n.h_dW && n.h_db; };
  DN_REQUIRE((!((nets & 2) && num_fine > 0) || complete(a.fine)) && (!(nets & 1) || complete(a.coarse)), "%s: a network's buffers are missing", name);
  a.coarse.dist_weight = dist_weight_c; a.fine.dist_weight = dist_weight_f;
  a.precision = precision; a.rays = rays; a.ray_stride = ray_stride; a.n_rays = n_rays;
  a.num_coarse = num_coarse; a.num_fine = num_fine; a.noise_std = noise_std; a.white_background = white_background; a.workspace = workspace;
  a.nets = nets; a.wgrad = true; a.rng_state = rng_state; a.wg_scratch = wg_scratch; a.wg_scratch_bytes = wg_scratch_bytes; a.stream = stream;
  a.reg_workspace = reg_workspace; a.reg2 = reg2;
  return render_rays_backward(a);
}

extern "C" int dn_render_rays_backward_ws(const dn_mlp_desc* desc_coarse, const void* packed_bwd_coarse,
                                          const dn_mlp_desc* desc_fine, const void* packed_bwd_fine, int precision,
                                          const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int num_fine,
                                          float noise_std, int white_background, const float* noise_c, const float* noise_f,
                                          const float* g_rgb_c, const float* g_depth_c, const float* g_acc_c,
                                          const float* g_rgb_f, const float* g_depth_f, const float* g_acc_f, void* workspace,
                                          const void* act_c, const void* masks_c, void* grads_c, const void* act_f,
                                          const void* masks_f, void* grads_f, float* const* h_dW_c, float* const* h_db_c,
                                          float* const* h_dW_f, float* const* h_db_f, int nets, const uint32_t* rng_state,
                                          void* wg_scratch, size_t wg_scratch_bytes, dn_stream_t stream) {
  return render_rays_backward_entry("dn_render_rays_backward", desc_coarse, packed_bwd_coarse, desc_fine, packed_bwd_fine, precision, rays, ray_stride,
                                    n_rays, num_coarse, num_fine, noise_std, white_background, noise_c, noise_f, g_rgb_c, g_depth_c, g_acc_c, g_rgb_f,
                                    g_depth_f, g_acc_f, workspace, act_c, masks_c, grads_c, act_f, masks_f, grads_f, h_dW_c, h_db_c, h_dW_f, h_db_f,
                                    nets, rng_state, wg_scratch, wg_scratch_bytes, 0.0f, 0.0f, nullptr, 0, nullptr, stream);
}

// ---- the same backward with the distortion regulariser (include/dexnerf_hip_ext.h) ---------------------------------------------------------
extern "C" size_t dn_render_reg_workspace_bytes(int64_t n_rays, int num_coarse, int num_fine) {
  if (n_rays < 0 || num_coarse < 1 || num_fine < 0) return 0;
  return carve_reg(nullptr, n_rays, num_coarse, num_fine).bytes;
}

extern "C" int dn_render_rays_backward_reg(const dn_mlp_desc* desc_coarse, const void* packed_bwd_coarse,
                                           const dn_mlp_desc* desc_fine, const void* packed_bwd_fine, int precision,
                                           const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int num_fine,
                                           float noise_std, int white_background, const float* noise_c, const float* noise_f,
                                           const float* g_rgb_c, const float* g_depth_c, const float* g_acc_c,
                                           const float* g_rgb_f, const float* g_depth_f, const float* g_acc_f, void* workspace,
                                           const void* act_c, const void* masks_c, void* grads_c, const void* act_f,
                                           const void* masks_f, void* grads_f, float* const* h_dW_c, float* const* h_db_c,
                                           float* const* h_dW_f, float* const* h_db_f, int nets, const uint32_t* rng_state,
                                           void* wg_scratch, size_t wg_scratch_bytes, float dist_weight_c, float dist_weight_f,
                                           void* reg_workspace, size_t reg_workspace_bytes, float* reg2, dn_stream_t stream) {
  return render_rays_backward_entry("dn_render_rays_backward_reg", desc_coarse, packed_bwd_coarse, desc_fine, packed_bwd_fine, precision, rays,
                                    ray_stride, n_rays, num_coarse, num_fine, noise_std, white_background, noise_c, noise_f, g_rgb_c, g_depth_c,
                                    g_acc_c, g_rgb_f, g_depth_f, g_acc_f, workspace, act_c, masks_c, grads_c, act_f, masks_f, grads_f, h_dW_c,
                                    h_db_c, h_dW_f, h_db_f, nets, rng_state, wg_scratch, wg_scratch_bytes, dist_weight_c, dist_weight_f,
                                    reg_workspace, reg_workspace_bytes, reg2, stream);
}

extern "C" int dn_render_rays_backward(const dn_mlp_desc* desc_coarse, const void* packed_bwd_coarse,
                                       const dn_mlp_desc* desc_fine, const void* packed_bwd_fine, int precision,
                                       const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int num_fine,
                                       float noise_std, int white_background, const float* noise_c, const float* noise_f,
                                       const float* g_rgb_c, const float* g_depth_c, const float* g_acc_c,
                                       const float* g_rgb_f, const float* g_depth_f, const float* g_acc_f, void* workspace,
                                       const void* act_c, const void* masks_c, void* grads_c, const void* act_f,
                                       const void* masks_f, void* grads_f, float* const* h_dW_c, float* const* h_db_c,
                                       float* const* h_dW_f, float* const* h_db_f, int nets, const uint32_t* rng_state,
                                       dn_stream_t stream) {
  return dn_render_rays_backward_ws(desc_coarse, packed_bwd_coarse, desc_fine, packed_bwd_fine, precision, rays, ray_stride, n_rays, num_coarse,
                                    num_fine, noise_std, white_background, noise_c, noise_f, g_rgb_c, g_depth_c, g_acc_c, g_rgb_f, g_depth_f,
                                    g_acc_f, workspace, act_c, masks_c, grads_c, act_f, masks_f, grads_f, h_dW_c, h_db_c, h_dW_f, h_db_f, nets,
                                    rng_state, nullptr, 0, stream);
}

extern "C" size_t dn_render_backward_geom_workspace_bytes(const dn_mlp_desc* desc_coarse, const dn_mlp_desc* desc_fine, int64_t n_rays,
                                                          int ray_stride, int num_coarse, int num_fine) {
  if (!desc_coarse || n_rays < 0 || ray_stride < 8 || num_coarse < 1 || num_fine < 0 || (num_fine > 0 && !desc_fine)) return 0;
  return carve_geom(nullptr, desc_coarse, desc_fine, n_rays, ray_stride, num_coarse, num_fine).bytes;
}

extern "C" int dn_render_rays_backward_geom(const dn_mlp_desc* desc_coarse, const void* packed_bwd_coarse, const void* packed_ig_coarse,
                                            const dn_mlp_desc* desc_fine, const void* packed_bwd_fine, const void* packed_ig_fine,
                                            int precision, const float* rays, int ray_stride, int64_t n_rays, int num_coarse, int num_fine,
                                            int lindisp, int perturb, float noise_std, int white_background, const float* t_rand,
                                            const float* noise_c, const float* noise_f, const float* z_samples, const float* g_rgb_c,
                                            const float* g_depth_c, const float* g_acc_c, const float* g_rgb_f, const float* g_depth_f,
                                            const float* g_acc_f, void* workspace, const void* act_c, const void* masks_c, void* grads_c,
                                            const void* act_f, const void* masks_f, void* grads_f, float* const* h_dW_c, float* const* h_db_c,
                                            float* const* h_dW_f, float* const* h_db_f, const uint32_t* rng_state, void* wg_scratch,
                                            size_t wg_scratch_bytes, void* geom_workspace, size_t geom_workspace_bytes, float* d_rays,
                                            dn_stream_t stream) {
  // every argument is judged before any GPU work
  const bool fine = num_fine > 0;
  DN_REQUIRE(n_rays >= 0 && num_coarse >= 1 && num_fine >= 0 && ray_stride >= 8, "dn_render_rays_backward_geom: bad sizes");
  DN_REQUIRE(desc_coarse && packed_bwd_coarse && packed_ig_coarse && rays && workspace && masks_c && grads_c && d_rays && geom_workspace,
             "dn_render_rays_backward_geom: bad arguments");
  DN_REQUIRE(!fine || (desc_fine && packed_bwd_fine && packed_ig_fine && masks_f && grads_f && z_samples),
             "dn_render_rays_backward_geom: fine pass without the fine net's buffers / z_samples");
  DN_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(geom_workspace)) & 255) == 0,
             "dn_render_rays_backward_geom: workspaces must be 256-byte aligned");
  DN_REQUIRE(wg_scratch != nullptr || wg_scratch_bytes == 0, "dn_render_rays_backward_geom: wg_scratch_bytes without wg_scratch");
  // weight gradients: all four arrays of the networks in use, or none (frozen networks: the weight-gradient launch is skipped)
  const bool wgrad = h_dW_c != nullptr;
  DN_REQUIRE(wgrad == (h_db_c != nullptr) && (!fine || (wgrad == (h_dW_f != nullptr) && wgrad == (h_db_f != nullptr))),
             "dn_render_rays_backward_geom: weight-gradient outputs are given for every network in use, or for none");
  DN_REQUIRE(!wgrad || (act_c && (!fine || act_f)), "dn_render_rays_backward_geom: weight gradients need the saved activations");
  if (precision == DN_PREC_F16 || precision == DN_PREC_BF16_S8) {
    set_error("dn_render_rays_backward_geom: DN_PREC_F32, or DN_PREC_BF16 with 16-bit saved tensors (as dn_mlp_backward_input)");
    return DN_E_UNSUPPORTED;
  }
  DN_REQUIRE(precision == DN_PREC_F32 || precision == DN_PREC_BF16, "dn_render_rays_backward_geom: unknown precision %d", precision);
  const size_t need = dn_render_backward_geom_workspace_bytes(desc_coarse, desc_fine, n_rays, ray_stride, num_coarse, num_fine);
  DN_REQUIRE(geom_workspace_bytes >= need, "dn_render_rays_backward_geom: geom_workspace too small (%zu bytes needed)", need);
  DN_REQUIRE(ray_stride >= (desc_coarse->use_viewdirs || (fine && desc_fine->use_viewdirs) ? 11 : 8),
             "dn_render_rays_backward_geom: ray_stride too small for view directions");
  if (n_rays == 0) return 0;
  RenderBackwardArgs a{};
  a.coarse = BackwardNet{desc_coarse, packed_bwd_coarse, packed_ig_coarse, noise_c, g_rgb_c, g_depth_c, g_acc_c, act_c, masks_c, grads_c, h_dW_c, h_db_c};
  a.fine = BackwardNet{desc_fine, packed_bwd_fine, packed_ig_fine, noise_f, g_rgb_f, g_depth_f, g_acc_f, act_f, masks_f, grads_f, h_dW_f, h_db_f};
  a.precision = precision; a.rays = rays; a.ray_stride = ray_stride; a.n_rays = n_rays; a.num_coarse = num_coarse; a.num_fine = num_fine;
  a.noise_std = noise_std; a.white_background = white_background; a.workspace = workspace;
  a.nets = 3; a.wgrad = wgrad;   // always both chains; the weight gradients all or none
  a.rng_state = rng_state; a.wg_scratch = wg_scratch; a.wg_scratch_bytes = wg_scratch_bytes;
  a.d_rays = d_rays; a.geom_workspace = geom_workspace; a.lindisp = lindisp; a.perturb = perturb; a.t_rand = t_rand; a.z_samples = z_samples;
  a.stream = stream;
  return render_rays_backward(a);
}
