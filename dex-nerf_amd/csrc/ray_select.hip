// Ray generation and training-ray selection (world and NDC rows, one camera or one per ray, given or drawn pixels), the NDC warp,
// ray-row packing, and the backward of ray generation w.r.t. the camera record.  Elementwise kernels; compiled with
// -ffp-contract=off so plain mul/add sequences round like ATen's.
#include "dn_common.h"
#include "dn_rng.h"

namespace dn {

// ------------------------------------------------------------------------------------------------
// S1 get_ray_bundle (reference nerf/nerf_helpers.py:67-112)
// ------------------------------------------------------------------------------------------------
struct RayBundleArgs {
  float cam[15];   // [rinv9, origin3, fx, cx, cy]: a camera record (select_ray_row) handed over by value from the host
  int height, width;
};

static RayBundleArgs ray_bundle_args(int height, int width, const float* h_rinv9, const float* h_origin3, float fx, float cx, float cy) {
  RayBundleArgs a;
  for (int i = 0; i < 9; ++i) a.cam[i] = h_rinv9[i];
  for (int i = 0; i < 3; ++i) a.cam[9 + i] = h_origin3[i];
  a.cam[12] = fx; a.cam[13] = cx; a.cam[14] = cy; a.height = height; a.width = width;
  return a;
}

__global__ void ray_bundle_kernel(RayBundleArgs a, float* __restrict__ ro, float* __restrict__ rd) {
  const int64_t pix = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t total = static_cast<int64_t>(a.height) * a.width;
  if (pix >= total) return;
  const int row = static_cast<int>(pix / a.width);
  const int col = static_cast<int>(pix - static_cast<int64_t>(row) * a.width);
  // dir = [(ii-cx)/fx, (jj-cy)/fx, 1]: fx divides the y term too (nerf_helpers.py:100-101)
  const float d0 = (static_cast<float>(col) - a.cam[13]) / a.cam[12];
  const float d1 = (static_cast<float>(row) - a.cam[14]) / a.cam[12];
  const float d2 = 1.0f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // sum over the last dim of dir[None,:] * Rinv  ->  ((p0 + p1) + p2), products rounded first
    const float p0 = d0 * a.cam[3 * j + 0];
    const float p1 = d1 * a.cam[3 * j + 1];
    const float p2 = d2 * a.cam[3 * j + 2];
    rd[pix * 3 + j] = (p0 + p1) + p2;
    ro[pix * 3 + j] = a.cam[9 + j];
  }
}

// Forward-facing NDC warp of one ray (reference nerf/nerf_helpers.py:172-199), op for op (compiled -ffp-contract=off): the body of
// dn_ndc_rays, and of the NDC selection kernels, whose rows must equal a plain draw followed by dn_ndc_rays bit for bit.
__device__ __forceinline__ void ndc_warp(double h, double w, double focal, double near_d, const float (&o)[3], const float (&d)[3],
                                         float* __restrict__ ro_out, float* __restrict__ rd_out) {
  const float dx = d[0], dy = d[1], dz = d[2];
  const float near = static_cast<float>(near_d);
  const float t = -(near + o[2]) / dz;
  const float ox = o[0] + t * dx, oy = o[1] + t * dy, oz = o[2] + t * dz;
  // python-float constants are computed in double and then meet fp32 tensors as fp32 scalars
  const float cw = static_cast<float>(-1.0 / (w / (2.0 * focal)));
  const float ch = static_cast<float>(-1.0 / (h / (2.0 * focal)));
  const float two_near = static_cast<float>(2.0 * near_d);
  ro_out[0] = cw * ox / oz;
  ro_out[1] = ch * oy / oz;
  ro_out[2] = 1.0f + two_near / oz;
  rd_out[0] = cw * (dx / dz - ox / oz);
  rd_out[1] = ch * (dy / dz - oy / oz);
  rd_out[2] = -two_near / oz;
}

// Training-ray selection (reference train_dexnerf_rgb.py:229-242 + the packing of train_utils.py:225-250): the packed row
// [ro3, rd3, near, far, viewdir3] of ray i (same arithmetic as ray_bundle_kernel for rd; viewdir = rd / ||rd||, train_utils.py:225) -
// pixel `px` of the camera record `cam`, target pixel from that view's image `img` (NULL target: none).  The body of both selection
// kernels - one sequence of fp32 operations (the unit is compiled with -ffp-contract=off), so their rows are bit-identical for the
// same (view, pixel).
// NDC: the origin and direction warped to NDC (ndc_warp with the image's height / width, `focal`, `ndc_near`); the view direction
// (columns 8:11) stays that of the unwarped direction, as in run_one_iter_of_nerf (reference train_utils.py:240-262).
template <bool NDC>
__device__ __forceinline__ void select_ray_row(const float* __restrict__ cam, int height, int width, float near, float far, int64_t px,
                                               const float* __restrict__ img, int channels, float* __restrict__ r, float* __restrict__ tgt,
                                               double focal, double ndc_near) {
  const float fx = cam[12], cx = cam[13], cy = cam[14];
  const int row = static_cast<int>(px / width);
  const int col = static_cast<int>(px - static_cast<int64_t>(row) * width);
  const float d0 = (static_cast<float>(col) - cx) / fx;
  const float d1 = (static_cast<float>(row) - cy) / fx;
  const float d2 = 1.0f;
  float rd[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float p0 = d0 * cam[3 * j + 0];
    const float p1 = d1 * cam[3 * j + 1];
    const float p2 = d2 * cam[3 * j + 2];
    rd[j] = (p0 + p1) + p2;
  }
  const float nrm = sqrtf((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2]);
  if constexpr (NDC) {
    const float o[3] = {cam[9], cam[10], cam[11]};
    ndc_warp(static_cast<double>(height), static_cast<double>(width), focal, ndc_near, o, rd, r, r + 3);
#pragma unroll
    for (int j = 0; j < 3; ++j) r[8 + j] = rd[j] / nrm;
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      r[j] = cam[9 + j];
      r[3 + j] = rd[j];
      r[8 + j] = rd[j] / nrm;
    }
  }
  r[6] = near;
  r[7] = far;
  if (tgt != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) tgt[c] = img[px * channels + c];
  }
}

// The camera constants by value from the host (dn_select_rays): one view, given pixels.
__global__ void select_rays_kernel(RayBundleArgs a, float near, float far, const int64_t* __restrict__ pix, int64_t n,
                                   const float* __restrict__ image, int channels, float* __restrict__ rays,
                                   float* __restrict__ target) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  select_ray_row<false>(a.cam, a.height, a.width, near, far, pix[i], image, channels, rays + i * 11,
                        target != nullptr ? target + i * 3 : nullptr, 0.0, 0.0);
}

// The same with the cameras on the device: `cams` holds one 16-float record per training view [rinv9, origin3, fx, cx, cy, -], so a
// captured HIP graph of the whole training iteration can be replayed for any view (host-side camera constants would be frozen into
// the graph).  Where (view, pixel) of ray i come from - five cases:
//   pix, view          given pixels of the view the device scalar `view` names;
//   pix, view_index    given pixels, every ray its own view (the caller's contract: 0 <= view_index[i] < n_views);
//   drawn, view        the pixels are DRAWN here - element i of this iteration's draw without replacement, a keyed permutation of
//                      the H W pixels (dn_rng.h feistel_permute; reference train_dexnerf_rgb.py:229-236: np.random.choice(H W, n,
//                      replace=False));
//   drawn, no view     the iteration's training view drawn here too (reference: img_idx = np.random.choice(i_train),
//                      train_dexnerf_rgb.py:223), from kRngStreamView;
//   drawn pairs        q = feistel_permute(i, V H W), the same keyed permutation over the pixels of ALL views, view = q / (H W),
//                      pixel = q - view H W: any prefix is a draw without replacement over (view, pixel) pairs, and with one view it
//                      is the drawn-pixels draw.
// A drawing launch is the first kernel of an iteration: it draws from the RNG state's NEXT iteration counter, which thread 0 then
// publishes as the CURRENT one for the rest of the iteration.
struct RaySource {
  const int64_t* pix;      // given pixels; NULL: drawn
  const int* view;         // the device scalar view
  const int* view_index;   // per-ray views of given pixels
  int n_views;
  bool pairs;              // drawn (view, pixel) pairs
  uint32_t* rng_state;
  int64_t* pix_out;        // drawn pixels / views, when wanted
  int* view_out;
};

template <bool NDC>
__global__ void select_rays_device_kernel(const float* __restrict__ cams, RaySource src, int height, int width, float near, float far,
                                          int64_t n, const float* __restrict__ images, int channels, float* __restrict__ rays,
                                          float* __restrict__ target, double focal, double ndc_near) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  uint32_t* const rng_state = src.rng_state;
  uint32_t iteration = 0;
  if (src.pix == nullptr) {
    iteration = rng_state[3];
    if (i == 0) rng_state[2] = iteration;   // (nobody in this launch reads word 2)
  }
  if (i >= n) return;
  const uint32_t per_view = static_cast<uint32_t>(height) * static_cast<uint32_t>(width);
  int v;
  int64_t px;
  if (src.pix != nullptr) {
    v = src.view_index != nullptr ? src.view_index[i] : *src.view;
    px = src.pix[i];
  } else if (src.pairs) {
    const uint32_t q = feistel_permute(static_cast<uint32_t>(i), static_cast<uint32_t>(src.n_views) * per_view, rng_state[0], rng_state[1], iteration);
    v = static_cast<int>(q / per_view);
    px = q - static_cast<uint32_t>(v) * per_view;
    if (src.view_out != nullptr) src.view_out[i] = v;
  } else {
    if (src.view != nullptr) v = *src.view;
    else {
      uint32_t w[4];
      rng_words(rng_state[0], rng_state[1], iteration, kRngStreamView, 0, w);
      v = static_cast<int>(w[0] % static_cast<uint32_t>(src.n_views));
    }
    px = feistel_permute(static_cast<uint32_t>(i), per_view, rng_state[0], rng_state[1], iteration);
  }
  if (src.pix == nullptr && src.pix_out != nullptr) src.pix_out[i] = px;
  select_ray_row<NDC>(cams + static_cast<int64_t>(v) * 16, height, width, near, far, px,
                      target != nullptr ? images + static_cast<int64_t>(v) * height * width * channels : nullptr, channels, rays + i * 11,
                      target != nullptr ? target + i * 3 : nullptr, focal, ndc_near);
}

// Forward-facing NDC warp (reference nerf/nerf_helpers.py:172-199), op for op (compiled -ffp-contract=off).
__global__ void ndc_rays_kernel(double h, double w, double focal, double near_d, const float* __restrict__ ro,
                                const float* __restrict__ rd, int64_t n, float* __restrict__ ro_out,
                                float* __restrict__ rd_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float o[3] = {ro[i * 3 + 0], ro[i * 3 + 1], ro[i * 3 + 2]};
  const float d[3] = {rd[i * 3 + 0], rd[i * 3 + 1], rd[i * 3 + 2]};
  ndc_warp(h, w, focal, near_d, o, d, ro_out + i * 3, rd_out + i * 3);
}

// Backward of ray generation w.r.t. the camera: the 16-float record [rinv9, origin3, fx, cx, cy, ndc_focal] of ray_bundle_kernel /
// select_rays*_kernel receives the gradient of the rays' origins, directions and unit view directions (NDC: of the warped origins /
// directions of ndc_warp, the view directions those of the unwarped directions).  Per ray, in fp64 from the fp32 record and the integer
// pixel: d = [(col - cx) / fx, (row - cy) / fx, 1], rd_j = sum_k d_k rinv[3j + k], v = rd / |rd|;
//   NDC: (g_o', g_d') pulled back through the six expressions of ndc_warp and the shift o + t rd to (g_o, g_d); o'_{0,1}, d'_{0,1} are
//        linear in the focal length, so g_focal = (g_o'_0 o'_0 + g_o'_1 o'_1 + g_d'_0 d'_0 + g_d'_1 d'_1) / focal;
//   g_d += (g_v - v (v . g_v)) / |rd|;
//   g_origin += g_o, g_rinv[3j + k] += g_d[j] d_k, e_k = sum_j g_d[j] rinv[3j + k], g_cx -= e_0 / fx, g_cy -= e_1 / fx,
//   g_fx -= (e_0 d_0 + e_1 d_1) / fx.
// The sums are formed in a fixed order: a lane adds its rays (thread index, then strides of the whole grid) in ascending order, the
// lanes of a wave meet in wave_sum's butterfly, the waves of a workgroup through LDS in wave order, and each workgroup stores 16
// doubles; camera_grad_finish_kernel adds those in workgroup order.  The grid is a function of n alone (camera_grad_blocks): plain
// stores, bit-reproducible on any device.
constexpr int kCamGradThreads = 256;
constexpr int kCamGradMaxBlocks = 64;

static int camera_grad_blocks(int64_t n) {
  const int64_t blocks = (n + kCamGradThreads - 1) / kCamGradThreads;
  return static_cast<int>(blocks < kCamGradMaxBlocks ? blocks : kCamGradMaxBlocks);
}

// The camera record in fp64 and the two NDC scales: what every ray of one camera shares.
struct CamGradCamera {
  double rinv[9], origin[3], fx, cx, cy, sx, sy;
};

__device__ __forceinline__ CamGradCamera camera_grad_load(const float* __restrict__ cam, int width, double height_d, double ndc_focal) {
  CamGradCamera c;
#pragma unroll
  for (int k = 0; k < 9; ++k) c.rinv[k] = static_cast<double>(cam[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) c.origin[k] = static_cast<double>(cam[9 + k]);
  c.fx = static_cast<double>(cam[12]);
  c.cx = static_cast<double>(cam[13]);
  c.cy = static_cast<double>(cam[14]);
  c.sx = -1.0 / (static_cast<double>(width) / (2.0 * ndc_focal));
  c.sy = -1.0 / (height_d / (2.0 * ndc_focal));
  return c;
}

// The Jacobian of ray i (pixel px of camera c) applied to its upstream gradients, added to the 16 sums of the record's gradient:
// the one statement of the formulas above, shared by camera_grad_kernel and camera_grad_views_kernel.
__device__ __forceinline__ void camera_grad_ray(const CamGradCamera& c, int width, int64_t px, int64_t i, const float* __restrict__ g_ro,
                                                int ro_stride, const float* __restrict__ g_rd, int rd_stride, const float* __restrict__ g_vd,
                                                int vd_stride, bool ndc, double ndc_focal, double ndc_near, double (&acc)[16]) {
  const double* rinv = c.rinv;
  const double* origin = c.origin;
  const double fx = c.fx, cx = c.cx, cy = c.cy, sx = c.sx, sy = c.sy;
  const int64_t row = px / width;
  const int64_t col = px - row * width;
  const double d[3] = {(static_cast<double>(col) - cx) / fx, (static_cast<double>(row) - cy) / fx, 1.0};
  double rd[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) rd[j] = (d[0] * rinv[3 * j + 0] + d[1] * rinv[3 * j + 1]) + d[2] * rinv[3 * j + 2];
  double go[3] = {0.0, 0.0, 0.0}, gd[3] = {0.0, 0.0, 0.0};
  if (g_ro != nullptr) {
#pragma unroll
    for (int j = 0; j < 3; ++j) go[j] = static_cast<double>(g_ro[i * ro_stride + j]);
  }
  if (g_rd != nullptr) {
#pragma unroll
    for (int j = 0; j < 3; ++j) gd[j] = static_cast<double>(g_rd[i * rd_stride + j]);
  }
  if (ndc) {
    // forward: t = -(near + o_z) / rd_z, p = o + t rd, o' = [sx p0 / p2, sy p1 / p2, 1 + 2 near / p2],
    //          d' = [sx (rd0 / rd2 - p0 / p2), sy (rd1 / rd2 - p1 / p2), -2 near / p2]
    const double t = -(ndc_near + origin[2]) / rd[2];
    const double p[3] = {origin[0] + t * rd[0], origin[1] + t * rd[1], origin[2] + t * rd[2]};
    const double ip = 1.0 / p[2], iz = 1.0 / rd[2];
    const double o0 = sx * p[0] * ip, o1 = sy * p[1] * ip;
    const double w0 = sx * (rd[0] * iz - p[0] * ip), w1 = sy * (rd[1] * iz - p[1] * ip);
    acc[15] += (go[0] * o0 + go[1] * o1 + gd[0] * w0 + gd[1] * w1) / ndc_focal;
    const double a0 = go[0] - gd[0], a1 = go[1] - gd[1];
    double gp[3];
    gp[0] = sx * ip * a0;
    gp[1] = sy * ip * a1;
    gp[2] = -(sx * p[0] * a0 + sy * p[1] * a1) * ip * ip + 2.0 * ndc_near * ip * ip * (gd[2] - go[2]);
    double gr[3];
    gr[0] = sx * iz * gd[0];
    gr[1] = sy * iz * gd[1];
    gr[2] = -(sx * rd[0] * gd[0] + sy * rd[1] * gd[1]) * iz * iz;
    const double gt = gp[0] * rd[0] + gp[1] * rd[1] + gp[2] * rd[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      go[j] = gp[j];
      gd[j] = gr[j] + t * gp[j];
    }
    go[2] -= gt * iz;
    gd[2] -= gt * t * iz;
  }
  if (g_vd != nullptr) {
    const double gv[3] = {static_cast<double>(g_vd[i * vd_stride + 0]), static_cast<double>(g_vd[i * vd_stride + 1]),
                          static_cast<double>(g_vd[i * vd_stride + 2])};
    const double inv_nrm = 1.0 / sqrt((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2]);
    const double v[3] = {rd[0] * inv_nrm, rd[1] * inv_nrm, rd[2] * inv_nrm};
    const double vg = (v[0] * gv[0] + v[1] * gv[1]) + v[2] * gv[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) gd[j] += (gv[j] - v[j] * vg) * inv_nrm;
  }
  double e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) e[k] = (gd[0] * rinv[k] + gd[1] * rinv[3 + k]) + gd[2] * rinv[6 + k];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    acc[9 + j] += go[j];
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[3 * j + k] += gd[j] * d[k];
  }
  acc[12] -= (e[0] * d[0] + e[1] * d[1]) / fx;
  acc[13] -= e[0] / fx;
  acc[14] -= e[1] / fx;
}

// The 16 sums of a workgroup: wave_sum's butterfly, the waves through LDS in wave order, 16 doubles stored.  Every thread of the
// workgroup calls it (it holds a barrier).
__device__ __forceinline__ void camera_grad_block_store(const double (&acc)[16], double* __restrict__ out16) {
  __shared__ double part[kCamGradThreads / 64][16];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane_id() == 0) part[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    double s = part[0][threadIdx.x];
    for (int w = 1; w < kCamGradThreads / 64; ++w) s += part[w][threadIdx.x];
    out16[threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(kCamGradThreads) void camera_grad_kernel(const float* __restrict__ cam, int width, const int64_t* __restrict__ pix,
                                                                      int64_t n, const float* __restrict__ g_ro, int ro_stride,
                                                                      const float* __restrict__ g_rd, int rd_stride,
                                                                      const float* __restrict__ g_vd, int vd_stride, double height_d,
                                                                      double ndc_focal, double ndc_near, double* __restrict__ partials) {
  const CamGradCamera c = camera_grad_load(cam, width, height_d, ndc_focal);
  const bool ndc = ndc_focal > 0.0;
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kCamGradThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kCamGradThreads + threadIdx.x; i < n; i += step) {
    const int64_t px = (pix != nullptr) ? pix[i] : i;
    camera_grad_ray(c, width, px, i, g_ro, ro_stride, g_rd, rd_stride, g_vd, vd_stride, ndc, ndc_focal, ndc_near, acc);
  }
  camera_grad_block_store(acc, partials + static_cast<int64_t>(blockIdx.x) * 16);
}

// Mixed-camera batches: workgroup (b, v) of a (camera_grad_blocks(n), V) grid walks the rays in camera_grad_kernel's order and adds
// those of view v (the others are skipped: the 4-byte view index of every ray is read once per view), then stores its 16 sums at
// partials[(v blocks + b) 16]; camera_grad_finish_kernel, one workgroup per view, adds a view's partials in workgroup order.  The
// order of every sum is a function of (n, V) and the view indices alone: plain stores, bit-reproducible on any device.
__global__ __launch_bounds__(kCamGradThreads) void camera_grad_views_kernel(const float* __restrict__ cams, int width, const int* __restrict__ view_index,
                                                                            const int64_t* __restrict__ pix, int64_t n,
                                                                            const float* __restrict__ g_ro, int ro_stride,
                                                                            const float* __restrict__ g_rd, int rd_stride,
                                                                            const float* __restrict__ g_vd, int vd_stride, double height_d,
                                                                            double ndc_focal, double ndc_near, double* __restrict__ partials) {
  const int view = static_cast<int>(blockIdx.y);
  const CamGradCamera c = camera_grad_load(cams + static_cast<int64_t>(view) * 16, width, height_d, ndc_focal);
  const bool ndc = ndc_focal > 0.0;
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kCamGradThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kCamGradThreads + threadIdx.x; i < n; i += step) {
    if (view_index[i] != view) continue;
    camera_grad_ray(c, width, pix[i], i, g_ro, ro_stride, g_rd, rd_stride, g_vd, vd_stride, ndc, ndc_focal, ndc_near, acc);
  }
  camera_grad_block_store(acc, partials + (static_cast<int64_t>(view) * gridDim.x + blockIdx.x) * 16);
}

// Workgroup v adds the n_blocks partials of record v in workgroup order (dn_camera_grad: one record, one workgroup).
__global__ __launch_bounds__(64) void camera_grad_finish_kernel(const double* __restrict__ partials, int n_blocks, float* __restrict__ g_cam) {
  if (threadIdx.x >= 16) return;
  const double* mine = partials + static_cast<int64_t>(blockIdx.x) * n_blocks * 16;
  double s = 0.0;
  for (int b = 0; b < n_blocks; ++b) s += mine[b * 16 + threadIdx.x];
  g_cam[static_cast<int64_t>(blockIdx.x) * 16 + threadIdx.x] = static_cast<float>(s);
}

}  // namespace dn

using namespace dn;

extern "C" int dn_ray_bundle(int height, int width, const float* h_rinv9, const float* h_origin3, float fx, float cx,
                             float cy, float* ro, float* rd, dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && h_rinv9 && h_origin3 && ro && rd, "dn_ray_bundle: bad arguments");
  const int64_t total = static_cast<int64_t>(height) * width;
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((total + block - 1) / block);
  hipLaunchKernelGGL(ray_bundle_kernel, dim3(grid), dim3(block), 0, as_stream(stream),
                     ray_bundle_args(height, width, h_rinv9, h_origin3, fx, cx, cy), ro, rd);
  return check_launch("dn_ray_bundle");
}

extern "C" int dn_select_rays(int height, int width, const float* h_rinv9, const float* h_origin3, float fx, float cx,
                              float cy, float near, float far, const int64_t* pixel_index, int64_t n_rays,
                              const float* image, int channels, float* rays, float* target, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(height > 0 && width > 0 && h_rinv9 && h_origin3 && pixel_index && rays && n_rays >= 0,
             "dn_select_rays: bad arguments");
  DN_REQUIRE(target == nullptr || (image != nullptr && channels >= 3), "dn_select_rays: target requested without an image of >= 3 channels");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(select_rays_kernel, dim3(grid), dim3(block), 0, as_stream(stream),
                     ray_bundle_args(height, width, h_rinv9, h_origin3, fx, cx, cy), near, far, pixel_index, n_rays, image, channels, rays,
                     target);
  return check_launch("dn_select_rays");
}

// What the six device-camera entry points share (`name`: theirs, for messages): the target check, the grid, and the NDC
// (ndc_focal > 0) or world instance of select_rays_device_kernel.  Each entry point judges what is its own first.
static int launch_select_rays(const char* name, int height, int width, const float* cams, const RaySource& src, float near, float far,
                              int64_t n_rays, const float* images, int channels, float* rays, float* target, double ndc_focal,
                              double ndc_near, dn_stream_t stream) {
  DN_REQUIRE(target == nullptr || (images != nullptr && channels >= 3), "%s: target requested without images of >= 3 channels", name);
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(ndc_focal > 0.0 ? select_rays_device_kernel<true> : select_rays_device_kernel<false>, dim3(grid), dim3(block), 0,
                     as_stream(stream), cams, src, height, width, near, far, n_rays, images, channels, rays, target, ndc_focal, ndc_near);
  return check_launch(name);
}

static RaySource given_pixels(const int64_t* pixel_index, const int32_t* view, const int32_t* view_index, int n_views) {
  return RaySource{pixel_index, view, view_index, n_views, false, nullptr, nullptr, nullptr};
}

static RaySource drawn_pixels(uint32_t* rng_state, const int32_t* view, int n_views, bool pairs, int64_t* pixel_index_out, int32_t* view_index_out) {
  return RaySource{nullptr, view, nullptr, n_views, pairs, rng_state, pixel_index_out, view_index_out};
}

extern "C" int dn_select_rays_indirect(int height, int width, const float* cams, const int32_t* view, float near,
                                       float far, const int64_t* pixel_index, int64_t n_rays, const float* images,
                                       int channels, float* rays, float* target, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(height > 0 && width > 0 && cams && view && pixel_index && rays && n_rays >= 0, "dn_select_rays_indirect: bad arguments");
  return launch_select_rays("dn_select_rays_indirect", height, width, cams, given_pixels(pixel_index, view, nullptr, 0), near, far, n_rays, images,
                            channels, rays, target, 0.0, 0.0, stream);
}

extern "C" int dn_select_rays_indirect_ndc(int height, int width, const float* cams, const int32_t* view, float near, float far,
                                           const int64_t* pixel_index, int64_t n_rays, const float* images, int channels, float* rays,
                                           float* target, double focal, double ndc_near, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(height > 0 && width > 0 && cams && view && pixel_index && rays && n_rays >= 0, "dn_select_rays_indirect_ndc: bad arguments");
  DN_REQUIRE(std::isfinite(focal) && focal > 0.0 && std::isfinite(ndc_near), "dn_select_rays_indirect_ndc: focal must be positive and finite, the near plane finite");
  return launch_select_rays("dn_select_rays_indirect_ndc", height, width, cams, given_pixels(pixel_index, view, nullptr, 0), near, far, n_rays,
                            images, channels, rays, target, focal, ndc_near, stream);
}

extern "C" size_t dn_camera_grad_scratch_bytes(int64_t n_rays) {
  const int blocks = camera_grad_blocks(n_rays > 0 ? n_rays : 0);
  return static_cast<size_t>(blocks > 0 ? blocks : 1) * 16 * sizeof(double);
}

extern "C" int dn_camera_grad(int height, int width, const float* cam16, const int64_t* pixel_index, int64_t n_rays, const float* g_ro,
                              int ro_stride, const float* g_rd, int rd_stride, const float* g_viewdir, int vd_stride, double ndc_focal,
                              double ndc_near, void* scratch, size_t scratch_bytes, float* g_cam16, dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && n_rays >= 0, "dn_camera_grad: bad arguments (image size, ray count)");
  DN_REQUIRE(cam16 != nullptr && g_cam16 != nullptr, "dn_camera_grad: the camera record and its gradient must be given");
  DN_REQUIRE(g_ro != nullptr || g_rd != nullptr || g_viewdir != nullptr, "dn_camera_grad: no upstream gradient given");
  DN_REQUIRE((g_ro == nullptr || ro_stride >= 3) && (g_rd == nullptr || rd_stride >= 3) && (g_viewdir == nullptr || vd_stride >= 3),
             "dn_camera_grad: the row stride of an upstream gradient must be >= 3 floats");
  DN_REQUIRE(static_cast<int64_t>(height) * width < (1LL << 31), "dn_camera_grad: image too large");
  DN_REQUIRE(pixel_index != nullptr || n_rays <= static_cast<int64_t>(height) * width, "dn_camera_grad: more rays than pixels without a pixel index");
  DN_REQUIRE(std::isfinite(ndc_focal) && ndc_focal >= 0.0 && std::isfinite(ndc_near),
             "dn_camera_grad: ndc_focal must be finite and >= 0 (0: world-space rays), the near plane finite");
  DN_REQUIRE(scratch != nullptr && scratch_bytes >= dn_camera_grad_scratch_bytes(n_rays),
             "dn_camera_grad: scratch smaller than dn_camera_grad_scratch_bytes(n_rays)");
  DN_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 8 == 0, "dn_camera_grad: scratch must be 8-byte aligned");
  const int blocks = camera_grad_blocks(n_rays);
  double* partials = static_cast<double*>(scratch);
  if (blocks > 0) {
    hipLaunchKernelGGL(camera_grad_kernel, dim3(blocks), dim3(kCamGradThreads), 0, as_stream(stream), cam16, width, pixel_index, n_rays, g_ro,
                       ro_stride, g_rd, rd_stride, g_viewdir, vd_stride, static_cast<double>(height), ndc_focal, ndc_near, partials);
    const int rc = check_launch("dn_camera_grad");
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(camera_grad_finish_kernel, dim3(1), dim3(64), 0, as_stream(stream), partials, blocks, g_cam16);   // (no rays: 16 zeros)
  return check_launch("dn_camera_grad");
}

extern "C" int dn_select_rays_draw(int height, int width, const float* cams, const int32_t* view, int n_views, float near, float far,
                                   uint32_t* rng_state, int64_t n_rays, const float* images, int channels, float* rays, float* target,
                                   int64_t* pixel_index_out, dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && cams && (view || n_views >= 1) && rng_state && rays && n_rays >= 1, "dn_select_rays_draw: bad arguments");
  DN_REQUIRE(n_rays <= static_cast<int64_t>(height) * width, "dn_select_rays_draw: more rays than pixels (the draw is without replacement)");
  DN_REQUIRE(static_cast<int64_t>(height) * width < (1LL << 31), "dn_select_rays_draw: image too large");
  return launch_select_rays("dn_select_rays_draw", height, width, cams, drawn_pixels(rng_state, view, n_views, false, pixel_index_out, nullptr), near,
                            far, n_rays, images, channels, rays, target, 0.0, 0.0, stream);
}

extern "C" int dn_select_rays_draw_ndc(int height, int width, const float* cams, const int32_t* view, int n_views, float near, float far,
                                       uint32_t* rng_state, int64_t n_rays, const float* images, int channels, float* rays, float* target,
                                       int64_t* pixel_index_out, double focal, double ndc_near, dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && cams && (view || n_views >= 1) && rng_state && rays && n_rays >= 1, "dn_select_rays_draw_ndc: bad arguments");
  DN_REQUIRE(n_rays <= static_cast<int64_t>(height) * width, "dn_select_rays_draw_ndc: more rays than pixels (the draw is without replacement)");
  DN_REQUIRE(static_cast<int64_t>(height) * width < (1LL << 31), "dn_select_rays_draw_ndc: image too large");
  DN_REQUIRE(std::isfinite(focal) && focal > 0.0 && std::isfinite(ndc_near), "dn_select_rays_draw_ndc: focal must be positive and finite, the near plane finite");
  return launch_select_rays("dn_select_rays_draw_ndc", height, width, cams, drawn_pixels(rng_state, view, n_views, false, pixel_index_out, nullptr),
                            near, far, n_rays, images, channels, rays, target, focal, ndc_near, stream);
}

extern "C" int dn_select_rays_views(int height, int width, const float* cams, int n_views, const int32_t* view_index, float near, float far,
                                    const int64_t* pixel_index, int64_t n_rays, const float* images, int channels, float* rays, float* target,
                                    double ndc_focal, double ndc_near, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(height > 0 && width > 0 && rays && n_rays >= 0, "dn_select_rays_views: bad arguments (image size, ray count, rows)");
  DN_REQUIRE(cams != nullptr && n_views >= 1, "dn_select_rays_views: the camera records (n_views >= 1) must be given");
  DN_REQUIRE(view_index != nullptr && pixel_index != nullptr, "dn_select_rays_views: view_index and pixel_index must be given");
  DN_REQUIRE(static_cast<int64_t>(n_views) * height * width < (1LL << 31), "dn_select_rays_views: n_views x image too large (V H W must be < 2^31)");
  DN_REQUIRE(std::isfinite(ndc_focal) && ndc_focal >= 0.0 && std::isfinite(ndc_near),
             "dn_select_rays_views: ndc_focal must be finite and >= 0 (0: world-space rays), the near plane finite");
  return launch_select_rays("dn_select_rays_views", height, width, cams, given_pixels(pixel_index, nullptr, view_index, n_views), near, far, n_rays,
                            images, channels, rays, target, ndc_focal, ndc_near, stream);
}

extern "C" int dn_select_rays_draw_views(int height, int width, const float* cams, int n_views, float near, float far, uint32_t* rng_state,
                                         int64_t n_rays, const float* images, int channels, float* rays, float* target,
                                         int64_t* pixel_index_out, int32_t* view_index_out, double ndc_focal, double ndc_near, dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && rng_state && rays, "dn_select_rays_draw_views: bad arguments (image size, RNG state, rows)");
  DN_REQUIRE(cams != nullptr && n_views >= 1, "dn_select_rays_draw_views: the camera records (n_views >= 1) must be given");
  DN_REQUIRE(static_cast<int64_t>(n_views) * height * width < (1LL << 31), "dn_select_rays_draw_views: n_views x image too large (V H W must be < 2^31)");
  DN_REQUIRE(n_rays >= 1 && n_rays <= static_cast<int64_t>(n_views) * height * width,
             "dn_select_rays_draw_views: need 1 <= n_rays <= V H W (the draw is without replacement)");
  DN_REQUIRE(std::isfinite(ndc_focal) && ndc_focal >= 0.0 && std::isfinite(ndc_near),
             "dn_select_rays_draw_views: ndc_focal must be finite and >= 0 (0: world-space rays), the near plane finite");
  return launch_select_rays("dn_select_rays_draw_views", height, width, cams, drawn_pixels(rng_state, nullptr, n_views, true, pixel_index_out, view_index_out),
                            near, far, n_rays, images, channels, rays, target, ndc_focal, ndc_near, stream);
}

extern "C" size_t dn_camera_grad_views_scratch_bytes(int64_t n_rays, int n_views) {
  const int blocks = camera_grad_blocks(n_rays > 0 ? n_rays : 0);
  return static_cast<size_t>(blocks > 0 ? blocks : 1) * static_cast<size_t>(n_views > 0 ? n_views : 1) * 16 * sizeof(double);
}

extern "C" int dn_camera_grad_views(int height, int width, const float* cams, int n_views, const int32_t* view_index, const int64_t* pixel_index,
                                    int64_t n_rays, const float* g_ro, int ro_stride, const float* g_rd, int rd_stride, const float* g_viewdir,
                                    int vd_stride, double ndc_focal, double ndc_near, void* scratch, size_t scratch_bytes, float* g_cams,
                                    dn_stream_t stream) {
  DN_REQUIRE(height > 0 && width > 0 && n_rays >= 0, "dn_camera_grad_views: bad arguments (image size, ray count)");
  DN_REQUIRE(cams != nullptr && g_cams != nullptr, "dn_camera_grad_views: the camera records and their gradient must be given");
  DN_REQUIRE(n_views >= 1 && n_views <= 65535, "dn_camera_grad_views: n_views must be in [1, 65535]");
  DN_REQUIRE(view_index != nullptr && pixel_index != nullptr, "dn_camera_grad_views: view_index and pixel_index must be given");
  DN_REQUIRE(g_ro != nullptr || g_rd != nullptr || g_viewdir != nullptr, "dn_camera_grad_views: no upstream gradient given");
  DN_REQUIRE((g_ro == nullptr || ro_stride >= 3) && (g_rd == nullptr || rd_stride >= 3) && (g_viewdir == nullptr || vd_stride >= 3),
             "dn_camera_grad_views: the row stride of an upstream gradient must be >= 3 floats");
  DN_REQUIRE(static_cast<int64_t>(n_views) * height * width < (1LL << 31), "dn_camera_grad_views: n_views x image too large (V H W must be < 2^31)");
  DN_REQUIRE(std::isfinite(ndc_focal) && ndc_focal >= 0.0 && std::isfinite(ndc_near),
             "dn_camera_grad_views: ndc_focal must be finite and >= 0 (0: world-space rays), the near plane finite");
  DN_REQUIRE(scratch != nullptr && scratch_bytes >= dn_camera_grad_views_scratch_bytes(n_rays, n_views),
             "dn_camera_grad_views: scratch smaller than dn_camera_grad_views_scratch_bytes(n_rays, n_views)");
  DN_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 8 == 0, "dn_camera_grad_views: scratch must be 8-byte aligned");
  const int blocks = camera_grad_blocks(n_rays);
  double* partials = static_cast<double*>(scratch);
  if (blocks > 0) {
    hipLaunchKernelGGL(camera_grad_views_kernel, dim3(blocks, n_views), dim3(kCamGradThreads), 0, as_stream(stream), cams, width, view_index,
                       pixel_index, n_rays, g_ro, ro_stride, g_rd, rd_stride, g_viewdir, vd_stride, static_cast<double>(height), ndc_focal,
                       ndc_near, partials);
    const int rc = check_launch("dn_camera_grad_views");
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(camera_grad_finish_kernel, dim3(n_views), dim3(64), 0, as_stream(stream), partials, blocks, g_cams);   // (no rays: V x 16 zeros)
  return check_launch("dn_camera_grad_views");
}

// ---- S2 ray packing of run_one_iter_of_nerf (nerf/train_utils.py:220-250): (N,3) origins / directions -> the (N, 8 | 11) rows
// [o, d, near, far, d_view / |d_view|] predict_and_render_radiance reads - the reference forms them with a norm, a division, two
// ones_like, two multiplies and a cat (eight launches per image); op for op as those run on the device.
namespace dn {
__global__ void pack_ray_rows_kernel(const float* __restrict__ ro, const float* __restrict__ rd, const float* __restrict__ rd_view,
                                     float near, float far, int64_t n, float* __restrict__ rows) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float* r = rows + i * (rd_view != nullptr ? 11 : 8);
#pragma unroll
  for (int j = 0; j < 3; ++j) { r[j] = ro[i * 3 + j]; r[3 + j] = rd[i * 3 + j]; }
  r[6] = near;
  r[7] = far;
  if (rd_view != nullptr) {
    const float x = rd_view[i * 3], y = rd_view[i * 3 + 1], z = rd_view[i * 3 + 2];
    // the order of torch's device reduction over three elements ((x x + z z) + y y: measured, scripts/rows_diag.py) - this kernel
    // replaces torch ops that ran on the device, and the rows stay bit-identical to them
    const float nrm = sqrtf((x * x + z * z) + y * y);
    r[8] = x / nrm; r[9] = y / nrm; r[10] = z / nrm;
  }
}
}  // namespace dn

extern "C" int dn_pack_ray_rows(const float* rays_o, const float* rays_d, const float* view_d, float near, float far, int64_t n_rays,
                                float* rows, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(rays_o && rays_d && rows && n_rays >= 0, "dn_pack_ray_rows: bad arguments");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(pack_ray_rows_kernel, dim3(grid), dim3(block), 0, as_stream(stream), rays_o, rays_d, view_d, near, far, n_rays, rows);
  return check_launch("dn_pack_ray_rows");
}

extern "C" int dn_ndc_rays(int height, int width, double focal, double near, const float* rays_o, const float* rays_d,
                           int64_t n_rays, float* rays_o_out, float* rays_d_out, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(rays_o && rays_d && rays_o_out && rays_d_out && n_rays >= 0 && height > 0 && width > 0, "dn_ndc_rays: bad arguments");
  const int block = 256;
  const unsigned grid = static_cast<unsigned>((n_rays + block - 1) / block);
  hipLaunchKernelGGL(ndc_rays_kernel, dim3(grid), dim3(block), 0, as_stream(stream), static_cast<double>(height),
                     static_cast<double>(width), focal, near, rays_o, rays_d, n_rays, rays_o_out, rays_d_out);
  return check_launch("dn_ndc_rays");
}
