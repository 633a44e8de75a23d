// Camera records from twists, on the device: xi = (omega, t) -> E = exp(twist(xi)) E0 -> the 16-float record of the ray kernels
// [rinv9, origin3, fx, cx, cy, ndc_focal], and the exact derivative of that map (pose refinement with nothing on the host:
// nerf/pose.py se3_exp + _ops.camera_record are the host forms).  One thread per view, everything in fp64 from the fp32 inputs,
// rounded once to fp32.
//
//   K = [omega]x, s = |omega|^2,  exp(twist) = [R, W t; 0, 1],  R = I + A K + B K^2,  W = I + B K + C K^2,
//   A = sin(th) / th, B = (1 - cos(th)) / th^2, C = (th - sin(th)) / th^3  (th = sqrt(s)),
//   M = R R0, p = R t0 + W t, rinv = adj(M) / det(M) (no rigidity assumed, as camera_record's torch.inverse), origin = -rinv p.
// A, B, C and their derivatives in s are entire functions of s: below s = 1e-2 they are summed as series (nine terms: the first
// neglected one is < 1e-24), where the closed forms cancel; above, the closed forms are accurate to a few ulp.
//
// Intrinsics (dn_camera_records and its backward; dn_pose_records copies K0's three entries): per refined camera phi = (a, b, c) fp32,
// K0 the given matrix, s > 0 the caller's intrinsics_scale,
//   fx = fx0 exp(s a),  cx = cx0 + s fx0 b,  cy = cy0 + s fx0 c   (fx0 = K0[0,0], cx0 = K0[0,2], cy0 = K0[1,2]),
// one focal length (fx also divides the y term of the ray kernels), all three components dimensionless and of a rotation's size: a
// principal-point shift of fx0 delta pixels looks like a rotation by delta, so one Adam with one lr drives twists and phi.  fp64 from
// the fp32 inputs, rounded once: at phi = 0 the record is dn_pose_records' bit for bit.  One phi (3) shared by all views or phi (V,3).
//   g_a = s fx g_fx,  g_b = s fx0 g_cx,  g_c = s fx0 g_cy  per view in fp64; a shared phi's gradient is their sum over the views added
// in view order v = 0 .. V-1 in fp64 by one thread per component - plain stores, no atomics, the order a function of V alone (never
// of the grid or the CU count).  The NDC warp's focal length is a constant of the scene's parameterisation (the selection and gradient
// kernels take it as a host scalar, the networks were trained in that warped space): slot 15 of g_cams stays ignored.
#include "dn_common.h"

namespace dn {

struct ExpCoef {
  double a, b, c;      // A, B, C
  double da, db, dc;   // dA/ds, dB/ds, dC/ds
};

__device__ inline ExpCoef exp_coefficients(double s) {
  ExpCoef e;
  if (s < 1e-2) {
    // A = sum (-s)^n / (2n+1)!, B = sum (-s)^n / (2n+2)!, C = sum (-s)^n / (2n+3)!; term-by-term derivatives
    double a = 0.0, b = 0.0, c = 0.0, da = 0.0, db = 0.0, dc = 0.0;
    double pw = 1.0, pw_prev = 0.0;   // (-s)^n and n (-1)^n s^(n-1)
    double fact = 1.0;                // (2n+1)!
    for (int n = 0; n < 9; ++n) {
      const double k1 = 2.0 * n + 1.0;
      if (n > 0) fact *= (k1 - 1.0) * k1;
      const double fa = fact, fb = fact * (k1 + 1.0), fc = fb * (k1 + 2.0);
      a += pw / fa; b += pw / fb; c += pw / fc;
      da += pw_prev / fa; db += pw_prev / fb; dc += pw_prev / fc;
      // next n: d/ds (-s)^(n+1) = -(n+1) (-s)^n
      pw_prev = -(n + 1.0) * pw;
      pw *= -s;
    }
    e.a = a; e.b = b; e.c = c; e.da = da; e.db = db; e.dc = dc;
    return e;
  }
  const double th = sqrt(s), sn = sin(th), cs = cos(th);
  e.a = sn / th;
  e.b = (1.0 - cs) / s;
  e.c = (1.0 - e.a) / s;
  e.da = (cs - e.a) / (2.0 * s);
  e.db = (0.5 * e.a - e.b) / s;
  e.dc = (-e.da - e.c) / s;
  return e;
}

struct PoseTerms {
  double K[3][3], K2[3][3], R[3][3], W[3][3];
  double M[3][3], p[3], rinv[3][3];
  ExpCoef e;
};

__device__ inline void mat3_mul(const double (&x)[3][3], const double (&y)[3][3], double (&out)[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out[i][j] = x[i][0] * y[0][j] + x[i][1] * y[1][j] + x[i][2] * y[2][j];
}

__device__ inline void pose_terms(const float* __restrict__ xi, const float* __restrict__ e0, PoseTerms& t) {
  const double wx = xi[0], wy = xi[1], wz = xi[2];
  const double tv[3] = {static_cast<double>(xi[3]), static_cast<double>(xi[4]), static_cast<double>(xi[5])};
  const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) t.K[i][j] = K[i][j];
  mat3_mul(t.K, t.K, t.K2);
  t.e = exp_coefficients((wx * wx + wy * wy) + wz * wz);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double id = (i == j) ? 1.0 : 0.0;
      t.R[i][j] = id + t.e.a * t.K[i][j] + t.e.b * t.K2[i][j];
      t.W[i][j] = id + t.e.b * t.K[i][j] + t.e.c * t.K2[i][j];
    }
  double R0[3][3], t0[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R0[i][j] = e0[4 * i + j];
    t0[i] = e0[4 * i + 3];
  }
  mat3_mul(t.R, R0, t.M);
  for (int i = 0; i < 3; ++i)
    t.p[i] = (t.R[i][0] * t0[0] + t.R[i][1] * t0[1] + t.R[i][2] * t0[2]) + (t.W[i][0] * tv[0] + t.W[i][1] * tv[1] + t.W[i][2] * tv[2]);
  // inverse by adjugate / determinant
  const double (&m)[3][3] = t.M;
  const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
  const double inv = 1.0 / det;
  t.rinv[0][0] = c00 * inv;
  t.rinv[1][0] = c01 * inv;
  t.rinv[2][0] = c02 * inv;
  t.rinv[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * inv;
  t.rinv[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * inv;
  t.rinv[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * inv;
  t.rinv[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * inv;
  t.rinv[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * inv;
  t.rinv[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * inv;
}

__global__ __launch_bounds__(64) void pose_records_kernel(const float* __restrict__ xi, const float* __restrict__ e0, const float* __restrict__ k,
                                                          int k_per_view, float ndc_focal, int n_views, float* __restrict__ cams,
                                                          float* __restrict__ extrinsics) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_views) return;
  PoseTerms t;
  pose_terms(xi + 6 * v, e0 + 16 * v, t);
  float* c = cams + 16 * v;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) c[3 * i + j] = static_cast<float>(t.rinv[i][j]);
    c[9 + i] = static_cast<float>(-(t.rinv[i][0] * t.p[0] + t.rinv[i][1] * t.p[1] + t.rinv[i][2] * t.p[2]));
  }
  const float* kv = k + (k_per_view ? 9 * v : 0);
  c[12] = kv[0]; c[13] = kv[2]; c[14] = kv[5]; c[15] = ndc_focal;
  if (extrinsics != nullptr) {
    float* e = extrinsics + 16 * v;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) e[4 * i + j] = static_cast<float>(t.M[i][j]);
      e[4 * i + 3] = static_cast<float>(t.p[i]);
    }
    e[12] = 0.0f; e[13] = 0.0f; e[14] = 0.0f; e[15] = 1.0f;
  }
}

// Backward, at the given xi (G = upstream of rinv, g_o of origin; <X, Y> = sum_ij X_ij Y_ij):
//   origin = -rinv p :  g_p = -rinv^T g_o,  G -= g_o p^T
//   rinv = M^-1      :  g_M = -rinv^T G rinv^T
//   M = R R0, p = R t0 + W t :  g_R = g_M R0^T + g_p t0^T,  g_W = g_p t^T,  g_t = W^T g_p
//   R, W in K and (A, B, C)(s):  g_K = A g_R + B (g_R K^T + K^T g_R) + B g_W + C (g_W K^T + K^T g_W),
//                                g_s = <g_R, K> A' + (<g_R, K^2> + <g_W, K>) B' + <g_W, K^2> C'
//   g_omega = vee(g_K - g_K^T) + 2 omega g_s.
// out[6] = the twist gradient of view v (zeros when its slots 0:12 are zero); g = g_cams + 16 v.
__device__ inline void pose_grad(const float* __restrict__ g, const float* __restrict__ xi, const float* __restrict__ e0, int v, double (&out)[6]) {
  for (int i = 0; i < 6; ++i) out[i] = 0.0;
  bool any = false;
  for (int i = 0; i < 12; ++i) any = any || (g[i] != 0.0f);
  if (any) {
    PoseTerms t;
    pose_terms(xi + 6 * v, e0 + 16 * v, t);
    double G[3][3], go[3], gp[3];
    for (int i = 0; i < 3; ++i) go[i] = g[9 + i];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) G[i][j] = static_cast<double>(g[3 * i + j]) - go[i] * t.p[j];
    for (int j = 0; j < 3; ++j) gp[j] = -(t.rinv[0][j] * go[0] + t.rinv[1][j] * go[1] + t.rinv[2][j] * go[2]);
    // g_M = -rinv^T G rinv^T
    double tmp[3][3], gM[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) tmp[i][j] = t.rinv[0][i] * G[0][j] + t.rinv[1][i] * G[1][j] + t.rinv[2][i] * G[2][j];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) gM[i][j] = -(tmp[i][0] * t.rinv[j][0] + tmp[i][1] * t.rinv[j][1] + tmp[i][2] * t.rinv[j][2]);
    const float* e = e0 + 16 * v;
    const double tv[3] = {static_cast<double>(xi[6 * v + 3]), static_cast<double>(xi[6 * v + 4]), static_cast<double>(xi[6 * v + 5])};
    double gR[3][3], gW[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        // (g_M R0^T)_ij = sum_k g_M[i][k] R0[j][k]
        gR[i][j] = (gM[i][0] * e[4 * j + 0] + gM[i][1] * e[4 * j + 1] + gM[i][2] * e[4 * j + 2]) + gp[i] * e[4 * j + 3];
        gW[i][j] = gp[i] * tv[j];
      }
    for (int j = 0; j < 3; ++j) out[3 + j] = t.W[0][j] * gp[0] + t.W[1][j] * gp[1] + t.W[2][j] * gp[2];
    double gK[3][3];
    double rk = 0.0, rk2 = 0.0, wk = 0.0, wk2 = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        // (X K^T)_ij = sum_k X[i][k] K[j][k];  (K^T X)_ij = sum_k K[k][i] X[k][j]
        const double r_kt = gR[i][0] * t.K[j][0] + gR[i][1] * t.K[j][1] + gR[i][2] * t.K[j][2];
        const double kt_r = t.K[0][i] * gR[0][j] + t.K[1][i] * gR[1][j] + t.K[2][i] * gR[2][j];
        const double w_kt = gW[i][0] * t.K[j][0] + gW[i][1] * t.K[j][1] + gW[i][2] * t.K[j][2];
        const double kt_w = t.K[0][i] * gW[0][j] + t.K[1][i] * gW[1][j] + t.K[2][i] * gW[2][j];
        gK[i][j] = t.e.a * gR[i][j] + t.e.b * (r_kt + kt_r) + t.e.b * gW[i][j] + t.e.c * (w_kt + kt_w);
        rk += gR[i][j] * t.K[i][j]; rk2 += gR[i][j] * t.K2[i][j];
        wk += gW[i][j] * t.K[i][j]; wk2 += gW[i][j] * t.K2[i][j];
      }
    const double gs = rk * t.e.da + (rk2 + wk) * t.e.db + wk2 * t.e.dc;
    out[0] = (gK[2][1] - gK[1][2]) + 2.0 * static_cast<double>(xi[6 * v + 0]) * gs;
    out[1] = (gK[0][2] - gK[2][0]) + 2.0 * static_cast<double>(xi[6 * v + 1]) * gs;
    out[2] = (gK[1][0] - gK[0][1]) + 2.0 * static_cast<double>(xi[6 * v + 2]) * gs;
  }
}

__global__ __launch_bounds__(64) void pose_records_bwd_kernel(const float* __restrict__ g_cams, const float* __restrict__ xi,
                                                              const float* __restrict__ e0, int n_views, float* __restrict__ g_xi,
                                                              float* __restrict__ g_xi_keep) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_views) return;
  double out[6];
  pose_grad(g_cams + 16 * v, xi, e0, v, out);
  for (int i = 0; i < 6; ++i) {
    const float r = static_cast<float>(out[i]);
    g_xi[6 * v + i] = r;
    if (g_xi_keep != nullptr) g_xi_keep[6 * v + i] = r;
  }
}

// fx, cx, cy of one view from K0 and phi = (a, b, c) (NULL: zeros), scale s - the parameterisation of the header comment.
struct Intrinsics {
  double fx0, fx, cx, cy;
};

__device__ inline Intrinsics intrinsics_terms(const float* __restrict__ kv, const float* __restrict__ phi, double s) {
  Intrinsics in;
  const double a = phi ? phi[0] : 0.0, b = phi ? phi[1] : 0.0, c = phi ? phi[2] : 0.0;
  in.fx0 = kv[0];
  in.fx = in.fx0 * exp(s * a);
  in.cx = static_cast<double>(kv[2]) + s * in.fx0 * b;
  in.cy = static_cast<double>(kv[5]) + s * in.fx0 * c;
  return in;
}

// pose_records_kernel with slots 12:15 from phi.
__global__ __launch_bounds__(64) void camera_records_kernel(const float* __restrict__ xi, const float* __restrict__ phi, int phi_per_view,
                                                            double scale, const float* __restrict__ e0, const float* __restrict__ k,
                                                            int k_per_view, float ndc_focal, int n_views, float* __restrict__ cams,
                                                            float* __restrict__ extrinsics) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_views) return;
  PoseTerms t;
  pose_terms(xi + 6 * v, e0 + 16 * v, t);
  float* c = cams + 16 * v;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) c[3 * i + j] = static_cast<float>(t.rinv[i][j]);
    c[9 + i] = static_cast<float>(-(t.rinv[i][0] * t.p[0] + t.rinv[i][1] * t.p[1] + t.rinv[i][2] * t.p[2]));
  }
  const Intrinsics in = intrinsics_terms(k + (k_per_view ? 9 * v : 0), phi ? phi + (phi_per_view ? 3 * v : 0) : nullptr, scale);
  c[12] = static_cast<float>(in.fx); c[13] = static_cast<float>(in.cx); c[14] = static_cast<float>(in.cy); c[15] = ndc_focal;
  if (extrinsics != nullptr) {
    float* e = extrinsics + 16 * v;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) e[4 * i + j] = static_cast<float>(t.M[i][j]);
      e[4 * i + 3] = static_cast<float>(t.p[i]);
    }
    e[12] = 0.0f; e[13] = 0.0f; e[14] = 0.0f; e[15] = 1.0f;
  }
}

// pose_records_bwd_kernel with a pose mask and the gradient of phi.  Per view: g_xi (zeros under pose_mask[v] == 0) and the three
// contributions (s fx g_fx, s fx0 g_cx, s fx0 g_cy) in fp64.  phi_per_view: rounded and stored, grid ceil(V / 64).  Shared phi: ONE
// workgroup walks the views (thread i: i, i + 64, ...), leaves the contributions in `contrib` (V,3) fp64, and after the barrier
// threads 0..2 add them v = 0, 1, ..., V - 1 - plain stores, the order a function of V alone.
__global__ __launch_bounds__(64) void camera_records_bwd_kernel(const float* __restrict__ g_cams, const float* __restrict__ xi,
                                                                const float* __restrict__ phi, int phi_per_view, double scale,
                                                                const float* __restrict__ e0, const float* __restrict__ k, int k_per_view,
                                                                const int32_t* __restrict__ pose_mask, int n_views, float* __restrict__ g_xi,
                                                                float* __restrict__ g_xi_keep, float* __restrict__ g_phi,
                                                                float* __restrict__ g_phi_keep, double* contrib) {
  const bool reduce = g_phi != nullptr && !phi_per_view;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n_views; v += gridDim.x * blockDim.x) {
    const float* g = g_cams + 16 * v;
    double out[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (pose_mask == nullptr || pose_mask[v] != 0) pose_grad(g, xi, e0, v, out);
    for (int i = 0; i < 6; ++i) {
      const float r = static_cast<float>(out[i]);
      g_xi[6 * v + i] = r;
      if (g_xi_keep != nullptr) g_xi_keep[6 * v + i] = r;
    }
    if (g_phi == nullptr) continue;
    const Intrinsics in = intrinsics_terms(k + (k_per_view ? 9 * v : 0), phi ? phi + (phi_per_view ? 3 * v : 0) : nullptr, scale);
    const double gp[3] = {scale * in.fx * g[12], scale * in.fx0 * g[13], scale * in.fx0 * g[14]};
    for (int i = 0; i < 3; ++i) {
      if (reduce) {
        contrib[3 * v + i] = gp[i];
      } else {
        const float r = static_cast<float>(gp[i]);
        g_phi[3 * v + i] = r;
        if (g_phi_keep != nullptr) g_phi_keep[3 * v + i] = r;
      }
    }
  }
  if (!reduce) return;
  __syncthreads();     // (with its workgroup-scope fence: the contributions written above are visible to threads 0..2)
  if (threadIdx.x < 3) {
    double sum = 0.0;
    for (int v = 0; v < n_views; ++v) sum += contrib[3 * v + threadIdx.x];
    const float r = static_cast<float>(sum);
    g_phi[threadIdx.x] = r;
    if (g_phi_keep != nullptr) g_phi_keep[threadIdx.x] = r;
  }
}

// The last kernel of dn_render_rays_backward_geom: what autograd leaves in rows.grad on the stage-by-stage route, from its terms -
// the two networks' input gradients (d_rays_*; near / far columns 0), the compositing passes' direction gradients (columns 3:6) and
// the coarse depths' near / far gradient (columns 6:8).  d_rays_f / g_rd_f NULL: coarse pass only.  One thread per element, the
// terms added in a fixed order.
__global__ void combine_ray_grads_kernel(const float* __restrict__ d_rays_c, const float* __restrict__ d_rays_f, const float* __restrict__ g_rd_c,
                                         const float* __restrict__ g_rd_f, const float* __restrict__ g_near_far, int64_t n_rays, int ray_stride,
                                         float* __restrict__ d_rays) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= n_rays * ray_stride) return;
  const int64_t r = idx / ray_stride;
  const int c = static_cast<int>(idx - r * ray_stride);
  if (c == 6 || c == 7) {
    d_rays[idx] = g_near_far[r * 2 + (c - 6)];
    return;
  }
  float v = d_rays_c[idx];
  if (d_rays_f != nullptr) v += d_rays_f[idx];
  if (c >= 3 && c < 6) {
    v += g_rd_c[r * 3 + (c - 3)];
    if (g_rd_f != nullptr) v += g_rd_f[r * 3 + (c - 3)];
  }
  d_rays[idx] = v;
}

int combine_ray_grads(const float* d_rays_c, const float* d_rays_f, const float* g_rd_c, const float* g_rd_f, const float* g_near_far,
                      int64_t n_rays, int ray_stride, float* d_rays, dn_stream_t stream) {
  if (n_rays == 0) return 0;
  DN_REQUIRE(d_rays_c && g_rd_c && g_near_far && d_rays && n_rays > 0 && ray_stride >= 8, "combine_ray_grads: bad arguments");
  const int64_t total = n_rays * ray_stride;
  const unsigned grid = static_cast<unsigned>((total + 255) / 256);
  hipLaunchKernelGGL(combine_ray_grads_kernel, dim3(grid), dim3(256), 0, as_stream(stream), d_rays_c, d_rays_f, g_rd_c, g_rd_f, g_near_far,
                     n_rays, ray_stride, d_rays);
  return check_launch("combine_ray_grads");
}

static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace dn

using namespace dn;

extern "C" int dn_pose_records(const float* xi, const float* e0, const float* k, int k_per_view, double ndc_focal, int n_views, float* cams,
                               float* extrinsics, dn_stream_t stream) {
  DN_REQUIRE(n_views >= 0, "dn_pose_records: negative view count");
  DN_REQUIRE(xi && e0 && k && cams, "dn_pose_records: NULL pointer");
  DN_REQUIRE(aligned4(xi) && aligned4(e0) && aligned4(k) && aligned4(cams) && aligned4(extrinsics), "dn_pose_records: pointers must be 4-byte aligned");
  DN_REQUIRE(ndc_focal >= 0.0 && ndc_focal < 3.0e38, "dn_pose_records: ndc_focal must be finite and >= 0 (0: world-space rays)");
  if (n_views == 0) return 0;
  const unsigned grid = static_cast<unsigned>((n_views + 63) / 64);
  hipLaunchKernelGGL(pose_records_kernel, dim3(grid), dim3(64), 0, as_stream(stream), xi, e0, k, k_per_view ? 1 : 0, static_cast<float>(ndc_focal),
                     n_views, cams, extrinsics);
  return check_launch("dn_pose_records");
}

extern "C" int dn_pose_records_backward(const float* g_cams, const float* xi, const float* e0, int n_views, float* g_xi, float* g_xi_keep,
                                        dn_stream_t stream) {
  DN_REQUIRE(n_views >= 0, "dn_pose_records_backward: negative view count");
  DN_REQUIRE(g_cams && xi && e0 && g_xi, "dn_pose_records_backward: NULL pointer");
  DN_REQUIRE(aligned4(g_cams) && aligned4(xi) && aligned4(e0) && aligned4(g_xi) && aligned4(g_xi_keep),
             "dn_pose_records_backward: pointers must be 4-byte aligned");
  if (n_views == 0) return 0;
  const unsigned grid = static_cast<unsigned>((n_views + 63) / 64);
  hipLaunchKernelGGL(pose_records_bwd_kernel, dim3(grid), dim3(64), 0, as_stream(stream), g_cams, xi, e0, n_views, g_xi, g_xi_keep);
  return check_launch("dn_pose_records_backward");
}

static bool scale_ok(double s) { return s > 0.0 && s < 3.0e38; }

extern "C" int dn_camera_records(const float* xi, const float* phi, int phi_per_view, double intrinsics_scale, const float* e0, const float* k,
                                 int k_per_view, double ndc_focal, int n_views, float* cams, float* extrinsics, dn_stream_t stream) {
  DN_REQUIRE(n_views >= 0, "dn_camera_records: negative view count");
  DN_REQUIRE(xi && e0 && k && cams, "dn_camera_records: NULL pointer");
  DN_REQUIRE(aligned4(xi) && aligned4(phi) && aligned4(e0) && aligned4(k) && aligned4(cams) && aligned4(extrinsics),
             "dn_camera_records: pointers must be 4-byte aligned");
  DN_REQUIRE(ndc_focal >= 0.0 && ndc_focal < 3.0e38, "dn_camera_records: ndc_focal must be finite and >= 0 (0: world-space rays)");
  DN_REQUIRE(scale_ok(intrinsics_scale), "dn_camera_records: intrinsics_scale must be finite and > 0");
  if (n_views == 0) return 0;
  const unsigned grid = static_cast<unsigned>((n_views + 63) / 64);
  hipLaunchKernelGGL(camera_records_kernel, dim3(grid), dim3(64), 0, as_stream(stream), xi, phi, phi_per_view ? 1 : 0, intrinsics_scale, e0, k,
                     k_per_view ? 1 : 0, static_cast<float>(ndc_focal), n_views, cams, extrinsics);
  return check_launch("dn_camera_records");
}

extern "C" size_t dn_camera_records_scratch_bytes(int n_views) {
  if (n_views <= 0) return 0;
  return (static_cast<size_t>(n_views) * 3 * sizeof(double) + 255) / 256 * 256;
}

extern "C" int dn_camera_records_backward(const float* g_cams, const float* xi, const float* phi, int phi_per_view, double intrinsics_scale,
                                          const float* e0, const float* k, int k_per_view, const int32_t* pose_mask, int n_views, float* g_xi,
                                          float* g_xi_keep, float* g_phi, float* g_phi_keep, void* scratch, size_t scratch_bytes,
                                          dn_stream_t stream) {
  DN_REQUIRE(n_views >= 0, "dn_camera_records_backward: negative view count");
  DN_REQUIRE(g_cams && xi && e0 && k && g_xi, "dn_camera_records_backward: NULL pointer");
  DN_REQUIRE(g_phi || !g_phi_keep, "dn_camera_records_backward: g_phi_keep without g_phi");
  DN_REQUIRE(aligned4(g_cams) && aligned4(xi) && aligned4(phi) && aligned4(e0) && aligned4(k) && aligned4(pose_mask) && aligned4(g_xi) &&
                 aligned4(g_xi_keep) && aligned4(g_phi) && aligned4(g_phi_keep),
             "dn_camera_records_backward: pointers must be 4-byte aligned");
  DN_REQUIRE(scale_ok(intrinsics_scale), "dn_camera_records_backward: intrinsics_scale must be finite and > 0");
  const bool reduce = g_phi != nullptr && !phi_per_view;
  const size_t need = reduce ? dn_camera_records_scratch_bytes(n_views) : 0;
  DN_REQUIRE(need == 0 || (scratch && (reinterpret_cast<uintptr_t>(scratch) & 7) == 0 && scratch_bytes >= need),
             "dn_camera_records_backward: a shared g_phi needs dn_camera_records_scratch_bytes(n_views) bytes of 8-byte aligned scratch");
  if (n_views == 0 && !reduce) return 0;
  // a shared g_phi: one workgroup, so that its sum needs no second launch (n_views == 0: it stores the three zeros)
  const unsigned grid = reduce ? 1u : static_cast<unsigned>((n_views + 63) / 64);
  hipLaunchKernelGGL(camera_records_bwd_kernel, dim3(grid), dim3(64), 0, as_stream(stream), g_cams, xi, phi, phi_per_view ? 1 : 0,
                     intrinsics_scale, e0, k, k_per_view ? 1 : 0, pose_mask, n_views, g_xi, g_xi_keep, g_phi, g_phi_keep,
                     static_cast<double*>(scratch));
  return check_launch("dn_camera_records_backward");
}
