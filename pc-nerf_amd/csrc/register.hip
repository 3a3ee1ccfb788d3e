// Scan-to-field registration against folded eval networks: one fused render pass that returns the depth, the hit
// probability and the per-ray Jacobian d depth / d (o, d), and the Gauss-Newton normal equations of a scan.
//
// SURVEY fact 1 (nof_eval.hip, k_fold_eval): the eval network is p = sigmoid(a . e(x) + c) with one 63-vector a.  The
// encoding's sincosf(2^k x_m) are at once the logit's features and, since d sin(2^k x)/dx = 2^k cos(2^k x), the
// factors of its gradient, so one evaluation per sample serves the forward and the backward of a render pass.
//
//   k_render_jac_fold<MAXB>  one wave per ray, four rays per 256-thread workgroup (as k_rays_grad_eval and
//                            k_composite<., 64>).  Lane l owns the contiguous samples l B .. l B + B - 1,
//                            B = ceil(S / 64) <= MAXB, and keeps their p, z and grad logit in registers: per sample
//                            only `weights` reaches memory, when asked for.  The logit is k_nof_eval_fold's
//                            expression (six float64 chains in its order, p = sigmoid_ref(fl32(acc))), grad logit is
//                            nof_eval_grad.hip's logit_grad_pos, both from the same 30 sincosf.  Compositing
//                            (render.py:51-61, no noise) runs in float64 from the float32 p and rounds each output
//                            once; d depth / d logit_s follows k_composite_bwd with dL/ddepth = 1: the reverse affine
//                            recurrence U_{j-1} = g~_j p_j + (1 - p_j) U_j, no division by 1 - p.
//                            jac6[r, 0:3] = sum_s g_s grad logit(x_s), jac6[r, 3:6] = sum_s z_s g_s grad logit(x_s):
//                            per-lane float64 partials in sample order, the xor butterfly, one rounding.
//   k_gn_normal_eq           per ray the pose Jacobian Jp = [J_o, o x J_o + d x J_d] of the left perturbation
//                            T' = exp(xi) T (delta o = rho + phi x o, delta d = phi x d) and the Huber-weighted terms
//                            of H = sum w Jp^T Jp (upper triangle), b = sum w Jp^T r, the cost and the valid count, in
//                            float64; at most GN_MAX_WG workgroups write 32-word partials.
//   k_gn_normal_eq_sum       one workgroup adds the partials in a fixed order (the k_eval_gmoments_sum pattern).
// No atomics: every output word has one writer and a fixed summation order; the launch geometry of the reduction is a
// function of the ray count alone.
#include "pcnerf_internal.h"

namespace pcn {

constexpr int RJ_MAX_S = 1024;    // 64 lanes x 16 samples per lane
constexpr int GN_MAX_WG = 1024;   // workgroups of the normal-equation pass
constexpr int GN_W = 32;          // words per partial: 21 + 6 + cost + n_valid, padded

// The logit a . e(x) + c (k_nof_eval_fold's chains and summation order) and its gradient to x (logit_grad_pos's
// chains) from one sincosf per encoding pair.  a: the 64 fold doubles in LDS.
__device__ __forceinline__ double rj_logit_and_grad(const float (&p)[3], const double* __restrict__ a,
                                                    double (&g)[3]) {
  double part[6];   // six independent chains (sin / cos per coordinate), summed at the end
  double gs[3], gc[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    part[m] = a[m] * (double)p[m];
    part[3 + m] = 0.0;
    g[m] = a[m];
    gs[m] = 0.0;
    gc[m] = 0.0;
  }
#pragma unroll 2
  for (int k = 0; k < 10; ++k) {   // partly rolled, as k_nof_eval_fold: the coefficients stay in LDS
    const float sc = (float)(1 << k);
    const double dsc = (double)(1 << k);
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      float sv, cv;
      sincosf(sc * p[m], &sv, &cv);
      part[m] += a[3 + 6 * k + m] * (double)sv;
      part[3 + m] += a[6 + 6 * k + m] * (double)cv;
      gs[m] += (dsc * a[3 + 6 * k + m]) * (double)cv;   // d sin(2^k x)/dx = 2^k cos
      gc[m] -= (dsc * a[6 + 6 * k + m]) * (double)sv;   // d cos(2^k x)/dx = -2^k sin
    }
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) g[m] += gs[m] + gc[m];
  double acc = a[63];
  acc += ((part[0] + part[1]) + (part[2] + part[3])) + (part[4] + part[5]);
  return acc;
}

// exclusive multiplicative scan of one double per lane (render.hip's wave_excl_prod)
__device__ __forceinline__ double rj_excl_prod(double v, int lane) {
  double incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double n = __shfl_up(incl, o, 64);
    if (lane >= o) incl *= n;
  }
  const double ex = __shfl_up(incl, 1, 64);
  return lane == 0 ? 1.0 : ex;
}

// U entering each lane's block from above: lanes l + 1 .. 63's affine maps (Y = A + Bm Y_next) composed, applied
// to 0 (render.hip's Grp<64>::suffix_affine)
__device__ __forceinline__ double rj_suffix_affine(double A, double Bm, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double An = __shfl_down(A, o, 64), Bn = __shfl_down(Bm, o, 64);
    if (lane + o < 64) {
      A = A + Bm * An;
      Bm = Bm * Bn;
    }
  }
  const double An1 = __shfl_down(A, 1, 64);
  return lane == 63 ? 0.0 : An1;
}

template <int MAXB>
__global__ __launch_bounds__(256) void k_render_jac_fold(const float* __restrict__ rays, int64_t n_rays, int stride,
                                                         const float* __restrict__ z, int S,
                                                         const double* __restrict__ fold, float eps,
                                                         float* __restrict__ depth, float* __restrict__ sumw,
                                                         float* __restrict__ weights, float* __restrict__ jac6) {
  __shared__ double a[64];
  if (threadIdx.x < 64) a[threadIdx.x] = fold[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_rays) return;   // whole waves leave: the shuffles below always have 64 lanes
  const int B = (S + 63) / 64;   // <= MAXB (the launcher's choice)
  const int i0 = lane * B;
  const int nb = max(0, min(B, S - i0));
  const float* __restrict__ row = rays + r * stride;
  const float* __restrict__ zr = z + r * S + i0;
  // samples past the lane's block count as p = 0 at z = 0: factors of one and terms of zero everywhere below
  float pv[MAXB], zv[MAXB];
  double gx[MAXB][3];
#pragma unroll
  for (int j = 0; j < MAXB; ++j) {
    pv[j] = 0.0f;
    zv[j] = 0.0f;
    gx[j][0] = gx[j][1] = gx[j][2] = 0.0;
  }
  // a rolled loop (one copy of the 30 sincosf); the unrolled selects keep the arrays' indices static
#pragma nounroll
  for (int j = 0; j < nb; ++j) {
    const float zs = zr[j];
    float x[3];
    sample_point(row, zs, x);
    double d[3];
    const double logit = rj_logit_and_grad(x, a, d);
    const float ps = sigmoid_ref((float)logit);
#pragma unroll
    for (int jj = 0; jj < MAXB; ++jj) {
      if (jj == j) {
        pv[jj] = ps;
        zv[jj] = zs;
        gx[jj][0] = d[0];
        gx[jj][1] = d[1];
        gx[jj][2] = d[2];
      }
    }
  }
  // compositing (render.py:51-61, noise = None) in float64 from the float32 p: 1 - p, the transmittance scan, the
  // weights and their sums carry no float32 rounding; each output rounds once
  double loc = 1.0;
#pragma unroll
  for (int j = 0; j < MAXB; ++j) loc *= 1.0 - (double)pv[j];
  double T = rj_excl_prod(loc, lane);
  double wv[MAXB], tv[MAXB];
  double sw = 0.0;
#pragma unroll
  for (int j = 0; j < MAXB; ++j) {
    tv[j] = T;
    wv[j] = T * (double)pv[j];
    sw += wv[j];
    T *= 1.0 - (double)pv[j];
  }
  const double hit = wave_sum_d(sw);   // sum of the unnormalised weights: the hit probability
  const double rden = 1.0 / (hit + (double)eps);
  double sd = 0.0;
#pragma unroll
  for (int j = 0; j < MAXB; ++j) {
    wv[j] = wv[j] * rden;
    sd += wv[j] * (double)zv[j];
  }
  const double dep = wave_sum_d(sd);
  if (lane == 0) {
    depth[r] = (float)dep;
    sumw[r] = (float)hit;
  }
  if (weights) {
    float* __restrict__ wr = weights + r * S + i0;
#pragma unroll
    for (int j = 0; j < MAXB; ++j)
      if (j < nb) wr[j] = (float)wv[j];
  }
  if (!jac6) return;   // (wave-uniform)

  // d depth / d logit_s (k_composite_bwd's recurrence with dL/ddepth = 1)
  double gw[MAXB];
#pragma unroll
  for (int j = 0; j < MAXB; ++j) gw[j] = ((double)zv[j] - dep) * rden;   // d depth / d w~_j
  double A = 0.0, Bm = 1.0;   // this lane's affine map U_end -> U_{i0 - 1}
#pragma unroll
  for (int j = MAXB - 1; j >= 0; --j) {
    const double aj = gw[j] * (double)pv[j], bj = 1.0 - (double)pv[j];
    A = aj + bj * A;
    Bm = bj * Bm;
  }
  double U = rj_suffix_affine(A, Bm, lane);
#pragma unroll
  for (int j = MAXB - 1; j >= 0; --j) {
    const double gp = tv[j] * (gw[j] - U);
    U = gw[j] * (double)pv[j] + (1.0 - (double)pv[j]) * U;
    gw[j] = gp * (1.0 - (double)pv[j]) * (double)pv[j];   // sigmoid backward: now d depth / d logit_j
  }
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < MAXB; ++j) {   // sample order
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const double g = gw[j] * gx[j][m];
      acc[m] += g;
      acc[3 + m] += (double)zv[j] * g;
    }
  }
#pragma unroll
  for (int m = 0; m < 6; ++m) acc[m] = wave_sum_d(acc[m]);
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < 6; ++m) jac6[6 * r + m] = (float)acc[m];
  }
}

inline int gn_workgroups(int64_t n_rays) {
  const int64_t w = (n_rays + 255) / 256;
  return (int)(w < 1 ? 1 : w > GN_MAX_WG ? GN_MAX_WG : w);
}

__global__ __launch_bounds__(256) void k_gn_normal_eq(const float* __restrict__ rays, int64_t n_rays, int stride,
                                                      const float* __restrict__ jac6,
                                                      const float* __restrict__ depth,
                                                      const float* __restrict__ sumw,
                                                      const float* __restrict__ target, double delta,
                                                      double min_sumw, double* __restrict__ part) {
  __shared__ double red[4][GN_W];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double acc[29];
#pragma unroll
  for (int k = 0; k < 29; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n_rays; i += (int64_t)gridDim.x * 256) {
    const float dv = depth[i], tg = target[i];
    const bool valid = (double)sumw[i] >= min_sumw && isfinite(dv) && isfinite(tg) && tg > 0.0f;
    if (!valid) continue;
    const float* __restrict__ row = rays + i * stride;
    const float* __restrict__ jr = jac6 + 6 * i;
    double o[3], d[3], Jo[3], Jd[3], Jp[6];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      o[m] = (double)row[m];
      d[m] = (double)row[3 + m];
      Jo[m] = (double)jr[m];
      Jd[m] = (double)jr[3 + m];
      Jp[m] = Jo[m];
    }
    Jp[3] = (o[1] * Jo[2] - o[2] * Jo[1]) + (d[1] * Jd[2] - d[2] * Jd[1]);
    Jp[4] = (o[2] * Jo[0] - o[0] * Jo[2]) + (d[2] * Jd[0] - d[0] * Jd[2]);
    Jp[5] = (o[0] * Jo[1] - o[1] * Jo[0]) + (d[0] * Jd[1] - d[1] * Jd[0]);
    const double res = (double)dv - (double)tg, ar = fabs(res);
    const bool lin = delta > 0.0 && ar > delta;   // Huber's linear branch; delta <= 0: plain least squares
    const double w = lin ? delta / ar : 1.0;
    int k = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const double wj = w * Jp[p];
#pragma unroll
      for (int q = p; q < 6; ++q) acc[k++] += wj * Jp[q];
      acc[21 + p] += wj * res;
    }
    acc[27] += lin ? delta * (ar - 0.5 * delta) : 0.5 * (res * res);
    acc[28] += 1.0;
  }
#pragma unroll
  for (int k = 0; k < 29; ++k) {
    const double v = wave_sum_d(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (tid < GN_W)
    part[(int64_t)blockIdx.x * GN_W + tid] =
        tid < 29 ? (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]) : 0.0;
}

// out30[f] = sum_w part[w][f]: thread (f, q) adds workgroups q, q + 8, ... in order, the eight chains in a fixed order
__global__ __launch_bounds__(256) void k_gn_normal_eq_sum(const double* __restrict__ part, int nwg,
                                                          double* __restrict__ out30) {
  __shared__ double red[8][GN_W];
  const int f = threadIdx.x & 31, q = threadIdx.x >> 5;
  double acc = 0.0;
  for (int w = q; w < nwg; w += 8) acc += part[(int64_t)w * GN_W + f];
  red[q][f] = acc;
  __syncthreads();
  if (q == 0 && f < 30)
    out30[f] = ((red[0][f] + red[1][f]) + (red[2][f] + red[3][f])) + ((red[4][f] + red[5][f]) + (red[6][f] + red[7][f]));
}

}  // namespace pcn

using namespace pcn;

// these entries report an argument error as -1 (the message in pcnerf_last_error)
#define REG_API_END                                       \
  return 0;                                               \
  }                                                       \
  catch (const std::exception& ex__) {                    \
    pcn::set_error(ex__.what());                          \
    return -1;                                            \
  }

extern "C" int pcnerf_render_depth_jac_fold(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                            int n_samples, const double* fold, float eps, float* depth, float* sumw,
                                            float* weights_or_null, float* jac6_or_null, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_rays >= 0, "pcnerf_render_depth_jac_fold: n_rays < 0");
  PCN_CHECK(ray_stride >= 6, "pcnerf_render_depth_jac_fold: ray_stride < 6");
  PCN_CHECK(n_samples >= 1, "pcnerf_render_depth_jac_fold: n_samples < 1");
  PCN_CHECK(n_samples <= RJ_MAX_S, "pcnerf_render_depth_jac_fold: n_samples > 1024 (one wave per ray, at most 16 "
                                   "samples per lane)");
  if (n_rays == 0) return 0;
  PCN_CHECK(rays && z && fold && depth && sumw, "pcnerf_render_depth_jac_fold: null argument");
  const int64_t blocks = (n_rays + 3) / 4;   // four waves, four rays per workgroup
  PCN_CHECK(blocks < (int64_t)1 << 31, "pcnerf_render_depth_jac_fold: too many rays for one launch");
  const int B = (n_samples + 63) / 64;
#define RJ_LAUNCH(MB)                                                                                             \
  hipLaunchKernelGGL(k_render_jac_fold<MB>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rays,      \
                     n_rays, ray_stride, z, n_samples, fold, eps, depth, sumw, weights_or_null, jac6_or_null)
  if (B <= 1) RJ_LAUNCH(1);
  else if (B <= 2) RJ_LAUNCH(2);
  else if (B <= 4) RJ_LAUNCH(4);
  else if (B <= 8) RJ_LAUNCH(8);
  else RJ_LAUNCH(16);
#undef RJ_LAUNCH
  PCN_LAUNCH_CHECK("pcnerf_render_depth_jac_fold");
  REG_API_END
}

extern "C" size_t pcnerf_gn_workspace_bytes(int64_t n_rays) {
  return (size_t)gn_workgroups(n_rays < 0 ? 0 : n_rays) * GN_W * sizeof(double);
}

extern "C" int pcnerf_gn_normal_eq(const float* rays, int64_t n_rays, int ray_stride, const float* jac6,
                                   const float* depth, const float* sumw, const float* target, double huber_delta,
                                   double min_sumw, void* workspace, double* out30, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_rays >= 0, "pcnerf_gn_normal_eq: n_rays < 0");
  PCN_CHECK(ray_stride >= 6, "pcnerf_gn_normal_eq: ray_stride < 6");
  PCN_CHECK(out30, "pcnerf_gn_normal_eq: null argument");
  if (n_rays == 0) {
    PCN_HIP(hipMemsetAsync(out30, 0, 30 * sizeof(double), (hipStream_t)stream));
    return 0;
  }
  PCN_CHECK(rays && jac6 && depth && sumw && target && workspace, "pcnerf_gn_normal_eq: null argument");
  const int nwg = gn_workgroups(n_rays);
  double* part = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(k_gn_normal_eq, dim3(nwg), dim3(256), 0, (hipStream_t)stream, rays, n_rays, ray_stride, jac6,
                     depth, sumw, target, huber_delta, min_sumw, part);
  hipLaunchKernelGGL(k_gn_normal_eq_sum, dim3(1), dim3(256), 0, (hipStream_t)stream, part, nwg, out30);
  PCN_LAUNCH_CHECK("pcnerf_gn_normal_eq");
  REG_API_END
}
