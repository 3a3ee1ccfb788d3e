// Scan-to-field registration against folded eval networks: one fused render pass that returns the depth, the hit
// probability and the per-ray Jacobian d depth / d (o, d), and the Gauss-Newton normal equations of a scan.  The pass
// and the per-ray Gauss-Newton pieces are fold_render.h's, shared with localize.hip and refine.hip.
//
//   k_render_jac_fold<MAXB>  one wave per ray, four rays per 256-thread workgroup (as k_rays_grad_eval and
//                            k_composite<., 64>); the depths come from global memory.  fr_pass keeps a lane's p, z
//                            and grad logit in registers: per sample only `weights` reaches memory, when asked for.
//                            Without jac6 the pass ends after its forward (a runtime, wave-uniform test).
//   k_gn_normal_eq           per ray the pose Jacobian Jp and the Huber-weighted terms of H = sum w Jp^T Jp (upper
//                            triangle), b = sum w Jp^T r, the cost and the valid count, in float64, accumulated
//                            grid-stride; at most GN_MAX_WG workgroups write 32-word partials.
//   k_gn_normal_eq_sum       one workgroup adds the partials in a fixed order (the k_eval_gmoments_sum pattern).
// No atomics: every output word has one writer and a fixed summation order; the launch geometry of the reduction is a
// function of the ray count alone.
#include "fold_render.h"

namespace pcn {

constexpr int GN_MAX_WG = 1024;   // workgroups of the normal-equation pass
constexpr int GN_W = 32;          // words per partial: 21 + 6 + cost + n_valid, padded

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
  const float* __restrict__ row = rays + r * stride;
  double dep, hit, acc[6];
  fr_pass<MAXB, true>(row, z + r * S, S, a, eps, lane, weights ? weights + r * S : nullptr, dep, hit, acc,
                      jac6 != nullptr);   // (wave-uniform: without jac6 the pass ends after its forward)
  if (lane == 0) {
    depth[r] = (float)dep;
    sumw[r] = (float)hit;
    if (jac6) {
#pragma unroll
      for (int m = 0; m < 6; ++m) jac6[6 * r + m] = (float)acc[m];
    }
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
    if (!gn_beam_valid(dv, sumw[i], tg, min_sumw)) continue;
    double Jp[6], w, rho;
    gn_pose_jacobian(rays + i * stride, jac6 + 6 * i, Jp);
    const double res = (double)dv - (double)tg;
    gn_huber(res, delta, w, rho);
    int k = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const double wj = w * Jp[p];
#pragma unroll
      for (int q = p; q < 6; ++q) acc[k++] += wj * Jp[q];
      acc[21 + p] += wj * res;
    }
    acc[27] += rho;
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

extern "C" int pcnerf_render_depth_jac_fold(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                            int n_samples, const double* fold, float eps, float* depth, float* sumw,
                                            float* weights_or_null, float* jac6_or_null, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_rays >= 0, "pcnerf_render_depth_jac_fold: n_rays < 0");
  PCN_CHECK(ray_stride >= 6, "pcnerf_render_depth_jac_fold: ray_stride < 6");
  PCN_CHECK(n_samples >= 1, "pcnerf_render_depth_jac_fold: n_samples < 1");
  PCN_CHECK(n_samples <= FR_MAX_S, "pcnerf_render_depth_jac_fold: n_samples > 1024 (one wave per ray, at most 16 "
                                   "samples per lane)");
  if (n_rays == 0) return 0;
  PCN_CHECK(rays && z && fold && depth && sumw, "pcnerf_render_depth_jac_fold: null argument");
  const int64_t blocks = (n_rays + 3) / 4;   // four waves, four rays per workgroup
  PCN_CHECK(blocks < (int64_t)1 << 31, "pcnerf_render_depth_jac_fold: too many rays for one launch");
  fr_dispatch_maxb(n_samples, [&](auto mb) {
    hipLaunchKernelGGL(k_render_jac_fold<decltype(mb)::value>, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, rays, n_rays, ray_stride, z, n_samples, fold, eps, depth, sumw,
                       weights_or_null, jac6_or_null);
  });
  PCN_LAUNCH_CHECK("pcnerf_render_depth_jac_fold");
  PCN_API_END_NEG
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
  PCN_API_END_NEG
}
