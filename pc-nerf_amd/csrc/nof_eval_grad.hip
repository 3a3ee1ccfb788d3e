// Eval-mode NOF: the gradient of the occupancy logit to the sample geometry (positions, ray origins / directions).
//
// SURVEY fact 1 (nof_eval.hip, k_fold_eval): every LeakyReLU of NOF has slope 1 and eval BatchNorm is affine, so the
// eval network is p = sigmoid(a . e(x) + c) with ONE 63-vector a for all samples.  The Jacobian of the logit with
// respect to the encoding is therefore the constant a -- exactly, whichever eval math evaluated p -- and
//   dL/dx_m = dL/dlogit * ( a[m] + sum_k 2^k ( a[3 + 6k + m] cos(2^k x_m) - a[6 + 6k + m] sin(2^k x_m) ) )
// in Embedding's column order [x, sin f0 x, cos f0 x, sin f1 x, ...] (models.py:27-41).  The encoding is recomputed
// with the forward's own arithmetic (sample_pos<PT> under -ffp-contract=off, sincosf of the exact product 2^k x as in
// encode_full), so this is the derivative of the function the forward evaluated at the float32 position it evaluated
// it at.  a stays float64; the 21-term dot per coordinate and every per-ray sum accumulate in float64 and round to
// float32 once.  No atomics: every output word has one writer and a fixed summation order.
//
//   k_points_grad_eval  one thread per point:  g_pts[g, m] = grad_logit[g] * dlogit/dx_m(pts[g])
//   k_rays_grad_eval    one wave per ray (as k_composite<., 64> groups rays), lane l takes samples l, l + 64, ...:
//                       g_rays6[r, 0:3] = sum_s g_x,s, g_rays6[r, 3:6] = sum_s z[r, s] g_x,s, per-lane float64 partials
//                       in sample order, then the xor butterfly (wave_sum_d); g_x never reaches memory.
#include "pcnerf_internal.h"

namespace pcn {

// dlogit/dx at p: 30 sincosf (encode_full's arguments) and three 21-term float64 dots against a (LDS)
__device__ __forceinline__ void logit_grad_pos(const float (&p)[3], const double* __restrict__ a, double (&g)[3]) {
  fold_dot<false, true>(p, a, g);
}

__global__ __launch_bounds__(256) void k_points_grad_eval(const float* __restrict__ pts, int64_t n,
                                                          const double* __restrict__ fold,
                                                          const float* __restrict__ g_logit,
                                                          float* __restrict__ g_pts) {
  __shared__ double a[64];
  if (threadIdx.x < 64) a[threadIdx.x] = fold[threadIdx.x];
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  float p[3];
  sample_pos<true>(nullptr, 0, nullptr, 1, pts, g, p);
  double d[3];
  logit_grad_pos(p, a, d);
  const double gl = (double)g_logit[g];
#pragma unroll
  for (int m = 0; m < 3; ++m) g_pts[3 * g + m] = (float)(gl * d[m]);
}

__global__ __launch_bounds__(256) void k_rays_grad_eval(const float* __restrict__ rays, int64_t n_rays, int stride,
                                                        const float* __restrict__ z, int S,
                                                        const double* __restrict__ fold,
                                                        const float* __restrict__ g_logit,
                                                        float* __restrict__ g_rays6) {
  __shared__ double a[64];
  if (threadIdx.x < 64) a[threadIdx.x] = fold[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= n_rays) return;   // whole waves leave: the butterfly below always has 64 lanes
  const float* __restrict__ row = rays + r * stride;
  const float* __restrict__ zr = z + r * S;
  const float* __restrict__ gr = g_logit + r * S;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int s = lane; s < S; s += 64) {
    const float zs = zr[s];
    float p[3];
    sample_point(row, zs, p);
    double d[3];
    logit_grad_pos(p, a, d);
    const double gl = (double)gr[s];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const double gx = gl * d[m];
      acc[m] += gx;
      acc[3 + m] += (double)zs * gx;
    }
  }
#pragma unroll
  for (int m = 0; m < 6; ++m) acc[m] = wave_sum_d(acc[m]);
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < 6; ++m) g_rays6[6 * r + m] = (float)acc[m];
  }
}

}  // namespace pcn

using namespace pcn;

extern "C" int pcnerf_nof_points_eval_backward(const float* pts, int64_t n, const double* fold,
                                               const float* grad_logit, float* grad_pts, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n >= 0, "pcnerf_nof_points_eval_backward: n < 0");
  if (n == 0) return 0;
  PCN_CHECK(pts && fold && grad_logit && grad_pts, "pcnerf_nof_points_eval_backward: null argument");
  const int64_t blocks = (n + 255) / 256;
  PCN_CHECK(blocks < (int64_t)1 << 31, "pcnerf_nof_points_eval_backward: too many points for one launch");
  hipLaunchKernelGGL(k_points_grad_eval, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pts, n, fold,
                     grad_logit, grad_pts);
  PCN_LAUNCH_CHECK("pcnerf_nof_points_eval_backward");
  PCN_API_END
}

extern "C" int pcnerf_nof_query_eval_backward(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                              int n_samples, const double* fold, const float* grad_logit,
                                              float* grad_rays6, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_rays >= 0, "pcnerf_nof_query_eval_backward: n_rays < 0");
  PCN_CHECK(ray_stride >= 6, "pcnerf_nof_query_eval_backward: ray_stride < 6");
  PCN_CHECK(n_samples >= 1, "pcnerf_nof_query_eval_backward: n_samples < 1");
  if (n_rays == 0) return 0;
  PCN_CHECK(rays && z && fold && grad_logit && grad_rays6, "pcnerf_nof_query_eval_backward: null argument");
  const int64_t blocks = (n_rays + 3) / 4;   // four waves, four rays per workgroup
  PCN_CHECK(blocks < (int64_t)1 << 31, "pcnerf_nof_query_eval_backward: too many rays for one launch");
  hipLaunchKernelGGL(k_rays_grad_eval, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rays, n_rays,
                     ray_stride, z, n_samples, fold, grad_logit, grad_rays6);
  PCN_LAUNCH_CHECK("pcnerf_nof_query_eval_backward");
  PCN_API_END
}
