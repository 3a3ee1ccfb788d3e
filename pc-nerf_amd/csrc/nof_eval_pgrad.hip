// Eval-mode NOF (frozen BatchNorm): the gradient of a pass's loss to the 34 trainable tensors.
//
// SURVEY fact 1 (nof_eval.hip, k_fold_eval): every LeakyReLU of NOF has slope 1 and eval BatchNorm is affine, so the
// eval network is logit_s = a(theta) . e_s + c(theta) with one (a, c) for all samples.  Then, with g_s = dL/dlogit_s,
//   dL/dtheta = sum_s g_s dlogit_s/dtheta = d/dtheta [ a(theta) . m + c(theta) s0 ],  m = sum_s g_s e_s, s0 = sum_s g_s:
// all parameter gradients of a pass over N samples are those of ONE pseudo-sample whose input is m and whose every
// additive constant (Linear bias, BatchNorm shift and running mean, occ_out bias) is scaled by s0.  Unlike train mode
// the Linear-bias and BatchNorm-shift gradients are not zero: there is no batch mean to remove.
//
//   k_eval_gmoments<SRC>   mom[0..62] = sum_g g_logit[g] e(x_g), mom[63] = sum_g g_logit[g] in float64.  SRC 0: o + d z
//                          (sample_pos<false>), 1: explicit points (sample_pos<true>), 2: an embedded (N, 63) batch.
//                          As k_tf_gmoments: each wave stages 64 samples' encodings as a [sample][feature] fp32 tile
//                          (the forward's own arithmetic: sincosf of the exact product 2^k x, as encode_full) and
//                          their g in LDS, then lane f accumulates sum_s g_s e_s[f] over the tile in float64 (every
//                          product of two float32 values is exact there; one accumulator per lane).  A workgroup
//                          owns a contiguous range of tiles and writes its 64 partial sums to the workspace;
//   k_eval_gmoments_sum    one workgroup adds the partials in a fixed order.  No atomics; the launch geometry is a
//                          function of N alone, so two runs give equal bits.
//   k_eval_param_grads     the pseudo-sample forward and backward through the 9 layers in float64 (8 workgroups of
//                          1024 threads; workgroup b keeps the chain down to layer b and ADDS fl32(value) to layer b's
//                          four gradient tensors, workgroup 0 also to occ_out's).  Fixed summation order, no atomics.
#include "pcnerf_internal.h"

namespace pcn {

constexpr int GM_MAX_WG = 1024;   // workgroups of the moments pass (4 waves, one 64-sample tile per wave at a time)

inline int64_t gm_tiles(int64_t n) { return (n + 63) / 64; }
inline int gm_workgroups(int64_t n) {
  const int64_t w = (gm_tiles(n) + 3) / 4;
  return (int)(w < 1 ? 1 : w > GM_MAX_WG ? GM_MAX_WG : w);
}

// sigmoid backward on the embedded form (p != NULL: g is dL/dp), as nof_fold.hip's fold_logit_grad
__device__ __forceinline__ float pg_logit_grad(const float* __restrict__ g, const float* __restrict__ p, int64_t i) {
  if (!p) return g[i];
  const float pv = p[i];
  return g[i] * (1.0f - pv) * pv;
}

template <int SRC>
__global__ __launch_bounds__(256) void k_eval_gmoments(const float* __restrict__ rays, int stride,
                                                       const float* __restrict__ z, int S,
                                                       const float* __restrict__ src, int64_t n,
                                                       const float* __restrict__ g, const float* __restrict__ p,
                                                       double* __restrict__ part) {
  __shared__ float tile[4][64 * 65];
  __shared__ float gs[4][64];
  __shared__ double red[4][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t ntile = (n + 63) / 64, per = (ntile + gridDim.x - 1) / gridDim.x;
  const int64_t t0 = std::min(ntile, (int64_t)blockIdx.x * per), t1 = std::min(ntile, t0 + per);
  float* my = tile[wave];
  double acc = 0.0;
  for (int64_t t = t0 + wave; t < t1; t += 4) {   // waves independent: wave-local LDS tiles
    const int64_t i = t * 64 + lane;
    const bool ok = i < n;
    if constexpr (SRC == 2) {
      // the tile's 64 x 63 floats are contiguous: coalesced loads, scattered to [sample][feature]
      const int64_t base = t * 64 * 63, end = n * 63;
#pragma unroll 7
      for (int j = 0; j < 63; ++j) {
        const int idx = j * 64 + lane;
        const int s = idx / 63, f = idx - 63 * s;
        my[s * 65 + f] = base + idx < end ? src[base + idx] : 0.0f;
      }
    } else {
      float pt[3] = {0.0f, 0.0f, 0.0f};
      if (ok) sample_pos<SRC == 1>(rays, stride, z, S, src, i, pt);
#pragma unroll
      for (int m = 0; m < 3; ++m) my[lane * 65 + m] = pt[m];
#pragma unroll 2
      for (int k = 0; k < 10; ++k) {
        const float sc = (float)(1 << k);
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          float sv, cv;
          sincosf(sc * pt[m], &sv, &cv);
          my[lane * 65 + 3 + 6 * k + m] = sv;
          my[lane * 65 + 6 + 6 * k + m] = cv;
        }
      }
    }
    my[lane * 65 + 63] = 1.0f;
    gs[wave][lane] = ok ? pg_logit_grad(g, p, i) : 0.0f;   // a tail lane's row counts with g = 0
    wave_lds_sync();
#pragma unroll 16
    for (int s = 0; s < 64; ++s) acc += (double)gs[wave][s] * (double)my[s * 65 + lane];
    wave_lds_sync();
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (tid < 64) part[(int64_t)blockIdx.x * 64 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// mom[f] = sum_w part[w][f]: thread (f, q) adds workgroups q, q + 4, ... in order, the four chains in a fixed order
__global__ __launch_bounds__(256) void k_eval_gmoments_sum(const double* __restrict__ part, int nwg,
                                                           double* __restrict__ mom) {
  __shared__ double red[4][64];
  const int f = threadIdx.x & 63, q = threadIdx.x >> 6;
  double acc = 0.0;
  for (int w = q; w < nwg; w += 4) acc += part[(int64_t)w * 64 + f];
  red[q][f] = acc;
  __syncthreads();
  if (q == 0) mom[f] = (red[0][f] + red[1][f]) + (red[2][f] + red[3][f]);
}

// sum_{n < 64} va[n] * w[n * ld] in float64, the loads issued in two batches of 32 before any use (nof_eval.hip's
// gemv_slice: load latency sets this kernel's time)
__device__ __forceinline__ double pg_gemv_slice(const float* __restrict__ w, int ld, const double* __restrict__ va) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int b = 0; b < 64; b += 32) {
    float x[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) x[j] = w[(size_t)(b + j) * ld];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j & 3] += va[b + j] * (double)x[j];
  }
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__device__ __forceinline__ void pg_add(float* __restrict__ dst, int i, double v) {
  if (dst) dst[i] += (float)v;
}

__global__ __launch_bounds__(1024) void k_eval_param_grads(NofParamsDev P, const double* __restrict__ mom,
                                                           pcnerf_nof_grads G) {
  // xs[L]: layer L's input X_L (L = 4: [m ; y_3]), xs[8] = y_7; xh[L] = (h_L - rm_L s0) / sqrt(rv_L + eps)
  __shared__ double xs[9][320];
  __shared__ double xh[8][256];
  __shared__ double ub[256], vb[256];
  __shared__ double ps[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = tid & 255, sl = tid >> 8;
  const int Lb = blockIdx.x;   // this workgroup's layer
  const double s0 = mom[63];
  if (tid < 63) {
    xs[0][tid] = mom[tid];
    xs[4][tid] = mom[tid];
  }
  __syncthreads();
  // forward: one wave per output row, lanes over the input columns (coalesced), the xor butterfly
  for (int L = 0; L < 8; ++L) {
    const int in_f = L == 0 ? 63 : L == 4 ? 319 : 256;
    const float* __restrict__ W = P.lin_w[L];
    const double* __restrict__ x = xs[L];
    double* __restrict__ y = L == 3 ? xs[4] + 63 : xs[L + 1];
    for (int n = wave; n < 256; n += 16) {
      const float* __restrict__ row = W + (size_t)n * in_f;
      double acc = 0.0;
      for (int k = lane; k < in_f; k += 64) acc += (double)row[k] * x[k];
      acc = wave_sum_d(acc);
      if (lane == 0) {
        const double h = acc + (double)P.lin_b[L][n] * s0;
        const double r = 1.0 / sqrt((double)P.bn_rv[L][n] + (double)P.eps);
        const double c = (h - (double)P.bn_rm[L][n] * s0) * r;
        xh[L][n] = c;
        y[n] = (double)P.bn_w[L][n] * c + (double)P.bn_b[L][n] * s0;
      }
    }
    __syncthreads();
  }
  if (Lb == 0) {
    if (tid < 256) pg_add(G.out_w, tid, xs[8][tid]);
    if (tid == 0) pg_add(G.out_b, 0, s0);
  }
  // backward down to this workgroup's layer: u_7 = out_w, v_L = u_L alpha_L, u_{L-1} = W_L^T v_L
  if (tid < 256) ub[tid] = (double)P.out_w[tid];
  __syncthreads();
  for (int L = 7; L >= Lb; --L) {
    const int in_f = L == 0 ? 63 : L == 4 ? 319 : 256;
    if (tid < 256) {
      const double u = ub[tid];
      const double v = u * ((double)P.bn_w[L][tid] / sqrt((double)P.bn_rv[L][tid] + (double)P.eps));
      vb[tid] = v;
      if (L == Lb) {
        pg_add(G.bn_b[L], tid, u * s0);
        pg_add(G.bn_w[L], tid, u * xh[L][tid]);
        pg_add(G.lin_b[L], tid, v * s0);
      }
    }
    __syncthreads();
    if (L == Lb) break;
    const int off = L == 4 ? 63 : 0;   // at the skip layer only the h_3 columns feed back
    ps[sl][t] = pg_gemv_slice(P.lin_w[L] + (size_t)(64 * sl) * in_f + off + t, in_f, vb + 64 * sl);
    __syncthreads();
    if (tid < 256) ub[tid] = (ps[0][tid] + ps[1][tid]) + (ps[2][tid] + ps[3][tid]);
    __syncthreads();
  }
  // dW_Lb = v (x) X: coalesced read-modify-write of the layer's gradient
  float* __restrict__ dW = G.lin_w[Lb];
  if (dW) {
    const int in_f = Lb == 0 ? 63 : Lb == 4 ? 319 : 256;
    const double* __restrict__ x = xs[Lb];
    for (int i = tid; i < 256 * in_f; i += 1024) {
      const int n = i / in_f, k = i - n * in_f;
      dW[i] += (float)(vb[n] * x[k]);
    }
  }
}

static size_t pgrad_workspace_bytes(int64_t total) {
  return (size_t)(64 + 64 * (int64_t)gm_workgroups(total)) * sizeof(double);
}

// the two launches of the moments stage: partials at workspace + 64 doubles, mom anywhere
template <int SRC>
static void launch_gmoments(const float* rays, int stride, const float* z, int S, const float* src, int64_t n,
                            const float* g, const float* p, void* workspace, double* mom, hipStream_t s) {
  double* part = reinterpret_cast<double*>(workspace) + 64;
  const int nwg = gm_workgroups(n);
  hipLaunchKernelGGL(k_eval_gmoments<SRC>, dim3(nwg), dim3(256), 0, s, rays, stride, z, S, src, n, g, p, part);
  hipLaunchKernelGGL(k_eval_gmoments_sum, dim3(1), dim3(256), 0, s, part, nwg, mom);
}

static void launch_param_grads(const NofParamsDev& P, const double* mom, const pcnerf_nof_grads* grads,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_eval_param_grads, dim3(8), dim3(1024), 0, s, P, mom, *grads);
}

}  // namespace pcn

using namespace pcn;

extern "C" size_t pcnerf_nof_eval_pgrad_workspace_bytes(int64_t total_samples) {
  return pgrad_workspace_bytes(total_samples < 0 ? 0 : total_samples);
}

#define PG_CHECK_RAYS(name)                                                  \
  PCN_CHECK(n_rays >= 0, name ": n_rays < 0");                               \
  PCN_CHECK(ray_stride >= 6, name ": ray_stride < 6");                       \
  PCN_CHECK(n_samples >= 1, name ": n_samples < 1")
#define PG_CHECK_WS(name, total)                                             \
  PCN_CHECK(workspace, name ": null argument");                              \
  PCN_CHECK(workspace_bytes >= pgrad_workspace_bytes(total), name ": workspace too small")

extern "C" int pcnerf_nof_eval_gmoments_rays(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                             int n_samples, const float* grad_logit, void* workspace,
                                             size_t workspace_bytes, double* mom, void* stream) {
  PCN_API_BEGIN
  PG_CHECK_RAYS("pcnerf_nof_eval_gmoments_rays");
  if (n_rays == 0) return 0;
  PCN_CHECK(rays && z && grad_logit && mom, "pcnerf_nof_eval_gmoments_rays: null argument");
  PG_CHECK_WS("pcnerf_nof_eval_gmoments_rays", n_rays * n_samples);
  launch_gmoments<0>(rays, ray_stride, z, n_samples, nullptr, n_rays * n_samples, grad_logit, nullptr, workspace, mom,
                     (hipStream_t)stream);
  PCN_LAUNCH_CHECK("pcnerf_nof_eval_gmoments_rays");
  PCN_API_END
}

extern "C" int pcnerf_nof_eval_gmoments_points(const float* pts, int64_t n, const float* grad_logit, void* workspace,
                                               size_t workspace_bytes, double* mom, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n >= 0, "pcnerf_nof_eval_gmoments_points: n < 0");
  if (n == 0) return 0;
  PCN_CHECK(pts && grad_logit && mom, "pcnerf_nof_eval_gmoments_points: null argument");
  PG_CHECK_WS("pcnerf_nof_eval_gmoments_points", n);
  launch_gmoments<1>(nullptr, 0, nullptr, 1, pts, n, grad_logit, nullptr, workspace, mom, (hipStream_t)stream);
  PCN_LAUNCH_CHECK("pcnerf_nof_eval_gmoments_points");
  PCN_API_END
}

extern "C" int pcnerf_nof_eval_gmoments_embedded(const float* emb, int64_t n, const float* p, const float* grad,
                                                 void* workspace, size_t workspace_bytes, double* mom, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n >= 0, "pcnerf_nof_eval_gmoments_embedded: n < 0");
  if (n == 0) return 0;
  PCN_CHECK(emb && grad && mom, "pcnerf_nof_eval_gmoments_embedded: null argument");
  PG_CHECK_WS("pcnerf_nof_eval_gmoments_embedded", n);
  launch_gmoments<2>(nullptr, 0, nullptr, 1, emb, n, grad, p, workspace, mom, (hipStream_t)stream);
  PCN_LAUNCH_CHECK("pcnerf_nof_eval_gmoments_embedded");
  PCN_API_END
}

extern "C" int pcnerf_nof_eval_param_grads(const pcnerf_nof_params* params, float eps, const double* mom,
                                           const pcnerf_nof_grads* grads, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(params && mom && grads, "pcnerf_nof_eval_param_grads: null argument");
  NofParamsDev P;
  PCN_CHECK(to_dev_params(params, eps, &P), "pcnerf_nof_eval_param_grads: null parameter pointer");
  launch_param_grads(P, mom, grads, (hipStream_t)stream);
  PCN_LAUNCH_CHECK("pcnerf_nof_eval_param_grads");
  PCN_API_END
}

extern "C" int pcnerf_nof_query_eval_param_backward(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                                    int n_samples, const pcnerf_nof_params* params, float eps,
                                                    const float* grad_logit, void* workspace, size_t workspace_bytes,
                                                    const pcnerf_nof_grads* grads, void* stream) {
  PCN_API_BEGIN
  PG_CHECK_RAYS("pcnerf_nof_query_eval_param_backward");
  if (n_rays == 0) return 0;
  PCN_CHECK(rays && z && grad_logit && params && grads, "pcnerf_nof_query_eval_param_backward: null argument");
  PG_CHECK_WS("pcnerf_nof_query_eval_param_backward", n_rays * n_samples);
  NofParamsDev P;
  PCN_CHECK(to_dev_params(params, eps, &P), "pcnerf_nof_query_eval_param_backward: null parameter pointer");
  double* mom = reinterpret_cast<double*>(workspace);
  launch_gmoments<0>(rays, ray_stride, z, n_samples, nullptr, n_rays * n_samples, grad_logit, nullptr, workspace, mom,
                     (hipStream_t)stream);
  launch_param_grads(P, mom, grads, (hipStream_t)stream);
  PCN_LAUNCH_CHECK("pcnerf_nof_query_eval_param_backward");
  PCN_API_END
}

extern "C" int pcnerf_nof_points_eval_param_backward(const float* pts, int64_t n, const pcnerf_nof_params* params,
                                                     float eps, const float* grad_logit, void* workspace,
                                                     size_t workspace_bytes, const pcnerf_nof_grads* grads,
                                                     void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n >= 0, "pcnerf_nof_points_eval_param_backward: n < 0");
  if (n == 0) return 0;
  PCN_CHECK(pts && grad_logit && params && grads, "pcnerf_nof_points_eval_param_backward: null argument");
  PG_CHECK_WS("pcnerf_nof_points_eval_param_backward", n);
  NofParamsDev P;
  PCN_CHECK(to_dev_params(params, eps, &P), "pcnerf_nof_points_eval_param_backward: null parameter pointer");
  double* mom = reinterpret_cast<double*>(workspace);
  launch_gmoments<1>(nullptr, 0, nullptr, 1, pts, n, grad_logit, nullptr, workspace, mom, (hipStream_t)stream);
  launch_param_grads(P, mom, grads, (hipStream_t)stream);
  PCN_LAUNCH_CHECK("pcnerf_nof_points_eval_param_backward");
  PCN_API_END
}

extern "C" int pcnerf_nof_forward_eval_param_backward(const float* emb, int64_t n, const pcnerf_nof_params* params,
                                                      float eps, const float* p, const float* grad_p, void* workspace,
                                                      size_t workspace_bytes, const pcnerf_nof_grads* grads,
                                                      void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n >= 0, "pcnerf_nof_forward_eval_param_backward: n < 0");
  if (n == 0) return 0;
  PCN_CHECK(emb && p && grad_p && params && grads, "pcnerf_nof_forward_eval_param_backward: null argument");
  PG_CHECK_WS("pcnerf_nof_forward_eval_param_backward", n);
  NofParamsDev P;
  PCN_CHECK(to_dev_params(params, eps, &P), "pcnerf_nof_forward_eval_param_backward: null parameter pointer");
  double* mom = reinterpret_cast<double*>(workspace);
  launch_gmoments<2>(nullptr, 0, nullptr, 1, emb, n, grad_p, p, workspace, mom, (hipStream_t)stream);
  launch_param_grads(P, mom, grads, (hipStream_t)stream);
  PCN_LAUNCH_CHECK("pcnerf_nof_forward_eval_param_backward");
  PCN_API_END
}
