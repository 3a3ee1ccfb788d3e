// The particle-filter update of Monte-Carlo localisation on the device, in float64: the block of every particle, the
// weights from the scores of pcnerf_score_poses_map, their normalisation and effective sample size, and systematic
// resampling with the decision taken on the device.  Nothing here reads a value back to the host.
//
//   k_assign_blocks        one thread per pose, a loop over the B boxes: the containing block with the largest
//                          clearance, the lowest index on ties, -1 for none or a NaN translation.
//   k_mcl_logw             logw_p = logw_prev_p - beta mean_p (localize_scan's mean cost), -inf without a block or with
//                          a non-finite mean; per workgroup the maximum and its lowest index (a fixed tree).
//   k_mcl_expsum           every workgroup reduces the per-workgroup maxima in the same fixed order (m, best), then
//                          e_p = exp(logw_p - m) and the workgroup's sums of e and e^2 (a fixed tree).
//   k_mcl_normalize        every workgroup reduces those sums in the same fixed order (Z, sum e^2), then
//                          w_p = e_p / Z, logw_p - m - log Z; workgroup 0 writes ess = Z^2 / sum e^2, best and the
//                          degenerate flag.  No finite logw: w = 1 / P, logw = 0, ess = P, degenerate = 1.
//   k_prefix_block_sums    per workgroup of 1,024 weights (256 threads x 4 contiguous, negative / NaN / infinite
//                          weights count as 0): its total and its last index with a positive weight.
//   k_prefix_scan_sums     one workgroup: the exclusive offsets off_{g+1} = off_g + T_g (one serial chain, so that the
//                          offset of a workgroup is bit for bit the last prefix sum of the one before), the total C
//                          and the last positive index.
//   k_prefix_local         c_i = off_g + local_i, local_i the workgroup's inclusive sum built the same way as T_g: a
//                          zero weight gives c_i == c_{i-1} exactly and c is non-decreasing.
//   k_systematic_resample  one thread per draw: u_j = (j + u0) / n_out * C, the first i with c_i > u_j (a binary search
//                          bounded by log2 P), clamped to the last positive index; the identity when ess >= the
//                          threshold (read from pcnerf_mcl_weights' output on the device).
//   k_mcl_gather           one thread per output word: poses12, block ids and log-weights of the ancestors (the
//                          log-weights kept under the identity, otherwise 0).
// No atomics, every output word has one writer, loops are bounded by P and B, every index is clamped, and launch
// geometry and summation order depend on P alone.
#include "pcnerf_internal.h"

namespace pcn {

constexpr int MC_T = 256;            // threads per workgroup
constexpr int MC_K = 4;              // contiguous weights per thread of the prefix kernels
constexpr int MC_E = MC_T * MC_K;    // weights per workgroup of the prefix kernels
// the particle limit of both entries: every workgroup of the weights re-reduces the per-workgroup partials, and one
// thread of the resampler walks the block totals (4,096 dependent adds at the limit)
constexpr int64_t MC_MAX_P = (int64_t)1 << 22;

__global__ __launch_bounds__(64) void k_assign_blocks(const double* __restrict__ poses12, int64_t n_poses,
                                                      const double* __restrict__ boxes6, int n_blocks, double margin,
                                                      int* __restrict__ block_of_pose) {
  const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (p >= n_poses) return;
  double t[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) t[m] = poses12[12 * p + 9 + m];
  int best = -1;
  double best_clear = 0.0;
  for (int b = 0; b < n_blocks; ++b) {
    bool in = true;
    double clear = 0.0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const double lo = boxes6[6 * b + m], hi = boxes6[6 * b + 3 + m];
      in = in && (lo + margin <= t[m]) && (t[m] <= hi - margin);   // (false for a NaN)
      const double c = fmin(t[m] - lo, hi - t[m]);
      clear = m == 0 ? c : fmin(clear, c);
    }
    if (in && (best < 0 || clear > best_clear)) {
      best = b;
      best_clear = clear;
    }
  }
  block_of_pose[p] = best;
}

// (v, i) of the larger value, the lower index on ties
__device__ __forceinline__ void mc_argmax(double& v, int& i, double v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

__global__ __launch_bounds__(MC_T) void k_mcl_logw(const double* __restrict__ logw_prev,
                                                   const double* __restrict__ scores4,
                                                   const int* __restrict__ block_of_pose,
                                                   const double* __restrict__ n_usable_ptr, double miss_cost,
                                                   double beta, int64_t n, double* __restrict__ logw_raw,
                                                   double* __restrict__ pmax, int* __restrict__ parg) {
  __shared__ double sv[MC_T];
  __shared__ int si[MC_T];
  const int tid = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * MC_T + tid;
  double v = -(double)INFINITY;
  int idx = 0x7fffffff;
  if (p < n) {
    const double n_usable = n_usable_ptr[0];
    const double cost = scores4[4 * p], n_valid = scores4[4 * p + 1];
    const double mean = (cost + miss_cost * (n_usable - n_valid)) / n_usable;
    double lw = logw_prev[p] - beta * mean;
    // no block, a non-finite mean, a NaN or +inf result: the particle carries no weight.  Precondition (header): the
    // ids are -1 .. B - 1, as pcnerf_assign_blocks writes them; the entry does not know B
    if (block_of_pose[p] < 0 || !isfinite(mean) || !(lw < (double)INFINITY)) lw = -(double)INFINITY;
    logw_raw[p] = lw;
    v = lw;
    idx = (int)p;
  }
  sv[tid] = v;
  si[tid] = idx;
  __syncthreads();
  for (int s = MC_T / 2; s > 0; s >>= 1) {
    if (tid < s) {
      double a = sv[tid];
      int ai = si[tid];
      mc_argmax(a, ai, sv[tid + s], si[tid + s]);
      sv[tid] = a;
      si[tid] = ai;
    }
    __syncthreads();
  }
  if (tid == 0) {
    pmax[blockIdx.x] = sv[0];
    parg[blockIdx.x] = si[0];
  }
}

// the maximum over the nwg partial maxima and its lowest index: thread t takes partials t, t + 256, ... in order, then
// a fixed tree; every thread of every workgroup ends with the same pair
__device__ __forceinline__ void mc_reduce_max(const double* __restrict__ pmax, const int* __restrict__ parg, int nwg,
                                              double* sv, int* si, double& m, int& best) {
  const int tid = threadIdx.x;
  double v = -(double)INFINITY;
  int idx = 0x7fffffff;
  for (int g = tid; g < nwg; g += MC_T) mc_argmax(v, idx, pmax[g], parg[g]);
  sv[tid] = v;
  si[tid] = idx;
  __syncthreads();
  for (int s = MC_T / 2; s > 0; s >>= 1) {
    if (tid < s) {
      double a = sv[tid];
      int ai = si[tid];
      mc_argmax(a, ai, sv[tid + s], si[tid + s]);
      sv[tid] = a;
      si[tid] = ai;
    }
    __syncthreads();
  }
  m = sv[0];
  best = si[0];
  __syncthreads();
}

__global__ __launch_bounds__(MC_T) void k_mcl_expsum(const double* __restrict__ logw_raw, int64_t n,
                                                     const double* __restrict__ pmax, const int* __restrict__ parg,
                                                     int nwg, double* __restrict__ e_out, double* __restrict__ psum,
                                                     double* __restrict__ psum2) {
  __shared__ double sv[MC_T];
  __shared__ double s2[MC_T];
  __shared__ int si[MC_T];
  const int tid = threadIdx.x;
  double m;
  int best;
  mc_reduce_max(pmax, parg, nwg, sv, si, m, best);
  const int64_t p = (int64_t)blockIdx.x * MC_T + tid;
  double e = 0.0;
  if (p < n) {
    const double lw = logw_raw[p];
    e = (lw == -(double)INFINITY) ? 0.0 : exp(lw - m);   // (m is finite wherever some lw is)
    e_out[p] = e;
  }
  sv[tid] = e;
  s2[tid] = e * e;
  __syncthreads();
  for (int s = MC_T / 2; s > 0; s >>= 1) {
    if (tid < s) {
      sv[tid] += sv[tid + s];
      s2[tid] += s2[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    psum[blockIdx.x] = sv[0];
    psum2[blockIdx.x] = s2[0];
  }
}

__global__ __launch_bounds__(MC_T) void k_mcl_normalize(const double* __restrict__ logw_raw,
                                                        const double* __restrict__ e_in, int64_t n,
                                                        const double* __restrict__ pmax, const int* __restrict__ parg,
                                                        const double* __restrict__ psum,
                                                        const double* __restrict__ psum2, int nwg,
                                                        double* __restrict__ w_out, double* __restrict__ logw_out,
                                                        double* __restrict__ ess_out, int* __restrict__ best_out,
                                                        int* __restrict__ degenerate_out) {
  __shared__ double sv[MC_T];
  __shared__ double s2[MC_T];
  __shared__ int si[MC_T];
  const int tid = threadIdx.x;
  double m;
  int best;
  mc_reduce_max(pmax, parg, nwg, sv, si, m, best);
  double a = 0.0, a2 = 0.0;
  for (int g = tid; g < nwg; g += MC_T) {
    a += psum[g];
    a2 += psum2[g];
  }
  sv[tid] = a;
  s2[tid] = a2;
  __syncthreads();
  for (int s = MC_T / 2; s > 0; s >>= 1) {
    if (tid < s) {
      sv[tid] += sv[tid + s];
      s2[tid] += s2[tid + s];
    }
    __syncthreads();
  }
  const double Z = sv[0], Z2 = s2[0];
  const bool degenerate = !(m > -(double)INFINITY);   // no finite logw
  const int64_t p = (int64_t)blockIdx.x * MC_T + tid;
  if (p < n) {
    if (degenerate) {
      w_out[p] = 1.0 / (double)n;
      logw_out[p] = 0.0;
    } else {
      const double lw = logw_raw[p];
      w_out[p] = e_in[p] / Z;
      logw_out[p] = (lw == -(double)INFINITY) ? lw : (lw - m) - log(Z);
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    ess_out[0] = degenerate ? (double)n : (Z * Z) / Z2;
    best_out[0] = best < n ? best : 0;
    degenerate_out[0] = degenerate ? 1 : 0;
  }
}

// a weight as the prefix sums count it
__device__ __forceinline__ double mc_weight(double w) { return (w > 0.0 && w < (double)INFINITY) ? w : 0.0; }

// The workgroup's 1,024 weights: thread t's K contiguous ones added in order (run[k] inclusive), the threads' bases by
// one serial chain base_{t+1} = base_t + tot_t from `start`.  Returns the base of this thread; *total (thread 0's
// chain end) is valid for every thread after the call.
__device__ __forceinline__ double mc_local_scan(const double* __restrict__ w, int64_t n, int64_t i0, double start,
                                                double (&run)[MC_K], double* tot, double* base, double* total) {
  const int tid = threadIdx.x;
  double r = 0.0;
#pragma unroll
  for (int k = 0; k < MC_K; ++k) {
    const int64_t i = i0 + k;
    r += i < n ? mc_weight(w[i]) : 0.0;
    run[k] = r;
  }
  tot[tid] = r;
  __syncthreads();
  if (tid == 0) {
    double b = start;
    for (int t = 0; t < MC_T; ++t) {
      base[t] = b;
      b += tot[t];
    }
    base[MC_T] = b;
  }
  __syncthreads();
  *total = base[MC_T];
  return base[tid];
}

__global__ __launch_bounds__(MC_T) void k_prefix_block_sums(const double* __restrict__ w, int64_t n,
                                                            double* __restrict__ totals, int* __restrict__ lastpos) {
  __shared__ double tot[MC_T];
  __shared__ double base[MC_T + 1];
  __shared__ int lp[MC_T];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * MC_E + (int64_t)tid * MC_K;
  double run[MC_K], total;
  mc_local_scan(w, n, i0, 0.0, run, tot, base, &total);
  int last = -1;
#pragma unroll
  for (int k = 0; k < MC_K; ++k) {
    const int64_t i = i0 + k;
    if (i < n && mc_weight(w[i]) > 0.0) last = (int)i;
  }
  lp[tid] = last;
  __syncthreads();
  for (int s = MC_T / 2; s > 0; s >>= 1) {
    if (tid < s) lp[tid] = max(lp[tid], lp[tid + s]);
    __syncthreads();
  }
  if (tid == 0) {
    totals[blockIdx.x] = total;
    lastpos[blockIdx.x] = lp[0];
  }
}

// offs[g] = the sum of totals[0 .. g - 1] as one serial chain; meta = [C]; last[0] = the last positive index or -1
__global__ __launch_bounds__(MC_T) void k_prefix_scan_sums(const double* __restrict__ totals,
                                                           const int* __restrict__ lastpos, int nwg,
                                                           double* __restrict__ offs, double* __restrict__ total_out,
                                                           int* __restrict__ last_out) {
  __shared__ int lp[MC_T];
  const int tid = threadIdx.x;
  int last = -1;
  for (int g = tid; g < nwg; g += MC_T) last = max(last, lastpos[g]);
  lp[tid] = last;
  __syncthreads();
  for (int s = MC_T / 2; s > 0; s >>= 1) {
    if (tid < s) lp[tid] = max(lp[tid], lp[tid + s]);
    __syncthreads();
  }
  if (tid == 0) {
    double b = 0.0;
    for (int g = 0; g < nwg; ++g) {
      offs[g] = b;
      b += totals[g];
    }
    total_out[0] = b;
    last_out[0] = lp[0];
  }
}

__global__ __launch_bounds__(MC_T) void k_prefix_local(const double* __restrict__ w, int64_t n,
                                                       const double* __restrict__ offs, double* __restrict__ c) {
  __shared__ double tot[MC_T];
  __shared__ double base[MC_T + 1];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * MC_E + (int64_t)tid * MC_K;
  double run[MC_K], total;
  const double b = mc_local_scan(w, n, i0, 0.0, run, tot, base, &total);
  const double off = offs[blockIdx.x];
#pragma unroll
  for (int k = 0; k < MC_K; ++k) {
    const int64_t i = i0 + k;
    if (i < n) c[i] = off + (b + run[k]);
  }
}

__global__ __launch_bounds__(MC_T) void k_systematic_resample(const double* __restrict__ c, int64_t n,
                                                              const double* __restrict__ total_ptr,
                                                              const int* __restrict__ last_ptr,
                                                              const double* __restrict__ u0_ptr,
                                                              const double* __restrict__ ess_ptr, double ess_threshold,
                                                              int64_t n_out, int* __restrict__ ancestors,
                                                              int* __restrict__ resampled_out) {
  const int64_t j = (int64_t)blockIdx.x * MC_T + threadIdx.x;
  // the decision, on the device: enough effective samples -> the identity (n_out == n was checked on the host)
  const bool keep = ess_ptr != nullptr && ess_ptr[0] >= ess_threshold;
  if (j == 0) resampled_out[0] = keep ? 0 : 1;
  if (j >= n_out) return;
  if (keep) {
    ancestors[j] = (int)(j < n ? j : n - 1);
    return;
  }
  const double C = total_ptr[0];
  double u0 = u0_ptr[0];
  if (!(u0 >= 0.0 && u0 < 1.0)) u0 = 0.0;
  const double u = ((double)j + u0) / (double)n_out * C;
  int64_t lo = 0, hi = n;   // the first i with c_i > u
  for (int it = 0; it < 40 && lo < hi; ++it) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid] <= u) lo = mid + 1; else hi = mid;
  }
  const int64_t last = max((int64_t)0, min((int64_t)last_ptr[0], n - 1));
  ancestors[j] = (int)min(lo, last);
}

// poses12_out[j] = poses12[a_j], blocks_out[j] = blocks[a_j], logw_out[j] = logw[a_j] under the identity, else 0
__global__ __launch_bounds__(MC_T) void k_mcl_gather(const int* __restrict__ ancestors, int64_t n, int64_t n_out,
                                                     const int* __restrict__ resampled,
                                                     const double* __restrict__ poses12,
                                                     const int* __restrict__ blocks, const double* __restrict__ logw,
                                                     double* __restrict__ poses12_out, int* __restrict__ blocks_out,
                                                     double* __restrict__ logw_out) {
  const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
  if (i >= n_out * 12) return;
  const int64_t j = i / 12;
  const int f = (int)(i - j * 12);
  const int64_t a = max((int64_t)0, min((int64_t)ancestors[j], n - 1));
  if (poses12_out) poses12_out[i] = poses12[12 * a + f];
  if (f == 0) {
    if (blocks_out) blocks_out[j] = blocks[a];
    if (logw_out) logw_out[j] = resampled[0] ? 0.0 : logw[a];
  }
}

inline int64_t mc_wg(int64_t n) { return (n + MC_T - 1) / MC_T; }
inline int64_t mc_pwg(int64_t n) { return (n + MC_E - 1) / MC_E; }
inline size_t mc_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace pcn

using namespace pcn;

extern "C" int pcnerf_assign_blocks(const double* poses12, int64_t n_poses, const double* boxes6, int n_blocks,
                                    double margin, int32_t* block_of_pose, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_poses >= 0, "pcnerf_assign_blocks: negative count");
  PCN_CHECK(n_blocks >= 1, "pcnerf_assign_blocks: n_blocks < 1");
  if (n_poses == 0) return 0;
  PCN_CHECK(poses12 && boxes6 && block_of_pose, "pcnerf_assign_blocks: null argument");
  PCN_CHECK(n_poses < (int64_t)1 << 31, "pcnerf_assign_blocks: too many poses for one launch");
  hipLaunchKernelGGL(k_assign_blocks, dim3((unsigned)((n_poses + 63) / 64)), dim3(64), 0, (hipStream_t)stream, poses12,
                     n_poses, boxes6, n_blocks, margin, block_of_pose);
  PCN_LAUNCH_CHECK("pcnerf_assign_blocks");
  PCN_API_END_NEG
}

// workspace: logw_raw (P) | e (P) | pmax, psum, psum2 (nwg each) | parg (nwg ints)
extern "C" size_t pcnerf_mcl_weights_workspace_bytes(int64_t n_particles) {
  if (n_particles <= 0) return 0;
  const size_t nwg = (size_t)mc_wg(n_particles);
  return mc_align(2 * (size_t)n_particles * sizeof(double)) + mc_align(3 * nwg * sizeof(double)) +
         mc_align(nwg * sizeof(int));
}

extern "C" int pcnerf_mcl_weights(const double* logw_prev, const double* scores4, const int32_t* block_of_pose,
                                  int64_t n_particles, const double* n_usable_dev, double miss_cost, double beta,
                                  void* workspace, size_t workspace_bytes, double* w, double* logw, double* ess,
                                  int32_t* best, int32_t* degenerate, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_particles >= 1, "pcnerf_mcl_weights: n_particles < 1");
  PCN_CHECK(n_particles <= MC_MAX_P, "pcnerf_mcl_weights: more than 4,194,304 particles");
  PCN_CHECK(logw_prev && scores4 && block_of_pose && n_usable_dev && workspace && w && logw && ess && best &&
                degenerate,
            "pcnerf_mcl_weights: null argument");
  PCN_CHECK(workspace_bytes >= pcnerf_mcl_weights_workspace_bytes(n_particles),
            "pcnerf_mcl_weights: workspace smaller than pcnerf_mcl_weights_workspace_bytes");
  const int64_t n = n_particles;
  const int nwg = (int)mc_wg(n);
  char* base = reinterpret_cast<char*>(workspace);
  double* logw_raw = reinterpret_cast<double*>(base);
  double* e = logw_raw + n;
  double* pmax = reinterpret_cast<double*>(base + mc_align(2 * (size_t)n * sizeof(double)));
  double* psum = pmax + nwg;
  double* psum2 = psum + nwg;
  int* parg = reinterpret_cast<int*>(reinterpret_cast<char*>(pmax) + mc_align(3 * (size_t)nwg * sizeof(double)));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mcl_logw, dim3((unsigned)nwg), dim3(MC_T), 0, s, logw_prev, scores4, block_of_pose,
                     n_usable_dev, miss_cost, beta, n, logw_raw, pmax, parg);
  hipLaunchKernelGGL(k_mcl_expsum, dim3((unsigned)nwg), dim3(MC_T), 0, s, logw_raw, n, pmax, parg, nwg, e, psum,
                     psum2);
  hipLaunchKernelGGL(k_mcl_normalize, dim3((unsigned)nwg), dim3(MC_T), 0, s, logw_raw, e, n, pmax, parg, psum, psum2,
                     nwg, w, logw, ess, best, degenerate);
  PCN_LAUNCH_CHECK("pcnerf_mcl_weights");
  PCN_API_END_NEG
}

// workspace: c (P) | totals, offs (nwg each), C (1) | lastpos (nwg ints), last (1), resampled (1)
extern "C" size_t pcnerf_systematic_resample_workspace_bytes(int64_t n_particles) {
  if (n_particles <= 0) return 0;
  const size_t nwg = (size_t)mc_pwg(n_particles);
  return mc_align((size_t)n_particles * sizeof(double)) + mc_align((2 * nwg + 1) * sizeof(double)) +
         mc_align((nwg + 2) * sizeof(int));
}

extern "C" int pcnerf_systematic_resample(const double* w, int64_t n_particles, const double* u0_dev, int64_t n_out,
                                          const double* ess_dev_or_null, double ess_threshold,
                                          const double* poses12_or_null, const int32_t* blocks_or_null,
                                          const double* logw_or_null, void* workspace, size_t workspace_bytes,
                                          int32_t* ancestors, double* poses12_out_or_null,
                                          int32_t* blocks_out_or_null, double* logw_out_or_null, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_particles >= 1, "pcnerf_systematic_resample: n_particles < 1");
  PCN_CHECK(n_out >= 1, "pcnerf_systematic_resample: n_out < 1");
  // (the serial chains of the prefix kernels: one thread walks ceil(n / 1024) block totals)
  PCN_CHECK(n_particles <= MC_MAX_P, "pcnerf_systematic_resample: more than 4,194,304 particles");
  PCN_CHECK(n_out * 12 < (int64_t)1 << 38, "pcnerf_systematic_resample: too many draws for one launch");
  PCN_CHECK(w && u0_dev && workspace && ancestors, "pcnerf_systematic_resample: null argument");
  PCN_CHECK(!ess_dev_or_null || n_out == n_particles,
            "pcnerf_systematic_resample: n_out != n_particles with the ESS switch on (the identity needs equal counts)");
  PCN_CHECK((!poses12_out_or_null || poses12_or_null) && (!blocks_out_or_null || blocks_or_null) &&
                (!logw_out_or_null || logw_or_null),
            "pcnerf_systematic_resample: an output without its input");
  PCN_CHECK(workspace_bytes >= pcnerf_systematic_resample_workspace_bytes(n_particles),
            "pcnerf_systematic_resample: workspace smaller than pcnerf_systematic_resample_workspace_bytes");
  const int64_t n = n_particles;
  const int nwg = (int)mc_pwg(n);
  char* base = reinterpret_cast<char*>(workspace);
  double* c = reinterpret_cast<double*>(base);
  double* totals = reinterpret_cast<double*>(base + mc_align((size_t)n * sizeof(double)));
  double* offs = totals + nwg;
  double* total = offs + nwg;
  int* lastpos = reinterpret_cast<int*>(reinterpret_cast<char*>(totals) +
                                        mc_align((2 * (size_t)nwg + 1) * sizeof(double)));
  int* last = lastpos + nwg;
  int* resampled = last + 1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_prefix_block_sums, dim3((unsigned)nwg), dim3(MC_T), 0, s, w, n, totals, lastpos);
  hipLaunchKernelGGL(k_prefix_scan_sums, dim3(1), dim3(MC_T), 0, s, totals, lastpos, nwg, offs, total, last);
  hipLaunchKernelGGL(k_prefix_local, dim3((unsigned)nwg), dim3(MC_T), 0, s, w, n, offs, c);
  hipLaunchKernelGGL(k_systematic_resample, dim3((unsigned)((n_out + MC_T - 1) / MC_T)), dim3(MC_T), 0, s, c, n, total,
                     last, u0_dev, ess_dev_or_null, ess_threshold, n_out, ancestors, resampled);
  if (poses12_out_or_null || blocks_out_or_null || logw_out_or_null)
    hipLaunchKernelGGL(k_mcl_gather, dim3((unsigned)((n_out * 12 + MC_T - 1) / MC_T)), dim3(MC_T), 0, s, ancestors, n,
                       n_out, resampled, poses12_or_null, blocks_or_null, logw_or_null, poses12_out_or_null,
                       blocks_out_or_null, logw_out_or_null);
  PCN_LAUNCH_CHECK("pcnerf_systematic_resample");
  PCN_API_END_NEG
}
