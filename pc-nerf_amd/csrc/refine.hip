// Batched pose refinement against folded eval networks: damped Gauss-Newton (Levenberg-Marquardt) on the range
// residuals of one scan for many poses at once, with no host synchronisation between evaluations.  Every pose is
// refined against ITS OWN block of a map of B blocks, fixed for the call; a single block is the map with B = 1 in
// which every pose has block 0: the same kernel body with that written in at compile time (MAP = false).  An
// evaluation is three launches in stream order:
//
//   k_pose_normal_eq<MAXB, MAP>
//                           k_score_poses' layout (localize.hip): one wave per (pose, beam), four beams per
//                           256-thread workgroup, ceil(R / 4) workgroups per pose; the folds and the box of the
//                           pose's block (MAP: fr_block_of; the single-block entries compile b = 0 in), the pose and
//                           the loss parameters through LDS; per wave an LDS slice zc (S) | draws (I) | weights +
//                           cdf, aliased by the merged depths.  Steps 1-5 are fold_render.h's, the same bits of
//                           depth and sumw as that kernel's; here two instantiations of the pass: the coarse one
//                           carries no Jacobian, the fine one k_render_jac_fold's (register.hip).  Then
//                           k_gn_normal_eq's terms on the float32 depth, sumw, jac6 and ray row, one term per lane:
//                           21 of H's upper triangle, 6 of b, rho(r) and 1.  The four waves' terms are added in
//                           wave order into one 32-double partial per workgroup.  Nothing per sample goes through
//                           memory.  A workgroup whose pose has status != 0 (the state the previous launch wrote)
//                           returns before its first barrier, and so does one whose pose has no block (an index
//                           outside 0 .. B - 1, never used to index); both tests are uniform across the workgroup
//                           and no partial is written.
//   k_pose_normal_eq_sum    one workgroup per pose adds its ceil(R / 4) partials, eight chains (partials q, q + 8,
//                           ...) and a fixed tree, into normal30[pose] (pcnerf_gn_normal_eq's out30); the row of a
//                           stopped pose and of a pose without a block is zeroed, so k_lm_update stops the latter
//                           with status 2 (zero valid beams) at the first update.
//   k_lm_update             one thread per pose, float64: nof.registration.register_scan_fold's state machine
//                           (accept / reject, lambda / 10 or x 10, the 6 x 6 solve by elimination with partial
//                           pivoting, T <- se3_exp(xi) T), kept fully in registers.
//   k_se3_apply             poses12_out[p] = se3_exp(xi[p]) poses12[p] with the same device function.
// pcnerf_pose_normal_eq_fold / _map and pcnerf_refine_poses_fold / _map are thin entries over pn_normal_eq and
// lm_refine_poses: the fold entries hand over no table, B = 1 and their one box and pair of folds.  Beams are clipped
// at their block's box exit; there is no compositing across blocks.
// No atomics, every output word has one writer, and geometry and summation order depend on (P, R) alone: a pose
// refines to the same bits alone or in a batch, with or without the per-beam outputs, as block b of a map or against
// block b alone.  NaN rays are not counted.
#include "fold_render.h"

namespace pcn {

constexpr int PN_W = 32;         // doubles per partial: 21 + 6 + cost + n_valid, padded (normal30 rows hold 30)
constexpr int LM_STATE = PCNERF_LM_STATE_DOUBLES;
// the state's fields (include/pcnerf_hip.h)
constexpr int LM_TACC = 0, LM_TTRIAL = 12, LM_N30 = 24, LM_LAMBDA = 54, LM_STATUS = 55, LM_EVALS = 56, LM_NACC = 57,
              LM_XI = 58;

template <int MAXB, bool MAP>
__global__ __launch_bounds__(256) void k_pose_normal_eq(
    const float* __restrict__ points, int64_t n_beams, const double* __restrict__ poses12,
    const double* __restrict__ state, const int* __restrict__ block_of_pose, int n_blocks, int bpp,
    const double* __restrict__ boxes6, float near, int S, int I, const double* __restrict__ folds_c,
    const double* __restrict__ folds_f, float eps, double delta_arg, double min_sumw_arg, double* __restrict__ part,
    float* __restrict__ depth_out, float* __restrict__ sumw_out, float* __restrict__ jac_out) {
  extern __shared__ float pn_lds[];
  __shared__ double fa[2][64];
  __shared__ double red[4][PN_W];
  __shared__ double pb[20];   // [R row-major (9), t (3), lo (3), hi (3), huber_delta, min_sumw]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t pose = blockIdx.x / (unsigned)bpp;
  // a stopped pose and a pose without a block cost nothing further (uniform, before the first barrier)
  if (state && state[LM_STATE * pose + LM_STATUS] != 0.0) return;
  const int b = MAP ? fr_block_of(block_of_pose, pose, n_blocks) : 0;
  if (MAP && b < 0) return;
  const double* __restrict__ psrc = state ? state + LM_STATE * pose + LM_TTRIAL : poses12 + 12 * pose;
  if (tid < 128) fa[tid >> 6][lane] = (tid < 64 ? folds_c : folds_f)[64 * b + lane];
  else if (tid < 140) pb[tid - 128] = psrc[tid - 128];
  else if (tid < 146) pb[tid - 128] = boxes6[6 * b + (tid - 140)];
  else if (tid < 148) pb[tid - 128] = tid == 146 ? delta_arg : min_sumw_arg;
  __syncthreads();
  const int64_t beam = (int64_t)(blockIdx.x - (unsigned)pose * (unsigned)bpp) * 4 + wave;
  double mine = 0.0;   // lane k < 29: term k of this wave's beam
  if (beam < n_beams) {   // (wave-uniform: the shuffles below always have 64 lanes)
    float* zc = pn_lds + (size_t)wave * fr_slice_floats(S, I);
    float* fs = zc + S;
    float* ws = fs + I;      // coarse weights (S)
    float* cdf = ws + S;     // (S - 1)
    float* zf = ws;          // the merged depths (S + I): ws and cdf are dead when it is written
    // 1. the ray (every lane the same values)
    float row[6], far, target;
    fr_pose_ray(pb, points + 3 * beam, near, row, far, target);
    // 2. coarse depths
#pragma nounroll
    for (int i = lane; i < S; i += 64) zc[i] = lerp_z(near, far, linspace01(i, S));
    wave_lds_sync();
    // 3. the coarse pass (no Jacobian), 4. resampling and the merge, 5. the fine pass with its Jacobian
    double dep = 0.0, hit = 0.0, jac[6];
    fr_pass<MAXB, false>(row, zc, S, fa[0], eps, lane, ws, dep, hit, jac);
    wave_lds_sync();
    fr_resample_merge(zc, fs, ws, cdf, zf, S, I, lane);
    fr_pass<MAXB, true>(row, zf, S + I, fa[1], eps, lane, nullptr, dep, hit, jac);
    // 6. k_gn_normal_eq's terms, on the float32 values the composed route hands to it
    const float dv = (float)dep, sv = (float)hit;
    float jf[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) jf[m] = (float)jac[m];
    const double delta = pb[18], min_sumw = pb[19];
    if (gn_beam_valid(dv, sv, target, min_sumw)) {
      double Jp[6], w, rho;
      gn_pose_jacobian(row, jf, Jp);
      const double res = (double)dv - (double)target;
      gn_huber(res, delta, w, rho);
      int k = 0;
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        const double wj = w * Jp[p];
#pragma unroll
        for (int q = p; q < 6; ++q) {
          if (lane == k) mine = wj * Jp[q];
          ++k;
        }
        if (lane == 21 + p) mine = wj * res;
      }
      if (lane == 27) mine = rho;
      if (lane == 28) mine = 1.0;
    }
    if (lane == 0) {
      const int64_t g = pose * n_beams + beam;
      if (depth_out) depth_out[g] = dv;
      if (sumw_out) sumw_out[g] = sv;
      if (jac_out) {
#pragma unroll
        for (int m = 0; m < 6; ++m) jac_out[6 * g + m] = jf[m];
      }
    }
  }
  if (lane < PN_W) red[wave][lane] = mine;
  __syncthreads();
  if (tid < PN_W)
    part[(int64_t)blockIdx.x * PN_W + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// normal30[p][f] = sum_w part[p bpp + w][f]: thread (f, q) adds partials q, q + 8, ... in order, the eight chains in a
// fixed tree.  The row of a stopped pose or of a pose without a block is zeroed (its partials were not written).
__global__ __launch_bounds__(256) void k_pose_normal_eq_sum(const double* __restrict__ part, int bpp,
                                                            const double* __restrict__ state,
                                                            const int* __restrict__ block_of_pose, int n_blocks,
                                                            double* __restrict__ normal30) {
  __shared__ double red[8][PN_W];
  const int f = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int64_t pose = blockIdx.x;
  if ((state && state[LM_STATE * pose + LM_STATUS] != 0.0) ||
      (block_of_pose && fr_block_of(block_of_pose, pose, n_blocks) < 0)) {   // (no table: the single block)
    if (threadIdx.x < 30) normal30[30 * pose + threadIdx.x] = 0.0;   // (uniform across the workgroup)
    return;
  }
  const double* __restrict__ pp = part + pose * bpp * PN_W;
  double acc = 0.0;
  for (int w = q; w < bpp; w += 8) acc += pp[(int64_t)w * PN_W + f];
  red[q][f] = acc;
  __syncthreads();
  if (q == 0 && f < 30)
    normal30[30 * pose + f] =
        ((red[0][f] + red[1][f]) + (red[2][f] + red[3][f])) + ((red[4][f] + red[5][f]) + (red[6][f] + red[7][f]));
}

// ------------------------------------------------------------------------------------------------ SE(3), float64
// sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3 without cancellation: nof.registration._abc's branches and series
__device__ __forceinline__ void lm_abc(double theta, double& a, double& b, double& c) {
  a = theta < 1e-8 ? 1.0 : sin(theta) / theta;
  const double h = 0.5 * theta;
  const double sh = h < 1e-8 ? 1.0 : sin(h) / h;
  b = 0.5 * sh * sh;
  if (theta < 0.5) {
    const double t2 = theta * theta;
    double term = 1.0 / 6.0;
    c = 0.0;
#pragma unroll
    for (int k = 1; k < 9; ++k) {   // 1/3! - t^2/5! + t^4/7! - ...
      c += term;
      term *= -t2 / (double)((2 * k + 2) * (2 * k + 3));
    }
  } else {
    c = (theta - sin(theta)) / (theta * theta * theta);
  }
}

// out = se3_exp(xi) T on 12-double rows [R row-major (9), t (3)], xi = (rho, phi)
__device__ __forceinline__ void lm_se3_exp_apply(const double (&xi)[6], const double (&T)[12], double (&out)[12]) {
  const double x = xi[3], y = xi[4], z = xi[5];
  const double theta = sqrt((x * x + y * y) + z * z);
  double a, b, c;
  lm_abc(theta, a, b, c);
  const double K[3][3] = {{0.0, -z, y}, {z, 0.0, -x}, {-y, x, 0.0}};
  double E[3][3], te[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double vr = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
      const double eye = i == j ? 1.0 : 0.0;
      E[i][j] = (eye + a * K[i][j]) + b * k2;
      const double v = (eye + b * K[i][j]) + c * k2;
      vr = j == 0 ? v * xi[0] : vr + v * xi[j];
    }
    te[i] = vr;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * i + j] = (E[i][0] * T[j] + E[i][1] * T[3 + j]) + E[i][2] * T[6 + j];
    out[9 + i] = ((E[i][0] * T[9] + E[i][1] * T[10]) + E[i][2] * T[11]) + te[i];
  }
}

// xi of (H + lam diag H) xi = -b, H's upper triangle and b from a normal30 row: elimination with partial pivoting
// (the first largest |entry| of the column, as LAPACK's), every index static.  false: a zero pivot or a non-finite xi.
__device__ __forceinline__ bool lm_solve(const double* __restrict__ n30, double lam, double (&xi)[6]) {
  double A[6][7];
  {
    int k = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
#pragma unroll
      for (int q = p; q < 6; ++q) {
        A[p][q] = n30[k];
        A[q][p] = n30[k];
        ++k;
      }
    }
  }
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    A[p][p] = A[p][p] + lam * A[p][p];
    A[p][6] = -n30[21 + p];
  }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    double best = fabs(A[c][c]);
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double v = fabs(A[r][c]);
      if (v > best) {
        best = v;
        piv = r;
      }
    }
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      if (r == piv) {
#pragma unroll
        for (int q = c; q < 7; ++q) {
          const double t = A[c][q];
          A[c][q] = A[r][q];
          A[r][q] = t;
        }
      }
    }
    const double pv = A[c][c];
    if (pv == 0.0) ok = false;
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double l = A[r][c] / pv;
#pragma unroll
      for (int q = c + 1; q < 7; ++q) A[r][q] -= l * A[c][q];
    }
  }
#pragma unroll
  for (int r = 5; r >= 0; --r) {
    double s = A[r][6];
#pragma unroll
    for (int q = r + 1; q < 6; ++q) s -= A[r][q] * xi[q];
    xi[r] = s / A[r][r];
    ok = ok && isfinite(xi[r]);
  }
  return ok;
}

__global__ __launch_bounds__(64) void k_lm_init(const double* __restrict__ poses12, int64_t n_poses, double damping,
                                                double* __restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;   // one thread per state word
  if (i >= n_poses * LM_STATE) return;
  const int64_t p = i / LM_STATE;
  const int f = (int)(i - p * LM_STATE);
  double v = 0.0;
  if (f < LM_N30) v = poses12[12 * p + (f < 12 ? f : f - 12)];   // T_acc = T_trial = the start
  else if (f == LM_LAMBDA) v = damping;
  state[i] = v;
}

__global__ __launch_bounds__(64) void k_lm_records_init(int64_t n, double* __restrict__ eval_costs,
                                                        uint8_t* __restrict__ accepted) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  if (eval_costs) eval_costs[i] = __builtin_nan("");
  if (accepted) accepted[i] = 0;
}

// register_scan_fold's state machine for one evaluation of every running pose (one thread per pose)
__global__ __launch_bounds__(64) void k_lm_update(const double* __restrict__ normal30, int64_t n_poses, double xi_tol,
                                                  double* __restrict__ state, double* __restrict__ eval_costs,
                                                  uint8_t* __restrict__ accepted, int iter_index, int iters) {
  const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (p >= n_poses) return;
  double* __restrict__ st = state + LM_STATE * p;
  if (st[LM_STATUS] != 0.0) return;
  const double* __restrict__ nq = normal30 + 30 * p;
  const double cost = nq[27], n_valid = nq[28];
  st[LM_EVALS] = st[LM_EVALS] + 1.0;
  const bool rec = iter_index >= 0 && iter_index < iters;
  if (rec && eval_costs) eval_costs[p * iters + iter_index] = cost;
  if (!(n_valid >= 6.0)) {   // the pose is not determined
    st[LM_STATUS] = 2.0;
    return;
  }
  double lam = st[LM_LAMBDA];
  const double nacc = st[LM_NACC];
  if (nacc == 0.0 || cost <= st[LM_N30 + 27]) {   // (a NaN cost: a rejection once something is accepted)
    if (nacc != 0.0) lam = lam / 10.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) st[LM_TACC + k] = st[LM_TTRIAL + k];
#pragma unroll
    for (int k = 0; k < 30; ++k) st[LM_N30 + k] = nq[k];
    st[LM_NACC] = nacc + 1.0;
    if (rec && accepted) accepted[p * iters + iter_index] = 1;
  } else {
    lam = lam * 10.0;
  }
  st[LM_LAMBDA] = lam;
  double xi[6], Ta[12], Tn[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) Ta[k] = st[LM_TACC + k];
  if (!lm_solve(st + LM_N30, lam, xi)) {   // the pose stays at the last accepted one
    st[LM_STATUS] = 3.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) st[LM_TTRIAL + k] = Ta[k];
    return;
  }
  lm_se3_exp_apply(xi, Ta, Tn);
  double n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    st[LM_XI + k] = xi[k];
    n2 += xi[k] * xi[k];
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) st[LM_TTRIAL + k] = Tn[k];
  if (sqrt(n2) < xi_tol) st[LM_STATUS] = 1.0;   // (the pose includes this last step)
}

// poses12_out = T_trial, or T_acc where the pose is undetermined or the solve failed
__global__ __launch_bounds__(64) void k_lm_poses_out(const double* __restrict__ state, int64_t n_poses,
                                                     double* __restrict__ poses12_out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n_poses * 12) return;
  const int64_t p = i / 12;
  const int f = (int)(i - p * 12);
  const double* __restrict__ st = state + LM_STATE * p;
  const double s = st[LM_STATUS];
  poses12_out[i] = st[(s == 2.0 || s == 3.0 ? LM_TACC : LM_TTRIAL) + f];
}

__global__ __launch_bounds__(64) void k_se3_apply(const double* __restrict__ xi6, const double* __restrict__ poses12,
                                                  int64_t n_poses, double* __restrict__ poses12_out) {
  const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (p >= n_poses) return;
  double xi[6], T[12], out[12];
#pragma unroll
  for (int k = 0; k < 6; ++k) xi[k] = xi6[6 * p + k];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = poses12[12 * p + k];
  lm_se3_exp_apply(xi, T, out);
#pragma unroll
  for (int k = 0; k < 12; ++k) poses12_out[12 * p + k] = out[k];
}

inline unsigned lm_blocks(int64_t n) { return (unsigned)((n + 63) / 64); }

size_t pn_workspace_bytes(int64_t n_poses, int64_t n_beams) {
  if (n_poses <= 0 || n_beams <= 0) return 0;
  return (size_t)n_poses * (size_t)fr_blocks_per_pose(n_beams) * PN_W * sizeof(double);
}

// The map a call renders against.  The single-block entries pass {false, nullptr, 1, box, fold, fold}: block 0 of 1
// for every pose (the MAP = false kernels); with_table: a map entry, whose block_of_pose must be given.
struct PnMap {
  bool with_table;
  const int* block_of_pose;
  int n_blocks;
  const double *boxes6, *folds_c, *folds_f;
};

// every check an evaluation makes, before anything is launched (n_poses > 0)
void pn_check_eval(const char* name, const float* points, int64_t n_beams, int64_t n_poses, const PnMap& m,
                   void* workspace, size_t workspace_bytes) {
  const std::string who(name);
  if (n_beams == 0) return;
  PCN_CHECK(points && (m.block_of_pose || !m.with_table) && m.boxes6 && m.folds_c && m.folds_f && workspace,
            who + ": null argument");
  PCN_CHECK(m.n_blocks >= 1, who + ": n_blocks < 1");
  PCN_CHECK(workspace_bytes >= pn_workspace_bytes(n_poses, n_beams),
            who + ": workspace smaller than pcnerf_pose_normal_eq_workspace_bytes");
  fr_check_pairs(name, n_poses, n_beams);
}

// one evaluation of all running poses (checked by pn_check_eval); n_poses > 0
void pn_launch_eval(const float* points, int64_t n_beams, const double* poses12, int64_t n_poses, const double* state,
                    const PnMap& m, float near, int S, int I, float eps, double delta, double min_sumw,
                    void* workspace, double* normal30, float* depth, float* sumw, float* jac6, hipStream_t stream) {
  if (n_beams == 0) {
    PCN_HIP(hipMemsetAsync(normal30, 0, (size_t)n_poses * 30 * sizeof(double), stream));
    return;
  }
  const int64_t bpp = fr_blocks_per_pose(n_beams);
  const size_t lds = (size_t)4 * fr_slice_floats(S, I) * sizeof(float);   // <= 48 KiB
  double* part = reinterpret_cast<double*>(workspace);
  fr_dispatch_maxb(S + I, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    const auto kernel = m.with_table ? &k_pose_normal_eq<MB, true> : &k_pose_normal_eq<MB, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n_poses * bpp)), dim3(256), lds, stream, points, n_beams, poses12,
                       state, m.block_of_pose, m.n_blocks, (int)bpp, m.boxes6, near, S, I, m.folds_c, m.folds_f, eps,
                       delta, min_sumw, part, depth, sumw, jac6);
  });
  hipLaunchKernelGGL(k_pose_normal_eq_sum, dim3((unsigned)n_poses), dim3(256), 0, stream, part, (int)bpp, state,
                     m.block_of_pose, m.n_blocks, normal30);
}

// pcnerf_pose_normal_eq_fold and _map: `name` prefixes the error texts
int pn_normal_eq(const char* name, const float* points, int64_t n_beams, const double* poses12_or_null,
                 int64_t n_poses, const double* state_or_null, const PnMap& m, float near, int S, int I, float eps,
                 double huber_delta, double min_sumw, void* workspace, size_t workspace_bytes, double* normal30,
                 float* depth_or_null, float* sumw_or_null, float* jac6_or_null, hipStream_t stream) {
  PCN_API_BEGIN
  const std::string who(name);
  PCN_CHECK(n_poses >= 0 && n_beams >= 0, who + ": negative count");
  fr_check_samples(name, S, I);
  if (n_poses == 0) return 0;
  PCN_CHECK(normal30 && (poses12_or_null || state_or_null), who + ": null argument");
  pn_check_eval(name, points, n_beams, n_poses, m, workspace, workspace_bytes);
  pn_launch_eval(points, n_beams, poses12_or_null, n_poses, state_or_null, m, near, S, I, eps, huber_delta, min_sumw,
                 workspace, normal30, depth_or_null, sumw_or_null, jac6_or_null, stream);
  PCN_LAUNCH_CHECK(name);
  PCN_API_END_NEG
}

// pcnerf_refine_poses_fold and _map: the init, iters x (evaluation, sum, update) and the pose output in stream order
int lm_refine_poses(const char* name, const float* points, int64_t n_beams, const double* poses12, int64_t n_poses,
                    const PnMap& m, float near, int S, int I, float eps, double huber_delta, double min_sumw,
                    double damping, double xi_tol, int iters, void* workspace, size_t workspace_bytes,
                    double* normal30, double* state, double* poses12_out, double* eval_costs, uint8_t* accepted,
                    hipStream_t s) {
  PCN_API_BEGIN
  const std::string who(name);
  PCN_CHECK(n_poses >= 0 && n_beams >= 0, who + ": negative count");
  PCN_CHECK(iters >= 0, who + ": iters < 0");
  fr_check_samples(name, S, I);
  if (n_poses == 0) return 0;
  PCN_CHECK(poses12 && normal30 && state && poses12_out, who + ": null argument");
  PCN_CHECK(iters == 0 || (eval_costs && accepted), who + ": null argument");
  PCN_CHECK(n_poses < (int64_t)1 << 31 && n_poses * ((int64_t)iters + LM_STATE) < (int64_t)1 << 37,
            who + ": too many poses for one launch");   // (one thread per state / record word)
  pn_check_eval(name, points, n_beams, n_poses, m, workspace, workspace_bytes);
  if (n_beams == 0)   // (a refinement over a map wants its table even when no beam reads it)
    PCN_CHECK(m.block_of_pose || !m.with_table, who + ": null argument");
  hipLaunchKernelGGL(k_lm_init, dim3(lm_blocks(n_poses * LM_STATE)), dim3(64), 0, s, poses12, n_poses, damping,
                     state);
  PCN_HIP(hipMemsetAsync(normal30, 0, (size_t)n_poses * 30 * sizeof(double), s));
  if (iters > 0)
    hipLaunchKernelGGL(k_lm_records_init, dim3(lm_blocks(n_poses * iters)), dim3(64), 0, s, n_poses * iters,
                       eval_costs, accepted);
  for (int it = 0; it < iters; ++it) {   // stream order is the only synchronisation between evaluations
    pn_launch_eval(points, n_beams, nullptr, n_poses, state, m, near, S, I, eps, huber_delta, min_sumw, workspace,
                   normal30, nullptr, nullptr, nullptr, s);
    hipLaunchKernelGGL(k_lm_update, dim3(lm_blocks(n_poses)), dim3(64), 0, s, normal30, n_poses, xi_tol, state,
                       eval_costs, accepted, it, iters);
  }
  hipLaunchKernelGGL(k_lm_poses_out, dim3(lm_blocks(n_poses * 12)), dim3(64), 0, s, state, n_poses, poses12_out);
  PCN_LAUNCH_CHECK(name);
  PCN_API_END_NEG
}

}  // namespace pcn

using namespace pcn;

extern "C" size_t pcnerf_pose_normal_eq_workspace_bytes(int64_t n_poses, int64_t n_beams) {
  return pn_workspace_bytes(n_poses, n_beams);
}

extern "C" int pcnerf_pose_normal_eq_fold(const float* points_sensor, int64_t n_beams, const double* poses12_or_null,
                                          int64_t n_poses, const double* state_or_null, const double* parent_box6,
                                          float near, int n_samples, int n_importance, const double* fold_coarse,
                                          const double* fold_fine, float eps, double huber_delta, double min_sumw,
                                          void* workspace, size_t workspace_bytes, double* normal30,
                                          float* depth_or_null, float* sumw_or_null, float* jac6_or_null,
                                          void* stream) {
  return pn_normal_eq("pcnerf_pose_normal_eq_fold", points_sensor, n_beams, poses12_or_null, n_poses, state_or_null,
                      {false, nullptr, 1, parent_box6, fold_coarse, fold_fine}, near, n_samples, n_importance, eps,
                      huber_delta, min_sumw, workspace, workspace_bytes, normal30, depth_or_null, sumw_or_null,
                      jac6_or_null, (hipStream_t)stream);
}

extern "C" int pcnerf_pose_normal_eq_map(const float* points_sensor, int64_t n_beams, const double* poses12_or_null,
                                         int64_t n_poses, const double* state_or_null, const int32_t* block_of_pose,
                                         int n_blocks, const double* boxes6, float near, int n_samples,
                                         int n_importance, const double* folds_coarse, const double* folds_fine,
                                         float eps, double huber_delta, double min_sumw, void* workspace,
                                         size_t workspace_bytes, double* normal30, float* depth_or_null,
                                         float* sumw_or_null, float* jac6_or_null, void* stream) {
  return pn_normal_eq("pcnerf_pose_normal_eq_map", points_sensor, n_beams, poses12_or_null, n_poses, state_or_null,
                      {true, block_of_pose, n_blocks, boxes6, folds_coarse, folds_fine}, near, n_samples, n_importance,
                      eps, huber_delta, min_sumw, workspace, workspace_bytes, normal30, depth_or_null, sumw_or_null,
                      jac6_or_null, (hipStream_t)stream);
}

extern "C" int pcnerf_lm_init(const double* poses12, int64_t n_poses, double damping, double* state, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_poses >= 0, "pcnerf_lm_init: negative count");
  if (n_poses == 0) return 0;
  PCN_CHECK(poses12 && state, "pcnerf_lm_init: null argument");
  PCN_CHECK(n_poses < (int64_t)1 << 31, "pcnerf_lm_init: too many poses for one launch");
  hipLaunchKernelGGL(k_lm_init, dim3(lm_blocks(n_poses * LM_STATE)), dim3(64), 0, (hipStream_t)stream, poses12,
                     n_poses, damping, state);
  PCN_LAUNCH_CHECK("pcnerf_lm_init");
  PCN_API_END_NEG
}

extern "C" int pcnerf_lm_update(const double* normal30, int64_t n_poses, double xi_tol, double* state,
                                double* eval_costs_or_null, uint8_t* accepted_or_null, int iter_index, int iters,
                                void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_poses >= 0, "pcnerf_lm_update: negative count");
  if (eval_costs_or_null || accepted_or_null)
    PCN_CHECK(iter_index >= 0 && iter_index < iters, "pcnerf_lm_update: iter_index outside [0, iters)");
  if (n_poses == 0) return 0;
  PCN_CHECK(normal30 && state, "pcnerf_lm_update: null argument");
  PCN_CHECK(n_poses < (int64_t)1 << 31, "pcnerf_lm_update: too many poses for one launch");
  hipLaunchKernelGGL(k_lm_update, dim3(lm_blocks(n_poses)), dim3(64), 0, (hipStream_t)stream, normal30, n_poses,
                     xi_tol, state, eval_costs_or_null, accepted_or_null, iter_index, iters);
  PCN_LAUNCH_CHECK("pcnerf_lm_update");
  PCN_API_END_NEG
}

extern "C" int pcnerf_refine_poses_fold(const float* points_sensor, int64_t n_beams, const double* poses12,
                                        int64_t n_poses, const double* parent_box6, float near, int n_samples,
                                        int n_importance, const double* fold_coarse, const double* fold_fine,
                                        float eps, double huber_delta, double min_sumw, double damping, double xi_tol,
                                        int iters, void* workspace, size_t workspace_bytes, double* normal30,
                                        double* state, double* poses12_out, double* eval_costs, uint8_t* accepted,
                                        void* stream) {
  return lm_refine_poses("pcnerf_refine_poses_fold", points_sensor, n_beams, poses12, n_poses,
                         {false, nullptr, 1, parent_box6, fold_coarse, fold_fine}, near, n_samples, n_importance, eps,
                         huber_delta, min_sumw, damping, xi_tol, iters, workspace, workspace_bytes, normal30, state,
                         poses12_out, eval_costs, accepted, (hipStream_t)stream);
}

extern "C" int pcnerf_refine_poses_map(const float* points_sensor, int64_t n_beams, const double* poses12,
                                       int64_t n_poses, const int32_t* block_of_pose, int n_blocks,
                                       const double* boxes6, float near, int n_samples, int n_importance,
                                       const double* folds_coarse, const double* folds_fine, float eps,
                                       double huber_delta, double min_sumw, double damping, double xi_tol, int iters,
                                       void* workspace, size_t workspace_bytes, double* normal30, double* state,
                                       double* poses12_out, double* eval_costs, uint8_t* accepted, void* stream) {
  return lm_refine_poses("pcnerf_refine_poses_map", points_sensor, n_beams, poses12, n_poses,
                         {true, block_of_pose, n_blocks, boxes6, folds_coarse, folds_fine}, near, n_samples,
                         n_importance, eps, huber_delta, min_sumw, damping, xi_tol, iters, workspace, workspace_bytes,
                         normal30, state, poses12_out, eval_costs, accepted, (hipStream_t)stream);
}

extern "C" int pcnerf_se3_apply(const double* xi6, const double* poses12, int64_t n_poses, double* poses12_out,
                                void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_poses >= 0, "pcnerf_se3_apply: negative count");
  if (n_poses == 0) return 0;
  PCN_CHECK(xi6 && poses12 && poses12_out, "pcnerf_se3_apply: null argument");
  PCN_CHECK(n_poses < (int64_t)1 << 31, "pcnerf_se3_apply: too many poses for one launch");
  hipLaunchKernelGGL(k_se3_apply, dim3(lm_blocks(n_poses)), dim3(64), 0, (hipStream_t)stream, xi6, poses12, n_poses,
                     poses12_out);
  PCN_LAUNCH_CHECK("pcnerf_se3_apply");
  PCN_API_END_NEG
}
