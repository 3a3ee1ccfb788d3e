// Localisation against a map of B parent blocks: localize.hip's scoring and refine.hip's Gauss-Newton evaluation with
// every pose rendered against ITS OWN block (its pair of fold vectors and its box), in one launch for the whole
// hypothesis set.  The numbered steps are fold_render.h's, unchanged: for a pose with block b every output has the
// bits the single-block kernels give for that pose with block b's folds and box.
//
//   k_score_poses_map<MAXB>    k_score_poses_fold's layout: one wave per (pose, beam), four beams per 256-thread
//                              workgroup, ceil(R / 4) workgroups per pose.  A workgroup never straddles two poses, so
//                              the prologue reads block_of_pose[pose] (uniform) and stages folds_c[b], folds_f[b],
//                              boxes[b] and the pose through LDS.  An index outside 0 .. B - 1 renders nothing: the
//                              workgroup writes its zero partial (and NaN depth, zero sumw when asked for) and returns
//                              before the first barrier; nothing is indexed with it.  The rolled two-pass loop with
//                              its single copy of fr_pass is kept.
//   k_score_map_sum            k_score_poses_sum's chains and tree.
//   k_pose_normal_eq_map<MAXB> k_pose_normal_eq_fold's render, Jacobian and 29 terms with the per-pose block; the
//                              stopped-pose early return and the no-block early return (no partial is written).
//   k_pose_normal_eq_map_sum   k_pose_normal_eq_sum's chains and tree; the row of a stopped pose and of a pose without
//                              a block is zeroed, so pcnerf_lm_update stops the latter with status 2 (zero valid beams)
//                              at the first update.
// pcnerf_refine_poses_map enqueues pcnerf_lm_init, iters x (evaluation, sum, pcnerf_lm_update) and the pose output:
// the state layout, the init and the state machine are refine.hip's (the two sums, the record init and the pose output
// are copies of its kernels, which have no entries of their own).  Beams are clipped at their block's box exit; there
// is no compositing across blocks.  No atomics, every output word has one writer, geometry and summation order depend
// on (P, R) alone.
#include "fold_render.h"

namespace pcn {

constexpr int MS_W = 4;    // localize.hip's partial: cost, n_valid, sum |r|, sum sumw
constexpr int MN_W = 32;   // refine.hip's partial: 21 + 6 + cost + n_valid, padded
constexpr int ML_STATE = PCNERF_LM_STATE_DOUBLES;
constexpr int ML_TACC = 0, ML_TTRIAL = 12, ML_STATUS = 55;   // the state's fields (include/pcnerf_hip.h)

// the block of a pose, or -1: never index with anything else
__device__ __forceinline__ int map_block(const int* __restrict__ block_of_pose, int64_t pose, int n_blocks) {
  const int b = block_of_pose[pose];
  return (b >= 0 && b < n_blocks) ? b : -1;
}

template <int MAXB>
__global__ __launch_bounds__(256) void k_score_poses_map(
    const float* __restrict__ points, int64_t n_beams, const double* __restrict__ poses12,
    const int* __restrict__ block_of_pose, int n_blocks, int bpp, const double* __restrict__ boxes6, float near, int S,
    int I, const double* __restrict__ folds_c, const double* __restrict__ folds_f, float eps, double delta_arg,
    double min_sumw_arg, double* __restrict__ part, float* __restrict__ depth_out, float* __restrict__ sumw_out) {
  extern __shared__ float sm_lds[];
  __shared__ double fa[2][64];
  __shared__ double red[4][MS_W];
  __shared__ double pb[20];   // [R row-major (9), t (3), lo (3), hi (3), huber_delta, min_sumw]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t pose = blockIdx.x / (unsigned)bpp;
  const int64_t beam = (int64_t)(blockIdx.x - (unsigned)pose * (unsigned)bpp) * 4 + wave;
  const int b = map_block(block_of_pose, pose, n_blocks);
  if (b < 0) {   // (uniform across the workgroup, before the first barrier)
    if (tid < MS_W) part[(int64_t)blockIdx.x * MS_W + tid] = 0.0;
    if (lane == 0 && beam < n_beams) {
      const int64_t g = pose * n_beams + beam;
      if (depth_out) depth_out[g] = __builtin_nanf("");
      if (sumw_out) sumw_out[g] = 0.0f;
    }
    return;
  }
  if (tid < 128) fa[tid >> 6][lane] = (tid < 64 ? folds_c : folds_f)[64 * b + lane];
  else if (tid < 140) pb[tid - 128] = poses12[12 * pose + (tid - 128)];
  else if (tid < 146) pb[tid - 128] = boxes6[6 * b + (tid - 140)];
  else if (tid < 148) pb[tid - 128] = tid == 146 ? delta_arg : min_sumw_arg;
  __syncthreads();
  double term[MS_W] = {0.0, 0.0, 0.0, 0.0};
  if (beam < n_beams) {   // (wave-uniform: the shuffles below always have 64 lanes)
    float* zc = sm_lds + (size_t)wave * fr_slice_floats(S, I);
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
    // 3. and 5.: the coarse pass on zc, then the fine pass on the merged depths (a rolled loop: one copy of the pass)
    double dep = 0.0, hit = 0.0, unused[6];
    const float* zs = zc;
    int ns = S;
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
      fr_pass<MAXB, false>(row, zs, ns, fa[pass], eps, lane, pass == 0 ? ws : nullptr, dep, hit, unused);
      if (pass == 1) break;
      zs = zf;
      ns = S + I;
      wave_lds_sync();
      fr_resample_merge(zc, fs, ws, cdf, zf, S, I, lane);   // 4.
    }
    // 6. residual terms, on the float32 values the composed route hands to pcnerf_gn_normal_eq
    const float dv = (float)dep, sv = (float)hit;
    const double delta = pb[18], min_sumw = pb[19];
    const bool usable = gn_target_usable(target);
    if (gn_beam_valid(dv, sv, target, min_sumw)) {
      const double res = (double)dv - (double)target;
      double w, rho;
      gn_huber(res, delta, w, rho);
      term[0] = rho;
      term[1] = 1.0;
      term[2] = fabs(res);
    }
    if (usable) term[3] = (double)sv;
    if (lane == 0) {
      const int64_t g = pose * n_beams + beam;
      if (depth_out) depth_out[g] = dv;
      if (sumw_out) sumw_out[g] = sv;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < MS_W; ++f) red[wave][f] = term[f];
  }
  __syncthreads();
  if (tid < MS_W)
    part[(int64_t)blockIdx.x * MS_W + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// scores4[p][f] = sum_w part[p bpp + w][f]: thread (f, q) adds partials q, q + 64, ... in order, then a fixed tree
// (k_score_poses_sum's order)
__global__ __launch_bounds__(256) void k_score_map_sum(const double* __restrict__ part, int bpp,
                                                       double* __restrict__ scores4) {
  __shared__ double red[64][MS_W];
  const int f = threadIdx.x & 3, q = threadIdx.x >> 2;
  const double* __restrict__ pp = part + (int64_t)blockIdx.x * bpp * MS_W;
  double acc = 0.0;
  for (int w = q; w < bpp; w += 64) acc += pp[(int64_t)w * MS_W + f];
  red[q][f] = acc;
  __syncthreads();
  for (int s = 32; s > 0; s >>= 1) {
    if (q < s) red[q][f] += red[q + s][f];
    __syncthreads();
  }
  if (q == 0) scores4[(int64_t)blockIdx.x * MS_W + f] = red[0][f];
}

template <int MAXB>
__global__ __launch_bounds__(256) void k_pose_normal_eq_map(
    const float* __restrict__ points, int64_t n_beams, const double* __restrict__ poses12,
    const double* __restrict__ state, const int* __restrict__ block_of_pose, int n_blocks, int bpp,
    const double* __restrict__ boxes6, float near, int S, int I, const double* __restrict__ folds_c,
    const double* __restrict__ folds_f, float eps, double delta_arg, double min_sumw_arg, double* __restrict__ part,
    float* __restrict__ depth_out, float* __restrict__ sumw_out, float* __restrict__ jac_out) {
  extern __shared__ float mn_lds[];
  __shared__ double fa[2][64];
  __shared__ double red[4][MN_W];
  __shared__ double pb[20];   // [R row-major (9), t (3), lo (3), hi (3), huber_delta, min_sumw]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t pose = blockIdx.x / (unsigned)bpp;
  // a stopped pose and a pose without a block cost nothing further (uniform, before the first barrier)
  if (state && state[ML_STATE * pose + ML_STATUS] != 0.0) return;
  const int b = map_block(block_of_pose, pose, n_blocks);
  if (b < 0) return;
  const double* __restrict__ psrc = state ? state + ML_STATE * pose + ML_TTRIAL : poses12 + 12 * pose;
  if (tid < 128) fa[tid >> 6][lane] = (tid < 64 ? folds_c : folds_f)[64 * b + lane];
  else if (tid < 140) pb[tid - 128] = psrc[tid - 128];
  else if (tid < 146) pb[tid - 128] = boxes6[6 * b + (tid - 140)];
  else if (tid < 148) pb[tid - 128] = tid == 146 ? delta_arg : min_sumw_arg;
  __syncthreads();
  const int64_t beam = (int64_t)(blockIdx.x - (unsigned)pose * (unsigned)bpp) * 4 + wave;
  double mine = 0.0;   // lane k < 29: term k of this wave's beam
  if (beam < n_beams) {   // (wave-uniform: the shuffles below always have 64 lanes)
    float* zc = mn_lds + (size_t)wave * fr_slice_floats(S, I);
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
  if (lane < MN_W) red[wave][lane] = mine;
  __syncthreads();
  if (tid < MN_W)
    part[(int64_t)blockIdx.x * MN_W + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// k_pose_normal_eq_sum's order: thread (f, q) adds partials q, q + 8, ... in order, the eight chains in a fixed tree.
// The row of a stopped pose or of a pose without a block is zeroed (its partials were not written).
__global__ __launch_bounds__(256) void k_pose_normal_eq_map_sum(const double* __restrict__ part, int bpp,
                                                                const double* __restrict__ state,
                                                                const int* __restrict__ block_of_pose, int n_blocks,
                                                                double* __restrict__ normal30) {
  __shared__ double red[8][MN_W];
  const int f = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int64_t pose = blockIdx.x;
  if ((state && state[ML_STATE * pose + ML_STATUS] != 0.0) || map_block(block_of_pose, pose, n_blocks) < 0) {
    if (threadIdx.x < 30) normal30[30 * pose + threadIdx.x] = 0.0;   // (uniform across the workgroup)
    return;
  }
  const double* __restrict__ pp = part + pose * bpp * MN_W;
  double acc = 0.0;
  for (int w = q; w < bpp; w += 8) acc += pp[(int64_t)w * MN_W + f];
  red[q][f] = acc;
  __syncthreads();
  if (q == 0 && f < 30)
    normal30[30 * pose + f] =
        ((red[0][f] + red[1][f]) + (red[2][f] + red[3][f])) + ((red[4][f] + red[5][f]) + (red[6][f] + red[7][f]));
}

__global__ __launch_bounds__(64) void k_map_records_init(int64_t n, double* __restrict__ eval_costs,
                                                         uint8_t* __restrict__ accepted) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  eval_costs[i] = __builtin_nan("");
  accepted[i] = 0;
}

// poses12_out = T_trial, or T_acc where the pose is undetermined or the solve failed.  A COPY of refine.hip's
// k_lm_poses_out, which has no entry of its own: the rule (T_acc for status 2 or 3) lives in both files and must be
// changed in both (test_map_localization_gpu compares the two entries' poses bit for bit)
__global__ __launch_bounds__(64) void k_map_poses_out(const double* __restrict__ state, int64_t n_poses,
                                                      double* __restrict__ poses12_out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n_poses * 12) return;
  const int64_t p = i / 12;
  const int f = (int)(i - p * 12);
  const double* __restrict__ st = state + ML_STATE * p;
  const double s = st[ML_STATUS];
  poses12_out[i] = st[(s == 2.0 || s == 3.0 ? ML_TACC : ML_TTRIAL) + f];
}

inline unsigned map_blocks64(int64_t n) { return (unsigned)((n + 63) / 64); }

// every check a map launch makes on its operands, before anything is launched (n_poses > 0, n_beams > 0)
void map_check(const char* name, const float* points, int64_t n_beams, int64_t n_poses, const int* block_of_pose,
               int n_blocks, const double* boxes6, const double* folds_c, const double* folds_f, void* workspace,
               size_t workspace_bytes, size_t need_bytes, const char* size_fn) {
  const std::string who(name);
  PCN_CHECK(points && block_of_pose && boxes6 && folds_c && folds_f && workspace, who + ": null argument");
  PCN_CHECK(n_blocks >= 1, who + ": n_blocks < 1");
  PCN_CHECK(workspace_bytes >= need_bytes, who + ": workspace smaller than " + size_fn);
  fr_check_pairs(name, n_poses, n_beams);
}

void map_launch_eval(const float* points, int64_t n_beams, const double* poses12, int64_t n_poses, const double* state,
                     const int* block_of_pose, int n_blocks, const double* boxes6, float near, int S, int I,
                     const double* folds_c, const double* folds_f, float eps, double delta, double min_sumw,
                     void* workspace, double* normal30, float* depth, float* sumw, float* jac6, hipStream_t stream) {
  if (n_beams == 0) {
    PCN_HIP(hipMemsetAsync(normal30, 0, (size_t)n_poses * 30 * sizeof(double), stream));
    return;
  }
  const int64_t bpp = fr_blocks_per_pose(n_beams);
  const size_t lds = (size_t)4 * fr_slice_floats(S, I) * sizeof(float);   // <= 48 KiB
  double* part = reinterpret_cast<double*>(workspace);
  fr_dispatch_maxb(S + I, [&](auto mb) {
    hipLaunchKernelGGL(k_pose_normal_eq_map<decltype(mb)::value>, dim3((unsigned)(n_poses * bpp)), dim3(256), lds,
                       stream, points, n_beams, poses12, state, block_of_pose, n_blocks, (int)bpp, boxes6, near, S, I,
                       folds_c, folds_f, eps, delta, min_sumw, part, depth, sumw, jac6);
  });
  hipLaunchKernelGGL(k_pose_normal_eq_map_sum, dim3((unsigned)n_poses), dim3(256), 0, stream, part, (int)bpp, state,
                     block_of_pose, n_blocks, normal30);
}

}  // namespace pcn

using namespace pcn;

extern "C" int pcnerf_score_poses_map(const float* points_sensor, int64_t n_beams, const double* poses12,
                                      int64_t n_poses, const int32_t* block_of_pose, int n_blocks,
                                      const double* boxes6, float near, int n_samples, int n_importance,
                                      const double* folds_coarse, const double* folds_fine, float eps,
                                      double huber_delta, double min_sumw, void* workspace, size_t workspace_bytes,
                                      double* scores4, float* depth_or_null, float* sumw_or_null, void* stream) {
  PCN_API_BEGIN
  const char* who = "pcnerf_score_poses_map";
  PCN_CHECK(n_poses >= 0 && n_beams >= 0, "pcnerf_score_poses_map: negative count");
  fr_check_samples(who, n_samples, n_importance);
  if (n_poses == 0) return 0;
  PCN_CHECK(scores4, "pcnerf_score_poses_map: null argument");
  if (n_beams == 0) {
    PCN_HIP(hipMemsetAsync(scores4, 0, (size_t)n_poses * MS_W * sizeof(double), (hipStream_t)stream));
    return 0;
  }
  PCN_CHECK(poses12, "pcnerf_score_poses_map: null argument");
  map_check(who, points_sensor, n_beams, n_poses, block_of_pose, n_blocks, boxes6, folds_coarse, folds_fine, workspace,
            workspace_bytes, pcnerf_score_poses_workspace_bytes(n_poses, n_beams),
            "pcnerf_score_poses_workspace_bytes");
  const int64_t bpp = fr_blocks_per_pose(n_beams);
  const size_t lds = (size_t)4 * fr_slice_floats(n_samples, n_importance) * sizeof(float);   // <= 48 KiB
  double* part = reinterpret_cast<double*>(workspace);
  fr_dispatch_maxb(n_samples + n_importance, [&](auto mb) {
    hipLaunchKernelGGL(k_score_poses_map<decltype(mb)::value>, dim3((unsigned)(n_poses * bpp)), dim3(256), lds,
                       (hipStream_t)stream, points_sensor, n_beams, poses12, block_of_pose, n_blocks, (int)bpp, boxes6,
                       near, n_samples, n_importance, folds_coarse, folds_fine, eps, huber_delta, min_sumw, part,
                       depth_or_null, sumw_or_null);
  });
  hipLaunchKernelGGL(k_score_map_sum, dim3((unsigned)n_poses), dim3(256), 0, (hipStream_t)stream, part, (int)bpp,
                     scores4);
  PCN_LAUNCH_CHECK(who);
  PCN_API_END_NEG
}

extern "C" int pcnerf_pose_normal_eq_map(const float* points_sensor, int64_t n_beams, const double* poses12_or_null,
                                         int64_t n_poses, const double* state_or_null, const int32_t* block_of_pose,
                                         int n_blocks, const double* boxes6, float near, int n_samples,
                                         int n_importance, const double* folds_coarse, const double* folds_fine,
                                         float eps, double huber_delta, double min_sumw, void* workspace,
                                         size_t workspace_bytes, double* normal30, float* depth_or_null,
                                         float* sumw_or_null, float* jac6_or_null, void* stream) {
  PCN_API_BEGIN
  const char* who = "pcnerf_pose_normal_eq_map";
  PCN_CHECK(n_poses >= 0 && n_beams >= 0, "pcnerf_pose_normal_eq_map: negative count");
  fr_check_samples(who, n_samples, n_importance);
  if (n_poses == 0) return 0;
  PCN_CHECK(normal30 && (poses12_or_null || state_or_null), "pcnerf_pose_normal_eq_map: null argument");
  if (n_beams > 0)
    map_check(who, points_sensor, n_beams, n_poses, block_of_pose, n_blocks, boxes6, folds_coarse, folds_fine,
              workspace, workspace_bytes, pcnerf_pose_normal_eq_workspace_bytes(n_poses, n_beams),
              "pcnerf_pose_normal_eq_workspace_bytes");
  map_launch_eval(points_sensor, n_beams, poses12_or_null, n_poses, state_or_null, block_of_pose, n_blocks, boxes6,
                  near, n_samples, n_importance, folds_coarse, folds_fine, eps, huber_delta, min_sumw, workspace,
                  normal30, depth_or_null, sumw_or_null, jac6_or_null, (hipStream_t)stream);
  PCN_LAUNCH_CHECK(who);
  PCN_API_END_NEG
}

extern "C" int pcnerf_refine_poses_map(const float* points_sensor, int64_t n_beams, const double* poses12,
                                       int64_t n_poses, const int32_t* block_of_pose, int n_blocks,
                                       const double* boxes6, float near, int n_samples, int n_importance,
                                       const double* folds_coarse, const double* folds_fine, float eps,
                                       double huber_delta, double min_sumw, double damping, double xi_tol, int iters,
                                       void* workspace, size_t workspace_bytes, double* normal30, double* state,
                                       double* poses12_out, double* eval_costs, uint8_t* accepted, void* stream) {
  PCN_API_BEGIN
  const char* who = "pcnerf_refine_poses_map";
  PCN_CHECK(n_poses >= 0 && n_beams >= 0, "pcnerf_refine_poses_map: negative count");
  PCN_CHECK(iters >= 0, "pcnerf_refine_poses_map: iters < 0");
  fr_check_samples(who, n_samples, n_importance);
  if (n_poses == 0) return 0;
  PCN_CHECK(poses12 && normal30 && state && poses12_out, "pcnerf_refine_poses_map: null argument");
  PCN_CHECK(iters == 0 || (eval_costs && accepted), "pcnerf_refine_poses_map: null argument");
  PCN_CHECK(n_poses < (int64_t)1 << 31 && n_poses * ((int64_t)iters + ML_STATE) < (int64_t)1 << 37,
            "pcnerf_refine_poses_map: too many poses for one launch");   // (one thread per state / record word)
  if (n_beams > 0)
    map_check(who, points_sensor, n_beams, n_poses, block_of_pose, n_blocks, boxes6, folds_coarse, folds_fine,
              workspace, workspace_bytes, pcnerf_pose_normal_eq_workspace_bytes(n_poses, n_beams),
              "pcnerf_pose_normal_eq_workspace_bytes");
  else
    PCN_CHECK(block_of_pose, "pcnerf_refine_poses_map: null argument");
  hipStream_t s = (hipStream_t)stream;
  // refine.hip's init and update through their entries: both only check and enqueue
  PCN_CHECK(pcnerf_lm_init(poses12, n_poses, damping, state, stream) == 0, pcnerf_last_error());
  PCN_HIP(hipMemsetAsync(normal30, 0, (size_t)n_poses * 30 * sizeof(double), s));
  if (iters > 0)
    hipLaunchKernelGGL(k_map_records_init, dim3(map_blocks64(n_poses * iters)), dim3(64), 0, s, n_poses * iters,
                       eval_costs, accepted);
  for (int it = 0; it < iters; ++it) {   // stream order is the only synchronisation between evaluations
    map_launch_eval(points_sensor, n_beams, nullptr, n_poses, state, block_of_pose, n_blocks, boxes6, near, n_samples,
                    n_importance, folds_coarse, folds_fine, eps, huber_delta, min_sumw, workspace, normal30, nullptr,
                    nullptr, nullptr, s);
    PCN_CHECK(pcnerf_lm_update(normal30, n_poses, xi_tol, state, eval_costs, accepted, it, iters, stream) == 0,
              pcnerf_last_error());
  }
  hipLaunchKernelGGL(k_map_poses_out, dim3(map_blocks64(n_poses * 12)), dim3(64), 0, s, state, n_poses, poses12_out);
  PCN_LAUNCH_CHECK(who);
  PCN_API_END_NEG
}
