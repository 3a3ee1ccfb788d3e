// Pose-hypothesis scoring against folded eval networks: the whole two-pass render of a scan (rays from the pose,
// coarse depths, coarse pass, deterministic resampling, fine pass) and the per-pose reduction of the range residuals
// in one launch, with nothing per sample through memory.  Every pose is rendered against ITS OWN block of a map of B
// blocks (its pair of fold vectors and its box); a single block is the map with B = 1 in which every pose has block
// 0, and is the same kernel body with that written in at compile time (MAP = false).  The numbered steps are
// fold_render.h's, shared with refine.hip and register.hip.
//
//   k_score_poses<MAXB, MAP>
//                        one wave per (pose, beam), four beams per 256-thread workgroup, ceil(R / 4) workgroups per
//                        pose.  A workgroup never straddles two poses, so its prologue takes the pose's block b
//                        (MAP: fr_block_of, uniform; the single-block entry compiles b = 0 in) and stages folds_c[b],
//                        folds_f[b], boxes[b], the pose and the loss parameters through LDS (as scalars they spilled
//                        SGPRs).  An index outside 0 .. B - 1 renders nothing: the workgroup writes its zero partial
//                        (and NaN depth, zero sumw when asked for) and returns before the first barrier; nothing is
//                        indexed with it.  Per wave, in its own LDS slice zc (S) | fs (I) | max(2 S, S + I) floats:
//                          1. the world ray (fr_pose_ray);
//                          2. zc = k_sample_coarse's plain path, lerp_z(near, far, linspace01(i, S));
//                          3. the coarse pass (fr_pass), the normalised weights rounded once to float32 into LDS;
//                          4. fr_resample_merge;
//                          5. the fine pass on the S + I merged depths -> depth, sumw, each rounded once;
//                          6. r = depth - rng on the float32 values, rho(r) as k_gn_normal_eq's cost term.
//                        The two passes share one rolled loop, so there is a single copy of the pass: the scalar
//                        register file is full, and unrolled forms spilled it.  The four waves' terms (rho, 1, |r|
//                        over the valid beams; sumw over the usable ones) are added in wave order into one 4-double
//                        partial per workgroup.
//   k_score_poses_sum    one workgroup per pose adds its ceil(R / 4) partials: 64 chains (partials q, q + 64, ...),
//                        then a fixed tree.
//   k_score_poses_through<MAXB>
//                        k_score_poses' geometry, prologue, early return and partial, with the beam carried through
//                        the blocks it crosses.  Segment 0 is k_score_poses' render (the same bits).  After segment k
//                        with float64 exit te, lane l tests blocks l, l + 64, ... (fr_box_interval on the boxes in
//                        memory, fr_next_candidate: tin <= te + seam_tol, tout > te, no NaN, non-empty in float32) and
//                        a wave reduction picks the largest tout, the lowest index on ties; tout > te strictly, so te
//                        grows and no block comes twice.  Segment k + 1 is steps 2 to 5 again for the unchanged ray
//                        from near = (float)max(te, tin) to that box's exit, with the block's folds reloaded into the
//                        WAVE's own pair (2 x 64 doubles of LDS per wave: the beams of a workgroup part ways after
//                        segment 0; its float64 ray waits in LDS for the search, not in registers through the
//                        passes: that cost a wave of occupancy).  fr_chain_step composites the segments' float32
//                        (depth, sumw) in float64; the chain ends at max_segments, at T <= min_transmittance or without a candidate.  One segment:
//                        its depth and sumw untouched; otherwise depth = N / (W + eps), sumw = W, and step 6 as
//                        before.  (Segment, pass) is one rolled nest around the single copy of fr_pass; no workgroup
//                        barrier between the prologue and the final add; loops bounded by S, I, B and max_segments.
// pcnerf_score_poses_fold (no table, B = 1, its one box and pair of folds) and pcnerf_score_poses_map are thin entries
// over one host function.  Beams are clipped at their block's box exit; there is no compositing across blocks unless
// asked: pcnerf_score_poses_through.
// No atomics, every output word has one writer, and geometry and summation order depend on (P, R) alone: a pose scores
// the same bits alone or in a batch, with or without the per-beam outputs, as block b of a map or against block b
// alone.  NaN rays are not counted.
#include "fold_render.h"

namespace pcn {

constexpr int SP_W = 4;   // doubles per partial and per pose: cost, n_valid, sum |r|, sum sumw

template <int MAXB, bool MAP>
__global__ __launch_bounds__(256) void k_score_poses(
    const float* __restrict__ points, int64_t n_beams, const double* __restrict__ poses12,
    const int* __restrict__ block_of_pose, int n_blocks, int bpp, const double* __restrict__ boxes6, float near, int S,
    int I, const double* __restrict__ folds_c, const double* __restrict__ folds_f, float eps, double delta_arg,
    double min_sumw_arg, double* __restrict__ part, float* __restrict__ depth_out, float* __restrict__ sumw_out) {
  extern __shared__ float sp_lds[];
  __shared__ double fa[2][64];
  __shared__ double red[4][SP_W];
  __shared__ double pb[20];   // [R row-major (9), t (3), lo (3), hi (3), huber_delta, min_sumw]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t pose = blockIdx.x / (unsigned)bpp;
  const int64_t beam = (int64_t)(blockIdx.x - (unsigned)pose * (unsigned)bpp) * 4 + wave;
  const int b = MAP ? fr_block_of(block_of_pose, pose, n_blocks) : 0;
  if (MAP && b < 0) {   // (uniform across the workgroup, before the first barrier)
    if (tid < SP_W) part[(int64_t)blockIdx.x * SP_W + tid] = 0.0;
    if (lane == 0 && beam < n_beams) {
      const int64_t g = pose * n_beams + beam;
      if (depth_out) depth_out[g] = __builtin_nanf("");
      if (sumw_out) sumw_out[g] = 0.0f;
    }
    return;
  }
  if (tid < 128) fa[tid >> 6][lane] = (tid < 64 ? folds_c : folds_f)[64 * b + lane];
  else if (tid < 140) pb[tid - 128] = poses12[12 * pose + (tid - 128)];   // the workgroup's pose and the box through
  else if (tid < 146) pb[tid - 128] = boxes6[6 * b + (tid - 140)];        // LDS: vector registers, not 36 scalar ones
  else if (tid < 148) pb[tid - 128] = tid == 146 ? delta_arg : min_sumw_arg;   // (needed last: not held in scalars)
  __syncthreads();
  double term[SP_W] = {0.0, 0.0, 0.0, 0.0};
  if (beam < n_beams) {   // (wave-uniform: the shuffles below always have 64 lanes)
    float* zc = sp_lds + (size_t)wave * fr_slice_floats(S, I);
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
    for (int f = 0; f < SP_W; ++f) red[wave][f] = term[f];
  }
  __syncthreads();
  if (tid < SP_W)
    part[(int64_t)blockIdx.x * SP_W + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// k_score_poses with the beam carried through the blocks it crosses (the header comment).  The prologue stages the
// pose and the parameters once and every wave's own copy of the start block's folds; after it the four waves do not
// meet again before the final add.
template <int MAXB>
__global__ __launch_bounds__(256) void k_score_poses_through(
    const float* __restrict__ points, int64_t n_beams, const double* __restrict__ poses12,
    const int* __restrict__ block_of_pose, int n_blocks, int bpp, const double* __restrict__ boxes6, float near, int S,
    int I, const double* __restrict__ folds_c, const double* __restrict__ folds_f, float eps, double delta_arg,
    double min_sumw_arg, int max_segments, double seam_tol_arg, double t_min_arg, double* __restrict__ part,
    float* __restrict__ depth_out, float* __restrict__ sumw_out, int* __restrict__ nseg_out,
    int* __restrict__ last_out) {
  extern __shared__ float sp_lds[];
  __shared__ double fa[4][2][64];   // per wave: the folds of the block its segment is in
  __shared__ double red[4][SP_W];
  __shared__ double pb[16];   // [R row-major (9), t (3), huber_delta, min_sumw, seam_tol, min_transmittance]
  __shared__ double od[4][6];   // per wave: the float64 ray (o, d), read again only by the next-block search
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t pose = blockIdx.x / (unsigned)bpp;
  const int64_t beam = (int64_t)(blockIdx.x - (unsigned)pose * (unsigned)bpp) * 4 + wave;
  const int b = fr_block_of(block_of_pose, pose, n_blocks);
  if (b < 0) {   // (uniform across the workgroup, before the first barrier)
    if (tid < SP_W) part[(int64_t)blockIdx.x * SP_W + tid] = 0.0;
    if (lane == 0 && beam < n_beams) {
      const int64_t g = pose * n_beams + beam;
      if (depth_out) depth_out[g] = __builtin_nanf("");
      if (sumw_out) sumw_out[g] = 0.0f;
      if (nseg_out) nseg_out[g] = 0;
      if (last_out) last_out[g] = -1;
    }
    return;
  }
  fa[wave][0][lane] = folds_c[64 * b + lane];
  fa[wave][1][lane] = folds_f[64 * b + lane];
  if (tid < 12) pb[tid] = poses12[12 * pose + tid];
  else if (tid < 14) pb[tid] = tid == 12 ? delta_arg : min_sumw_arg;
  else if (tid < 16) pb[tid] = tid == 14 ? seam_tol_arg : t_min_arg;
  __syncthreads();
  double term[SP_W] = {0.0, 0.0, 0.0, 0.0};
  if (beam < n_beams) {   // (wave-uniform: the shuffles below always have 64 lanes)
    float* zc = sp_lds + (size_t)wave * fr_slice_floats(S, I);
    float* fs = zc + S;
    float* ws = fs + I;
    float* cdf = ws + S;
    float* zf = ws;
    // 1. the ray, kept in float64 for the walk over the blocks (every lane the same values)
    float row[6], target;
    double te;   // the float64 exit of the segment being rendered
    {
      double o[3], d[3], rng, tin, tout;
      fr_pose_od(pb, points + 3 * beam, o, d, rng);
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        row[m] = (float)o[m];
        row[3 + m] = (float)d[m];
        if (lane == 0) {
          od[wave][m] = o[m];
          od[wave][3 + m] = d[m];
        }
      }
      target = (float)rng;
      fr_box_interval(o, d, boxes6 + 6 * b, tin, tout);
      te = fr_segment_exit(tout, near);
    }
    float near_k = near;
    int cur = b, nseg = 0;
    double T = 1.0, W = 0.0, N = 0.0;
    float dv = __builtin_nanf(""), sv = 0.0f;
    const int K = min(max(max_segments, 1), 16);
#pragma nounroll
    for (int k = 0; k < K; ++k) {
      const float far = (float)te;
      // 2. coarse depths of the segment
#pragma nounroll
      for (int i = lane; i < S; i += 64) zc[i] = lerp_z(near_k, far, linspace01(i, S));
      wave_lds_sync();
      // 3. to 5.: k_score_poses' rolled pair of passes, with this wave's folds
      double dep = 0.0, hit = 0.0, unused[6];
      const float* zs = zc;
      int ns = S;
#pragma nounroll
      for (int pass = 0; pass < 2; ++pass) {
        fr_pass<MAXB, false>(row, zs, ns, fa[wave][pass], eps, lane, pass == 0 ? ws : nullptr, dep, hit, unused);
        if (pass == 1) break;
        zs = zf;
        ns = S + I;
        wave_lds_sync();
        fr_resample_merge(zc, fs, ws, cdf, zf, S, I, lane);   // 4.
      }
      dv = (float)dep;
      sv = (float)hit;
      fr_chain_step(dv, sv, eps, T, W, N);
      nseg = k + 1;
      if (k + 1 >= K || T <= pb[15]) break;
      // the next block: lane l tests blocks l, l + 64, ... in ascending order, then the wave agrees on the largest
      // tout, the lowest index on ties
      const double seam_tol = pb[14];
      double bt = 0.0, btin = 0.0, o[3], d[3];
      int bi = -1;
#pragma unroll
      for (int m = 0; m < 3; ++m) {   // (written before the first wave_lds_sync of segment 0)
        o[m] = od[wave][m];
        d[m] = od[wave][3 + m];
      }
#pragma nounroll
      for (int j = lane; j < n_blocks; j += 64) {
        double tn, tm;
        fr_box_interval(o, d, boxes6 + 6 * (int64_t)j, tn, tm);
        if (j != cur && fr_next_candidate(tn, tm, te, seam_tol) && (bi < 0 || tm > bt)) {
          bt = tm;
          btin = tn;
          bi = j;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ot = __shfl_xor(bt, off, 64), otin = __shfl_xor(btin, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (oi >= 0 && (bi < 0 || ot > bt || (ot == bt && oi < bi))) {
          bt = ot;
          btin = otin;
          bi = oi;
        }
      }
      if (bi < 0) break;   // (every lane holds the same winner)
      cur = min(bi, n_blocks - 1);
      near_k = (float)fmax(te, btin);
      te = fr_segment_exit(bt, near_k);
      wave_lds_sync();   // the last pass has read this wave's folds
      fa[wave][0][lane] = folds_c[64 * cur + lane];
      fa[wave][1][lane] = folds_f[64 * cur + lane];
      wave_lds_sync();
    }
    if (nseg > 1) {   // one segment: its depth and sumw untouched
      dv = (float)(N / (W + (double)eps));
      sv = (float)W;
    }
    // 6. residual terms, as k_score_poses
    const double delta = pb[12], min_sumw = pb[13];
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
      if (nseg_out) nseg_out[g] = nseg;
      if (last_out) last_out[g] = cur;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < SP_W; ++f) red[wave][f] = term[f];
  }
  __syncthreads();
  if (tid < SP_W)
    part[(int64_t)blockIdx.x * SP_W + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// scores4[p][f] = sum_w part[p bpp + w][f]: thread (f, q) adds partials q, q + 64, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void k_score_poses_sum(const double* __restrict__ part, int bpp,
                                                         double* __restrict__ scores4) {
  __shared__ double red[64][SP_W];
  const int f = threadIdx.x & 3, q = threadIdx.x >> 2;
  const double* __restrict__ pp = part + (int64_t)blockIdx.x * bpp * SP_W;
  double acc = 0.0;
  for (int w = q; w < bpp; w += 64) acc += pp[(int64_t)w * SP_W + f];
  red[q][f] = acc;
  __syncthreads();
  for (int s = 32; s > 0; s >>= 1) {
    if (q < s) red[q][f] += red[q + s][f];
    __syncthreads();
  }
  if (q == 0) scores4[(int64_t)blockIdx.x * SP_W + f] = red[0][f];
}

// Both entries: `name` prefixes the error texts; with_table: the map entry, whose block_of_pose must be given
int sp_score_poses(const char* name, bool with_table, const float* points, int64_t n_beams, const double* poses12,
                   int64_t n_poses, const int* block_of_pose, int n_blocks, const double* boxes6, float near, int S,
                   int I, const double* folds_c, const double* folds_f, float eps, double huber_delta, double min_sumw,
                   void* workspace, size_t workspace_bytes, double* scores4, float* depth_or_null, float* sumw_or_null,
                   hipStream_t stream) {
  PCN_API_BEGIN
  const std::string who(name);
  PCN_CHECK(n_poses >= 0 && n_beams >= 0, who + ": negative count");
  fr_check_samples(name, S, I);
  if (n_poses == 0) return 0;
  PCN_CHECK(scores4, who + ": null argument");
  if (n_beams == 0) {
    PCN_HIP(hipMemsetAsync(scores4, 0, (size_t)n_poses * SP_W * sizeof(double), stream));
    return 0;
  }
  PCN_CHECK(points && poses12 && (block_of_pose || !with_table) && boxes6 && folds_c && folds_f && workspace,
            who + ": null argument");
  PCN_CHECK(n_blocks >= 1, who + ": n_blocks < 1");
  PCN_CHECK(workspace_bytes >= pcnerf_score_poses_workspace_bytes(n_poses, n_beams),
            who + ": workspace smaller than pcnerf_score_poses_workspace_bytes");
  fr_check_pairs(name, n_poses, n_beams);
  const int64_t bpp = fr_blocks_per_pose(n_beams);
  const size_t lds = (size_t)4 * fr_slice_floats(S, I) * sizeof(float);   // <= 48 KiB
  double* part = reinterpret_cast<double*>(workspace);
  fr_dispatch_maxb(S + I, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    const auto kernel = with_table ? &k_score_poses<MB, true> : &k_score_poses<MB, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n_poses * bpp)), dim3(256), lds, stream, points, n_beams, poses12,
                       block_of_pose, n_blocks, (int)bpp, boxes6, near, S, I, folds_c, folds_f, eps, huber_delta,
                       min_sumw, part, depth_or_null, sumw_or_null);
  });
  hipLaunchKernelGGL(k_score_poses_sum, dim3((unsigned)n_poses), dim3(256), 0, stream, part, (int)bpp, scores4);
  PCN_LAUNCH_CHECK(name);
  PCN_API_END_NEG
}

// pcnerf_score_poses_through: sp_score_poses' checks and launches with the chain's three parameters and two outputs
int sp_score_through(const char* name, const float* points, int64_t n_beams, const double* poses12, int64_t n_poses,
                     const int* block_of_pose, int n_blocks, const double* boxes6, float near, int S, int I,
                     const double* folds_c, const double* folds_f, float eps, double huber_delta, double min_sumw,
                     int max_segments, double seam_tol, double min_transmittance, void* workspace,
                     size_t workspace_bytes, double* scores4, float* depth_or_null, float* sumw_or_null,
                     int* n_segments_or_null, int* last_block_or_null, hipStream_t stream) {
  PCN_API_BEGIN
  const std::string who(name);
  PCN_CHECK(n_poses >= 0 && n_beams >= 0, who + ": negative count");
  fr_check_samples(name, S, I);
  PCN_CHECK(max_segments >= 1 && max_segments <= 16, who + ": max_segments outside 1 .. 16");
  PCN_CHECK(seam_tol >= 0.0, who + ": seam_tol is negative or NaN");
  PCN_CHECK(min_transmittance >= 0.0 && min_transmittance < 1.0, who + ": min_transmittance outside [0, 1)");
  if (n_poses == 0) return 0;
  PCN_CHECK(scores4, who + ": null argument");
  if (n_beams == 0) {
    PCN_HIP(hipMemsetAsync(scores4, 0, (size_t)n_poses * SP_W * sizeof(double), stream));
    return 0;
  }
  PCN_CHECK(points && poses12 && block_of_pose && boxes6 && folds_c && folds_f && workspace, who + ": null argument");
  PCN_CHECK(n_blocks >= 1, who + ": n_blocks < 1");
  PCN_CHECK(workspace_bytes >= pcnerf_score_poses_workspace_bytes(n_poses, n_beams),
            who + ": workspace smaller than pcnerf_score_poses_workspace_bytes");
  fr_check_pairs(name, n_poses, n_beams);
  const int64_t bpp = fr_blocks_per_pose(n_beams);
  const size_t lds = (size_t)4 * fr_slice_floats(S, I) * sizeof(float);   // <= 48 KiB, and 4.25 KiB static
  double* part = reinterpret_cast<double*>(workspace);
  fr_dispatch_maxb(S + I, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    hipLaunchKernelGGL(k_score_poses_through<MB>, dim3((unsigned)(n_poses * bpp)), dim3(256), lds, stream, points,
                       n_beams, poses12, block_of_pose, n_blocks, (int)bpp, boxes6, near, S, I, folds_c, folds_f, eps,
                       huber_delta, min_sumw, max_segments, seam_tol, min_transmittance, part, depth_or_null,
                       sumw_or_null, n_segments_or_null, last_block_or_null);
  });
  hipLaunchKernelGGL(k_score_poses_sum, dim3((unsigned)n_poses), dim3(256), 0, stream, part, (int)bpp, scores4);
  PCN_LAUNCH_CHECK(name);
  PCN_API_END_NEG
}

}  // namespace pcn

using namespace pcn;

extern "C" size_t pcnerf_score_poses_workspace_bytes(int64_t n_poses, int64_t n_beams) {
  if (n_poses <= 0 || n_beams <= 0) return 0;
  return (size_t)n_poses * (size_t)fr_blocks_per_pose(n_beams) * SP_W * sizeof(double);
}

extern "C" int pcnerf_score_poses_fold(const float* points_sensor, int64_t n_beams, const double* poses12,
                                       int64_t n_poses, const double* parent_box6, float near, int n_samples,
                                       int n_importance, const double* fold_coarse, const double* fold_fine,
                                       float eps, double huber_delta, double min_sumw, void* workspace,
                                       size_t workspace_bytes, double* scores4, float* depth_or_null,
                                       float* sumw_or_null, void* stream) {
  return sp_score_poses("pcnerf_score_poses_fold", false, points_sensor, n_beams, poses12, n_poses, nullptr, 1,
                        parent_box6, near, n_samples, n_importance, fold_coarse, fold_fine, eps, huber_delta, min_sumw,
                        workspace, workspace_bytes, scores4, depth_or_null, sumw_or_null, (hipStream_t)stream);
}

extern "C" int pcnerf_score_poses_map(const float* points_sensor, int64_t n_beams, const double* poses12,
                                      int64_t n_poses, const int32_t* block_of_pose, int n_blocks,
                                      const double* boxes6, float near, int n_samples, int n_importance,
                                      const double* folds_coarse, const double* folds_fine, float eps,
                                      double huber_delta, double min_sumw, void* workspace, size_t workspace_bytes,
                                      double* scores4, float* depth_or_null, float* sumw_or_null, void* stream) {
  return sp_score_poses("pcnerf_score_poses_map", true, points_sensor, n_beams, poses12, n_poses, block_of_pose,
                        n_blocks, boxes6, near, n_samples, n_importance, folds_coarse, folds_fine, eps, huber_delta,
                        min_sumw, workspace, workspace_bytes, scores4, depth_or_null, sumw_or_null,
                        (hipStream_t)stream);
}

extern "C" int pcnerf_score_poses_through(const float* points_sensor, int64_t n_beams, const double* poses12,
                                          int64_t n_poses, const int32_t* block_of_pose, int n_blocks,
                                          const double* boxes6, float near, int n_samples, int n_importance,
                                          const double* folds_coarse, const double* folds_fine, float eps,
                                          double huber_delta, double min_sumw, int max_segments, double seam_tol,
                                          double min_transmittance, void* workspace, size_t workspace_bytes,
                                          double* scores4, float* depth_or_null, float* sumw_or_null,
                                          int32_t* n_segments_or_null, int32_t* last_block_or_null, void* stream) {
  return sp_score_through("pcnerf_score_poses_through", points_sensor, n_beams, poses12, n_poses, block_of_pose,
                          n_blocks, boxes6, near, n_samples, n_importance, folds_coarse, folds_fine, eps, huber_delta,
                          min_sumw, max_segments, seam_tol, min_transmittance, workspace, workspace_bytes, scores4,
                          depth_or_null, sumw_or_null, n_segments_or_null, last_block_or_null, (hipStream_t)stream);
}
