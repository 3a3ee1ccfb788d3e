// Pose-hypothesis scoring against folded eval networks: the whole two-pass render of a scan (rays from the pose,
// coarse depths, coarse pass, deterministic resampling, fine pass) and the per-pose reduction of the range residuals
// in one launch, with nothing per sample through memory.
//
//   k_score_poses_fold<MAXB>  one wave per (pose, beam), four beams per 256-thread workgroup, ceil(R / 4) workgroups
//                             per pose (a workgroup never straddles two poses).  Both fold vectors, the workgroup's
//                             pose, the box and the loss parameters sit in LDS (as scalars they spilled SGPRs).  Per
//                             wave, in its own LDS slice zc (S) | fs (I) | max(2 S, S + I) floats:
//                               1. the world ray in float64 (nof.registration.scan_rays' arithmetic: rng = |p|,
//                                  d = R (p / rng) summed in x, y, z order and renormalised, o = t, far the exit from
//                                  the box by the slab test, a NaN t2 counting as +inf, never below near), cast once
//                                  to float32;
//                               2. zc = k_sample_coarse's plain path, lerp_z(near, far, linspace01(i, S));
//                               3. the coarse pass: k_render_jac_fold's forward (rj_logit_and_grad's six float64
//                                  chains, p = sigmoid_ref(fl32(logit)), compositing in float64), the normalised
//                                  weights rounded once to float32 into LDS;
//                               4. k_resample at u == NULL: mid-point bins (formed from zc where they are read),
//                                  weights w[1:-1] + 1e-5f, float64 running sums rounded to a float32 cdf, the
//                                  right-sided search, denom < 1e-5f -> 1; then the merge with zc.  With u = linspace
//                                  the draws are almost always ascending already, but not provably (the last draw of
//                                  a bin can round an ulp above the next bin's first), so the wave votes: in order
//                                  (and no NaN), each value lands at its index plus its rank in the other list
//                                  (k_resample's merge); otherwise every value takes its all-pairs rank in the
//                                  concatenation, NaNs last (k_sample_coarse's fallback).  Either way the result is
//                                  sort(cat(zc, draws)).  The merged list aliases the weights and the cdf, dead by
//                                  then;
//                               5. the fine pass on the S + I merged depths -> depth, sumw, each rounded once;
//                               6. r = depth - rng on the float32 values, rho(r) as k_gn_normal_eq's cost term.
//                             The four waves' terms (rho, 1, |r| over the valid beams; sumw over the usable ones) are
//                             added in wave order into one 4-double partial per workgroup.
//   k_score_poses_sum         one workgroup per pose adds its ceil(R / 4) partials: 64 chains (partials q, q + 64,
//                             ...), then a fixed tree.
// No atomics, every output word has one writer, and geometry and summation order depend on (P, R) alone: a pose scores
// the same bits alone or in a batch, with or without the per-beam outputs.  Loops are bounded by S and I (the binary
// searches by their logarithm), never by data, and every LDS index is clamped, so NaN rays (rng == 0, a non-finite
// point) cost time but cannot leave the slice; they are not counted.
#include "pcnerf_internal.h"

namespace pcn {

constexpr int SP_MAX_S = 1024;   // 64 lanes x 16 samples per lane, the fine pass's S + I
constexpr int SP_W = 4;          // doubles per partial and per pose: cost, n_valid, sum |r|, sum sumw

__device__ __forceinline__ void sp_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// floats of one wave's LDS slice
__host__ __device__ inline int sp_slice_floats(int S, int I) { return S + I + (2 * S > S + I ? 2 * S : S + I); }

// The logit a . e(x) + c: register.hip's rj_logit_and_grad without the gradient (k_nof_eval_fold's chains and order)
__device__ __forceinline__ double sp_logit(const float (&p)[3], const double* __restrict__ a) {
  double part[6];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    part[m] = a[m] * (double)p[m];
    part[3 + m] = 0.0;
  }
#pragma unroll 2
  for (int k = 0; k < 10; ++k) {
    const float sc = (float)(1 << k);
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      float sv, cv;
      sincosf(sc * p[m], &sv, &cv);
      part[m] += a[3 + 6 * k + m] * (double)sv;
      part[3 + m] += a[6 + 6 * k + m] * (double)cv;
    }
  }
  double acc = a[63];
  acc += ((part[0] + part[1]) + (part[2] + part[3])) + (part[4] + part[5]);
  return acc;
}

__device__ __forceinline__ double sp_excl_prod(double v, int lane) {
  double incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double n = __shfl_up(incl, o, 64);
    if (lane >= o) incl *= n;
  }
  const double ex = __shfl_up(incl, 1, 64);
  return lane == 0 ? 1.0 : ex;
}

__device__ __forceinline__ double sp_excl_sum(double v, int lane) {
  double incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double n = __shfl_up(incl, o, 64);
    if (lane >= o) incl += n;
  }
  const double ex = __shfl_up(incl, 1, 64);
  return lane == 0 ? 0.0 : ex;
}

// One render pass of the wave's ray over the n depths zs (LDS): k_render_jac_fold's forward.  Lane l owns the samples
// l B .. l B + B - 1, B = ceil(n / 64) <= MAXB.  w_out (LDS, n floats) or NULL.
template <int MAXB>
__device__ __forceinline__ void sp_pass(const float (&row)[6], const float* zs, int n, const double* __restrict__ a,
                                        float eps, int lane, float* w_out, double& dep, double& hit) {
  const int B = (n + 63) / 64;
  const int i0 = lane * B;
  const int nb = max(0, min(min(B, MAXB), n - i0));
  float pv[MAXB], zv[MAXB];
#pragma unroll
  for (int j = 0; j < MAXB; ++j) {
    pv[j] = 0.0f;
    zv[j] = 0.0f;
  }
#pragma nounroll
  for (int j = 0; j < nb; ++j) {
    const float z = zs[i0 + j];
    float x[3];
    sample_point(row, z, x);
    const float ps = sigmoid_ref((float)sp_logit(x, a));
#pragma unroll
    for (int jj = 0; jj < MAXB; ++jj) {
      if (jj == j) {
        pv[jj] = ps;
        zv[jj] = z;
      }
    }
  }
  double loc = 1.0;
#pragma unroll
  for (int j = 0; j < MAXB; ++j) loc *= 1.0 - (double)pv[j];
  double T = sp_excl_prod(loc, lane);
  double wv[MAXB];
  double sw = 0.0;
#pragma unroll
  for (int j = 0; j < MAXB; ++j) {
    wv[j] = T * (double)pv[j];
    sw += wv[j];
    T *= 1.0 - (double)pv[j];
  }
  hit = wave_sum_d(sw);
  const double rden = 1.0 / (hit + (double)eps);
  double sd = 0.0;
#pragma unroll
  for (int j = 0; j < MAXB; ++j) {
    wv[j] = wv[j] * rden;
    sd += wv[j] * (double)zv[j];
  }
  dep = wave_sum_d(sd);
  if (w_out) {
#pragma unroll
    for (int j = 0; j < MAXB; ++j)
      if (j < nb) w_out[i0 + j] = (float)wv[j];
  }
}

// value a of cat(zc, fs)
__device__ __forceinline__ float sp_cat(const float* zc, const float* fs, int S, int a) {
  return a < S ? zc[a] : fs[a - S];
}

template <int MAXB>
__global__ __launch_bounds__(256) void k_score_poses_fold(
    const float* __restrict__ points, int64_t n_beams, const double* __restrict__ poses12, int bpp,
    const double* __restrict__ box6, float near, int S, int I, const double* __restrict__ fold_c,
    const double* __restrict__ fold_f, float eps, double delta_arg, double min_sumw_arg, double* __restrict__ part,
    float* __restrict__ depth_out, float* __restrict__ sumw_out) {
  extern __shared__ float sp_lds[];
  __shared__ double fa[2][64];
  __shared__ double red[4][SP_W];
  __shared__ double pb[20];   // [R row-major (9), t (3), lo (3), hi (3), huber_delta, min_sumw]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t pose = blockIdx.x / (unsigned)bpp;
  if (tid < 128) fa[tid >> 6][lane] = (tid < 64 ? fold_c : fold_f)[lane];
  else if (tid < 140) pb[tid - 128] = poses12[12 * pose + (tid - 128)];   // the workgroup's pose and the box through
  else if (tid < 146) pb[tid - 128] = box6[tid - 140];                    // LDS: vector registers, not 36 scalar ones
  else if (tid < 148) pb[tid - 128] = tid == 146 ? delta_arg : min_sumw_arg;   // (needed last: not held in scalars)
  __syncthreads();
  const int64_t beam = (int64_t)(blockIdx.x - (unsigned)pose * (unsigned)bpp) * 4 + wave;
  double term[SP_W] = {0.0, 0.0, 0.0, 0.0};
  if (beam < n_beams) {   // (wave-uniform: the shuffles below always have 64 lanes)
    float* zc = sp_lds + (size_t)wave * sp_slice_floats(S, I);
    float* fs = zc + S;
    float* ws = fs + I;      // coarse weights (S)
    float* cdf = ws + S;     // (S - 1)
    float* zf = ws;          // the merged depths (S + I): ws and cdf are dead when it is written
    // 1. the ray (every lane the same values)
    const double* T = pb;
    const double* box = pb + 12;
    const float* __restrict__ pt = points + 3 * beam;
    const double px = (double)pt[0], py = (double)pt[1], pz = (double)pt[2];
    const double rng = sqrt((px * px + py * py) + pz * pz);
    const double ux = px / rng, uy = py / rng, uz = pz / rng;
    double d[3], o[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      d[m] = (T[3 * m] * ux + T[3 * m + 1] * uy) + T[3 * m + 2] * uz;
      o[m] = T[9 + m];
    }
    const double dn = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const double nan64 = __builtin_nan("");
    double tmin = 0.0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      d[m] = d[m] / dn;
      const double inv = 1.0 / d[m];
      const double t1 = (box[m] - o[m]) * inv, t2 = (box[3 + m] - o[m]) * inv;
      // torch.maximum / min propagate NaN; a NaN t2 counts as +inf
      const double tm = t2 != t2 ? (double)INFINITY : (t1 != t1 ? nan64 : fmax(t1, t2));
      tmin = m == 0 ? tm : ((tmin != tmin || tm != tm) ? nan64 : fmin(tmin, tm));
    }
    const double far64 = tmin != tmin ? tmin : fmax(tmin, (double)near);
    float row[6];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      row[m] = (float)o[m];
      row[3 + m] = (float)d[m];
    }
    const float far = (float)far64, target = (float)rng;
    // 2. coarse depths
#pragma nounroll
    for (int i = lane; i < S; i += 64) zc[i] = lerp_z(near, far, linspace01(i, S));
    sp_wave_lds_sync();
    // 3. and 5.: the coarse pass on zc, then the fine pass on the merged depths (a rolled loop: one copy of the pass)
    double dep = 0.0, hit = 0.0;
    const float* zs = zc;
    int ns = S;
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
      sp_pass<MAXB>(row, zs, ns, fa[pass], eps, lane, pass == 0 ? ws : nullptr, dep, hit);
      if (pass == 1) break;
      zs = zf;
      ns = S + I;
      sp_wave_lds_sync();
      // 4. resampling (k_resample, u == NULL)
      const int nbin = S - 1, npdf = nbin - 1;
      const float* w = ws + 1;
      const int B = (npdf + 63) / 64, i0 = lane * B;
      double ls = 0.0;
#pragma nounroll
      for (int j = 0; j < B; ++j) {
        const int i = i0 + j;
        if (i < npdf) ls += (double)(w[i] + 1e-5f);
      }
      const float tot = (float)wave_sum_d(ls);
      double lp = 0.0;
#pragma nounroll
      for (int j = 0; j < B; ++j) {
        const int i = i0 + j;
        if (i < npdf) lp += (double)((w[i] + 1e-5f) / tot);
      }
      double run = sp_excl_sum(lp, lane);
      if (lane == 0) cdf[0] = 0.0f;
#pragma nounroll
      for (int j = 0; j < B; ++j) {
        const int i = i0 + j;
        if (i < npdf) {
          run += (double)((w[i] + 1e-5f) / tot);
          cdf[i + 1] = (float)run;
        }
      }
      sp_wave_lds_sync();
#pragma nounroll
      for (int k = lane; k < I; k += 64) {
        const float u = linspace01(k, I);
        int lo = 0, hi = nbin;   // first index with cdf > u (searchsorted right=True)
#pragma nounroll
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
        }
        const int below = max(lo - 1, 0), above = max(min(lo, nbin - 1), 0);
        const float c0 = cdf[below], c1 = cdf[above];
        float denom = c1 - c0;
        if (denom < 1e-5f) denom = 1.0f;
        const float t = (u - c0) / denom;
        const float b0 = 0.5f * (zc[below + 1] + zc[below]), b1 = 0.5f * (zc[above + 1] + zc[above]);
        fs[k] = b0 + t * (b1 - b0);
      }
      sp_wave_lds_sync();   // (also orders the last ws / cdf read before zf's first write)
      bool ok = true;
#pragma nounroll
      for (int i = lane; i < S; i += 64) ok = ok && (zc[i] == zc[i]) && (i + 1 >= S || zc[i] <= zc[i + 1]);
#pragma nounroll
      for (int k = lane; k < I; k += 64) ok = ok && (fs[k] == fs[k]) && (k + 1 >= I || fs[k] <= fs[k + 1]);
      const int n = S + I;
      if (__all(ok)) {
#pragma nounroll
        for (int i = lane; i < S; i += 64) {
          const float v = zc[i];
          int lo = 0, hi = I;
#pragma nounroll
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (fs[mid] < v) lo = mid + 1; else hi = mid;
          }
          zf[min(i + lo, n - 1)] = v;
        }
#pragma nounroll
        for (int k = lane; k < I; k += 64) {
          const float v = fs[k];
          int lo = 0, hi = S;
#pragma nounroll
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (zc[mid] <= v) lo = mid + 1; else hi = mid;
          }
          zf[min(k + lo, n - 1)] = v;
        }
      } else {
#pragma nounroll
        for (int a = lane; a < n; a += 64) {
          const float va = sp_cat(zc, fs, S, a);
          const bool na = !(va == va);
          int rank = 0;
#pragma nounroll
          for (int b = 0; b < n; ++b) {
            const float vb = sp_cat(zc, fs, S, b);
            const bool nb = !(vb == vb);
            rank += (vb < va) || (na && !nb) || ((vb == va || (na && nb)) && b < a);   // NaNs after every number
          }
          zf[min(rank, n - 1)] = va;
        }
      }
      sp_wave_lds_sync();
    }
    // 6. residual terms, on the float32 values the composed route hands to pcnerf_gn_normal_eq
    const float dv = (float)dep, sv = (float)hit;
    const double delta = pb[18], min_sumw = pb[19];
    const bool usable = isfinite(target) && target > 0.0f;
    const bool valid = usable && (double)sv >= min_sumw && isfinite(dv);
    if (valid) {
      const double res = (double)dv - (double)target, ar = fabs(res);
      const bool lin = delta > 0.0 && ar > delta;
      term[0] = lin ? delta * (ar - 0.5 * delta) : 0.5 * (res * res);
      term[1] = 1.0;
      term[2] = ar;
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

inline int64_t sp_blocks_per_pose(int64_t n_beams) { return (n_beams + 3) / 4; }

}  // namespace pcn

using namespace pcn;

// these entries report an argument error as -1 (the message in pcnerf_last_error)
#define LOC_API_END                                       \
  return 0;                                               \
  }                                                       \
  catch (const std::exception& ex__) {                    \
    pcn::set_error(ex__.what());                          \
    return -1;                                            \
  }

extern "C" size_t pcnerf_score_poses_workspace_bytes(int64_t n_poses, int64_t n_beams) {
  if (n_poses <= 0 || n_beams <= 0) return 0;
  return (size_t)n_poses * (size_t)sp_blocks_per_pose(n_beams) * SP_W * sizeof(double);
}

extern "C" int pcnerf_score_poses_fold(const float* points_sensor, int64_t n_beams, const double* poses12,
                                       int64_t n_poses, const double* parent_box6, float near, int n_samples,
                                       int n_importance, const double* fold_coarse, const double* fold_fine,
                                       float eps, double huber_delta, double min_sumw, void* workspace,
                                       size_t workspace_bytes, double* scores4, float* depth_or_null,
                                       float* sumw_or_null, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(n_poses >= 0 && n_beams >= 0, "pcnerf_score_poses_fold: negative count");
  PCN_CHECK(n_samples >= 3, "pcnerf_score_poses_fold: n_samples < 3 (the resampling needs one interior weight)");
  PCN_CHECK(n_importance >= 1, "pcnerf_score_poses_fold: n_importance < 1");
  PCN_CHECK((int64_t)n_samples + n_importance <= SP_MAX_S,
            "pcnerf_score_poses_fold: n_samples + n_importance > 1024 (one wave per beam, at most 16 samples per "
            "lane)");
  if (n_poses == 0) return 0;
  PCN_CHECK(scores4, "pcnerf_score_poses_fold: null argument");
  if (n_beams == 0) {
    PCN_HIP(hipMemsetAsync(scores4, 0, (size_t)n_poses * SP_W * sizeof(double), (hipStream_t)stream));
    return 0;
  }
  PCN_CHECK(points_sensor && poses12 && parent_box6 && fold_coarse && fold_fine && workspace,
            "pcnerf_score_poses_fold: null argument");
  PCN_CHECK(workspace_bytes >= pcnerf_score_poses_workspace_bytes(n_poses, n_beams),
            "pcnerf_score_poses_fold: workspace smaller than pcnerf_score_poses_workspace_bytes");
  const int64_t bpp = sp_blocks_per_pose(n_beams);
  PCN_CHECK(bpp < (int64_t)1 << 31 && n_poses < (int64_t)1 << 31 && n_poses * bpp < (int64_t)1 << 31,
            "pcnerf_score_poses_fold: too many (pose, beam) pairs for one launch");
  const size_t lds = (size_t)4 * sp_slice_floats(n_samples, n_importance) * sizeof(float);   // <= 48 KiB
  const int B = (n_samples + n_importance + 63) / 64;
  double* part = reinterpret_cast<double*>(workspace);
#define SP_LAUNCH(MB)                                                                                              \
  hipLaunchKernelGGL(k_score_poses_fold<MB>, dim3((unsigned)(n_poses * bpp)), dim3(256), lds, (hipStream_t)stream, \
                     points_sensor, n_beams, poses12, (int)bpp, parent_box6, near, n_samples, n_importance,        \
                     fold_coarse, fold_fine, eps, huber_delta, min_sumw, part, depth_or_null, sumw_or_null)
  if (B <= 1) SP_LAUNCH(1);
  else if (B <= 2) SP_LAUNCH(2);
  else if (B <= 4) SP_LAUNCH(4);
  else if (B <= 8) SP_LAUNCH(8);
  else SP_LAUNCH(16);
#undef SP_LAUNCH
  hipLaunchKernelGGL(k_score_poses_sum, dim3((unsigned)n_poses), dim3(256), 0, (hipStream_t)stream, part, (int)bpp,
                     scores4);
  PCN_LAUNCH_CHECK("pcnerf_score_poses_fold");
  LOC_API_END
}
