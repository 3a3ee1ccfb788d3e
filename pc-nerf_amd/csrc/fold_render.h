// The folded scan render shared by register.hip (k_render_jac_fold, k_gn_normal_eq), localize.hip
// (k_score_poses) and refine.hip (k_pose_normal_eq): one wave renders one ray through the folded eval
// network p = sigmoid(a . e(x) + c) (fold_dot, pcnerf_internal.h).  The three kernels must agree
// bit for bit on depth, sumw and jac6 (the tests compare them with the composed route), so every step they share is
// defined here once:
//
//   fr_pose_ray        1. the world ray of a beam from a pose, in float64 (nof.registration.scan_rays' arithmetic:
//                         rng = |p|, d = R (p / rng) summed in x, y, z order and renormalised, o = t, far the exit from
//                         the box by the slab test, a NaN t2 counting as +inf, never below near), cast once to float32;
//   fr_pass            3./5. a render pass: lane l owns the contiguous samples l B .. l B + B - 1, B = ceil(n / 64)
//                         <= MAXB, and keeps their p, z and (JAC) grad logit in registers (a rolled sample loop, one
//                         copy of the 30 sincosf, with unrolled selects); compositing (render.py:51-61, no noise) in
//                         float64 from the float32 p, each output rounded once; the normalised weights go out only
//                         when asked for.  JAC: d depth / d logit_s by k_composite_bwd's recurrence with
//                         dL/ddepth = 1 (the reverse affine recurrence U_{j-1} = g~_j p_j + (1 - p_j) U_j, no division
//                         by 1 - p), then jac6[0:3] = sum_s g_s grad logit(x_s), jac6[3:6] = sum_s z_s g_s
//                         grad logit(x_s): per-lane float64 partials in sample order, the xor butterfly;
//   fr_resample_merge  4. k_resample at u == NULL (mid-point bins formed from zc where they are read, weights
//                         w[1:-1] + 1e-5f, float64 running sums rounded to a float32 cdf, the right-sided search,
//                         denom < 1e-5f -> 1), then the merge with zc.  With u = linspace the draws are almost always
//                         ascending already, but not provably (the last draw of a bin can round an ulp above the next
//                         bin's first), so the wave votes: in order (and no NaN), each value lands at its index plus
//                         its rank in the other list (k_resample's merge); otherwise every value takes its all-pairs
//                         rank in the concatenation, NaNs last (k_sample_coarse's fallback).  Either way the result is
//                         sort(cat(zc, draws)).  The merged list aliases the weights and the cdf, dead by then;
//   gn_*               6. the per-beam Gauss-Newton pieces: the validity rule, the pose Jacobian
//                         Jp = [J_o, o x J_o + d x J_d] of the left perturbation T' = exp(xi) T (delta o = rho + phi x o,
//                         delta d = phi x d), the Huber weight and cost term.  Each kernel keeps its own accumulation;
//   fr_block_of        which block of a map a pose of the two pose kernels is rendered against;
//   fr_pose_od, fr_box_interval, fr_segment_exit, fr_next_candidate, fr_chain_step
//                      the walk of a beam over the blocks of a map and the compositing of its segments
//                      (k_score_poses_through): nothing is composited across blocks unless asked.
// Loops are bounded by S and I (the binary searches by their logarithm), never by data, and every LDS index is clamped,
// so NaN rays (rng == 0, a non-finite point) cost time but cannot leave their slice.
// Host side: the LDS slice size, the blocks per pose, the sample-count checks and the MAXB dispatch of the launchers.
#pragma once
#include <type_traits>

#include "pcnerf_internal.h"

namespace pcn {

constexpr int FR_MAX_S = 1024;   // 64 lanes x 16 samples per lane (the two-pass kernels' fine pass: S + I)

// The block of a pose in a map of n_blocks, or -1 for "no block": never index with anything else.  (The single-block
// entries have no table: their kernels are compiled with block 0 for every pose and do not call this.)
__device__ __forceinline__ int fr_block_of(const int* __restrict__ block_of_pose, int64_t pose, int n_blocks) {
  const int b = block_of_pose[pose];
  return (b >= 0 && b < n_blocks) ? b : -1;
}

// One render pass of the wave's ray `row` (o, d) over the n depths zs (LDS or global memory), B = ceil(n / 64) <= MAXB:
// dep and hit in float64 (every lane the same values); w_out (the n normalised weights) or NULL.  JAC: the samples
// also keep grad logit, and when want_jac (wave-uniform) jac = d depth / d (o, d), every lane the same six sums.
// The per-lane arrays are locals of this one function: handed in by reference, the compiler turned the unrolled
// selects below into branches.
template <int MAXB, bool JAC>
__device__ __forceinline__ void fr_pass(const float* row, const float* zs, int n, const double* __restrict__ a,
                                        float eps, int lane, float* w_out, double& dep, double& hit,
                                        double (&jac)[6], bool want_jac = true) {
  const int B = (n + 63) / 64;
  const int i0 = lane * B;
  const int nb = max(0, min(min(B, MAXB), n - i0));
  // samples past the lane's block count as p = 0 at z = 0: factors of one and terms of zero everywhere below
  float pv[MAXB], zv[MAXB];
  double gx[JAC ? MAXB : 1][3];
#pragma unroll
  for (int j = 0; j < MAXB; ++j) {
    pv[j] = 0.0f;
    zv[j] = 0.0f;
    if constexpr (JAC) gx[j][0] = gx[j][1] = gx[j][2] = 0.0;
  }
#pragma nounroll
  for (int j = 0; j < nb; ++j) {   // a rolled loop (one copy of the 30 sincosf); the selects keep the indices static
    const float z = zs[i0 + j];
    float x[3];
    sample_point(row, z, x);
    double d[3];
    double logit = a[63];
    logit += fold_dot<true, JAC>(x, a, d);
    const float ps = sigmoid_ref((float)logit);
#pragma unroll
    for (int jj = 0; jj < MAXB; ++jj) {
      if (jj == j) {
        pv[jj] = ps;
        zv[jj] = z;
        if constexpr (JAC) {
          gx[jj][0] = d[0];
          gx[jj][1] = d[1];
          gx[jj][2] = d[2];
        }
      }
    }
  }
  double loc = 1.0;
#pragma unroll
  for (int j = 0; j < MAXB; ++j) loc *= 1.0 - (double)pv[j];
  double T = wave_excl_prod(loc, lane);
  double wv[MAXB], tv[JAC ? MAXB : 1];
  double sw = 0.0;
#pragma unroll
  for (int j = 0; j < MAXB; ++j) {
    if constexpr (JAC) tv[j] = T;
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
  if constexpr (JAC) {
    if (!want_jac) return;
    // d depth / d logit_s (k_composite_bwd's recurrence with dL/ddepth = 1); wv is dead, its registers hold g
#pragma unroll
    for (int j = 0; j < MAXB; ++j) wv[j] = ((double)zv[j] - dep) * rden;   // d depth / d w~_j
    double A = 0.0, Bm = 1.0;   // this lane's affine map U_end -> U_{i0 - 1}
#pragma unroll
    for (int j = MAXB - 1; j >= 0; --j) {
      const double aj = wv[j] * (double)pv[j], bj = 1.0 - (double)pv[j];
      A = aj + bj * A;
      Bm = bj * Bm;
    }
    double U = wave_suffix_affine(A, Bm, lane);
#pragma unroll
    for (int j = MAXB - 1; j >= 0; --j) {
      const double gp = tv[j] * (wv[j] - U);
      U = wv[j] * (double)pv[j] + (1.0 - (double)pv[j]) * U;
      wv[j] = gp * (1.0 - (double)pv[j]) * (double)pv[j];   // sigmoid backward: now d depth / d logit_j
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) jac[m] = 0.0;
#pragma unroll
    for (int j = 0; j < MAXB; ++j) {   // sample order
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const double g = wv[j] * gx[j][m];
        jac[m] += g;
        jac[3 + m] += (double)zv[j] * g;
      }
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) jac[m] = wave_sum_d(jac[m]);
  }
}

// 1. The ray of the beam to the sensor-frame point pt from the pose and box in pb (LDS): [R row-major (9), t (3),
// lo (3), hi (3)].  row = (o, d), far the box exit, target the measured range; every lane the same values.
__device__ __forceinline__ void fr_pose_ray(const double* pb, const float* __restrict__ pt, float near,
                                            float (&row)[6], float& far, float& target) {
  const double* T = pb;
  const double* box = pb + 12;
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
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    row[m] = (float)o[m];
    row[3 + m] = (float)d[m];
  }
  far = (float)far64;
  target = (float)rng;
}

// The pieces of a render carried through several blocks (k_score_poses_through, localize.hip): the float64 ray that
// fr_pose_ray forms before its casts, the interval of a ray in a box, and one step of the chain over segments.
// fr_pose_ray's operations one for one (the build does not contract), so the casts of o, d and rng are its row and
// target, and fr_box_interval's tout is its box exit before the clamp to near.
__device__ __forceinline__ void fr_pose_od(const double* T, const float* __restrict__ pt, double (&o)[3],
                                           double (&d)[3], double& rng) {
  const double px = (double)pt[0], py = (double)pt[1], pz = (double)pt[2];
  rng = sqrt((px * px + py * py) + pz * pz);
  const double ux = px / rng, uy = py / rng, uz = pz / rng;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    d[m] = (T[3 * m] * ux + T[3 * m + 1] * uy) + T[3 * m + 2] * uz;
    o[m] = T[9 + m];
  }
  const double dn = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
  for (int m = 0; m < 3; ++m) d[m] = d[m] / dn;
}

// [tin, tout] of the ray o + t d in box = [lo (3), hi (3)]: tout the minimum over the axes of max(t1, t2) (a NaN t2
// counting as +inf), tin the mirror image, the maximum over the axes of min(t1, t2) (a NaN t1 counting as -inf); any
// other NaN propagates
__device__ __forceinline__ void fr_box_interval(const double (&o)[3], const double (&d)[3],
                                                const double* __restrict__ box, double& tin, double& tout) {
  const double nan64 = __builtin_nan("");
  tin = 0.0;
  tout = 0.0;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const double inv = 1.0 / d[m];
    const double t1 = (box[m] - o[m]) * inv, t2 = (box[3 + m] - o[m]) * inv;
    const double tm = t2 != t2 ? (double)INFINITY : (t1 != t1 ? nan64 : fmax(t1, t2));
    const double tn = t1 != t1 ? -(double)INFINITY : (t2 != t2 ? nan64 : fmin(t1, t2));
    tout = m == 0 ? tm : ((tout != tout || tm != tm) ? nan64 : fmin(tout, tm));
    tin = m == 0 ? tn : ((tin != tin || tn != tn) ? nan64 : fmax(tin, tn));
  }
}

// far of a segment that starts at near and leaves its box at tout: fr_pose_ray's clamp, in float64
__device__ __forceinline__ double fr_segment_exit(double tout, float near) {
  return tout != tout ? tout : fmax(tout, (double)near);
}

// Is the box with interval [tin, tout] a candidate for the segment after one that ended at te?  It must begin no later
// than seam_tol past te, end after te, and be non-empty in float32, where the segment is rendered.
__device__ __forceinline__ bool fr_next_candidate(double tin, double tout, double te, double seam_tol) {
  return tin == tin && tout == tout && tin <= te + seam_tol && tout > te && (float)tout > (float)fmax(te, tin);
}

// One segment (depth dv, hit probability sv, each rounded to float32) joins the chain: T the transmittance in front of
// it, W the hit probability so far, N the unnormalised depth sum.  1 - sum w = prod (1 - p) (render.py:51-61), so this
// is the compositing of the concatenated sample lists.
__device__ __forceinline__ void fr_chain_step(float dv, float sv, float eps, double& T, double& W, double& N) {
  const double s = (double)sv, v = (double)dv;
  const double c = T * s;
  W = W + c;
  N = N + T * (v * (s + (double)eps));
  T = T * (1.0 - s);
  if (T < 0.0) T = 0.0;
}

// value a of cat(zc, fs)
__device__ __forceinline__ float fr_cat(const float* zc, const float* fs, int S, int a) {
  return a < S ? zc[a] : fs[a - S];
}

// 4. k_resample at u == NULL and the merge with zc, on the wave's slice: zc (S) the coarse depths, ws (S) their
// weights, cdf (S - 1) and fs (I) scratch, zf (S + I, may alias ws and cdf) the merged depths.  Ends synchronised.
__device__ __forceinline__ void fr_resample_merge(const float* zc, float* fs, const float* ws, float* cdf, float* zf,
                                                  int S, int I, int lane) {
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
  double run = wave_excl_sum(lp, lane);
  if (lane == 0) cdf[0] = 0.0f;
#pragma nounroll
  for (int j = 0; j < B; ++j) {
    const int i = i0 + j;
    if (i < npdf) {
      run += (double)((w[i] + 1e-5f) / tot);
      cdf[i + 1] = (float)run;
    }
  }
  wave_lds_sync();
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
  wave_lds_sync();   // (also orders the last ws / cdf read before zf's first write)
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
      const float va = fr_cat(zc, fs, S, a);
      const bool na = !(va == va);
      int rank = 0;
#pragma nounroll
      for (int b = 0; b < n; ++b) {
        const float vb = fr_cat(zc, fs, S, b);
        const bool nb = !(vb == vb);
        rank += (vb < va) || (na && !nb) || ((vb == va || (na && nb)) && b < a);   // NaNs after every number
      }
      zf[min(rank, n - 1)] = va;
    }
  }
  wave_lds_sync();
}

// 6. A beam with a usable target contributes when it was hit and its depth is finite.
__device__ __forceinline__ bool gn_target_usable(float target) { return isfinite(target) && target > 0.0f; }
__device__ __forceinline__ bool gn_beam_valid(float depth, float sumw, float target, double min_sumw) {
  return (double)sumw >= min_sumw && isfinite(depth) && gn_target_usable(target);
}

// Jp = [J_o, o x J_o + d x J_d] from the float32 ray row (o, d) and jac6 = (J_o, J_d)
__device__ __forceinline__ void gn_pose_jacobian(const float* row, const float* jac6, double (&Jp)[6]) {
  double o[3], d[3], Jo[3], Jd[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    o[m] = (double)row[m];
    d[m] = (double)row[3 + m];
    Jo[m] = (double)jac6[m];
    Jd[m] = (double)jac6[3 + m];
    Jp[m] = Jo[m];
  }
  Jp[3] = (o[1] * Jo[2] - o[2] * Jo[1]) + (d[1] * Jd[2] - d[2] * Jd[1]);
  Jp[4] = (o[2] * Jo[0] - o[0] * Jo[2]) + (d[2] * Jd[0] - d[0] * Jd[2]);
  Jp[5] = (o[0] * Jo[1] - o[1] * Jo[0]) + (d[0] * Jd[1] - d[1] * Jd[0]);
}

// Huber's weight and cost term of a residual; delta <= 0: plain least squares
__device__ __forceinline__ void gn_huber(double res, double delta, double& w, double& rho) {
  const double ar = fabs(res);
  const bool lin = delta > 0.0 && ar > delta;   // the linear branch
  w = lin ? delta / ar : 1.0;
  rho = lin ? delta * (ar - 0.5 * delta) : 0.5 * (res * res);
}

// ------------------------------------------------------------------------------------------------------ host side
// floats of one wave's LDS slice of a two-pass kernel: zc (S) | draws (I) | weights (S) + cdf, aliased by the merged
// depths (S + I); four slices are at most 48 KiB
__host__ __device__ inline int fr_slice_floats(int S, int I) { return S + I + (2 * S > S + I ? 2 * S : S + I); }

// one wave per (pose, beam), four beams per workgroup: a workgroup never straddles two poses
inline int64_t fr_blocks_per_pose(int64_t n_beams) { return (n_beams + 3) / 4; }

inline void fr_check_samples(const char* name, int n_samples, int n_importance) {
  const std::string who(name);
  PCN_CHECK(n_samples >= 3, who + ": n_samples < 3 (the resampling needs one interior weight)");
  PCN_CHECK(n_importance >= 1, who + ": n_importance < 1");
  PCN_CHECK((int64_t)n_samples + n_importance <= FR_MAX_S,
            who + ": n_samples + n_importance > 1024 (one wave per beam, at most 16 samples per lane)");
}

inline void fr_check_pairs(const char* name, int64_t n_poses, int64_t n_beams) {
  const int64_t bpp = fr_blocks_per_pose(n_beams);
  PCN_CHECK(bpp < (int64_t)1 << 31 && n_poses < (int64_t)1 << 31 && n_poses * bpp < (int64_t)1 << 31,
            std::string(name) + ": too many (pose, beam) pairs for one launch");
}

// launch(std::integral_constant<int, MAXB>) for the smallest MAXB of 1, 2, 4, 8, 16 that holds n samples per ray
template <typename Launch>
inline void fr_dispatch_maxb(int n, Launch&& launch) {
  const int B = (n + 63) / 64;
  if (B <= 1) launch(std::integral_constant<int, 1>());
  else if (B <= 2) launch(std::integral_constant<int, 2>());
  else if (B <= 4) launch(std::integral_constant<int, 4>());
  else if (B <= 8) launch(std::integral_constant<int, 8>());
  else launch(std::integral_constant<int, 16>());
}

}  // namespace pcn
