// Ray-table construction on the GPU: ray/AABB intersection against the parent block and the child boxes
// (SURVEY.md 8(a) a3-a5).  float64 throughout, like the reference's numpy; one thread per LiDAR point.
//   train/val rows (nof/dataset/ipb2dmapping.py:736-768): KD-tree child lookup (find_aabb_box :174-197, the
//     first of the 10 nearest centres whose box holds the point), child near/far from the face-hit test
//     (compute_far_bound0606 :119-172), +-surface_expand, parent far (compute_far_bound :36-77), 15 columns;
//   two-step rows (eval_kitti_render.py:675-803): parent far by slab (ray_aabb_distances :213-235), children whose
//     centre lies within 0.65 m of the ray line (distance_to_ray :237-244), exactly-two-face-hit test
//     (compute_far_bound0429 :170-211), cumulative 0.05 m expansion retries, hits sorted by near, 13 columns.
// Variable-length outputs: pass 0 counts rows per point, a one-block scan gives offsets, pass 1 recomputes and
// writes (the work is cheap next to the memory it would take to keep every point's hits).
// Child lookup: the flat kernels test every child; the grid kernels (second half of this file) find the children
// near a point or a ray through a uniform grid over the child centres and apply the same arithmetic to those.
#include <stdint.h>

#include "common.h"
#include "pcnerf_internal.h"

namespace pcn {

constexpr int KNN = 10;      // find_aabb_box: tree.query(k=10)
constexpr int HIT_MAX = 64;  // max child hits kept per ray (KITTI logs: <= 28)
constexpr int CTILE = 1024;  // child centres per LDS tile

__device__ __forceinline__ int face_hits(const double (&p)[3], const double (&d)[3], const double* lo,
                                         const double* hi, double (&out)[6]) {
  int n = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const double b = s == 0 ? lo[i] : hi[i];
      if (d[i] * (b - p[i]) > 0) {
        const double dist = (b - p[i]) / d[i];
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (k == i) continue;
          const double pe = p[k] + dist * d[k];
          cnt += (pe >= lo[k] && pe <= hi[k]) ? 1 : 0;
        }
        if (cnt >= 2) out[n++] = dist;
      }
    }
  }
  return n;
}

__device__ __forceinline__ double parent_far_train(const double (&o)[3], const double (&d)[3], const double* P6) {
  // compute_far_bound: x_max, x_min, y_max, y_min, z_max, z_min planes; t < 0 or d == 0 -> inf; all inf -> None
  double t = __builtin_inf();
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const double b = s == 0 ? P6[3 + a] : P6[a];
      double ti = __builtin_inf();
      if (d[a] != 0) {
        ti = (b - o[a]) / d[a];
        if (ti < 0) ti = __builtin_inf();
      }
      t = ti < t ? ti : t;
    }
  }
  return t == __builtin_inf() ? __builtin_nan("") : t;
}

__device__ __forceinline__ void ray_of(const double* q, const double (&o)[3], double (&d)[3], double& rng) {
  const double v0 = q[0] - o[0], v1 = q[1] - o[1], v2 = q[2] - o[2];
  rng = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  d[0] = v0 / rng;
  d[1] = v1 / rng;
  d[2] = v2 / rng;
}

// ------------------------------------------------------------------------------- train/val rows
// Everything after the neighbour search, shared by the flat and the grid kernel: the first of the KNN nearest
// centres (ki, ascending by (distance, index)) whose box holds q, its face hits under the face rule, and the row.
__device__ __forceinline__ void train_row(int pass, int64_t i, const double (&q)[3], const double (&o)[3],
                                          const int (&ki)[KNN], const double* __restrict__ b6,
                                          const double* __restrict__ P6, double se, int rule, int* __restrict__ cnt,
                                          const int64_t* __restrict__ off, float* __restrict__ rows,
                                          int* __restrict__ nshort) {
  int child = -1;
#pragma unroll
  for (int k = 0; k < KNN; ++k) {
    const int c = ki[k];
    if (child < 0 && c >= 0) {
      const double* b = b6 + 6 * c;
      if (q[0] >= b[0] && q[1] >= b[1] && q[2] >= b[2] && q[0] <= b[3] && q[1] <= b[4] && q[2] <= b[5]) child = c;
    }
  }
  int ok = 0;
  double near = 0, far = 0, d[3], rng;
  ray_of(q, o, d, rng);
  if (child >= 0) {
    double h[6];
    const int nh = face_hits(o, d, b6 + 6 * child, b6 + 6 * child + 3, h);
    if (rule == 1) {
      // compute_far_bound0406 (MaiCity, ipb2dmapping.py:82-114): the first two hits in face order; every point in a
      // child box yields a row; fewer than two hits is the reference's IndexError (counted, the caller raises)
      ok = 1;
      if (nh >= 2) {
        near = h[0] < h[1] ? h[0] : h[1];
        far = h[0] < h[1] ? h[1] : h[0];
      } else if (pass == 0) {
        atomicAdd(nshort, 1);
      }
    } else if (nh > 0) {  // compute_far_bound0606 (KITTI, :119-172): min / max over all hits, none -> dropped
      ok = 1;
      near = h[0];
      far = h[0];
      for (int k = 1; k < nh; ++k) {
        near = h[k] < near ? h[k] : near;
        far = h[k] > far ? h[k] : far;
      }
    }
  }
  if (pass == 0) {
    cnt[i] = ok;
    return;
  }
  if (!ok) return;
  near = near - se;
  far = far + se;
  double pf = parent_far_train(o, d, P6);
  if (pf < far) pf = far;
  float* r = rows + 15 * off[i];
  r[0] = (float)o[0];
  r[1] = (float)o[1];
  r[2] = (float)o[2];
  r[3] = (float)d[0];
  r[4] = (float)d[1];
  r[5] = (float)d[2];
  r[6] = 0.0f;
  r[7] = (float)pf;
  r[8] = 3.0f;
  r[9] = (float)(child + 1);
  r[10] = (float)near;
  r[11] = (float)far;
  r[12] = (float)(rng - se);
  r[13] = (float)far;  // ipb2dmapping.py:815: the point-far column takes the child far bound
  r[14] = (float)rng;
}

// pass 0: cnt[i] = 1 if point i yields a row; pass 1: rows[off[i]] = the row.
__global__ __launch_bounds__(256) void k_train_rays(int pass, const double* __restrict__ pts, int64_t n,
                                                    const double* __restrict__ origin, const double* __restrict__ ctr,
                                                    const double* __restrict__ b6, int64_t C,
                                                    const double* __restrict__ P6, double se, int rule,
                                                    int* __restrict__ cnt, const int64_t* __restrict__ off,
                                                    float* __restrict__ rows, int* __restrict__ nshort) {
  __shared__ double sc[CTILE * 3];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = i < n;
  const double o[3] = {origin[0], origin[1], origin[2]};
  double q[3] = {0, 0, 0};
  if (act) {
    q[0] = pts[3 * i];
    q[1] = pts[3 * i + 1];
    q[2] = pts[3 * i + 2];
  }
  // the KNN nearest child centres (squared Euclidean distance, ties by index), sorted ascending
  double kd[KNN];
  int ki[KNN];
#pragma unroll
  for (int k = 0; k < KNN; ++k) {
    kd[k] = __builtin_inf();
    ki[k] = -1;
  }
  for (int64_t c0 = 0; c0 < C; c0 += CTILE) {
    const int nt = (int)(C - c0 < CTILE ? C - c0 : CTILE);
    __syncthreads();
    for (int t = threadIdx.x; t < nt * 3; t += blockDim.x) sc[t] = ctr[c0 * 3 + t];
    __syncthreads();
    if (!act) continue;
    for (int t = 0; t < nt; ++t) {
      const double a = q[0] - sc[3 * t], b = q[1] - sc[3 * t + 1], e = q[2] - sc[3 * t + 2];
      const double ds = a * a + b * b + e * e;
      if (ds < kd[KNN - 1]) {
        int pos = KNN - 1;
        const int ci = (int)(c0 + t);
#pragma unroll
        for (int k = KNN - 1; k > 0; --k) {
          if (kd[k - 1] > ds) {
            kd[k] = kd[k - 1];
            ki[k] = ki[k - 1];
            pos = k - 1;
          } else {
            break;
          }
        }
        kd[pos] = ds;
        ki[pos] = ci;
      }
    }
  }
  if (!act) return;
  train_row(pass, i, q, o, ki, b6, P6, se, rule, cnt, off, rows, nshort);
}

// ------------------------------------------------------------------------------- two-step rows
struct ViewHit {
  double near, far, col7;
  int tin;
};

// parent far: slab exit (NaN-propagating min/max like numpy), inf when the slabs miss
__device__ __forceinline__ double parent_far_view(const double (&o)[3], const double (&d)[3], const double* P6) {
  double tmin = -__builtin_inf(), tmax = __builtin_inf();
  {
    double lo_t[3], hi_t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double t1 = (P6[a] - o[a]) / d[a], t2 = (P6[3 + a] - o[a]) / d[a];
      const bool nan = t1 != t1 || t2 != t2;
      lo_t[a] = nan ? __builtin_nan("") : (t1 < t2 ? t1 : t2);
      hi_t[a] = nan ? __builtin_nan("") : (t1 > t2 ? t1 : t2);
    }
    bool nan = false;
    for (int a = 0; a < 3; ++a) nan |= lo_t[a] != lo_t[a];
    tmin = nan ? __builtin_nan("") : fmax(fmax(lo_t[0], lo_t[1]), lo_t[2]);
    nan = false;
    for (int a = 0; a < 3; ++a) nan |= hi_t[a] != hi_t[a];
    tmax = nan ? __builtin_nan("") : fmin(fmin(hi_t[0], hi_t[1]), hi_t[2]);
  }
  return tmax >= tmin ? tmax : __builtin_inf();
}

// the child filter: distance_to_ray of the centre of the ORIGINAL box (a distance to the whole line) <= radius;
// NaN (a centre on the origin, a non-finite direction) fails
__device__ __forceinline__ bool centre_near_line(const double* b, const double (&o)[3], const double (&d)[3],
                                                 double radius) {
  const double cx = (b[0] + b[3]) / 2, cy = (b[1] + b[4]) / 2, cz = (b[2] + b[5]) / 2;
  const double v0 = cx - o[0], v1 = cy - o[1], v2 = cz - o[2];
  const double dist = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  const double cs = (v0 * d[0] + v1 * d[1] + v2 * d[2]) / dist;
  const double dr = dist * sqrt(1 - cs * cs);
  return dr <= radius;
}

// box b after `rounds` expansion rounds (it grew by ext_1, then ext_2, ..., ext_r = ext_{r-1} + step) -> lo, hi;
// exactly two face hits (h[0], h[1]) make it a hit of the ray
__device__ __forceinline__ bool view_faces(const double* b, int rounds, double step, const double (&o)[3],
                                           const double (&d)[3], double (&lo)[3], double (&hi)[3], double (&h)[6]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = b[a];
    hi[a] = b[3 + a];
  }
  double e = 0.0;
  for (int r = 1; r <= rounds; ++r) {
    e = e + step;
    for (int a = 0; a < 3; ++a) {
      lo[a] = lo[a] - e;
      hi[a] = hi[a] + e;
    }
  }
  return face_hits(o, d, lo, hi, h) == 2;
}

__device__ __forceinline__ void view_hit(ViewHit& H, const double (&h)[6], const double (&lo)[3],
                                         const double (&hi)[3], const double (&q)[3], int method, int rule,
                                         double pnear, double pfar) {
  const double a0 = h[0] < h[1] ? h[0] : h[1], a1 = h[0] < h[1] ? h[1] : h[0];
  H.near = method == 1 ? pnear : a0;
  H.far = method == 1 ? pfar : a1;
  H.col7 = rule == 1 ? pfar : (pfar < a1 ? a1 : pfar);   // MaiCity keeps the parent far bound as is
  H.tin = (q[0] >= lo[0] && q[0] <= hi[0] && q[1] >= lo[1] && q[1] <= hi[1] && q[2] >= lo[2] && q[2] <= hi[2]);
}

// the k hits of one ray (in child-index order) -> its rows at `base`, sorted by near
__device__ __forceinline__ void view_emit(ViewHit (&hits)[HIT_MAX], int k, const double (&o)[3],
                                          const double (&d)[3], double rng, int64_t base, float* __restrict__ rows,
                                          float* __restrict__ ranges, int64_t* __restrict__ other,
                                          uint8_t* __restrict__ tin) {
  const double pnear = 0.0;
  // sort by near (stable insertion sort)
  for (int a = 1; a < k; ++a) {
    const ViewHit t = hits[a];
    int b = a - 1;
    while (b >= 0 && hits[b].near > t.near) {
      hits[b + 1] = hits[b];
      --b;
    }
    hits[b + 1] = t;
  }
  for (int j = 0; j < k; ++j) {
    float* r = rows + 13 * (base + j);
    r[0] = (float)o[0];
    r[1] = (float)o[1];
    r[2] = (float)o[2];
    r[3] = (float)d[0];
    r[4] = (float)d[1];
    r[5] = (float)d[2];
    r[6] = (float)hits[j].near;
    r[7] = (float)hits[j].far;
    r[8] = 3.0f;
    r[9] = (float)pnear;
    r[10] = (float)hits[j].col7;
    r[11] = (float)(j + 1);
    r[12] = j == 0 ? (float)(k - 1) : -1.0f;
    ranges[base + j] = (float)rng;
    other[base + j] = j == 0 ? (int64_t)(k - 1) : 0;
    tin[base + j] = (uint8_t)hits[j].tin;
  }
}

__global__ __launch_bounds__(256) void k_view_rays(int pass, const double* __restrict__ pts, int64_t n,
                                                   const double* __restrict__ origin, const double* __restrict__ b6,
                                                   int64_t C, const double* __restrict__ P6, int method, int rule,
                                                   double radius, int* __restrict__ cnt,
                                                   const int64_t* __restrict__ off, float* __restrict__ rows,
                                                   float* __restrict__ ranges, int64_t* __restrict__ other,
                                                   uint8_t* __restrict__ tin, int* __restrict__ overflow) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double o[3] = {origin[0], origin[1], origin[2]};
  const double q[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  double d[3], rng;
  ray_of(q, o, d, rng);
  const double pfar = parent_far_view(o, d, P6);
  const double pnear = 0.0;
  ViewHit hits[HIT_MAX];
  int nh = 0;
  // expansion rounds: ext_r = ext_{r-1} + step (float64; KITTI 0.05, MaiCity 0.005), the filtered boxes grow by
  // ext_1, then ext_2, ... (the reference updates them in place); give up once ext > 0.5
  const double step = rule == 1 ? 0.005 : 0.05;
  double ext_now = 0.0;
  int rounds = 0;
  bool drop = false;
  for (;;) {
    for (int64_t c = 0; c < C && !(method == 1 && nh > 0); ++c) {
      const double* b = b6 + 6 * c;
      if (!centre_near_line(b, o, d, radius)) continue;
      double lo[3], hi[3], h[6];
      if (!view_faces(b, rounds, step, o, d, lo, hi, h)) continue;
      if (nh >= HIT_MAX) {
        atomicAdd(overflow, 1);
        break;
      }
      view_hit(hits[nh++], h, lo, hi, q, method, rule, pnear, pfar);
    }
    if (nh > 0) break;
    if (ext_now > 0.5) {
      drop = true;
      break;
    }
    ext_now = ext_now + step;
    ++rounds;
  }
  const int k = drop ? 0 : nh;
  if (pass == 0) {
    cnt[i] = k;
    return;
  }
  if (k == 0) return;
  view_emit(hits, k, o, d, rng, off[i], rows, ranges, other, tin);
}

// exclusive scan of int counts -> int64 offsets, total in off[n]; one block
__global__ __launch_bounds__(1024) void k_scan_counts(const int* __restrict__ cnt, int64_t n,
                                                      int64_t* __restrict__ off) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (n + 1023) / 1024;
  const int64_t a = t * per, b = a + per < n ? a + per : n;
  int64_t s = 0;
  for (int64_t i = a; i < b; ++i) s += cnt[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int k = 0; k < 1024; ++k) {
      const int64_t v = part[k];
      part[k] = run;
      run += v;
    }
    off[n] = run;
  }
  __syncthreads();
  int64_t run = part[t];
  for (int64_t i = a; i < b; ++i) {
    off[i] = run;
    run += cnt[i];
  }
}

// ------------------------------------------------------------------------------- uniform grid over child centres
// The child boxes are ~1 m cells of the parent cloud, so a point's 10 nearest centres and a ray's 0.65 m cylinder
// touch a few hundred of them.  The grid bins the centres a query measures distances from (train rows: `centers`;
// two-step rows: the box midpoints, which k_view_rays computes as (b[0] + b[3]) / 2, ...) into cubic cells of edge
// h, CSR layout: cell_start[n_cells + 1], cell_items[C] = child indices, ascending inside each cell, cells
// linearised x fastest so a run of cells along x is one run of items.  The grid queries below produce the rows of
// the flat kernels bit for bit: they only choose which children the same arithmetic is applied to.
constexpr int GRID_CELL_CAP = 1 << 22;            // most cells of a grid; the edge doubles until it fits
constexpr uint64_t GRID_MAGIC = 0x31444952474e4350ull;   // "PCNGRID1"
constexpr size_t GRID_HEADER_BYTES = 256;

struct GridHeader {   // the first bytes of the grid buffer
  uint64_t magic;
  int64_t C;
  double org[3];      // componentwise minimum of the centres
  double h;           // the edge in use
  int dim[3];
  int n_cells;
};

struct GridView {     // what a query kernel takes by value
  double org[3], h;
  int dim[3];
  const int* __restrict__ cell_start;
  const int* __restrict__ cell_items;
};

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t grid_start_bytes() { return align256(((size_t)GRID_CELL_CAP + 1) * 4); }

// cell coordinate of x along axis a, clamped into the grid (x finite, or +-inf from an overflowed difference)
__device__ __forceinline__ int grid_coord(double x, double org, double h, int dim) {
  double t = floor((x - org) / h);
  t = t < 0 ? 0 : t;
  t = t > dim - 1 ? dim - 1 : t;
  return (int)t;
}
__device__ __forceinline__ int grid_cell(const double* c, const double (&org)[3], double h, const int (&dim)[3]) {
  const int x = grid_coord(c[0], org[0], h, dim[0]), y = grid_coord(c[1], org[1], h, dim[1]),
            z = grid_coord(c[2], org[2], h, dim[2]);
  return (z * dim[1] + y) * dim[0] + x;
}

// out[0..2] = min, out[3..5] = max, out[6] = number of non-finite coordinates; one block
__global__ __launch_bounds__(1024) void k_grid_bounds(const double* __restrict__ ctr, int64_t C,
                                                      double* __restrict__ out) {
  __shared__ double smn[3][1024], smx[3][1024];
  __shared__ int sbad[1024];
  const int t = threadIdx.x;
  double mn[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()};
  double mx[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
  int bad = 0;
  for (int64_t i = t; i < C; i += 1024) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v = ctr[3 * i + a];
      if (!(fabs(v) < __builtin_inf())) ++bad;
      mn[a] = v < mn[a] ? v : mn[a];
      mx[a] = v > mx[a] ? v : mx[a];
    }
  }
  for (int a = 0; a < 3; ++a) {
    smn[a][t] = mn[a];
    smx[a][t] = mx[a];
  }
  sbad[t] = bad;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (t < s) {
      for (int a = 0; a < 3; ++a) {
        smn[a][t] = smn[a][t + s] < smn[a][t] ? smn[a][t + s] : smn[a][t];
        smx[a][t] = smx[a][t + s] > smx[a][t] ? smx[a][t + s] : smx[a][t];
      }
      sbad[t] += sbad[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    for (int a = 0; a < 3; ++a) {
      out[a] = smn[a][0];
      out[3 + a] = smx[a][0];
    }
    out[6] = (double)sbad[0];
  }
}

__global__ void k_grid_header(GridHeader hd, GridHeader* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *out = hd;
}

// count: start[cell] += 1 per centre
__global__ __launch_bounds__(256) void k_grid_count(const double* __restrict__ ctr, int64_t C, GridView G,
                                                    int* __restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C) return;
  atomicAdd(start + grid_cell(ctr + 3 * i, G.org, G.h, G.dim), 1);
}

// inclusive scan in place over m ints (m = n_cells + 1, the last count is 0): a[c] = end of cell c; one block
__global__ __launch_bounds__(1024) void k_grid_scan(int* __restrict__ a, int64_t m) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int64_t per = (m + 1023) / 1024;
  const int64_t lo = t * per < m ? t * per : m, hi = lo + per < m ? lo + per : m;
  int s = 0;
  for (int64_t i = lo; i < hi; ++i) s += a[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < 1024; ++k) {
      const int v = part[k];
      part[k] = run;
      run += v;
    }
  }
  __syncthreads();
  int run = part[t];
  for (int64_t i = lo; i < hi; ++i) {
    run += a[i];
    a[i] = run;
  }
}

// fill: each centre takes the next slot below its cell's end (any order), which leaves start[c] = begin of cell c
__global__ __launch_bounds__(256) void k_grid_fill(const double* __restrict__ ctr, int64_t C, GridView G,
                                                   int* __restrict__ start, int* __restrict__ unsorted) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C) return;
  const int pos = atomicSub(start + grid_cell(ctr + 3 * i, G.org, G.h, G.dim), 1) - 1;
  unsorted[pos] = (int)i;
}

// per-cell sort by rank: an item goes to its cell's begin + the number of smaller items of that cell (the indices
// are distinct), so cell_items does not depend on the order the atomics of the fill resolved in
__global__ __launch_bounds__(256) void k_grid_rank(const double* __restrict__ ctr, int64_t C, GridView G,
                                                   const int* __restrict__ unsorted, int* __restrict__ items) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= C) return;
  const int v = unsorted[p];
  const int cell = grid_cell(ctr + 3 * (int64_t)v, G.org, G.h, G.dim);
  const int s = G.cell_start[cell], e = G.cell_start[cell + 1];
  int rank = 0;
  for (int j = s; j < e; ++j) rank += unsorted[j] < v ? 1 : 0;
  items[s + rank] = v;
}

// ---- train rows: the exact KNN nearest centres by expanding rings of cells around the point's cell
// insertion ordered by (ds, index): candidates arrive in cell order, and the flat scan's strict < over ascending
// indices keeps exactly this order
__device__ __forceinline__ void knn_insert(double (&kd)[KNN], int (&ki)[KNN], double ds, int ci) {
  if (!(ds < kd[KNN - 1] || (ds == kd[KNN - 1] && ci < ki[KNN - 1]))) return;
  int pos = KNN - 1;
#pragma unroll
  for (int k = KNN - 1; k > 0; --k) {
    if (kd[k - 1] > ds || (kd[k - 1] == ds && ki[k - 1] > ci)) {
      kd[k] = kd[k - 1];
      ki[k] = ki[k - 1];
      pos = k - 1;
    } else {
      break;
    }
  }
  kd[pos] = ds;
  ki[pos] = ci;
}

__device__ __forceinline__ void knn_cells(double (&kd)[KNN], int (&ki)[KNN], const double (&q)[3],
                                          const double* __restrict__ ctr, const GridView& G, int first, int last) {
  const int e = G.cell_start[last + 1];
  for (int j = G.cell_start[first]; j < e; ++j) {
    const int ci = G.cell_items[j];
    const double* c = ctr + 3 * (int64_t)ci;
    const double a = q[0] - c[0], b = q[1] - c[1], f = q[2] - c[2];
    knn_insert(kd, ki, a * a + b * b + f * f, ci);
  }
}

__global__ __launch_bounds__(256) void k_train_rays_grid(int pass, const double* __restrict__ pts, int64_t n,
                                                         const double* __restrict__ origin,
                                                         const double* __restrict__ ctr,
                                                         const double* __restrict__ b6,
                                                         const double* __restrict__ P6, double se, int rule,
                                                         GridView G, int* __restrict__ cnt,
                                                         const int64_t* __restrict__ off, float* __restrict__ rows,
                                                         int* __restrict__ nshort) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double o[3] = {origin[0], origin[1], origin[2]};
  const double q[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  double kd[KNN];
  int ki[KNN];
#pragma unroll
  for (int k = 0; k < KNN; ++k) {
    kd[k] = __builtin_inf();
    ki[k] = -1;
  }
  // a non-finite point is at distance NaN or inf of every centre: the flat scan keeps none, so no cell is visited
  if (fabs(q[0]) < __builtin_inf() && fabs(q[1]) < __builtin_inf() && fabs(q[2]) < __builtin_inf()) {
    int cq[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) cq[a] = grid_coord(q[a], G.org[a], G.h, G.dim[a]);
    for (int r = 0;; ++r) {
      // ring r: the cells of the block within Chebyshev radius r of cq that ring r - 1 has not visited
      int lo[3], hi[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = cq[a] - r > 0 ? cq[a] - r : 0;
        hi[a] = cq[a] + r < G.dim[a] - 1 ? cq[a] + r : G.dim[a] - 1;
      }
      for (int z = lo[2]; z <= hi[2]; ++z) {
        const bool zin = z > cq[2] - r && z < cq[2] + r;
        for (int y = lo[1]; y <= hi[1]; ++y) {
          const int row = (z * G.dim[1] + y) * G.dim[0];
          if (zin && y > cq[1] - r && y < cq[1] + r) {   // an inner row: only its two end cells are new
            if (cq[0] - r >= 0) knn_cells(kd, ki, q, ctr, G, row + cq[0] - r, row + cq[0] - r);
            if (cq[0] + r < G.dim[0]) knn_cells(kd, ki, q, ctr, G, row + cq[0] + r, row + cq[0] + r);
          } else {
            knn_cells(kd, ki, q, ctr, G, row + lo[0], row + hi[0]);
          }
        }
      }
      // q lies inside the visited block once the block's faces on the grid boundary are pushed to infinity, and
      // every unvisited centre lies beyond one of the other faces, so it is at least `gap` from q: the smallest
      // distance from q to such a face.  The slack covers the rounding of the binning (a centre can sit ~1e-16 of
      // its offset outside its cell) and of the face coordinate; it only ever delays the stop.
      double gap = __builtin_inf();
      bool whole = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double slack = 1e-12 * (fabs(q[a] - G.org[a]) + (G.dim[a] + 1) * G.h);
        if (lo[a] > 0) {
          whole = false;
          const double g = (q[a] - (G.org[a] + lo[a] * G.h)) - slack;
          gap = g < gap ? g : gap;
        }
        if (hi[a] < G.dim[a] - 1) {
          whole = false;
          const double g = ((G.org[a] + (hi[a] + 1) * G.h) - q[a]) - slack;
          gap = g < gap ? g : gap;
        }
      }
      if (whole) break;
      gap = gap > 0 ? gap : 0;
      // strict: a centre at exactly the tenth distance with a lower index must still be seen
      if (kd[KNN - 1] < gap * gap * (1 - 1e-9)) break;
    }
  }
  train_row(pass, i, q, o, ki, b6, P6, se, rule, cnt, off, rows, nshort);
}

// ---- two-step rows: the children whose centre can pass the 0.65 m filter, from a walk of the ray's line
// The filter (centre_near_line) is a distance to the infinite line, so the whole line is walked, both directions.
// Walk: A = the direction's dominant axis (|d_A| >= 1/sqrt 3).  For each layer of cells iA, [x0, x1] its extent
// along A.  A centre p of that layer within R of the line has its closest line point L within R of p, so L_A lies
// in [x0 - R, x1 + R]; along another axis B the line's coordinate is linear in L_A, so L_B lies between its values
// at the two ends of that interval, and p_B within R of that.  The cells of layer iA whose B and C extents meet
// those ranges are visited; each cell is visited once, so no child comes twice.
// R = radius + 2e-6: the filter's computed dist * sqrt(1 - cs * cs) can accept a centre whose true distance is
// above the radius; its error is about 1e-15 * dist^2 / (2 * radius), below 1e-6 for centres within 3e4 m of the
// origin (5e-12 m at 170 m); the second 1e-6 covers the rounding of the walk and of the binning (~1e-12 m).
template <class F>
__device__ __forceinline__ void walk_line(const double (&o)[3], const double (&d)[3], double radius,
                                          const GridView& G, F&& visit) {
  if (!(fabs(d[0]) <= 1.0 && fabs(d[1]) <= 1.0 && fabs(d[2]) <= 1.0)) return;   // q == origin or non-finite
  const double R = radius + 2e-6;
  const double a0 = fabs(d[0]), a1 = fabs(d[1]), a2 = fabs(d[2]);
  const int A = a0 >= a1 ? (a0 >= a2 ? 0 : 2) : (a1 >= a2 ? 1 : 2);
  if (!(fabs(d[A]) > 0.5)) return;   // not a unit vector: cannot happen for a finite direction
  const double inv = 1.0 / G.h;
  for (int iA = 0; iA < G.dim[A]; ++iA) {
    const double x0 = G.org[A] + iA * G.h - R, x1 = G.org[A] + (iA + 1) * G.h + R;
    int lo[3], hi[3];
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (a == A) {
        lo[a] = hi[a] = iA;
        continue;
      }
      const double s = d[a] / d[A];
      const double e0 = o[a] + (x0 - o[A]) * s, e1 = o[a] + (x1 - o[A]) * s;
      const double f0 = floor(((e0 < e1 ? e0 : e1) - R - G.org[a]) * inv);
      const double f1 = floor(((e0 < e1 ? e1 : e0) + R - G.org[a]) * inv);
      if (!(f1 >= 0 && f0 <= G.dim[a] - 1)) any = false;   // the line passes this layer outside the grid
      lo[a] = f0 > 0 ? (int)(f0 < G.dim[a] - 1 ? f0 : G.dim[a] - 1) : 0;
      hi[a] = f1 < G.dim[a] - 1 ? (int)(f1 > 0 ? f1 : 0) : G.dim[a] - 1;
    }
    if (!any) continue;
    for (int z = lo[2]; z <= hi[2]; ++z) {
      for (int y = lo[1]; y <= hi[1]; ++y) {
        const int row = (z * G.dim[1] + y) * G.dim[0];
        const int e = G.cell_start[row + hi[0] + 1];
        for (int j = G.cell_start[row + lo[0]]; j < e; ++j) visit(G.cell_items[j]);
      }
    }
  }
}

// count pass: per ray the round it succeeded at and the child indices of its hits, ascending, in
// hidx[slot * n + ray]: the HIT_MAX lowest indices (method 1: the lowest), as the flat scan over ascending c keeps
__global__ __launch_bounds__(256) void k_view_count_grid(const double* __restrict__ pts, int64_t n,
                                                         const double* __restrict__ origin,
                                                         const double* __restrict__ b6, int method, int rule,
                                                         double radius, GridView G, int* __restrict__ cnt,
                                                         int* __restrict__ round_of, int* __restrict__ hidx,
                                                         int* __restrict__ overflow) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double o[3] = {origin[0], origin[1], origin[2]};
  const double q[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  double d[3], rng;
  ray_of(q, o, d, rng);
  const int keep = method == 1 ? 1 : HIT_MAX;
  int* __restrict__ mine = hidx + i;
  int nh = 0;
  bool over = false;
  const double step = rule == 1 ? 0.005 : 0.05;
  double ext_now = 0.0;
  int rounds = 0;
  bool drop = false;
  for (;;) {
    // the filter does not depend on the round, so a round walks the same cells and re-tests the same candidates
    walk_line(o, d, radius, G, [&](int c) {
      const double* b = b6 + 6 * (int64_t)c;
      if (!centre_near_line(b, o, d, radius)) return;
      double lo[3], hi[3], h[6];
      if (!view_faces(b, rounds, step, o, d, lo, hi, h)) return;
      int pos = nh;
      if (nh == keep) {
        over = true;
        if (c > mine[(int64_t)(keep - 1) * n]) return;
        pos = keep - 1;
      } else {
        ++nh;
      }
      for (; pos > 0 && mine[(int64_t)(pos - 1) * n] > c; --pos)
        mine[(int64_t)pos * n] = mine[(int64_t)(pos - 1) * n];
      mine[(int64_t)pos * n] = c;
    });
    if (nh > 0) break;
    if (ext_now > 0.5) {
      drop = true;
      break;
    }
    ext_now = ext_now + step;
    ++rounds;
  }
  if (over && method != 1) atomicAdd(overflow, 1);
  cnt[i] = drop ? 0 : nh;
  round_of[i] = rounds;
}

// writing pass: the face tests of the stored hits only, then the rows as k_view_rays writes them
__global__ __launch_bounds__(256) void k_view_emit_grid(const double* __restrict__ pts, int64_t n,
                                                        const double* __restrict__ origin,
                                                        const double* __restrict__ b6, int64_t C,
                                                        const double* __restrict__ P6, int method, int rule,
                                                        const int* __restrict__ cnt,
                                                        const int* __restrict__ round_of,
                                                        const int* __restrict__ hidx,
                                                        const int64_t* __restrict__ off, float* __restrict__ rows,
                                                        float* __restrict__ ranges, int64_t* __restrict__ other,
                                                        uint8_t* __restrict__ tin) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int k = cnt[i];
  if (k <= 0) return;
  k = k < HIT_MAX ? k : HIT_MAX;
  const double o[3] = {origin[0], origin[1], origin[2]};
  const double q[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  double d[3], rng;
  ray_of(q, o, d, rng);
  const double pfar = parent_far_view(o, d, P6);
  const double step = rule == 1 ? 0.005 : 0.05;
  const int rounds = round_of[i];
  ViewHit hits[HIT_MAX];
  for (int j = 0; j < k; ++j) {
    const int c = hidx[(int64_t)j * n + i];
    double lo[3], hi[3], h[6] = {0, 0, 0, 0, 0, 0};
    view_faces(b6 + 6 * (int64_t)(c >= 0 && c < C ? c : 0), rounds, step, o, d, lo, hi, h);
    view_hit(hits[j], h, lo, hi, q, method, rule, 0.0, pfar);
  }
  view_emit(hits, k, o, d, rng, off[i], rows, ranges, other, tin);
}

}  // namespace pcn

using namespace pcn;

extern "C" size_t pcnerf_rays_workspace_bytes(int64_t n_points) {
  return (size_t)((n_points + 1) * 8 + n_points * 4 + 64 + 255) & ~(size_t)255;
}

extern "C" int pcnerf_build_train_rays(const double* points, int64_t n_points, const double* origin,
                                       const double* centers, const double* bounds6, int64_t n_children,
                                       const double* parent6, double surface_expand, int face_rule, void* workspace,
                                       float* rows, int64_t* n_rows, int* n_short, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(points && origin && centers && bounds6 && parent6 && workspace && rows && n_rows,
            "pcnerf_build_train_rays: null argument");
  PCN_CHECK(n_points > 0 && n_children >= KNN, "pcnerf_build_train_rays: need points and >= 10 child boxes");
  PCN_CHECK(face_rule == 0 || (face_rule == 1 && n_short),
            "pcnerf_build_train_rays: face_rule must be 0 (0606) or 1 (0406, with n_short)");
  hipStream_t s = (hipStream_t)stream;
  int64_t* off = (int64_t*)workspace;
  int* cnt = (int*)(off + n_points + 1);
  const dim3 g((unsigned)((n_points + 255) / 256)), b(256);
  if (n_short) PCN_HIP(hipMemsetAsync(n_short, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_train_rays, g, b, 0, s, 0, points, n_points, origin, centers, bounds6, n_children, parent6,
                     surface_expand, face_rule, cnt, (const int64_t*)nullptr, rows, n_short);
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, cnt, n_points, off);
  hipLaunchKernelGGL(k_train_rays, g, b, 0, s, 1, points, n_points, origin, centers, bounds6, n_children, parent6,
                     surface_expand, face_rule, cnt, off, rows, n_short);
  PCN_HIP(hipMemcpyAsync(n_rows, off + n_points, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  PCN_LAUNCH_CHECK("pcnerf_build_train_rays");
  PCN_API_END
}

extern "C" int pcnerf_count_view_rows(const double* points, int64_t n_points, const double* origin,
                                      const double* bounds6, int64_t n_children, const double* parent6, int method,
                                      int rule, void* workspace, int64_t* n_rows, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(points && origin && bounds6 && parent6 && workspace && n_rows, "pcnerf_count_view_rows: null argument");
  PCN_CHECK(n_points > 0 && n_children > 0, "pcnerf_count_view_rows: empty input");
  PCN_CHECK(rule == 0 || rule == 1, "pcnerf_count_view_rows: rule must be 0 (KITTI) or 1 (MaiCity)");
  hipStream_t s = (hipStream_t)stream;
  int64_t* off = (int64_t*)workspace;
  int* cnt = (int*)(off + n_points + 1);
  int* ovf = (int*)(cnt + n_points);
  PCN_HIP(hipMemsetAsync(ovf, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_view_rays, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, s, 0, points, n_points,
                     origin, bounds6, n_children, parent6, method, rule, 0.65, cnt, (const int64_t*)nullptr,
                     (float*)nullptr, (float*)nullptr, (int64_t*)nullptr, (uint8_t*)nullptr, ovf);
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, cnt, n_points, off);
  PCN_HIP(hipMemcpyAsync(n_rows, off + n_points, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  PCN_LAUNCH_CHECK("pcnerf_count_view_rows");
  PCN_API_END
}

extern "C" int pcnerf_emit_view_rows(const double* points, int64_t n_points, const double* origin,
                                     const double* bounds6, int64_t n_children, const double* parent6, int method,
                                     int rule, void* workspace, float* rows, float* ranges, int64_t* other,
                                     uint8_t* true_in, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(points && origin && bounds6 && parent6 && workspace && rows && ranges && other && true_in,
            "pcnerf_emit_view_rows: null argument");
  int64_t* off = (int64_t*)workspace;
  int* cnt = (int*)(off + n_points + 1);
  int* ovf = (int*)(cnt + n_points);
  hipLaunchKernelGGL(k_view_rays, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream, 1,
                     points, n_points, origin, bounds6, n_children, parent6, method, rule, 0.65, cnt,
                     (const int64_t*)off, rows, ranges, other, true_in, ovf);
  PCN_LAUNCH_CHECK("pcnerf_emit_view_rows");
  PCN_API_END
}

// ------------------------------------------------------------------------------- grid entry points
extern "C" size_t pcnerf_child_grid_bytes(int64_t n_children) {
  const size_t c = n_children > 0 ? (size_t)n_children : 0;
  return GRID_HEADER_BYTES + grid_start_bytes() + 2 * align256(c * 4);
}

extern "C" size_t pcnerf_rays_grid_workspace_bytes(int64_t n_points) {
  const size_t n = n_points > 0 ? (size_t)n_points : 0;
  return pcnerf_rays_workspace_bytes(n_points > 0 ? n_points : 0) + align256(n * (8 + HIT_MAX * 4));
}

namespace {

struct GridBuffers {
  int* start;
  int* unsorted;
  int* items;
};
GridBuffers grid_buffers(const void* grid, int64_t C) {
  char* base = (char*)grid + GRID_HEADER_BYTES;
  return {(int*)base, (int*)(base + grid_start_bytes()),
          (int*)(base + grid_start_bytes() + align256((size_t)C * 4))};
}

GridView grid_view(const GridHeader& hd, const GridBuffers& B) {
  GridView G;
  for (int a = 0; a < 3; ++a) {
    G.org[a] = hd.org[a];
    G.dim[a] = hd.dim[a];
  }
  G.h = hd.h;
  G.cell_start = B.start;
  G.cell_items = B.items;
  return G;
}

// the header of a built grid (one small device-to-host copy, which waits for the stream), checked against the
// caller's child count before anything is launched
GridView load_grid(const void* grid, int64_t C, hipStream_t s, const std::string& who) {
  GridHeader hd;
  PCN_HIP(hipMemcpyAsync(&hd, grid, sizeof(hd), hipMemcpyDeviceToHost, s));
  PCN_HIP(hipStreamSynchronize(s));
  PCN_CHECK(hd.magic == GRID_MAGIC, who + ": grid is not a grid built by pcnerf_build_child_grid");
  PCN_CHECK(hd.C == C, who + ": size mismatch, the grid was built over another number of children");
  PCN_CHECK(hd.h > 0 && hd.dim[0] > 0 && hd.dim[1] > 0 && hd.dim[2] > 0 && hd.n_cells <= GRID_CELL_CAP &&
                (int64_t)hd.dim[0] * hd.dim[1] * hd.dim[2] == hd.n_cells,
            who + ": corrupt grid header");
  return grid_view(hd, grid_buffers(grid, C));
}

}  // namespace

extern "C" int pcnerf_build_child_grid(const double* centers, int64_t n_children, double cell, void* grid,
                                       size_t grid_bytes, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(centers && grid, "pcnerf_build_child_grid: null argument");
  PCN_CHECK(n_children > 0 && n_children < 0x7fffffff, "pcnerf_build_child_grid: need at least one child centre");
  PCN_CHECK(cell > 0 && cell < __builtin_inf(), "pcnerf_build_child_grid: the cell edge must be positive and finite");
  PCN_CHECK(grid_bytes >= pcnerf_child_grid_bytes(n_children),
            "pcnerf_build_child_grid: size mismatch, grid_bytes is below pcnerf_child_grid_bytes(n_children)");
  hipStream_t s = (hipStream_t)stream;
  const GridBuffers B = grid_buffers(grid, n_children);
  PCN_HIP(hipMemsetAsync(grid, 0, GRID_HEADER_BYTES, s));   // no valid header until the build is through
  // bounds of the centres (7 doubles, parked in the sort's scratch) decide the dimensions on the host
  double bd[7];
  hipLaunchKernelGGL(k_grid_bounds, dim3(1), dim3(1024), 0, s, centers, n_children, (double*)B.unsorted);
  PCN_HIP(hipMemcpyAsync(bd, B.unsorted, sizeof(bd), hipMemcpyDeviceToHost, s));
  PCN_HIP(hipStreamSynchronize(s));
  PCN_LAUNCH_CHECK("pcnerf_build_child_grid");
  PCN_CHECK(bd[6] == 0, "pcnerf_build_child_grid: non-finite child centre");
  GridHeader hd;
  hd.magic = GRID_MAGIC;
  hd.C = n_children;
  hd.h = cell;
  double ext[3];
  for (int a = 0; a < 3; ++a) {
    hd.org[a] = bd[a];
    ext[a] = bd[3 + a] - bd[a];
    PCN_CHECK(ext[a] < __builtin_inf(), "pcnerf_build_child_grid: the centres' extent overflows");
  }
  for (;;) {   // floor(extent / h) + 1 cells per axis; the edge doubles until the grid fits the cap
    double total = 1;
    for (int a = 0; a < 3; ++a) total *= floor(ext[a] / hd.h) + 1;
    if (total <= GRID_CELL_CAP) break;
    hd.h *= 2;
  }
  for (int a = 0; a < 3; ++a) hd.dim[a] = (int)(floor(ext[a] / hd.h) + 1);
  hd.n_cells = hd.dim[0] * hd.dim[1] * hd.dim[2];
  GridView G = grid_view(hd, B);
  const dim3 g((unsigned)((n_children + 255) / 256)), b(256);
  PCN_HIP(hipMemsetAsync(B.start, 0, ((size_t)hd.n_cells + 1) * 4, s));
  hipLaunchKernelGGL(k_grid_count, g, b, 0, s, centers, n_children, G, B.start);
  hipLaunchKernelGGL(k_grid_scan, dim3(1), dim3(1024), 0, s, B.start, (int64_t)hd.n_cells + 1);
  hipLaunchKernelGGL(k_grid_fill, g, b, 0, s, centers, n_children, G, B.start, B.unsorted);
  hipLaunchKernelGGL(k_grid_rank, g, b, 0, s, centers, n_children, G, (const int*)B.unsorted, B.items);
  hipLaunchKernelGGL(k_grid_header, dim3(1), dim3(64), 0, s, hd, (GridHeader*)grid);
  PCN_LAUNCH_CHECK("pcnerf_build_child_grid");
  PCN_API_END
}

extern "C" int pcnerf_build_train_rays_grid(const double* points, int64_t n_points, const double* origin,
                                            const double* centers, const double* bounds6, int64_t n_children,
                                            const double* parent6, double surface_expand, int face_rule,
                                            const void* grid, void* workspace, float* rows, int64_t* n_rows,
                                            int* n_short, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(points && origin && centers && bounds6 && parent6 && grid && workspace && rows && n_rows,
            "pcnerf_build_train_rays_grid: null argument");
  PCN_CHECK(n_points > 0 && n_children >= KNN, "pcnerf_build_train_rays_grid: need points and >= 10 child boxes");
  PCN_CHECK(face_rule == 0 || (face_rule == 1 && n_short),
            "pcnerf_build_train_rays_grid: face_rule must be 0 (0606) or 1 (0406, with n_short)");
  hipStream_t s = (hipStream_t)stream;
  const GridView G = load_grid(grid, n_children, s, "pcnerf_build_train_rays_grid");
  int64_t* off = (int64_t*)workspace;
  int* cnt = (int*)(off + n_points + 1);
  const dim3 g((unsigned)((n_points + 255) / 256)), b(256);
  if (n_short) PCN_HIP(hipMemsetAsync(n_short, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_train_rays_grid, g, b, 0, s, 0, points, n_points, origin, centers, bounds6, parent6,
                     surface_expand, face_rule, G, cnt, (const int64_t*)nullptr, rows, n_short);
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, cnt, n_points, off);
  hipLaunchKernelGGL(k_train_rays_grid, g, b, 0, s, 1, points, n_points, origin, centers, bounds6, parent6,
                     surface_expand, face_rule, G, cnt, off, rows, n_short);
  PCN_HIP(hipMemcpyAsync(n_rows, off + n_points, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  PCN_LAUNCH_CHECK("pcnerf_build_train_rays_grid");
  PCN_API_END
}

namespace {
// the grid workspace: the flat one (offsets, counts, overflow counter), then per ray its round and its hits
struct GridWorkspace {
  int64_t* off;
  int *cnt, *ovf, *round_of, *hidx;
};
GridWorkspace grid_workspace(void* workspace, int64_t n) {
  GridWorkspace W;
  W.off = (int64_t*)workspace;
  W.cnt = (int*)(W.off + n + 1);
  W.ovf = W.cnt + n;
  W.round_of = (int*)((char*)workspace + pcnerf_rays_workspace_bytes(n));
  W.hidx = W.round_of + 2 * n;
  return W;
}
}  // namespace

extern "C" int pcnerf_count_view_rows_grid(const double* points, int64_t n_points, const double* origin,
                                           const double* bounds6, int64_t n_children, const double* parent6,
                                           int method, int rule, const void* grid, void* workspace, int64_t* n_rows,
                                           void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(points && origin && bounds6 && parent6 && grid && workspace && n_rows,
            "pcnerf_count_view_rows_grid: null argument");
  PCN_CHECK(n_points > 0 && n_children > 0, "pcnerf_count_view_rows_grid: empty input");
  PCN_CHECK(rule == 0 || rule == 1, "pcnerf_count_view_rows_grid: rule must be 0 (KITTI) or 1 (MaiCity)");
  hipStream_t s = (hipStream_t)stream;
  const GridView G = load_grid(grid, n_children, s, "pcnerf_count_view_rows_grid");
  const GridWorkspace W = grid_workspace(workspace, n_points);
  PCN_HIP(hipMemsetAsync(W.ovf, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_view_count_grid, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, s, points, n_points,
                     origin, bounds6, method, rule, 0.65, G, W.cnt, W.round_of, W.hidx, W.ovf);
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, W.cnt, n_points, W.off);
  PCN_HIP(hipMemcpyAsync(n_rows, W.off + n_points, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  PCN_LAUNCH_CHECK("pcnerf_count_view_rows_grid");
  PCN_API_END
}

extern "C" int pcnerf_emit_view_rows_grid(const double* points, int64_t n_points, const double* origin,
                                          const double* bounds6, int64_t n_children, const double* parent6,
                                          int method, int rule, const void* grid, void* workspace, float* rows,
                                          float* ranges, int64_t* other, uint8_t* true_in, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(points && origin && bounds6 && parent6 && grid && workspace && rows && ranges && other && true_in,
            "pcnerf_emit_view_rows_grid: null argument");
  PCN_CHECK(n_points > 0 && n_children > 0, "pcnerf_emit_view_rows_grid: empty input");
  PCN_CHECK(rule == 0 || rule == 1, "pcnerf_emit_view_rows_grid: rule must be 0 (KITTI) or 1 (MaiCity)");
  const GridWorkspace W = grid_workspace(workspace, n_points);
  hipLaunchKernelGGL(k_view_emit_grid, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     points, n_points, origin, bounds6, n_children, parent6, method, rule, (const int*)W.cnt,
                     (const int*)W.round_of, (const int*)W.hidx, (const int64_t*)W.off, rows, ranges, other, true_in);
  PCN_LAUNCH_CHECK("pcnerf_emit_view_rows_grid");
  PCN_API_END
}
