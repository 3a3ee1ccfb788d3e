"""Numpy float64 restatement of the map / particle-filter layer (tests of nof.localization.assign_blocks,
pcnerf::mcl_weights and pcnerf::systematic_resample) and the two-block analytic scene -- test infrastructure only.

The restatement uses the kernels' float64 operations one for one where the result is a decision (block assignment,
the -inf pattern, best, the ancestors of exactly representable weights), so those are compared for equality; sums are
numpy's own (sequential cumsum, pairwise sum), compared within a rounding bound."""
import functools
import math

import numpy as np
import torch

import localization_ref as LR
import registration_ref as RR

TWO_PI = 2.0 * math.pi
# block 1 of the two-block scene: analytic_fold with this coefficient of cos y in place of -0.8 s (a wider cavity along
# y, not merely a sharper one).  test_map_localization_cpu checks that every one of the 256 beams is a hit with it.
BLOCK1_COS_Y = -0.5
RESAMPLE_SEEDS = (11, 12, 13)   # the tolerant resampling cases (checked on the CPU against the hierarchical prefix)
EDGE_TOL = 1e-12                # a draw within EDGE_TOL * C of a prefix edge may fall to either side
EDGE_CAP = 0.01                 # at most this fraction of a case's draws


# ----------------------------------------------------------------------------------------------- assign_blocks
def assign_blocks(boxes, t, margin=0.0):
    """boxes (B, 6) [lo, hi], t (P, 3) float64 -> (P,) int32: the containing block with the largest clearance, the
    lowest index on ties, -1 for none or a NaN."""
    boxes, t = np.asarray(boxes, np.float64), np.asarray(t, np.float64)
    out = np.full(t.shape[0], -1, np.int32)
    for p in range(t.shape[0]):
        best, best_clear = -1, 0.0
        for b in range(boxes.shape[0]):
            lo, hi = boxes[b, :3], boxes[b, 3:]
            with np.errstate(invalid="ignore"):
                inside = bool(np.all((lo + margin <= t[p]) & (t[p] <= hi - margin)))
                clear = float(np.min(np.minimum(t[p] - lo, hi - t[p])))
            if inside and (best < 0 or clear > best_clear):
                best, best_clear = b, clear
        out[p] = best
    return out


# ----------------------------------------------------------------------------------------------- mcl_weights
def mcl_weights(logw_prev, scores4, blocks, n_usable, miss_cost, beta):
    """-> dict(w, logw (P,), ess, best, degenerate)."""
    logw_prev, s4 = np.asarray(logw_prev, np.float64), np.asarray(scores4, np.float64)
    blocks = np.asarray(blocks)
    n = logw_prev.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = (s4[:, 0] + miss_cost * (float(n_usable) - s4[:, 1])) / float(n_usable)
        lw = logw_prev - beta * mean
        lw = np.where((blocks < 0) | ~np.isfinite(mean) | ~(lw < np.inf), -np.inf, lw)
    m = lw.max()
    if not m > -np.inf:
        return {"w": np.full(n, 1.0 / n), "logw": np.zeros(n), "ess": float(n), "best": 0, "degenerate": 1}
    e = np.where(lw == -np.inf, 0.0, np.exp(np.where(lw == -np.inf, 0.0, lw - m)))
    Z = e.sum()
    w = e / Z
    with np.errstate(invalid="ignore"):
        logw = np.where(lw == -np.inf, -np.inf, (lw - m) - math.log(Z))
    return {"w": w, "logw": logw, "ess": 1.0 / float((w * w).sum()), "best": int(np.argmax(lw)), "degenerate": 0}


# ----------------------------------------------------------------------------------------------- systematic_resample
def clamp_weights(w):
    w = np.asarray(w, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where((w > 0) & (w < np.inf), w, 0.0)


def hierarchical_prefix(w, per_thread=4, threads=256):
    """The kernels' order: runs of ``per_thread`` weights added in order, the runs' bases by one serial chain inside a
    group of ``threads`` runs, the groups' offsets by one serial chain: c_i = off_g + (base_t + run_i)."""
    w = clamp_weights(w)
    n = w.shape[0]
    group = per_thread * threads
    c = np.zeros(n)
    off = 0.0
    for g0 in range(0, n, group):
        base = 0.0
        for t0 in range(g0, min(g0 + group, n), per_thread):
            run = 0.0
            for i in range(t0, min(t0 + per_thread, n)):
                run += w[i]
                c[i] = off + (base + run)
            base += run
        off += base
    return c


def draws(c_total, u0, n_out):
    return (np.arange(n_out, dtype=np.float64) + u0) / float(n_out) * c_total


def ancestors_of(c, w, u0, n_out):
    """The first i with c_i > u_j, clamped to the last i with w_i > 0."""
    pos = np.nonzero(clamp_weights(w) > 0)[0]
    last = int(pos[-1]) if pos.size else 0
    u = draws(c[-1], u0, n_out)
    return np.minimum(np.searchsorted(c, u, side="right"), last).astype(np.int32)


def systematic_resample(w, u0, n_out, ess=None, ess_threshold=0.0):
    """-> (ancestors (n_out,) int32, resampled: bool) with numpy's sequential cumsum as the prefix."""
    w = clamp_weights(w)
    if ess is not None and ess >= ess_threshold:
        assert n_out == w.shape[0]
        return np.arange(n_out, dtype=np.int32), False
    return ancestors_of(np.cumsum(w), w, u0, n_out), True


def near_an_edge(c, u, tol=EDGE_TOL):
    """Draws whose u lies within tol * C of a prefix edge (they may fall to either side in another summation order)."""
    C = c[-1]
    k = np.searchsorted(c, u, side="left")
    lo = np.abs(u - c[np.clip(k - 1, 0, c.shape[0] - 1)])
    hi = np.abs(u - c[np.clip(k, 0, c.shape[0] - 1)])
    return np.minimum(lo, hi) <= tol * C


def exact_weights(n, seed):
    """Integer multiples of 2^-20 (every prefix sum is exact in any order), with several zeros, the last entries among
    them (the single weight of n == 1 stays positive)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 200, size=n).astype(np.float64)
    if n >= 3:
        k[rng.integers(0, n, size=max(1, n // 5))] = 0.0
        k[-2:] = 0.0
        k[0] = 7.0
    else:
        k[0] = 7.0
    return k * 2.0 ** -20


def random_weights(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.random(n) ** 4
    return w / w.sum()


def count_property(anc, w, n_out):
    """|count_i - n_out w_i / C| < 1 + 1e-9 n_out for all i."""
    w = clamp_weights(w)
    counts = np.bincount(anc, minlength=w.shape[0]).astype(np.float64)
    return bool(np.all(np.abs(counts - n_out * w / w.sum()) < 1.0 + 1e-9 * n_out))


# ----------------------------------------------------------------------------------------------- the two-block scene
def block1_fold(coef=BLOCK1_COS_Y, s=RR.S_FIELD):
    a = RR.analytic_fold(s).clone()
    a[7] = coef * s
    return a


def shifted(T, dx=TWO_PI):
    T = torch.as_tensor(T, dtype=torch.float64).clone()
    T[0, 3] += dx
    return T


BOX0 = (tuple(RR.PARENT_LO), tuple(RR.PARENT_HI))
BOX1 = ((RR.PARENT_LO[0] + TWO_PI, RR.PARENT_LO[1], RR.PARENT_LO[2]),
        (RR.PARENT_HI[0] + TWO_PI, RR.PARENT_HI[1], RR.PARENT_HI[2]))


@functools.lru_cache(maxsize=None)
def two_block_scene():
    """Block 0: the analytic cavity in [-2.5, 2.5]^3; block 1: block1_fold in the box shifted by (2 pi, 0, 0) (the
    encoding's lowest frequency has period 2 pi, so the field is the same function of x - 2 pi).  256 directions
    (seed 0) seen from T*_1 = T* shifted into block 1, their float64 ranges and hit probabilities, and 125 + 125
    hypotheses: pose_grid (0.2 m / 5 degrees) around se3_exp(GRID_OFFSET) @ T*_0 and around se3_exp(GRID_OFFSET) @ T*_1."""
    from nof.localization import pose_grid
    from nof.registration import se3_exp
    f0, f1 = RR.analytic_fold(), block1_fold()
    T0 = se3_exp(RR.XI_STAR)
    T1 = shifted(T0)
    dirs = RR.unit_directions(256, 0)
    ranges, sumw = LR.render_poses(f1, f1, dirs, [T1], 64, 128, lo=BOX1[0], hi=BOX1[1])
    ranges, sumw = ranges[0], sumw[0]
    points = (dirs * ranges[:, None]).float()
    off = se3_exp(LR.GRID_OFFSET)
    c0, c1 = off @ T0, off @ T1
    grid = lambda c: pose_grid(c, 0.4, 0.2, math.radians(10.0), math.radians(5.0))   # noqa: E731
    poses = torch.cat([grid(c0), grid(c1)])
    boxes = np.array([list(BOX0[0]) + list(BOX0[1]), list(BOX1[0]) + list(BOX1[1])], np.float64)
    return {"folds": torch.stack([f0, f1]), "boxes": boxes, "T0": T0, "T1": T1, "dirs": dirs, "ranges": ranges,
            "sumw": sumw, "points": points, "center1": c1, "poses": poses}
