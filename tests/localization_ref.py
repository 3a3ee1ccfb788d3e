"""Float64 restatement of pose-hypothesis scoring (tests of nof.localization and pcnerf::score_poses_fold) -- test
infrastructure only, torch CPU / numpy: the rays of registration_ref.rays_f64 with scan_rays' ``far >= near`` clamp,
registration_ref.render_two_pass, and a numpy float64 reduction with the kernel's validity rule (usable: the target is
finite and > 0; valid: usable, sumw >= min_sumw, depth finite)."""
import functools
import math

import numpy as np
import torch

import registration_ref as RR

PLANE_POSES = ((0, 0, 0, 0, 0, 0), (0.3, -0.2, 0.1, 0.02, -0.05, 0.4), (-0.5, 0.4, 0, 0, 0, -1.0),
               (0.1, 0.1, 0.3, 0.1, 0.1, 2.5), (0.6, 0, 0, 0, 0, 3.1))
GRID_OFFSET = (0.07, -0.06, 0.03, 0.0, 0.0, 0.0)


def plane_fold(k=40.0, x0=1.0):
    """The open field logit = k (x - x0): occupied beyond the plane x = x0."""
    a = torch.zeros(64, dtype=torch.float64)
    a[0], a[63] = k, -k * x0
    return a


def rays_f64(dirs_sensor, T, near=RR.NEAR, lo=RR.PARENT_LO, hi=RR.PARENT_HI):
    """registration_ref.rays_f64 with far never below near (nof.registration.scan_rays)."""
    rays = RR.rays_f64(dirs_sensor, T, near, lo, hi)
    rays[:, 7] = torch.clamp(rays[:, 7], min=near)
    return rays


def dirs_of(points32):
    """Unit directions (float64) and float32 ranges of float32 sensor-frame points, as the kernel forms them."""
    p = points32.double()
    rng = p.norm(dim=-1)
    return p / rng[:, None], rng.float()


def render_poses(fold_c, fold_f, dirs, poses, n_samples, n_importance, dtype=torch.float64, **box):
    """(depth (P, R), sumw (P, R)) of the two-pass render per pose; dtype float32: the same restatement on
    rays.float()."""
    depth, sumw = [], []
    for T in poses:
        rays = rays_f64(dirs, T, **box).to(dtype)
        d, s, _ = RR.render_two_pass(fold_c, fold_f, rays, n_samples, n_importance, want_jac=False)
        depth.append(d)
        sumw.append(s)
    return torch.stack(depth), torch.stack(sumw)


def reduce_scores(depth, sumw, target, huber_delta, min_sumw):
    """-> (out (P, 4), mag (P, 4)) numpy float64 from per-beam depth / sumw (P, R) and the targets (R,): cost, n_valid,
    sum |r| over the valid beams and sum sumw over the usable ones; mag the sums of the terms' absolute values."""
    depth, sumw = np.asarray(depth, np.float64), np.asarray(sumw, np.float64)
    t32 = np.asarray(target, np.float32)
    target = t32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        usable = np.isfinite(t32) & (t32 > 0)
        valid = usable[None, :] & (sumw >= min_sumw) & np.isfinite(depth)
        r = np.where(valid, depth - target[None, :], 0.0)
    ar = np.abs(r)
    lin = (huber_delta > 0) & (ar > huber_delta)
    rho = np.where(lin, huber_delta * (ar - 0.5 * huber_delta), 0.5 * r * r)
    hit = np.where(usable[None, :], sumw, 0.0)
    out = np.stack([rho.sum(1), valid.sum(1).astype(np.float64), ar.sum(1), hit.sum(1)], 1)
    mag = np.stack([rho.sum(1), valid.sum(1).astype(np.float64), ar.sum(1), np.abs(hit).sum(1)], 1)
    return out, mag


def mean_cost(out4, n_usable, miss_cost):
    """nof.localization's hypothesis score from the reduced rows."""
    return (out4[:, 0] + miss_cost * (n_usable - out4[:, 1])) / n_usable


@functools.lru_cache(maxsize=None)
def grid_scene():
    """The localisation tests' scene, computed once per process: the analytic cavity, 256 directions (seed 0), targets
    from the float64 render at T* = se3_exp(XI_STAR), and the 125 hypotheses of
    pose_grid(se3_exp(GRID_OFFSET) @ T*, 0.4, 0.2, 10 deg, 5 deg) with their float64 scores (64 + 128 samples)."""
    from nof.localization import default_miss_cost, pose_grid
    from nof.registration import se3_exp
    fold = RR.analytic_fold()
    T_star = se3_exp(RR.XI_STAR)
    dirs = RR.unit_directions(256, 0)
    ranges, _ = render_poses(fold, fold, dirs, [T_star], 64, 128)
    ranges = ranges[0]
    points = (dirs * ranges[:, None]).float()
    center = se3_exp(GRID_OFFSET) @ T_star
    poses = pose_grid(center, 0.4, 0.2, math.radians(10.0), math.radians(5.0))
    d64, s64 = render_poses(fold, fold, dirs_of(points)[0], poses, 64, 128)
    out, _ = reduce_scores(d64.numpy(), s64.numpy(), dirs_of(points)[1].numpy(), 0.0, 0.5)
    miss = default_miss_cost(RR.PARENT_LO, RR.PARENT_HI, 0.0)
    return {"fold": fold, "T_star": T_star, "dirs": dirs, "ranges": ranges, "points": points, "center": center,
            "poses": poses, "out": out, "scores": mean_cost(out, 256, miss), "miss_cost": miss}
