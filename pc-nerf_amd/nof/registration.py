"""Scan-to-field registration: the pose of a LiDAR scan against a trained (frozen, eval-mode) parent block.

A pose ``T`` (4 x 4, sensor -> world, float64 on the host) is refined by damped Gauss-Newton on the range residuals
``depth_r(T) - |p_r|`` of the scan's points ``p_r`` (sensor frame).  Each iteration renders the scan's rays through
the two networks exactly as ``render_rays_val`` does at ``perturb = 0, noise_std = 0`` (render.py:485-536) -- coarse
pass, deterministic resampling, fine pass -- with both passes in one kernel launch each
(``torch.ops.pcnerf.render_jac_fold``: the folded eval network sigmoid(a . Embedding(x) + c), compositing and, for the
fine pass, the per-ray Jacobian d depth / d (o, d)), reduces the Jacobians to the 6 x 6 normal equations on the device
(``torch.ops.pcnerf.gn_normal_eq``) and reads 30 doubles back.  No process-wide selector is read or written.

Pose convention: left perturbation ``T' = se3_exp(xi) @ T`` with ``xi = (rho, phi)`` (translation first), so a world
ray (o, d) moves by ``delta o = rho + phi x o``, ``delta d = phi x d`` and its pose Jacobian is
``Jp = [J_o, o x J_o + d x J_d]`` (``pose_jacobian``).

What is NOT differentiated: the sample depths.  The coarse depths come from the rays' near / far bounds and the fine
depths from the coarse weights; both are constants of the Jacobian, as the reference detaches them (render.py:523).
The fine samples follow the surface from one iteration to the next, so the iteration converges, but linearly, not
quadratically.  At most 1024 samples per ray and pass (``N_samples + N_importance <= 1024``).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _autograd, _ops, _torch_ops

P = torch.ops.pcnerf
EPSILON = 1e-10   # render.py:514


class RegistrationResult(NamedTuple):
    pose: torch.Tensor      # (4, 4) float64, host
    costs: list             # the accepted evaluations' costs, in order (never increasing)
    n_valid: int            # valid rays of the last accepted evaluation
    iterations: int         # evaluations made
    converged: bool         # an accepted step fell below the step threshold


# ----------------------------------------------------------------------------------------------- SE(3), float64, host
def _hat(v):
    x, y, z = (float(c) for c in v)
    return torch.tensor([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]], dtype=torch.float64)


def _abc(theta: float):
    """sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3 without cancellation."""
    if theta < 1e-8:
        a = 1.0
    else:
        a = math.sin(theta) / theta
    h = 0.5 * theta
    sh = 1.0 if h < 1e-8 else math.sin(h) / h
    b = 0.5 * sh * sh
    if theta < 0.5:
        t2 = theta * theta
        c, term = 0.0, 1.0 / 6.0
        for k in range(1, 9):   # 1/3! - t^2/5! + t^4/7! - ...
            c += term
            term *= -t2 / ((2 * k + 2) * (2 * k + 3))
    else:
        c = (theta - math.sin(theta)) / theta ** 3
    return a, b, c


def se3_exp(xi) -> torch.Tensor:
    """exp of the twist xi = (rho, phi) (translation part first) -> (4, 4) float64."""
    xi = torch.as_tensor(xi, dtype=torch.float64).detach().cpu().reshape(6)
    rho, phi = xi[:3], xi[3:]
    theta = float(torch.linalg.norm(phi))
    a, b, c = _abc(theta)
    K = _hat(phi)
    K2 = K @ K
    eye = torch.eye(3, dtype=torch.float64)
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = eye + a * K + b * K2
    T[:3, 3] = (eye + b * K + c * K2) @ rho
    return T


def se3_log(T) -> torch.Tensor:
    """The twist (rho, phi) with se3_exp(.) = T, |phi| <= pi -> (6,) float64."""
    T = torch.as_tensor(T, dtype=torch.float64).detach().cpu()
    R, t = T[:3, :3], T[:3, 3]
    v = 0.5 * torch.stack([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])   # sin(theta) axis
    s, c = float(torch.linalg.norm(v)), 0.5 * (float(torch.trace(R)) - 1.0)
    theta = math.atan2(s, c)
    if theta < 1e-8:
        phi = v.clone()
    elif math.pi - theta > 1e-3:
        phi = v * (theta / s)
    else:   # near pi: the axis from the largest column of R + I, its sign from v
        M = R + torch.eye(3, dtype=torch.float64)
        j = int(torch.argmax(torch.diagonal(M)))
        axis = M[:, j] / torch.linalg.norm(M[:, j])
        if float(axis @ v) < 0:
            axis = -axis
        phi = axis * theta
    _, b, cc = _abc(theta)
    K = _hat(phi)
    V = torch.eye(3, dtype=torch.float64) + b * K + cc * (K @ K)
    rho = torch.linalg.solve(V, t)
    return torch.cat([rho, phi])


def pose_jacobian(rays6: torch.Tensor, jac6: torch.Tensor) -> torch.Tensor:
    """(R, 6) d depth / d xi at xi = 0 of T' = se3_exp(xi) T from the world-frame rows rays6 = [o, d] and the per-ray
    Jacobian jac6 = [J_o, J_d]: [J_o, o x J_o + d x J_d] (pcnerf_gn_normal_eq's Jp, in the inputs' dtype)."""
    o, d = rays6[:, 0:3], rays6[:, 3:6]
    Jo, Jd = jac6[:, 0:3], jac6[:, 3:6]
    return torch.cat([Jo, torch.linalg.cross(o, Jo, dim=-1) + torch.linalg.cross(d, Jd, dim=-1)], -1)


# ----------------------------------------------------------------------------------------------- rays of a scan
def scan_rays(points_sensor: torch.Tensor, pose, parent_lo, parent_hi, near: float = 0.05):
    """The scan's world-frame rays under ``pose`` -> (rays (R, 8) float32 [o, d, near, far], ranges (R,) float32).
    d is the unit direction to each point, far the ray's exit from the parent box [parent_lo, parent_hi] (the slab
    test of nof.synthetic._slab, an axis the ray runs parallel to inside its slab not limiting), never below near.
    Everything is float64 on the points' device until the final cast."""
    if points_sensor.dim() != 2 or points_sensor.shape[1] != 3:
        raise RuntimeError(f"points_sensor must be (R, 3); got {tuple(points_sensor.shape)}")
    dev = points_sensor.device
    T = torch.as_tensor(pose, dtype=torch.float64).detach().to(dev)
    lo = torch.as_tensor(np.asarray(parent_lo, dtype=np.float64)).to(dev)
    hi = torch.as_tensor(np.asarray(parent_hi, dtype=np.float64)).to(dev)
    p = points_sensor.detach().double()
    rng = torch.linalg.norm(p, dim=-1)
    d = (p / rng[:, None]) @ T[:3, :3].T
    d = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    o = T[:3, 3].expand_as(d)
    inv = 1.0 / d
    t1, t2 = (lo - o) * inv, (hi - o) * inv
    tmax = torch.where(torch.isnan(t2), torch.full_like(t2, math.inf), torch.maximum(t1, t2))
    far = torch.clamp(tmax.min(-1)[0], min=float(near))
    rays = torch.cat([o, d, torch.full_like(far, float(near))[:, None], far[:, None]], -1)
    return rays.float().contiguous(), rng.float().contiguous()


def render_scan(fold_c: torch.Tensor, fold_f: torch.Tensor, rays: torch.Tensor, N_samples: int = 64,
                N_importance: int = 128, want_jac: bool = True):
    """The two passes of render_rays_val (perturb = 0, noise_std = 0) on folded networks -> (depth_fine (R,), sumw (R,)
    the fine pass's hit probability, jac6 (R, 6) = d depth_fine / d rays[:, 0:6] or an empty tensor).  The fine sample
    depths are constants of the Jacobian (render.py:523)."""
    if N_samples + N_importance > _torch_ops.RENDER_JAC_MAX_SAMPLES:
        raise RuntimeError(f"render_scan: N_samples + N_importance = {N_samples + N_importance} exceeds the "
                           f"{_torch_ops.RENDER_JAC_MAX_SAMPLES} samples per ray the fused pass supports")
    z = P.sample_coarse(rays, int(N_samples), int(N_samples), 6, 7, 0, 0, False)
    _, _, w, _ = P.render_jac_fold(rays, z, fold_c, EPSILON, True, False)
    zf = P.resample(z, w, int(N_importance), None)
    depth, sumw, _, jac6 = P.render_jac_fold(rays, zf, fold_f, EPSILON, False, bool(want_jac))
    return depth, sumw, jac6


# ----------------------------------------------------------------------------------------------- the solver
def unpack_normal_eq(out30):
    """The 30 doubles of pcnerf::gn_normal_eq -> (H (6, 6), b (6,), cost, n_valid) in numpy float64."""
    v = np.asarray(out30, dtype=np.float64)
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = v[:21]
    H = H + np.triu(H, 1).T
    return H, v[21:27].copy(), float(v[27]), int(round(float(v[28])))


def lm_step(H, b, lam):
    """xi of (H + lam diag(H)) xi = -b in float64."""
    return np.linalg.solve(H + lam * np.diag(np.diag(H)), -b)


def register_scan_fold(fold_c: torch.Tensor, fold_f: torch.Tensor, points_sensor: torch.Tensor, init_pose,
                       parent_lo, parent_hi, *, N_samples: int = 64, N_importance: int = 128, iters: int = 20,
                       huber_delta: float = 0.0, min_sumw: float = 0.5, damping: float = 1e-6, near: float = 0.05,
                       xi_tol: float = 1e-9) -> RegistrationResult:
    """register_scan on the two folded networks (pcnerf::fold_eval's 64 doubles each).

    Iteration: rays of the scan at the current pose, the two render passes, the normal equations, one 30-double
    read-back, then on the host: the evaluation is accepted when its cost does not exceed the last accepted one
    (lambda / 10), else the pose goes back to the last accepted one (lambda x 10); xi = -(H + lambda diag H)^-1 b from
    the accepted evaluation, T <- se3_exp(xi) T.  Stops after ``iters`` evaluations or when |xi| < ``xi_tol`` (the
    pose returned includes that last step)."""
    if not points_sensor.is_cuda:
        raise RuntimeError("nof.registration renders device-resident scans; move points_sensor with .to('cuda') -- "
                           "there is no CPU path")
    T = torch.as_tensor(init_pose, dtype=torch.float64).detach().cpu().clone()
    lam = float(damping)
    acc = None            # (T, H, b, cost, n_valid) of the last accepted evaluation
    costs, done, converged = [], 0, False
    for _ in range(int(iters)):
        rays, ranges = scan_rays(points_sensor, T, parent_lo, parent_hi, near)
        depth, sumw, jac6 = render_scan(fold_c, fold_f, rays, N_samples, N_importance, True)
        out = P.gn_normal_eq(rays, jac6, depth, sumw, ranges, float(huber_delta), float(min_sumw))
        H, b, cost, n_valid = unpack_normal_eq(out.cpu().numpy())
        done += 1
        if n_valid < 6:
            raise RuntimeError(f"register_scan: {n_valid} valid rays (sumw >= {min_sumw}, finite depth): the pose "
                               "is not determined")
        if acc is None or cost <= acc[3]:
            if acc is not None:
                lam = lam / 10.0
            acc = (T, H, b, cost, n_valid)
            costs.append(cost)
        else:
            lam = lam * 10.0
        xi = lm_step(acc[1], acc[2], lam)
        T = se3_exp(xi) @ acc[0]
        if float(np.linalg.norm(xi)) < xi_tol:
            converged = True
            break
    return RegistrationResult(T, costs, acc[4] if acc else 0, done, converged)


def _check_frozen(model, name: str) -> None:
    if not model.supported():
        raise NotImplementedError("HIP render supports NOF(feature_size=256, in_channels_xy=63, use_skip=True)")
    _autograd.check_frozen_eval(model, "the pose")
    if any(t.requires_grad for t in model.parameters()):
        raise NotImplementedError(f"register_scan is forward-only in the networks: {name}'s parameters require grad; "
                                  "freeze them (requires_grad_(False))")
    _ops._bn_config(model)


def register_scan(model_coarse, model_fine, points_sensor: torch.Tensor, init_pose, parent_lo, parent_hi, *,
                  N_samples: int = 64, N_importance: int = 128, iters: int = 20, huber_delta: float = 0.0,
                  min_sumw: float = 0.5, damping: float = 1e-6, near: float = 0.05,
                  xi_tol: float = 1e-9) -> RegistrationResult:
    """Refine ``init_pose`` (4 x 4, sensor -> world) of the scan ``points_sensor`` (R, 3, sensor frame, on the
    device) against the frozen eval-mode networks of a parent block [parent_lo, parent_hi].  Their folds are composed
    once (pcnerf::fold_eval); see register_scan_fold for the iteration.  A train-mode module and parameters that
    require grad raise."""
    _check_frozen(model_coarse, "model_coarse")
    _check_frozen(model_fine, "model_fine")
    with torch.no_grad():
        fold_c = P.fold_eval(_torch_ops.eval_params(model_coarse))
        fold_f = P.fold_eval(_torch_ops.eval_params(model_fine))
    return register_scan_fold(fold_c, fold_f, points_sensor, init_pose, parent_lo, parent_hi, N_samples=N_samples,
                              N_importance=N_importance, iters=iters, huber_delta=huber_delta, min_sumw=min_sumw,
                              damping=damping, near=near, xi_tol=xi_tol)


# ----------------------------------------------------------------------------------------------- many poses at once
class RefineResult(NamedTuple):
    poses: torch.Tensor          # (P, 4, 4) float64, device: T_trial, or the last accepted pose where status is 2 / 3
    cost: torch.Tensor           # (P,) float64: the last accepted evaluation's cost (0 when none was accepted)
    n_valid: torch.Tensor        # (P,) int64: its valid beams
    iterations: torch.Tensor     # (P,) int64: evaluations made
    accepted: torch.Tensor       # (P,) int64: evaluations accepted
    status: torch.Tensor         # (P,) int64: 0 ran all iterations, 1 |xi| < xi_tol, 2 fewer than 6 valid beams,
    #                              3 the damped normal equations were singular
    eval_costs: torch.Tensor     # (P, iters) float64: every evaluation's cost, NaN where the pose had stopped
    accepted_mask: torch.Tensor  # (P, iters) bool
    lam: torch.Tensor            # (P,) float64: the final damping factor
    state: torch.Tensor          # (P, 64) float64: the solver's state rows (include/pcnerf_hip.h)


def _pose_rows(poses, device) -> torch.Tensor:
    """(P, 4, 4) poses, host or device -> (P, 12) float64 device rows [R row-major, t] (copies only: the same bits
    from either side)."""
    T = torch.as_tensor(poses, dtype=torch.float64).detach()
    if T.dim() != 3 or tuple(T.shape[1:]) != (4, 4):
        raise RuntimeError(f"poses must be (P, 4, 4); got {tuple(T.shape)}")
    return torch.cat([T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], -1).to(device).contiguous()


def _rows_to_poses(rows: torch.Tensor) -> torch.Tensor:
    """(P, 12) rows -> (P, 4, 4) on the rows' device (copies only)."""
    T = torch.zeros((rows.shape[0], 4, 4), dtype=torch.float64, device=rows.device)
    T[:, :3, :3] = rows[:, :9].reshape(-1, 3, 3)
    T[:, :3, 3] = rows[:, 9:12]
    T[:, 3, 3] = 1.0
    return T


def refine_poses_fold(fold_c: torch.Tensor, fold_f: torch.Tensor, points_sensor: torch.Tensor, poses, parent_lo,
                      parent_hi, *, N_samples: int = 64, N_importance: int = 128, iters: int = 20,
                      huber_delta: float = 0.0, min_sumw: float = 0.5, damping: float = 1e-6, near: float = 0.05,
                      xi_tol: float = 1e-9) -> RefineResult:
    """register_scan_fold's iteration for the P poses ``poses`` (P, 4, 4 float64, sensor -> world, host or device) of
    one scan at once, entirely on the device (``torch.ops.pcnerf.refine_poses_fold``): per evaluation one fused launch
    renders every running pose's scan with its Jacobian and forms the normal-equation terms, a small reduction adds
    them per pose, and a small kernel runs the accept / reject rule, the damped 6 x 6 solve and
    ``T <- se3_exp(xi) T`` per pose in float64.  Nothing is read back between evaluations; a pose that has stopped
    (converged, undetermined or singular: ``status``) costs nothing further.  Every pose follows register_scan_fold's
    branches, but where that raises for fewer than 6 valid beams this records status 2 and returns the start (or the
    last accepted pose).  A pose refines to the same bits alone or in a batch.  3 <= N_samples, 1 <= N_importance,
    N_samples + N_importance <= 1024."""
    if not points_sensor.is_cuda:
        raise RuntimeError("nof.registration renders device-resident scans; move points_sensor with .to('cuda') -- "
                           "there is no CPU path")
    if points_sensor.dim() != 2 or points_sensor.shape[1] != 3:
        raise RuntimeError(f"points_sensor must be (R, 3); got {tuple(points_sensor.shape)}")
    _torch_ops.check_score_samples("refine_poses_fold", int(N_samples), int(N_importance))
    dev = points_sensor.device
    box = torch.as_tensor(np.concatenate([np.asarray(parent_lo, dtype=np.float64).reshape(3),
                                          np.asarray(parent_hi, dtype=np.float64).reshape(3)])).to(dev)
    pts = points_sensor.detach().float().contiguous()
    rows, state, costs, acc = P.refine_poses_fold(pts, _pose_rows(poses, dev), box, fold_c, fold_f, float(near),
                                                  int(N_samples), int(N_importance), EPSILON, float(huber_delta),
                                                  float(min_sumw), float(damping), float(xi_tol), int(iters))
    as_int = lambda c: state[:, c].round().to(torch.int64)   # noqa: E731
    return RefineResult(_rows_to_poses(rows), state[:, 24 + 27].clone(), as_int(24 + 28), as_int(56), as_int(57),
                        as_int(55), costs, acc.bool(), state[:, 54].clone(), state)


def refine_poses(model_coarse, model_fine, points_sensor: torch.Tensor, poses, parent_lo, parent_hi,
                 **kw) -> RefineResult:
    """refine_poses_fold on the frozen eval-mode networks of a parent block: their folds are composed once
    (pcnerf::fold_eval).  A train-mode module and parameters that require grad raise, as in register_scan."""
    _check_frozen(model_coarse, "model_coarse")
    _check_frozen(model_fine, "model_fine")
    if not points_sensor.is_cuda:
        raise RuntimeError("nof.registration renders device-resident scans; move points_sensor with .to('cuda') -- "
                           "there is no CPU path")
    with torch.no_grad():
        fold_c = P.fold_eval(_torch_ops.eval_params(model_coarse))
        fold_f = P.fold_eval(_torch_ops.eval_params(model_fine))
    return refine_poses_fold(fold_c, fold_f, points_sensor, poses, parent_lo, parent_hi, **kw)


def apply_twists(poses: torch.Tensor, xi: torch.Tensor) -> torch.Tensor:
    """(P, 4, 4) float64 ``se3_exp(xi[p]) @ poses[p]`` on the device (``torch.ops.pcnerf.se3_apply``): the left
    perturbation of every pose by its own twist xi = (rho, phi), e.g. the motion-model update of a particle set.
    ``poses`` (P, 4, 4) and ``xi`` (P, 6) are device tensors."""
    if not (torch.is_tensor(poses) and poses.is_cuda and torch.is_tensor(xi) and xi.is_cuda):
        raise RuntimeError("nof.registration.apply_twists takes device tensors -- there is no CPU path")
    rows = _pose_rows(poses, poses.device)
    x = xi.detach().to(torch.float64).contiguous()
    if x.dim() != 2 or tuple(x.shape) != (rows.shape[0], 6):
        raise RuntimeError(f"xi must be (P, 6) with P = {rows.shape[0]}; got {tuple(x.shape)}")
    return _rows_to_poses(P.se3_apply(x, rows))


def _block_ids(block_map, rows: torch.Tensor, blocks) -> torch.Tensor:
    """(P,) int32 device block ids of the (P, 12) pose rows: the caller's, or pcnerf::assign_blocks' at margin 0 (for
    another margin, call assign_blocks and pass its result)."""
    if blocks is None:
        return P.assign_blocks(rows, block_map.boxes, 0.0)
    b = torch.as_tensor(blocks).detach().to(device=rows.device, dtype=torch.int32).contiguous()
    if tuple(b.shape) != (rows.shape[0],):
        raise RuntimeError(f"blocks must be (P,) with P = {rows.shape[0]}; got {tuple(b.shape)}")
    return b


def refine_poses_map(block_map, points_sensor: torch.Tensor, poses, blocks=None, *, N_samples: int = 64,
                     N_importance: int = 128, iters: int = 20, huber_delta: float = 0.0, min_sumw: float = 0.5,
                     damping: float = 1e-6, near: float = 0.05, xi_tol: float = 1e-9) -> RefineResult:
    """refine_poses_fold against a map of blocks (``nof.localization.BlockMap``): pose p is refined against block
    ``blocks[p]`` ((P,) integers, -1 for none; None: ``assign_blocks`` of the start poses), in one call for the whole
    set (``torch.ops.pcnerf.refine_poses_map``).  Every pose refines to the bits refine_poses_fold gives with its
    block alone.  The block of a pose is fixed for the call: a pose that leaves its box on the way behaves as in the
    single-block solver (its beams are clipped by the box it started in), and blocks are not re-assigned between
    evaluations.  A pose without a block stops with status 2 at the first update and returns its input."""
    if not points_sensor.is_cuda:
        raise RuntimeError("nof.registration renders device-resident scans; move points_sensor with .to('cuda') -- "
                           "there is no CPU path")
    if points_sensor.dim() != 2 or points_sensor.shape[1] != 3:
        raise RuntimeError(f"points_sensor must be (R, 3); got {tuple(points_sensor.shape)}")
    _torch_ops.check_score_samples("refine_poses_map", int(N_samples), int(N_importance))
    dev = points_sensor.device
    pts = points_sensor.detach().float().contiguous()
    rows_in = _pose_rows(poses, dev)
    ids = _block_ids(block_map, rows_in, blocks)
    rows, state, costs, acc = P.refine_poses_map(pts, rows_in, ids, block_map.boxes, block_map.folds_c,
                                                 block_map.folds_f, float(near), int(N_samples), int(N_importance),
                                                 EPSILON, float(huber_delta), float(min_sumw), float(damping),
                                                 float(xi_tol), int(iters))
    as_int = lambda c: state[:, c].round().to(torch.int64)   # noqa: E731
    return RefineResult(_rows_to_poses(rows), state[:, 24 + 27].clone(), as_int(24 + 28), as_int(56), as_int(57),
                        as_int(55), costs, acc.bool(), state[:, 54].clone(), state)
