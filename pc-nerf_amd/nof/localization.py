"""Pose-hypothesis scoring and global localisation of a LiDAR scan against a trained (frozen, eval-mode) parent block.

``nof.registration.register_scan`` is a local solver: damped Gauss-Newton on range residuals needs a start inside its
basin.  This module produces that start.  ``score_poses`` renders the scan under every one of P candidate poses --
the rays of ``scan_rays``, the two passes of ``render_scan`` (coarse pass, deterministic resampling, fine pass) and the
cost sum of ``pcnerf::gn_normal_eq`` -- in ONE kernel launch plus a small fixed-order reduction
(``torch.ops.pcnerf.score_poses_fold``): one wave per (pose, beam), nothing per sample through memory, four float64 sums
per pose.  That is the observation model of Monte-Carlo localisation (IR-MCL), of relocalisation after tracking loss
and of a sanity check of odometry priors.  ``localize_scan`` scores a set of hypotheses (``pose_grid`` builds a regular
one), refines the best few with ``register_scan_fold`` and returns the best basin.  No process-wide selector is read or
written.

Per (pose, beam): r = depth - |p|; the beam is *usable* when |p| is finite and > 0 and *valid* when usable, the fine
pass's hit probability sumw >= ``min_sumw`` and the depth is finite; rho(r) = r^2 / 2, or
``huber_delta`` (|r| - ``huber_delta`` / 2) beyond ``huber_delta`` > 0 (pcnerf_gn_normal_eq's cost term).  A beam with
|p| == 0 or a non-finite point is simply not counted.  3 <= N_samples, 1 <= N_importance,
N_samples + N_importance <= 1024.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _torch_ops
from .registration import (EPSILON, RegistrationResult, _block_ids, _check_frozen, refine_poses_fold,
                           refine_poses_map, register_scan_fold, se3_exp)

P = torch.ops.pcnerf


class PoseScores(NamedTuple):
    cost: torch.Tensor            # (P,) float64: sum over the valid beams of rho(r)
    n_valid: torch.Tensor         # (P,) int64
    abs_residual: torch.Tensor    # (P,) float64: sum over the valid beams of |r|
    hit: torch.Tensor             # (P,) float64: sum over the usable beams of sumw
    depth: Optional[torch.Tensor]   # (P, R) float32 or None
    sumw: Optional[torch.Tensor]    # (P, R) float32 or None


class LocalizationResult(NamedTuple):
    pose: torch.Tensor      # (4, 4) float64, host: the refined candidate with the lowest final mean cost
    score: float            # its final mean cost
    index: int              # the hypothesis it was refined from
    scores: torch.Tensor    # (P,) float64, device: every hypothesis' mean cost
    refined: list           # RegistrationResult of the top_k hypotheses, best hypothesis score first


def pose_grid(center_pose, xy_half_extent: float, xy_step: float, yaw_half_extent: float, yaw_step: float,
              z_offsets=(0.0,)) -> torch.Tensor:
    """(P, 4, 4) float64 hypotheses ``se3_exp((dx, dy, dz, 0, 0, yaw)) @ center_pose`` (left perturbations, world
    frame; yaw in radians about the world z axis): dx, dy in {-n, ..., n} * xy_step with n = floor(xy_half_extent /
    xy_step), yaw likewise, dz over ``z_offsets``.  x varies slowest, then y, then z, yaw fastest.  The offsets are
    symmetric around zero, so the centre itself is a hypothesis whenever ``z_offsets`` contains 0."""
    def ticks(half, step):
        if step <= 0 or half < 0:
            raise ValueError("pose_grid: steps must be > 0 and half extents >= 0")
        n = int(math.floor(half / step + 1e-9))
        return [k * step for k in range(-n, n + 1)]

    C = torch.as_tensor(center_pose, dtype=torch.float64).detach().cpu()
    if tuple(C.shape) != (4, 4):
        raise ValueError(f"pose_grid: center_pose must be (4, 4); got {tuple(C.shape)}")
    xs, yaws = ticks(xy_half_extent, xy_step), ticks(yaw_half_extent, yaw_step)
    out = [se3_exp((dx, dy, float(dz), 0.0, 0.0, yaw)) @ C
           for dx in xs for dy in xs for dz in z_offsets for yaw in yaws]
    return torch.stack(out)


def _poses12(poses, device) -> torch.Tensor:
    T = torch.as_tensor(poses, dtype=torch.float64).detach()
    if T.dim() != 3 or tuple(T.shape[1:]) != (4, 4):
        raise RuntimeError(f"poses must be (P, 4, 4); got {tuple(T.shape)}")
    rows = torch.cat([T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], -1)   # copies only: the same bits from either side
    return rows.to(device).contiguous()


def score_poses_fold(fold_c: torch.Tensor, fold_f: torch.Tensor, points_sensor: torch.Tensor, poses, parent_lo,
                     parent_hi, *, N_samples: int = 64, N_importance: int = 128, huber_delta: float = 0.0,
                     min_sumw: float = 0.5, near: float = 0.05, want_depth: bool = False) -> PoseScores:
    """Score the scan ``points_sensor`` (R, 3, sensor frame, on the device) under ``poses`` (P, 4, 4 float64, sensor ->
    world, host or device) against the two folded networks (pcnerf::fold_eval's 64 doubles each) of the parent block
    [parent_lo, parent_hi].  ``want_depth`` also returns the (P, R) fine depths and hit probabilities; it does not
    change a bit of the scores.  Each pose's sums depend on (P, R) alone in their order, so a pose scores the same
    bits alone or in a batch."""
    if not points_sensor.is_cuda:
        raise RuntimeError("nof.localization renders device-resident scans; move points_sensor with .to('cuda') -- "
                           "there is no CPU path")
    if points_sensor.dim() != 2 or points_sensor.shape[1] != 3:
        raise RuntimeError(f"points_sensor must be (R, 3); got {tuple(points_sensor.shape)}")
    _torch_ops.check_score_samples("score_poses_fold", int(N_samples), int(N_importance))
    dev = points_sensor.device
    box = torch.as_tensor(np.concatenate([np.asarray(parent_lo, dtype=np.float64).reshape(3),
                                          np.asarray(parent_hi, dtype=np.float64).reshape(3)])).to(dev)
    pts = points_sensor.detach().float().contiguous()
    s4, depth, sumw = P.score_poses_fold(pts, _poses12(poses, dev), box, fold_c, fold_f, float(near), int(N_samples),
                                         int(N_importance), EPSILON, float(huber_delta), float(min_sumw),
                                         bool(want_depth))
    cost, n_valid, abs_r, hit = s4.t().contiguous()
    return PoseScores(cost, n_valid.round().to(torch.int64), abs_r, hit, depth if want_depth else None,
                      sumw if want_depth else None)


def _folds(model_coarse, model_fine):
    _check_frozen(model_coarse, "model_coarse")
    _check_frozen(model_fine, "model_fine")
    with torch.no_grad():
        return (P.fold_eval(_torch_ops.eval_params(model_coarse)), P.fold_eval(_torch_ops.eval_params(model_fine)))


def score_poses(model_coarse, model_fine, points_sensor: torch.Tensor, poses, parent_lo, parent_hi,
                **kw) -> PoseScores:
    """score_poses_fold on the frozen eval-mode networks: their folds are composed once.  A train-mode module and
    parameters that require grad raise."""
    fold_c, fold_f = _folds(model_coarse, model_fine)
    return score_poses_fold(fold_c, fold_f, points_sensor, poses, parent_lo, parent_hi, **kw)


def rho(r: float, huber_delta: float) -> float:
    """pcnerf_gn_normal_eq's cost term of one residual."""
    a = abs(float(r))
    if huber_delta > 0.0 and a > huber_delta:
        return huber_delta * (a - 0.5 * huber_delta)
    return 0.5 * a * a


def default_miss_cost(parent_lo, parent_hi, huber_delta: float = 0.0) -> float:
    """rho(D), D = |parent_hi - parent_lo| the box diagonal: a measured range and a rendered depth of a hit both lie
    inside the box, so no valid beam of any hypothesis can be charged more; a usable beam that misses (sumw <
    min_sumw) is charged exactly that, and a hypothesis cannot win by seeing less of the scene."""
    D = float(np.linalg.norm(np.asarray(parent_hi, dtype=np.float64) - np.asarray(parent_lo, dtype=np.float64)))
    return rho(D, float(huber_delta))


def pose_distance(A, B):
    """(translation distance, rotation angle) between two (4, 4) poses, host float64."""
    A, B = (torch.as_tensor(v, dtype=torch.float64).detach().cpu() for v in (A, B))
    dR = A[:3, :3] @ B[:3, :3].T
    v = torch.stack([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    ang = math.atan2(0.5 * float(torch.linalg.norm(v)), 0.5 * (float(torch.trace(dR)) - 1.0))
    return float(torch.linalg.norm(A[:3, 3] - B[:3, 3])), ang


def localize_scan_fold(fold_c: torch.Tensor, fold_f: torch.Tensor, points_sensor: torch.Tensor, poses, parent_lo,
                       parent_hi, *, top_k: int = 4, miss_cost: Optional[float] = None, refine_iters: int = 20,
                       same_basin_tol=(1e-3, 1e-3), N_samples: int = 64, N_importance: int = 128,
                       huber_delta: float = 0.0, min_sumw: float = 0.5, near: float = 0.05,
                       refine: str = "sequential") -> LocalizationResult:
    """localize_scan on the two folded networks.

    Every hypothesis p gets the mean cost ``score_p = (cost_p + miss_cost (n_usable - n_valid_p)) / n_usable`` over the
    n_usable beams with a finite range > 0; ``miss_cost`` defaults to ``default_miss_cost`` (rho of the box diagonal).
    The ``top_k`` lowest (ties: the lower index) are refined with ``register_scan_fold`` (``refine_iters``
    evaluations each, the same sampling, loss and validity settings), best hypothesis first; the winner is the refined
    candidate whose last accepted evaluation has the lowest mean cost by the same formula.

    Neighbouring hypotheses usually fall into the same basin, where their final costs differ only by how far the
    linearly convergent iteration got.  So a candidate whose refined pose lies within ``same_basin_tol`` = (metres,
    radians) of an earlier (better-scored) candidate's found that candidate's basin again: it is returned in
    ``refined`` but does not compete, and the basin is credited to the better hypothesis.  The default, 1 mm and
    1 mrad, is far above what 20 evaluations leave of a start inside the basin (some 1e-5) and far below the spacing
    of any useful hypothesis set.

    ``refine``: "sequential" refines the candidates one after the other with ``register_scan_fold`` (a host round trip
    per evaluation); "batched" refines them in one ``refine_poses_fold`` call (no host synchronisation between
    evaluations) and applies the same winner rule.  There a candidate left with fewer than 6 valid beams or a singular
    solve (status 2 or 3) does not compete instead of raising; if none is left, RuntimeError."""
    if refine not in ("sequential", "batched"):
        raise ValueError(f"localize_scan: refine must be 'sequential' or 'batched'; got {refine!r}")
    kw = dict(N_samples=N_samples, N_importance=N_importance, huber_delta=huber_delta, min_sumw=min_sumw, near=near)
    T = torch.as_tensor(poses, dtype=torch.float64).detach()
    s = score_poses_fold(fold_c, fold_f, points_sensor, T, parent_lo, parent_hi, **kw)
    if s.cost.shape[0] == 0:
        raise RuntimeError("localize_scan: no hypotheses")
    rng = torch.linalg.norm(points_sensor.detach().double(), dim=-1).float()
    n_usable = int((torch.isfinite(rng) & (rng > 0)).sum())
    if n_usable == 0:
        raise RuntimeError("localize_scan: the scan has no beam with a finite range > 0")
    mc = default_miss_cost(parent_lo, parent_hi, huber_delta) if miss_cost is None else float(miss_cost)
    scores = (s.cost + mc * (n_usable - s.n_valid).double()) / n_usable
    order = np.argsort(scores.cpu().numpy(), kind="stable")[:max(1, int(top_k))]
    T_host = T.cpu()
    refined, best = [], None
    if refine == "batched":
        return _localize_batched(fold_c, fold_f, points_sensor, T_host, order, parent_lo, parent_hi, int(refine_iters),
                                 same_basin_tol, mc, n_usable, scores, kw)
    for i in order:
        res = register_scan_fold(fold_c, fold_f, points_sensor, T_host[int(i)], parent_lo, parent_hi,
                                 iters=int(refine_iters), **kw)
        again = any(dt <= same_basin_tol[0] and dr <= same_basin_tol[1]
                    for dt, dr in (pose_distance(res.pose, r.pose) for r in refined))
        refined.append(res)
        final = (res.costs[-1] + mc * (n_usable - res.n_valid)) / n_usable
        if best is None or (not again and final < best[0]):
            best = (final, int(i), res)
    return LocalizationResult(best[2].pose, float(best[0]), best[1], scores, refined)


def _localize_batched(fold_c, fold_f, points_sensor, T_host, order, parent_lo, parent_hi, refine_iters,
                      same_basin_tol, mc, n_usable, scores, kw) -> LocalizationResult:
    """The refinement stage of localize_scan_fold with all candidates in one refine_poses_fold call; one read-back at
    the end, then the sequential path's winner rule on the host."""
    idx = torch.as_tensor(np.asarray(order, dtype=np.int64))
    r = refine_poses_fold(fold_c, fold_f, points_sensor, T_host[idx], parent_lo, parent_hi, iters=refine_iters, **kw)
    best, refined = _winner_of_refined(r, order, same_basin_tol, mc, n_usable)
    return LocalizationResult(best[2].pose, float(best[0]), best[1], scores, refined)


def _winner_of_refined(r, order, same_basin_tol, mc, n_usable):
    """The sequential path's winner rule on a RefineResult of the candidates ``order`` (one read-back) ->
    ((final mean cost, hypothesis index, RegistrationResult), refined list)."""
    poses, status = r.poses.cpu(), r.status.cpu().tolist()
    n_valid, iterations = r.n_valid.cpu().tolist(), r.iterations.cpu().tolist()
    eval_costs, mask = r.eval_costs.cpu(), r.accepted_mask.cpu()
    refined, best = [], None
    for k, i in enumerate(order):
        costs = eval_costs[k][mask[k]].tolist()
        res = RegistrationResult(poses[k], costs, int(n_valid[k]), int(iterations[k]), status[k] == 1)
        again = any(dt <= same_basin_tol[0] and dr <= same_basin_tol[1]
                    for dt, dr in (pose_distance(res.pose, q.pose) for q in refined))
        refined.append(res)
        if status[k] in (2, 3) or not costs:
            continue
        final = (costs[-1] + mc * (n_usable - res.n_valid)) / n_usable
        if best is None or (not again and final < best[0]):
            best = (final, int(i), res)
    if best is None:
        raise RuntimeError("localize_scan: no candidate is left after the refinement (fewer than 6 valid beams or a "
                           "singular solve for each)")
    return best, refined


def localize_scan(model_coarse, model_fine, points_sensor: torch.Tensor, poses, parent_lo, parent_hi, *,
                  top_k: int = 4, miss_cost: Optional[float] = None, refine_iters: int = 20,
                  **render_kw) -> LocalizationResult:
    """The pose of the scan ``points_sensor`` (R, 3, sensor frame, on the device) among the hypotheses ``poses``
    (P, 4, 4, sensor -> world) against the frozen eval-mode networks of a parent block: score all, refine the
    ``top_k`` best, return the best basin (localize_scan_fold).  ``render_kw``: N_samples, N_importance, huber_delta,
    min_sumw, near, and refine ("sequential", the default, or "batched": localize_scan_fold)."""
    fold_c, fold_f = _folds(model_coarse, model_fine)
    return localize_scan_fold(fold_c, fold_f, points_sensor, poses, parent_lo, parent_hi, top_k=top_k,
                              miss_cost=miss_cost, refine_iters=refine_iters, **render_kw)


# ----------------------------------------------------------------------------------------------- maps of blocks
# A PC-NeRF map is several parent blocks, each with its own pair of networks and its own AABB.  Every pose is rendered
# against exactly one block -- its own -- and a beam is clipped where it leaves that block's box: nothing is composited
# across blocks unless asked: ``score_poses_through`` (below) carries a beam on into the blocks it enters.  A block's
# AABB encloses the scans it was built from, so the sensor's own block sees the scene.
class BlockMap:
    """B >= 1 parent blocks on the device: ``folds_c`` / ``folds_f`` (B, 64) float64 (row b = pcnerf::fold_eval's
    output of block b's coarse / fine network) and ``boxes`` (B, 6) float64 rows [lo, hi].  Boxes may overlap."""

    def __init__(self, folds_c: torch.Tensor, folds_f: torch.Tensor, boxes: torch.Tensor):
        fc, ff, bx = (torch.as_tensor(t).detach() for t in (folds_c, folds_f, boxes))
        if not (fc.is_cuda and ff.is_cuda and bx.is_cuda):
            raise RuntimeError("BlockMap holds device tensors; move the folds and boxes with .to('cuda') -- there is "
                               "no CPU path")
        if fc.dim() != 2 or fc.shape[0] < 1 or fc.shape[1] != 64 or tuple(ff.shape) != tuple(fc.shape):
            raise RuntimeError(f"BlockMap: folds must be (B, 64) with B >= 1; got {tuple(fc.shape)} and "
                               f"{tuple(ff.shape)}")
        if tuple(bx.shape) != (fc.shape[0], 6):
            raise RuntimeError(f"BlockMap: boxes must be (B, 6) with B = {fc.shape[0]}; got {tuple(bx.shape)}")
        self.folds_c = fc.to(torch.float64).contiguous()
        self.folds_f = ff.to(torch.float64).contiguous()
        self.boxes = bx.to(torch.float64).contiguous()
        self._boxes_host = self.boxes.cpu().numpy()   # (one copy at construction: default_miss_cost reads it)

    @property
    def n_blocks(self) -> int:
        return int(self.boxes.shape[0])

    @property
    def device(self):
        return self.boxes.device

    @classmethod
    def from_models(cls, blocks) -> "BlockMap":
        """From [(model_coarse, model_fine, lo, hi), ...]: the frozen eval-mode networks of every block are folded once
        (a train-mode module and parameters that require grad raise, as in score_poses)."""
        blocks = list(blocks)
        if not blocks:
            raise RuntimeError("BlockMap.from_models: no blocks")
        fcs, ffs, boxes = [], [], []
        for mc, mf, lo, hi in blocks:
            fc, ff = _folds(mc, mf)
            fcs.append(fc)
            ffs.append(ff)
            boxes.append(np.concatenate([np.asarray(lo, dtype=np.float64).reshape(3),
                                         np.asarray(hi, dtype=np.float64).reshape(3)]))
        dev = fcs[0].device
        return cls(torch.stack(fcs), torch.stack(ffs), torch.as_tensor(np.stack(boxes)).to(dev))

    def default_miss_cost(self, huber_delta: float = 0.0) -> float:
        """The largest ``default_miss_cost`` over the blocks: no block's valid beam can be charged more than a miss."""
        return max(default_miss_cost(b[:3], b[3:], huber_delta) for b in self._boxes_host)


class MapLocalizationResult(NamedTuple):
    pose: torch.Tensor      # (4, 4) float64, host: the refined candidate with the lowest final mean cost
    score: float            # its final mean cost
    index: int              # the hypothesis it was refined from
    scores: torch.Tensor    # (P,) float64, device: every hypothesis' mean cost
    refined: list           # RegistrationResult of the top_k hypotheses, best hypothesis score first
    block: int              # the winner's block
    blocks: torch.Tensor    # (P,) int32, device: every hypothesis' block (-1: none)


def assign_blocks(block_map: BlockMap, poses, margin: float = 0.0) -> torch.Tensor:
    """(P,) int32 on the device: per pose (P, 4, 4, host or device) the block whose box contains its translation with
    ``margin`` to spare on every side -- among several the one with the largest clearance
    min_m min(t_m - lo_m, hi_m - t_m), the lowest index on ties -- or -1 when none does or the translation has a
    NaN (``torch.ops.pcnerf.assign_blocks``, float64)."""
    return P.assign_blocks(_poses12(poses, block_map.device), block_map.boxes, float(margin))


def _scan_points(points_sensor: torch.Tensor) -> torch.Tensor:
    if not points_sensor.is_cuda:
        raise RuntimeError("nof.localization renders device-resident scans; move points_sensor with .to('cuda') -- "
                           "there is no CPU path")
    if points_sensor.dim() != 2 or points_sensor.shape[1] != 3:
        raise RuntimeError(f"points_sensor must be (R, 3); got {tuple(points_sensor.shape)}")
    return points_sensor.detach().float().contiguous()


def score_poses_map(block_map: BlockMap, points_sensor: torch.Tensor, poses, blocks=None, *, N_samples: int = 64,
                    N_importance: int = 128, huber_delta: float = 0.0, min_sumw: float = 0.5, near: float = 0.05,
                    want_depth: bool = False) -> PoseScores:
    """score_poses_fold against a map of blocks: pose p is rendered against block ``blocks[p]`` ((P,) integers, -1 for
    none; None: ``assign_blocks``), the whole set in one launch (``torch.ops.pcnerf.score_poses_map``).  Every pose
    scores the bits score_poses_fold gives with its block alone.  A pose without a block (-1, or an index outside the
    map) renders nothing: zero sums, and NaN depth and zero sumw with ``want_depth``."""
    pts = _scan_points(points_sensor)
    _torch_ops.check_score_samples("score_poses_map", int(N_samples), int(N_importance))
    rows = _poses12(poses, pts.device)
    ids = _block_ids(block_map, rows, blocks)
    s4, depth, sumw = P.score_poses_map(pts, rows, ids, block_map.boxes, block_map.folds_c, block_map.folds_f,
                                        float(near), int(N_samples), int(N_importance), EPSILON, float(huber_delta),
                                        float(min_sumw), bool(want_depth))
    cost, n_valid, abs_r, hit = s4.t().contiguous()
    return PoseScores(cost, n_valid.round().to(torch.int64), abs_r, hit, depth if want_depth else None,
                      sumw if want_depth else None)


def localize_scan_map(block_map: BlockMap, points_sensor: torch.Tensor, poses, *, top_k: int = 4,
                      miss_cost: Optional[float] = None, refine_iters: int = 20, same_basin_tol=(1e-3, 1e-3),
                      N_samples: int = 64, N_importance: int = 128, huber_delta: float = 0.0, min_sumw: float = 0.5,
                      near: float = 0.05, blocks=None) -> MapLocalizationResult:
    """localize_scan_fold over a map of blocks: every hypothesis is scored against its own block (``blocks``, or
    ``assign_blocks`` at margin 0) in one launch, the ``top_k`` lowest mean costs are refined in one
    ``refine_poses_map`` call against the blocks they were scored in, and localize_scan_fold's batched winner rule picks the basin.  A
    hypothesis without a block is charged ``miss_cost`` for every usable beam; ``miss_cost`` defaults to the map's
    ``default_miss_cost`` (the largest over the blocks).  Returns the winner's block as well."""
    kw = dict(N_samples=N_samples, N_importance=N_importance, huber_delta=huber_delta, min_sumw=min_sumw, near=near)
    T = torch.as_tensor(poses, dtype=torch.float64).detach()
    pts = _scan_points(points_sensor)
    ids = _block_ids(block_map, _poses12(T, pts.device), blocks)
    s = score_poses_map(block_map, pts, T, ids, **kw)
    if s.cost.shape[0] == 0:
        raise RuntimeError("localize_scan: no hypotheses")
    rng = torch.linalg.norm(points_sensor.detach().double(), dim=-1).float()
    n_usable = int((torch.isfinite(rng) & (rng > 0)).sum())
    if n_usable == 0:
        raise RuntimeError("localize_scan: the scan has no beam with a finite range > 0")
    mc = block_map.default_miss_cost(huber_delta) if miss_cost is None else float(miss_cost)
    scores = (s.cost + mc * (n_usable - s.n_valid).double()) / n_usable
    order = np.argsort(scores.cpu().numpy(), kind="stable")[:max(1, int(top_k))]
    idx = torch.as_tensor(np.asarray(order, dtype=np.int64))
    ids_host = ids.cpu()
    r = refine_poses_map(block_map, pts, T.cpu()[idx], ids_host[idx], iters=int(refine_iters), **kw)
    best, refined = _winner_of_refined(r, order, same_basin_tol, mc, n_usable)
    return MapLocalizationResult(best[2].pose, float(best[0]), best[1], scores, refined, int(ids_host[best[1]]), ids)


# ----------------------------------------------------------------------------------------------- through the blocks
# The one exception to "every pose is rendered against one block": a beam that leaves its block's box goes on into the
# block it enters, and the segments are composited (torch.ops.pcnerf.score_poses_through).  Scoring and scan synthesis
# only: the refinement stays clipped, so localize_scan_map scores and refines under one model.
class ThroughScores(NamedTuple):
    cost: torch.Tensor            # (P,) float64: sum over the valid beams of rho(r)
    n_valid: torch.Tensor         # (P,) int64
    abs_residual: torch.Tensor    # (P,) float64: sum over the valid beams of |r|
    hit: torch.Tensor             # (P,) float64: sum over the usable beams of sumw
    depth: Optional[torch.Tensor]   # (P, R) float32 or None
    sumw: Optional[torch.Tensor]    # (P, R) float32 or None
    n_segments: Optional[torch.Tensor]   # (P, R) int32 or None: the segments rendered (0: the pose has no block)
    last_block: Optional[torch.Tensor]   # (P, R) int32 or None: the block of the last segment (-1: none)


class SynthesizedScan(NamedTuple):
    points_sensor: torch.Tensor   # (R, 3) float32: unit direction x depth
    depth: torch.Tensor           # (R,) float32
    hit: torch.Tensor             # (R,) float32: the chain's sumw
    n_segments: torch.Tensor      # (R,) int32
    last_block: torch.Tensor      # (R,) int32


def score_poses_through(block_map: BlockMap, points_sensor: torch.Tensor, poses, blocks=None, *,
                        max_segments: int = 4, seam_tol: float = 1e-3, min_transmittance: float = 1e-3,
                        N_samples: int = 64, N_importance: int = 128, huber_delta: float = 0.0, min_sumw: float = 0.5,
                        near: float = 0.05, want_depth: bool = False) -> ThroughScores:
    """score_poses_map with every beam carried through the blocks it crosses.  Segment 0 is score_poses_map's render in
    the pose's own block; where the beam leaves that box, the block it enters within ``seam_tol`` metres (among several
    the one it stays in longest) renders the next segment with its own networks and its own N_samples + N_importance
    samples, and so on for at most ``max_segments`` segments or until the transmittance in front of the next segment
    is at most ``min_transmittance``.  The segments are composited as one sample list; a beam that never leaves its
    block keeps score_poses_map's bits.  ``want_depth`` also returns the (P, R) depth, sumw, segment count and last
    block; it changes no bit of the scores."""
    pts = _scan_points(points_sensor)
    _torch_ops.check_score_samples("score_poses_through", int(N_samples), int(N_importance))
    _torch_ops.check_through_params("score_poses_through", int(max_segments), float(seam_tol),
                                    float(min_transmittance))
    rows = _poses12(poses, pts.device)
    ids = _block_ids(block_map, rows, blocks)
    s4, depth, sumw, nseg, last = P.score_poses_through(
        pts, rows, ids, block_map.boxes, block_map.folds_c, block_map.folds_f, float(near), int(N_samples),
        int(N_importance), EPSILON, float(huber_delta), float(min_sumw), int(max_segments), float(seam_tol),
        float(min_transmittance), bool(want_depth))
    cost, n_valid, abs_r, hit = s4.t().contiguous()
    beams = (depth, sumw, nseg, last) if want_depth else (None, None, None, None)
    return ThroughScores(cost, n_valid.round().to(torch.int64), abs_r, hit, *beams)


def synthesize_scan(block_map: BlockMap, directions_sensor: torch.Tensor, pose, blocks=None, *,
                    max_segments: int = 4, seam_tol: float = 1e-3, min_transmittance: float = 1e-3,
                    N_samples: int = 64, N_importance: int = 128, near: float = 0.05) -> SynthesizedScan:
    """The scan the map predicts from ``pose`` (4, 4) along ``directions_sensor`` (R, 3, sensor frame, on the device,
    any non-zero length): one call of ``torch.ops.pcnerf.score_poses_through`` whose scoring terms are not used.
    ``blocks``: the pose's block (one integer in a sequence; None: ``assign_blocks``)."""
    dirs = _scan_points(directions_sensor)
    T = torch.as_tensor(pose, dtype=torch.float64).detach()
    if tuple(T.shape) != (4, 4):
        raise RuntimeError(f"synthesize_scan: pose must be (4, 4); got {tuple(T.shape)}")
    s = score_poses_through(block_map, dirs, T[None], blocks, max_segments=max_segments, seam_tol=seam_tol,
                            min_transmittance=min_transmittance, N_samples=N_samples, N_importance=N_importance,
                            near=near, want_depth=True)
    d = dirs.double()
    unit = (d / torch.linalg.norm(d, dim=-1, keepdim=True)).float()
    depth = s.depth[0]
    return SynthesizedScan(unit * depth[:, None], depth, s.sumw[0], s.n_segments[0], s.last_block[0])
