"""Monte-Carlo localisation of a LiDAR against a map of PC-NeRF blocks: a particle filter whose state lives on the
device and whose step is a handful of enqueued launches with no host synchronisation.

``ParticleFilter.step`` is predict (every particle moves by the odometry twist plus Gaussian noise drawn on the
device, ``apply_twists``' kernel, then ``torch.ops.pcnerf.assign_blocks``), update (``torch.ops.pcnerf.score_poses_map``
renders the scan under every particle against the particle's own block -- or, with ``through=True``,
``torch.ops.pcnerf.score_poses_through`` carries its beams on through the blocks they cross;
``torch.ops.pcnerf.mcl_weights`` turns the
sums into normalised float64 weights, their effective sample size and the best particle) and resample
(``torch.ops.pcnerf.systematic_resample``: the decision ``ess >= ess_frac * P`` is taken on the device from the
weights' own output buffer, and the particles, their blocks and their log-weights are gathered there).  Nothing is read
back: the particle count is fixed, every scalar that steers a launch (the usable-beam count, the resampling offset, the
effective sample size) stays in device memory.

The observation model is ``localize_scan``'s mean cost: ``logw_p <- logw_p - beta (cost_p + miss_cost (n_usable -
n_valid_p)) / n_usable``; a particle outside every block carries no weight.  No process-wide selector is read or written.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _torch_ops
from .localization import BlockMap, _poses12
from .registration import EPSILON, _rows_to_poses

P = torch.ops.pcnerf


class MclEstimate(NamedTuple):
    pose: torch.Tensor          # (4, 4) float64, device: the weighted mean translation and the chordal mean rotation
    best_pose: torch.Tensor     # (4, 4) float64, device: the particle with the largest weight (lowest index on ties)
    best_index: torch.Tensor    # (1,) int32, device
    best_block: torch.Tensor    # (1,) int32, device: its block


def _six(v, name: str, scalar_ok: bool = False):
    """A twist or a sigma as six Python floats, or a (6,) device tensor as it is; with ``scalar_ok`` (sigma only) one
    number stands for all six.  Nothing here touches the device."""
    if torch.is_tensor(v) and v.is_cuda:
        if tuple(v.shape) != (6,):
            raise RuntimeError(f"{name} must be (6,); got {tuple(v.shape)}")
        return v.detach().to(torch.float64)
    if isinstance(v, (int, float)):
        if not scalar_ok:
            raise RuntimeError(f"{name} must have six components (rho, phi); got a scalar")
        return [float(v)] * 6
    vals = [float(x) for x in (v.tolist() if torch.is_tensor(v) else list(v))]
    if len(vals) != 6:
        raise RuntimeError(f"{name} must have six components (rho, phi); got {len(vals)}")
    return vals


class ParticleFilter:
    """P particles (poses, sensor -> world) over a ``BlockMap``.  ``poses`` (P, 4, 4) float64, host or device;
    the render settings are score_poses' (N_samples, N_importance, huber_delta, min_sumw, near); ``miss_cost``
    defaults to the map's ``default_miss_cost``; ``beta`` scales the mean cost into a log-likelihood.  ``through``:
    the update carries every beam through the blocks it crosses (``nof.localization.score_poses_through`` with
    ``max_segments``, ``seam_tol`` and ``min_transmittance``) instead of clipping it at the particle's own block.

    State (device): ``poses12`` (P, 12) float64 rows [R row-major, t], ``blocks`` (P,) int32, ``logw`` and ``w`` (P,)
    float64 (normalised), ``ess`` (1,) float64, ``best`` and ``degenerate`` (1,) int32, ``scores4`` (P, 4)."""

    def __init__(self, block_map: BlockMap, poses, *, beta: float = 1.0, miss_cost: Optional[float] = None,
                 margin: float = 0.0, N_samples: int = 64, N_importance: int = 128, huber_delta: float = 0.0,
                 min_sumw: float = 0.5, near: float = 0.05, through: bool = False, max_segments: int = 4,
                 seam_tol: float = 1e-3, min_transmittance: float = 1e-3):
        _torch_ops.check_score_samples("ParticleFilter", int(N_samples), int(N_importance))
        _torch_ops.check_through_params("ParticleFilter", int(max_segments), float(seam_tol),
                                        float(min_transmittance))
        self.through = bool(through)
        self.chain = dict(max_segments=int(max_segments), seam_tol=float(seam_tol),
                          min_transmittance=float(min_transmittance))
        self.map = block_map
        dev = block_map.device
        self.poses12 = _poses12(poses, dev)
        n = self.poses12.shape[0]
        if n < 1:
            raise RuntimeError("ParticleFilter: no particles")
        self.beta = float(beta)
        self.margin = float(margin)
        self.miss_cost = block_map.default_miss_cost(huber_delta) if miss_cost is None else float(miss_cost)
        self.render = dict(near=float(near), N_samples=int(N_samples), N_importance=int(N_importance),
                           huber_delta=float(huber_delta), min_sumw=float(min_sumw))
        self.blocks = P.assign_blocks(self.poses12, block_map.boxes, self.margin)
        self.logw = torch.zeros((n,), dtype=torch.float64, device=dev)
        self.w = torch.full((n,), 1.0 / n, dtype=torch.float64, device=dev)
        self.ess = torch.full((1,), float(n), dtype=torch.float64, device=dev)
        self.best = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.degenerate = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.scores4 = torch.zeros((n, 4), dtype=torch.float64, device=dev)
        self.ancestors = torch.arange(n, dtype=torch.int32, device=dev)

    @property
    def n_particles(self) -> int:
        return int(self.poses12.shape[0])

    @property
    def poses(self) -> torch.Tensor:
        """(P, 4, 4) float64 on the device."""
        return _rows_to_poses(self.poses12)

    def predict(self, twist, sigma, generator=None) -> None:
        """Every particle moves by ``se3_exp(twist + sigma * n) @ T``, n ~ N(0, I_6) drawn on the device (``twist`` and
        ``sigma``: six numbers (rho, phi) or a (6,) device tensor each; sigma may be one number for all six); then the
        blocks are re-assigned."""
        n, dev = self.n_particles, self.poses12.device
        t, s = _six(twist, "twist"), _six(sigma, "sigma", scalar_ok=True)
        noise = torch.randn((n, 6), dtype=torch.float64, device=dev, generator=generator)
        # xi = noise * sigma + twist.  A host twist or sigma must not become a tensor here: the host-to-device copy
        # would synchronise.  So each column is scaled and shifted by a Python scalar (a kernel argument) and the six
        # columns are stacked again; a (6,) device tensor broadcasts directly.
        if torch.is_tensor(s):
            xi = noise * s
        else:
            xi = torch.stack([noise[:, k] * s[k] for k in range(6)], -1)
        if torch.is_tensor(t):
            xi = xi + t
        else:
            xi = torch.stack([xi[:, k] + t[k] for k in range(6)], -1)
        self.poses12 = P.se3_apply(xi.contiguous(), self.poses12)
        self.blocks = P.assign_blocks(self.poses12, self.map.boxes, self.margin)

    def update(self, points_sensor: torch.Tensor, beta: Optional[float] = None) -> None:
        """Weight every particle by the scan ``points_sensor`` (R, 3, sensor frame, on the device) rendered against
        the particle's own block."""
        if not points_sensor.is_cuda:
            raise RuntimeError("nof.mcl renders device-resident scans; move points_sensor with .to('cuda') -- there is "
                               "no CPU path")
        if points_sensor.dim() != 2 or points_sensor.shape[1] != 3:
            raise RuntimeError(f"points_sensor must be (R, 3); got {tuple(points_sensor.shape)}")
        pts = points_sensor.detach().float().contiguous()
        r = self.render
        if self.through:
            c = self.chain
            self.scores4 = P.score_poses_through(pts, self.poses12, self.blocks, self.map.boxes, self.map.folds_c,
                                                 self.map.folds_f, r["near"], r["N_samples"], r["N_importance"],
                                                 EPSILON, r["huber_delta"], r["min_sumw"], c["max_segments"],
                                                 c["seam_tol"], c["min_transmittance"], False)[0]
        else:
            self.scores4, _, _ = P.score_poses_map(pts, self.poses12, self.blocks, self.map.boxes, self.map.folds_c,
                                                   self.map.folds_f, r["near"], r["N_samples"], r["N_importance"],
                                                   EPSILON, r["huber_delta"], r["min_sumw"], False)
        rng = torch.linalg.norm(points_sensor.detach().double(), dim=-1).float()   # localize_scan's count, on the device
        n_usable = (torch.isfinite(rng) & (rng > 0)).sum().to(torch.float64).reshape(1)
        self.w, self.logw, self.ess, self.best, self.degenerate = P.mcl_weights(
            self.logw, self.scores4, self.blocks, n_usable, self.miss_cost, self.beta if beta is None else float(beta))
        self.ancestors = torch.arange(self.n_particles, dtype=torch.int32, device=pts.device)   # `best` indexes these

    def resample(self, ess_frac: float = 0.5, u0=None, generator=None) -> None:
        """Systematic resampling when the effective sample size is below ``ess_frac * P``, decided on the device: then
        the particles are redrawn in proportion to their weights and the weights become uniform; otherwise nothing
        moves.  ``u0`` in [0, 1): the offset of the comb (None: drawn on the device; a (1,) device tensor is used
        as it is)."""
        n, dev = self.n_particles, self.poses12.device
        if u0 is None:
            u = torch.rand((1,), dtype=torch.float64, device=dev, generator=generator)
        elif torch.is_tensor(u0) and u0.is_cuda:
            u = u0.detach().to(torch.float64).reshape(1).contiguous()
        else:
            u = torch.full((1,), float(u0), dtype=torch.float64, device=dev)
        self.ancestors, self.poses12, self.blocks, self.logw = P.systematic_resample(
            self.w, u, n, self.ess, float(ess_frac) * n, self.poses12, self.blocks, self.logw)
        self.w = torch.softmax(self.logw, 0)   # (logw is normalised, or zero after a redraw)

    def step(self, points_sensor: torch.Tensor, twist, sigma, *, ess_frac: float = 0.5, generator=None) -> None:
        """predict, update and resample, enqueued with no host synchronisation."""
        self.predict(twist, sigma, generator=generator)
        self.update(points_sensor)
        self.resample(ess_frac, generator=generator)

    def estimate(self) -> MclEstimate:
        """The weighted mean translation, the chordal mean rotation (the rotation nearest to sum_p w_p R_p: its SVD
        with the determinant fixed, plain torch on the device) and the best particle of the last update (after a
        redraw: its first copy)."""
        w = self.w
        t = (w[:, None] * self.poses12[:, 9:12]).sum(0)
        M = (w[:, None] * self.poses12[:, :9]).sum(0).reshape(3, 3)
        U, _, Vh = torch.linalg.svd(M)
        d = torch.sign(torch.linalg.det(U @ Vh))
        D = torch.diag(torch.stack([torch.ones_like(d), torch.ones_like(d), d]))
        T = torch.eye(4, dtype=torch.float64, device=w.device)
        T[:3, :3] = U @ D @ Vh
        T[:3, 3] = t
        # the best particle of the update, found among the current particles through the ancestors
        is_best = (self.ancestors == self.best).to(torch.int32)
        k = torch.argmax(is_best).reshape(1)   # (the first copy; index 0 if it was not drawn)
        found = is_best.sum() > 0
        k = torch.where(found, k, torch.argmax(w).reshape(1))
        return MclEstimate(T, _rows_to_poses(self.poses12[k])[0], k.to(torch.int32), self.blocks[k])
