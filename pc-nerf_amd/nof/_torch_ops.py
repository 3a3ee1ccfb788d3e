"""The render path's C-ABI entries as PyTorch custom operators (``torch.ops.pcnerf.*``).

Each operator is a ``torch.library.custom_op`` whose implementation is the ctypes launcher in ``nof._ops`` (the
``extern "C"`` kernels of lib/libpcnerf_hip.so, enqueued on the current HIP stream), with a fake (meta)
implementation giving the output shapes and dtypes, so torch's dispatcher, FakeTensor tracing and ``torch.compile``
see the path as graph nodes instead of opaque Python.  The loss operator carries its backward through
``register_autograd``.  ``nof.render`` calls the tensor-level stages through these operators; the stages that take a
whole ``nn.Module`` (the train-mode queries and their backward, ``nof._autograd``) stay autograd Functions, since an
operator schema holds tensors, not modules -- the eval query is an operator on the packed weight image instead.

Reference boundary replaced: render.py:416 (render_rays_train), :485 (render_rays_val), :614
(render_rays_view_0525_2_2) and their helpers -- same arguments, the operators are an implementation layer below.
"""
from typing import Optional

import torch
from torch import Tensor

from . import _hip as H
from . import _ops

NS = "pcnerf"
_PACKED = []


def _packed_floats() -> int:
    if not _PACKED:
        _PACKED.append(int(H.lib().pcnerf_nof_eval_packed_floats()))
    return _PACKED[0]


def _need(op: str, name: str, t: Optional[Tensor], shape: tuple, dtype=torch.float32) -> None:
    """Host-side check of one operand against the layout its kernel's grid and reads assume: a contiguous ``dtype``
    device tensor of ``shape`` (None: any size, ``('min', k)``: at least k)."""
    if t is None:
        return
    H.require_device(t)
    _layout(op, name, t, shape, dtype)


def _layout(op: str, name: str, t: Tensor, shape: tuple, dtype=torch.float32) -> None:
    """_need's dtype / contiguity / shape part alone (wherever the tensor lives)."""
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"pcnerf::{op}: {name} must be a contiguous {dtype} device tensor")
    ok = t.dim() == len(shape)
    for have, want in zip(t.shape, shape):
        if want is None:
            continue
        if isinstance(want, tuple):
            ok = ok and have >= want[1]
        else:
            ok = ok and have == want
    if not ok:
        raise RuntimeError(f"pcnerf::{op}: {name} has shape {tuple(t.shape)}, expected {shape}")


# ----------------------------------------------------------------------------------------------- embedding
@torch.library.custom_op(f"{NS}::embed", mutates_args=())
def embed(x: Tensor) -> Tensor:
    """Embedding(3, 10) (models.py:27-41)."""
    return _ops.embed(x)


@embed.register_fake
def _(x):
    return x.new_empty((*x.shape[:-1], 63), dtype=torch.float32)


# ----------------------------------------------------------------------------------------------- sampling
@torch.library.custom_op(f"{NS}::sample_coarse", mutates_args=())
def sample_coarse(rays: Tensor, n_samples: int, n_parent: int, near_col: int, far_col: int, cn_col: int,
                  cf_col: int, disparity: bool) -> Tensor:
    """Coarse z (render.py:429-442; the segmented merge when n_parent < n_samples)."""
    _need("sample_coarse", "rays", rays, (None, None))
    return _ops.sample_coarse(rays, n_samples, n_parent, near_col, far_col, cn_col, cf_col, disparity)


@sample_coarse.register_fake
def _(rays, n_samples, n_parent, near_col, far_col, cn_col, cf_col, disparity):
    return rays.new_empty((rays.shape[0], n_samples), dtype=torch.float32)


@torch.library.custom_op(f"{NS}::perturb", mutates_args=())
def perturb(z: Tensor, amount: float, rand: Tensor) -> Tensor:
    """Stratified perturbation (render.py:449-454)."""
    _need("perturb", "z", z, (None, None))
    _need("perturb", "rand", rand, tuple(z.shape))
    return _ops.perturb(z, amount, rand)


@perturb.register_fake
def _(z, amount, rand):
    return torch.empty_like(z)


@torch.library.custom_op(f"{NS}::resample", mutates_args=())
def resample(z: Tensor, w: Tensor, n_importance: int, u: Optional[Tensor]) -> Tensor:
    """sample_pdf + sort(cat(z, samples)) (render.py:371-412, 463-467)."""
    _need("resample", "z", z, (None, None))
    _need("resample", "w", w, tuple(z.shape))
    return _ops.resample(z, w, n_importance, u)


@resample.register_fake
def _(z, w, n_importance, u):
    return z.new_empty((z.shape[0], z.shape[1] + n_importance), dtype=torch.float32)


@torch.library.custom_op(f"{NS}::sample_pdf", mutates_args=())
def sample_pdf(bins: Tensor, weights: Tensor, n_samples: int, det: bool, u: Optional[Tensor]) -> Tensor:
    """sample_pdf (render.py:371-412), unsorted draws."""
    return _ops.sample_pdf_standalone(bins, weights, n_samples, det, u)


@sample_pdf.register_fake
def _(bins, weights, n_samples, det, u):
    return bins.new_empty((bins.shape[0], n_samples), dtype=torch.float32)


# ----------------------------------------------------------------------------------------------- network (eval)
# pcnerf_nof_params' tensor shapes (models.py: 4 + 4 Linear/BatchNorm1d layers of 256, the skip layer's input
# [x, h_3] 63 + 256 wide, occ_out 256 -> 1): the kernels index them at these sizes, so the operator checks them
_LIN_IN = (63, 256, 256, 256, 319, 256, 256, 256)


def _param_shapes() -> list:
    return ([(256, k) for k in _LIN_IN] + [(256,)] * 40 + [(1, 256), (1,)])


def _check_query(rays: Tensor, z: Tensor, packed: Tensor) -> None:
    """The host-side checks before pcnerf_nof_query_eval's launch: its grid and reads assume these layouts."""
    H.require_device(rays, z, packed)
    for name, t in (("rays", rays), ("z", z), ("packed", packed)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"pcnerf::query_eval: {name} must be a contiguous float32 device tensor")
    if z.dim() != 2 or rays.dim() != 2 or rays.shape[0] != z.shape[0] or rays.shape[1] < 6:
        raise RuntimeError(f"pcnerf::query_eval: rays (R, >=6) and z (R, S) expected, got {tuple(rays.shape)} and "
                           f"{tuple(z.shape)}")
    if packed.numel() != _packed_floats():
        raise RuntimeError(f"pcnerf::query_eval: packed must be pcnerf::pack_eval's image ({_packed_floats()} floats), "
                           f"got {packed.numel()}")
    if not (rays.device == z.device == packed.device):
        raise RuntimeError("pcnerf::query_eval: rays, z and packed must be on one device")


def _params_struct(op: str, params: list) -> "H.NofParams":
    """The 50 tensors of pcnerf_nof_params order, checked against the module's layout, as the C struct."""
    if len(params) != 50:
        raise RuntimeError(f"pcnerf::{op} takes 50 parameter tensors, got {len(params)}")
    s = H.NofParams()
    for i, (t, shp) in enumerate(zip(params, _param_shapes())):
        H.require_device(t)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("NOF parameters must be contiguous float32 device tensors")
        if tuple(t.shape) != shp:
            raise RuntimeError(f"pcnerf::{op}: parameter {i} has shape {tuple(t.shape)}, expected {shp} "
                               "(NOF(feature_size=256, in_channels_xy=63, use_skip=True))")
    for i in range(8):
        s.lin_w[i], s.lin_b[i] = params[i].data_ptr(), params[8 + i].data_ptr()
        s.bn_w[i], s.bn_b[i] = params[16 + i].data_ptr(), params[24 + i].data_ptr()
        s.bn_rm[i], s.bn_rv[i] = params[32 + i].data_ptr(), params[40 + i].data_ptr()
    s.out_w, s.out_b = params[48].data_ptr(), params[49].data_ptr()
    return s


@torch.library.custom_op(f"{NS}::pack_eval", mutates_args=())
def pack_eval(params: list[Tensor]) -> Tensor:
    """The eval network image (BatchNorm folded, MFMA operand order) from the module's 50 tensors in
    pcnerf_nof_params order: lin_w[8], lin_b[8], bn_w[8], bn_b[8], bn_rm[8], bn_rv[8], out_w, out_b."""
    s = _params_struct("pack_eval", params)
    import ctypes
    out = torch.empty(_packed_floats(), dtype=torch.float32, device=params[0].device)
    H.check(H.lib().pcnerf_nof_pack_eval(ctypes.byref(s), out.data_ptr(), H.stream_of(out)))
    return out


@pack_eval.register_fake
def _(params):
    return params[0].new_empty((_packed_floats(),), dtype=torch.float32)


def eval_params(model) -> list:
    """A NOF module's tensors in pcnerf::pack_eval's order."""
    lins, norms = model.linears(), model.norms()
    return ([l.weight for l in lins] + [l.bias for l in lins] + [b.weight for b in norms] + [b.bias for b in norms]
            + [b.running_mean for b in norms] + [b.running_var for b in norms]
            + [model.occ_out[0].weight, model.occ_out[0].bias])


@torch.library.custom_op(f"{NS}::query_eval", mutates_args=())
def query_eval(rays: Tensor, z: Tensor, packed: Tensor) -> Tensor:
    """Eval-mode occupancy p (R, S) of o + d z through Embedding + NOF (render.py:18-25, models.py:183-203)."""
    _check_query(rays, z, packed)
    R, S = z.shape
    p = torch.empty((R, S), dtype=torch.float32, device=z.device)
    H.check(H.lib().pcnerf_nof_query_eval(rays.data_ptr(), R, rays.shape[1], z.data_ptr(), S, packed.data_ptr(),
                                          p.data_ptr(), H.stream_of(z)))
    return p


@query_eval.register_fake
def _(rays, z, packed):
    return torch.empty_like(z)


def _check_points_query(pts: Tensor, packed: Tensor) -> None:
    """The host-side checks before pcnerf_nof_points_eval's launch: its grid and reads assume these layouts."""
    H.require_device(pts, packed)
    for name, t in (("pts", pts), ("packed", packed)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"pcnerf::query_points_eval: {name} must be a contiguous float32 device tensor")
    if pts.dim() not in (2, 3) or pts.shape[-1] != 3 or pts.numel() == 0:
        raise RuntimeError(f"pcnerf::query_points_eval: pts (N, 3) or (R, S, 3) expected, got {tuple(pts.shape)}")
    if packed.numel() != _packed_floats():
        raise RuntimeError(f"pcnerf::query_points_eval: packed must be pcnerf::pack_eval's image ({_packed_floats()} "
                           f"floats), got {packed.numel()}")
    if pts.device != packed.device:
        raise RuntimeError("pcnerf::query_points_eval: pts and packed must be on one device")


@torch.library.custom_op(f"{NS}::query_points_eval", mutates_args=())
def query_points_eval(pts: Tensor, packed: Tensor) -> Tensor:
    """Eval-mode occupancy of explicit sample positions through Embedding + NOF (render.py:18-25 on a caller's
    samples_xy, models.py:183-203): pts (N, 3) -> (N,), pts (R, S, 3) -> (R, S).  The positions are taken as given."""
    _check_points_query(pts, packed)
    p = torch.empty(tuple(pts.shape[:-1]), dtype=torch.float32, device=pts.device)
    H.check(H.lib().pcnerf_nof_points_eval(pts.data_ptr(), p.numel(), packed.data_ptr(), p.data_ptr(),
                                           H.stream_of(pts)))
    return p


@query_points_eval.register_fake
def _(pts, packed):
    return pts.new_empty(tuple(pts.shape[:-1]), dtype=torch.float32)


# ----------------------------------------------------------------------------------------------- eval gradients
# The eval network is sigmoid(a . Embedding(x) + c), so the logit's gradient to a position is
# J(x)^T a with the constant a of pcnerf::fold_eval -- whichever eval math computed p.  These are the backward
# kernels of nof._autograd.EvalPass / EvalPassPoints; they are plain operators (no autograd formula of their own).
@torch.library.custom_op(f"{NS}::fold_eval", mutates_args=())
def fold_eval(params: list[Tensor]) -> Tensor:
    """(a, c) of the eval network, 64 float64 (a = fold[:63], c = fold[63]), composed in float64 from the module's 50
    tensors in pcnerf::pack_eval's order (pcnerf_nof_fold_eval)."""
    s = _params_struct("fold_eval", params)
    import ctypes
    out = torch.empty(64, dtype=torch.float64, device=params[0].device)
    H.check(H.lib().pcnerf_nof_fold_eval(ctypes.byref(s), out.data_ptr(), H.stream_of(out)))
    return out


@fold_eval.register_fake
def _(params):
    return params[0].new_empty((64,), dtype=torch.float64)


def _one_device(op: str, *ts: Tensor) -> None:
    if any(t.device != ts[0].device for t in ts):
        raise RuntimeError(f"pcnerf::{op}: all operands must be on one device")


@torch.library.custom_op(f"{NS}::points_grad_eval", mutates_args=())
def points_grad_eval(pts: Tensor, grad_logit: Tensor, fold: Tensor) -> Tensor:
    """d/d pts of the eval query of explicit positions (autograd of render.py:18-25 to samples_xy): pts (N, 3) or
    (R, S, 3), grad_logit (N,) or (R, S) = dL/dlogit per sample, fold = pcnerf::fold_eval -> pts' shape."""
    op = "points_grad_eval"
    H.require_device(pts)
    if pts.dim() not in (2, 3) or pts.shape[-1] != 3:
        raise RuntimeError(f"pcnerf::{op}: pts has shape {tuple(pts.shape)}, expected (N, 3) or (R, S, 3)")
    _need(op, "pts", pts, tuple(pts.shape))
    _need(op, "grad_logit", grad_logit, tuple(pts.shape[:-1]))
    _need(op, "fold", fold, (64,), torch.float64)
    _one_device(op, pts, grad_logit, fold)
    out = torch.empty_like(pts)
    H.check(H.lib().pcnerf_nof_points_eval_backward(pts.data_ptr(), grad_logit.numel(), fold.data_ptr(),
                                                    grad_logit.data_ptr(), out.data_ptr(), H.stream_of(pts)))
    return out


@points_grad_eval.register_fake
def _(pts, grad_logit, fold):
    return torch.empty_like(pts, dtype=torch.float32)


@torch.library.custom_op(f"{NS}::rays_grad_eval", mutates_args=())
def rays_grad_eval(rays: Tensor, z: Tensor, grad_logit: Tensor, fold: Tensor) -> Tensor:
    """d/d rays[:, 0:6] of the eval query of o + d z (autograd of render.py:518-520 + :18-25 to the origins and
    directions, z constant): rays (R, >=6), z (R, S), grad_logit (R, S), fold = pcnerf::fold_eval -> (R, 6), columns
    0:3 sum_s g_s, 3:6 sum_s z_s g_s."""
    op = "rays_grad_eval"
    _need(op, "z", z, (None, ("min", 1)))
    _need(op, "rays", rays, (z.shape[0], ("min", 6)))
    _need(op, "grad_logit", grad_logit, tuple(z.shape))
    _need(op, "fold", fold, (64,), torch.float64)
    _one_device(op, rays, z, grad_logit, fold)
    R, S = z.shape
    out = torch.empty((R, 6), dtype=torch.float32, device=z.device)
    H.check(H.lib().pcnerf_nof_query_eval_backward(rays.data_ptr(), R, rays.shape[1], z.data_ptr(), S,
                                                   fold.data_ptr(), grad_logit.data_ptr(), out.data_ptr(),
                                                   H.stream_of(z)))
    return out


@rays_grad_eval.register_fake
def _(rays, z, grad_logit, fold):
    return z.new_empty((z.shape[0], 6), dtype=torch.float32)


# ----------------------------------------------------------------------------------------------- registration
# One render pass of a folded eval network with its per-ray Jacobian, and the Gauss-Newton normal equations of a scan
# (nof.registration).  Neither reads a process-wide selector: the pass is the fold whatever the eval math is.
RENDER_JAC_MAX_SAMPLES = 1024   # one wave per ray, at most 16 samples per lane (pcnerf_render_depth_jac_fold)


@torch.library.custom_op(f"{NS}::render_jac_fold", mutates_args=())
def render_jac_fold(rays: Tensor, z: Tensor, fold: Tensor, eps: float, want_weights: bool,
                    want_jac: bool) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(depth (R,), sumw (R,), weights (R, S) or (0,), jac6 (R, 6) or (0,)) of one eval render pass (render.py:13-36
    at noise_std = 0) of sigmoid(a . Embedding(o + d z) + c), fold = pcnerf::fold_eval: sumw is the unnormalised
    weight sum (the hit probability), jac6 = d depth / d rays[:, 0:6] with z constant (what torch autograd of the
    pass gives).  1 <= S <= 1024."""
    op = "render_jac_fold"
    _layout(op, "z", z, (None, ("min", 1)))
    if z.shape[1] > RENDER_JAC_MAX_SAMPLES:
        raise RuntimeError(f"pcnerf::{op}: z has {z.shape[1]} samples per ray, at most {RENDER_JAC_MAX_SAMPLES} "
                           "are supported")
    _layout(op, "rays", rays, (z.shape[0], ("min", 6)))
    _layout(op, "fold", fold, (64,), torch.float64)
    H.require_device(rays, z, fold)
    _one_device(op, rays, z, fold)
    R, S = z.shape
    depth = torch.empty((R,), dtype=torch.float32, device=z.device)
    sumw = torch.empty((R,), dtype=torch.float32, device=z.device)
    w = torch.empty((R, S) if want_weights else (0,), dtype=torch.float32, device=z.device)
    jac = torch.empty((R, 6) if want_jac else (0,), dtype=torch.float32, device=z.device)
    H.check(H.lib().pcnerf_render_depth_jac_fold(rays.data_ptr(), R, rays.shape[1], z.data_ptr(), S, fold.data_ptr(),
                                                 float(eps), depth.data_ptr(), sumw.data_ptr(),
                                                 w.data_ptr() if want_weights else None,
                                                 jac.data_ptr() if want_jac else None, H.stream_of(z)))
    return depth, sumw, w, jac


@render_jac_fold.register_fake
def _(rays, z, fold, eps, want_weights, want_jac):
    R, S = z.shape
    return (z.new_empty((R,), dtype=torch.float32), z.new_empty((R,), dtype=torch.float32),
            z.new_empty((R, S) if want_weights else (0,), dtype=torch.float32),
            z.new_empty((R, 6) if want_jac else (0,), dtype=torch.float32))


@torch.library.custom_op(f"{NS}::gn_normal_eq", mutates_args=())
def gn_normal_eq(rays: Tensor, jac6: Tensor, depth: Tensor, sumw: Tensor, target: Tensor, huber_delta: float,
                 min_sumw: float) -> Tensor:
    """(30,) float64: the upper triangle of H = sum w Jp^T Jp (21, row-major), b = sum w Jp^T r (6), the cost
    sum rho(r), the number of valid rays and one pad word, for r = depth - target over the rays with sumw >= min_sumw
    and finite depth and target > 0; Jp = [J_o, o x J_o + d x J_d] (left perturbation T' = exp(xi) T of the pose that
    produced the world-frame rows); Huber weights, huber_delta <= 0: least squares (pcnerf_gn_normal_eq)."""
    op = "gn_normal_eq"
    _layout(op, "depth", depth, (None,))
    R = depth.shape[0]
    _layout(op, "rays", rays, (R, ("min", 6)))
    _layout(op, "jac6", jac6, (R, 6))
    _layout(op, "sumw", sumw, (R,))
    _layout(op, "target", target, (R,))
    H.require_device(rays, jac6, depth, sumw, target)
    _one_device(op, rays, jac6, depth, sumw, target)
    out = torch.empty((30,), dtype=torch.float64, device=depth.device)
    ws = torch.empty((max(int(H.lib().pcnerf_gn_workspace_bytes(R)), 8),), dtype=torch.uint8, device=depth.device)
    H.check(H.lib().pcnerf_gn_normal_eq(rays.data_ptr(), R, rays.shape[1], jac6.data_ptr(), depth.data_ptr(),
                                        sumw.data_ptr(), target.data_ptr(), float(huber_delta), float(min_sumw),
                                        ws.data_ptr(), out.data_ptr(), H.stream_of(depth)))
    return out


@gn_normal_eq.register_fake
def _(rays, jac6, depth, sumw, target, huber_delta, min_sumw):
    return depth.new_empty((30,), dtype=torch.float64)


# ----------------------------------------------------------------------------------------------- localisation
# The whole two-pass render of a scan under many poses and the per-pose residual sums in one launch (nof.localization).
# Reads no process-wide selector.
SCORE_POSES_MIN_SAMPLES = 3        # the resampling needs one interior weight
SCORE_POSES_MAX_SAMPLES = 1024     # N_samples + N_importance: one wave per beam, at most 16 samples per lane


def check_score_samples(op: str, n_samples: int, n_importance: int) -> None:
    if n_samples < SCORE_POSES_MIN_SAMPLES:
        raise RuntimeError(f"pcnerf::{op}: N_samples = {n_samples}, at least {SCORE_POSES_MIN_SAMPLES} samples are "
                           "needed")
    if n_importance < 1:
        raise RuntimeError(f"pcnerf::{op}: N_importance = {n_importance}, at least 1 sample is needed")
    if n_samples + n_importance > SCORE_POSES_MAX_SAMPLES:
        raise RuntimeError(f"pcnerf::{op}: N_samples + N_importance = {n_samples + n_importance} samples per beam, at "
                           f"most {SCORE_POSES_MAX_SAMPLES} are supported")


@torch.library.custom_op(f"{NS}::score_poses_fold", mutates_args=())
def score_poses_fold(points: Tensor, poses12: Tensor, box6: Tensor, fold_coarse: Tensor, fold_fine: Tensor,
                     near: float, n_samples: int, n_importance: int, eps: float, huber_delta: float,
                     min_sumw: float, want_depth: bool) -> tuple[Tensor, Tensor, Tensor]:
    """(scores4 (P, 4) float64 = [sum_valid rho(r), n_valid, sum_valid |r|, sum_usable sumw], depth (P, R) or (0,),
    sumw (P, R) or (0,)) of the scan points (R, 3) (sensor frame) under the poses12 (P, 12) rows [R row-major, t]
    against the two folded networks inside the box6 = [lo, hi]: scan_rays + render_scan + the cost of gn_normal_eq
    per pose, fused (pcnerf_score_poses_fold).  want_depth does not change a bit of scores4."""
    op = "score_poses_fold"
    _layout(op, "points", points, (None, 3))
    _layout(op, "poses12", poses12, (None, 12), torch.float64)
    _layout(op, "box6", box6, (6,), torch.float64)
    _layout(op, "fold_coarse", fold_coarse, (64,), torch.float64)
    _layout(op, "fold_fine", fold_fine, (64,), torch.float64)
    check_score_samples(op, n_samples, n_importance)
    H.require_device(points, poses12, box6, fold_coarse, fold_fine)
    _one_device(op, points, poses12, box6, fold_coarse, fold_fine)
    R, Pn = points.shape[0], poses12.shape[0]
    dev = points.device
    scores = torch.empty((Pn, 4), dtype=torch.float64, device=dev)
    depth = torch.empty((Pn, R) if want_depth else (0,), dtype=torch.float32, device=dev)
    sumw = torch.empty((Pn, R) if want_depth else (0,), dtype=torch.float32, device=dev)
    nbytes = int(H.lib().pcnerf_score_poses_workspace_bytes(Pn, R))
    ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=dev)
    H.check(H.lib().pcnerf_score_poses_fold(points.data_ptr(), R, poses12.data_ptr(), Pn, box6.data_ptr(),
                                            float(near), int(n_samples), int(n_importance),
                                            fold_coarse.data_ptr(), fold_fine.data_ptr(), float(eps),
                                            float(huber_delta), float(min_sumw), ws.data_ptr(), nbytes,
                                            scores.data_ptr(), depth.data_ptr() if want_depth else None,
                                            sumw.data_ptr() if want_depth else None, H.stream_of(points)))
    return scores, depth, sumw


@score_poses_fold.register_fake
def _(points, poses12, box6, fold_coarse, fold_fine, near, n_samples, n_importance, eps, huber_delta, min_sumw,
      want_depth):
    R, Pn = points.shape[0], poses12.shape[0]
    return (points.new_empty((Pn, 4), dtype=torch.float64),
            points.new_empty((Pn, R) if want_depth else (0,), dtype=torch.float32),
            points.new_empty((Pn, R) if want_depth else (0,), dtype=torch.float32))


# ----------------------------------------------------------------------------------------------- frozen BatchNorm
# Parameter gradients of the eval-mode network: logit = a(theta) . e + c(theta), so the gradients of a pass are those of
# one pseudo-sample with input m = sum_s g_s e_s and constants scaled by s0 = sum_s g_s (include/pcnerf_hip.h).  The
# backward kernels of nof._autograd.FrozenPass / FrozenPassPoints; plain operators.
def _gmoments_checked(op: str, *ts: Tensor) -> None:
    _one_device(op, *ts)


@torch.library.custom_op(f"{NS}::eval_gmoments_rays", mutates_args=())
def eval_gmoments_rays(rays: Tensor, z: Tensor, grad_logit: Tensor) -> Tensor:
    """(64,) float64: [:63] = sum_s g_s Embedding(o + d z_s), [63] = sum_s g_s over the pass (autograd of
    render.py:44-51 to the eval network's parameters, first stage): rays (R, >=6), z (R, S), grad_logit (R, S)."""
    op = "eval_gmoments_rays"
    _need(op, "z", z, (None, ("min", 1)))
    _need(op, "rays", rays, (z.shape[0], ("min", 6)))
    _need(op, "grad_logit", grad_logit, tuple(z.shape))
    _gmoments_checked(op, rays, z, grad_logit)
    return _ops.eval_gmoments_rays(rays, z, grad_logit)


@eval_gmoments_rays.register_fake
def _(rays, z, grad_logit):
    return z.new_empty((64,), dtype=torch.float64)


@torch.library.custom_op(f"{NS}::eval_gmoments_points", mutates_args=())
def eval_gmoments_points(pts: Tensor, grad_logit: Tensor) -> Tensor:
    """eval_gmoments_rays on explicit positions, read verbatim: pts (N, 3) or (R, S, 3), grad_logit (N,) or (R, S)."""
    op = "eval_gmoments_points"
    H.require_device(pts)
    if pts.dim() not in (2, 3) or pts.shape[-1] != 3:
        raise RuntimeError(f"pcnerf::{op}: pts has shape {tuple(pts.shape)}, expected (N, 3) or (R, S, 3)")
    _need(op, "pts", pts, tuple(pts.shape))
    _need(op, "grad_logit", grad_logit, tuple(pts.shape[:-1]))
    _gmoments_checked(op, pts, grad_logit)
    return _ops.eval_gmoments_points(pts, grad_logit)


@eval_gmoments_points.register_fake
def _(pts, grad_logit):
    return pts.new_empty((64,), dtype=torch.float64)


@torch.library.custom_op(f"{NS}::eval_gmoments_embedded", mutates_args=())
def eval_gmoments_embedded(emb: Tensor, grad_logit: Tensor) -> Tensor:
    """eval_gmoments_rays on an embedded batch (models.py:103-123's input): emb (N, 63), grad_logit (N,)."""
    op = "eval_gmoments_embedded"
    _need(op, "emb", emb, (None, 63))
    _need(op, "grad_logit", grad_logit, (emb.shape[0],))
    _gmoments_checked(op, emb, grad_logit)
    return _ops.eval_gmoments_embedded(emb, grad_logit)


@eval_gmoments_embedded.register_fake
def _(emb, grad_logit):
    return emb.new_empty((64,), dtype=torch.float64)


@torch.library.custom_op(f"{NS}::eval_param_grads", mutates_args=())
def eval_param_grads(params: list[Tensor], mom: Tensor, eps: float) -> list[Tensor]:
    """The 34 parameter gradients (nof._ops.grad_params order: lin_w[8], lin_b[8], bn_w[8], bn_b[8], out_w, out_b) of
    the eval network's pseudo-sample with moments ``mom`` (pcnerf::eval_gmoments_*), float64 algebra rounded to
    float32 once (pcnerf_nof_eval_param_grads).  params: the 50 tensors in pcnerf::pack_eval's order; the running
    statistics are read, never written."""
    op = "eval_param_grads"
    s = _params_struct(op, params)
    _need(op, "mom", mom, (64,), torch.float64)
    _one_device(op, params[0], mom)
    import ctypes
    shapes = _param_shapes()
    # an operator's outputs own their memory (no views of one buffer): 34 zeroed tensors the kernel adds into
    out = [torch.zeros(shp, dtype=torch.float32, device=mom.device) for shp in shapes[:32] + shapes[48:]]
    g = H.NofGrads()
    for i in range(8):
        g.lin_w[i], g.lin_b[i] = out[i].data_ptr(), out[8 + i].data_ptr()
        g.bn_w[i], g.bn_b[i] = out[16 + i].data_ptr(), out[24 + i].data_ptr()
    g.out_w, g.out_b = out[32].data_ptr(), out[33].data_ptr()
    H.check(H.lib().pcnerf_nof_eval_param_grads(ctypes.byref(s), float(eps), mom.data_ptr(), ctypes.byref(g),
                                                H.stream_of(mom)))
    return out


@eval_param_grads.register_fake
def _(params, mom, eps):
    shapes = _param_shapes()
    return [mom.new_empty(s, dtype=torch.float32) for s in shapes[:32] + shapes[48:]]


# ----------------------------------------------------------------------------------------------- compositing
@torch.library.custom_op(f"{NS}::composite", mutates_args=())
def composite(p: Tensor, z: Tensor, noise: Optional[Tensor], noise_std: float, eps: float, rays: Optional[Tensor],
              cn_col: int, cf_col: int, range_col: int, want_weights: bool) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(weights (R,S) or (0,), depth (R,), free_ray (R,) or (0,), sl1_ray (R,) or (0,)): render.py:51-61, 75-159."""
    _need("composite", "z", z, (None, None))
    _need("composite", "p", p, tuple(z.shape))
    _need("composite", "rays", rays, (z.shape[0], None))
    w, d, fr, sl = _ops.composite(p, z, noise, noise_std, eps, rays, cn_col, cf_col, range_col, want_weights)
    e = z.new_empty((0,))
    return (w if w is not None else e), d, (fr if fr is not None else e.clone()), (sl if sl is not None else e.clone())


@composite.register_fake
def _(p, z, noise, noise_std, eps, rays, cn_col, cf_col, range_col, want_weights):
    R, S = z.shape
    w = z.new_empty((R, S) if want_weights else (0,))
    r = (R,) if rays is not None else (0,)
    return w, z.new_empty((R,)), z.new_empty(r), z.new_empty(r)


@torch.library.custom_op(f"{NS}::composite_extras", mutates_args=())
def composite_extras(p: Tensor, z: Tensor, noise: Optional[Tensor], noise_std: float,
                     eps: float) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """render_rays's compositing (render.py:538-611): (weights, depth, opacity mean (), depth2 (R,))."""
    _need("composite_extras", "z", z, (None, None))
    _need("composite_extras", "p", p, tuple(z.shape))
    w, d, _, _, om, d2 = _ops.composite(p, z, noise, noise_std, eps, extras=True)
    return w, d, om, d2


@composite_extras.register_fake
def _(p, z, noise, noise_std, eps):
    R, S = z.shape
    return z.new_empty((R, S)), z.new_empty((R,)), z.new_empty(()), z.new_empty((R,))


@torch.library.custom_op(f"{NS}::child_losses", mutates_args=())
def child_losses(free_ray: Tensor, sl1_ray: Tensor, rays: Tensor, divide: bool,
                 sub_nerf_test_num: int) -> tuple[Tensor, Tensor]:
    """(child_free_loss, child_depth_loss): (1,) each in the divide branch, () otherwise (render.py:102-159)."""
    _need("child_losses", "free_ray", free_ray, (None,))
    _need("child_losses", "sl1_ray", sl1_ray, tuple(free_ray.shape))
    _need("child_losses", "rays", rays, (free_ray.shape[0], ("min", 10)))
    a, b = _ops.child_losses(free_ray, sl1_ray, rays, divide, sub_nerf_test_num)
    return a.clone(), b.clone()


@child_losses.register_fake
def _(free_ray, sl1_ray, rays, divide, sub_nerf_test_num):
    shp = (1,) if (divide and sub_nerf_test_num > 0) else ()
    return free_ray.new_empty(shp), free_ray.new_empty(shp)


# ----------------------------------------------------------------------------------------------- two-step view
@torch.library.custom_op(f"{NS}::view_rows", mutates_args=())
def view_rows(p: Tensor, z: Tensor, rows: Tensor, method: int,
              eps: float) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """inference_0525_2's per-row stage (render.py:229-330): weights, depth, at_peak (uint8), child sum, per-row
    opacity terms (float64), points (R, 3)."""
    _need("view_rows", "z", z, (None, None))
    _need("view_rows", "p", p, tuple(z.shape))
    _need("view_rows", "rows", rows, (z.shape[0], ("min", 8)))
    return _ops.view_rows(p, z, rows, method, eps)


@view_rows.register_fake
def _(p, z, rows, method, eps):
    R, S = z.shape
    return (z.new_empty((R, S)), z.new_empty((R,)), z.new_empty((R,), dtype=torch.uint8), z.new_empty((R,)),
            z.new_empty((R,), dtype=torch.float64), z.new_empty((R, 3)))


@torch.library.custom_op(f"{NS}::view_walk", mutates_args=())
def view_walk(other: Tensor, at_peak: Tensor, child_sum: Tensor, opac_row: Tensor,
              n_samples: int) -> tuple[Tensor, Tensor]:
    """inference_0525_2's ray-group walk (render.py:331-368): effective-row flags (R, 1) bool, opacity ()."""
    return _ops.view_walk(other, at_peak, child_sum, opac_row, n_samples)


@view_walk.register_fake
def _(other, at_peak, child_sum, opac_row, n_samples):
    R = at_peak.shape[0]
    return at_peak.new_empty((R, 1), dtype=torch.bool), at_peak.new_empty((), dtype=torch.float32)


# ----------------------------------------------------------------------------------------------- losses
@torch.library.custom_op(f"{NS}::pointwise_loss", mutates_args=())
def pointwise_loss(pred: Tensor, target: Tensor, kind: str, valid_mask: Optional[Tensor]) -> Tensor:
    """mean(loss(pred, target)) of nof/criteria/loss.py (MSE / L1 / SmoothL1)."""
    return _ops.pointwise_loss(pred, target, kind, valid_mask)


@pointwise_loss.register_fake
def _(pred, target, kind, valid_mask):
    return pred.new_empty((), dtype=torch.float32)


@torch.library.custom_op(f"{NS}::pointwise_loss_backward", mutates_args=())
def pointwise_loss_backward(pred: Tensor, target: Tensor, kind: str, valid_mask: Optional[Tensor],
                            grad_out: Tensor) -> Tensor:
    return _ops.pointwise_loss_backward(pred, target, kind, valid_mask, grad_out).reshape(pred.shape)


@pointwise_loss_backward.register_fake
def _(pred, target, kind, valid_mask, grad_out):
    return torch.empty_like(pred, dtype=torch.float32)


def _pl_setup(ctx, inputs, output):
    pred, target, kind, valid_mask = inputs
    ctx.kind = kind
    ctx.save_for_backward(pred, target, valid_mask)


def _pl_backward(ctx, g):
    pred, target, m = ctx.saved_tensors
    return torch.ops.pcnerf.pointwise_loss_backward(pred, target, ctx.kind, m, g.contiguous()), None, None, None


pointwise_loss.register_autograd(_pl_backward, setup_context=_pl_setup)


def op_names() -> list:
    """The registered operator names (tests)."""
    return ["embed", "sample_coarse", "perturb", "resample", "sample_pdf", "pack_eval", "query_eval", "query_points_eval", "composite",
            "composite_extras", "child_losses", "view_rows", "view_walk", "pointwise_loss",
            "pointwise_loss_backward", "fold_eval", "points_grad_eval", "rays_grad_eval", "eval_gmoments_rays",
            "eval_gmoments_points", "eval_gmoments_embedded", "eval_param_grads", "render_jac_fold", "gn_normal_eq",
            "score_poses_fold", "pose_normal_eq_fold", "lm_init", "lm_update", "refine_poses_fold", "se3_apply"]


# ----------------------------------------------------------------------------------------------- batched refinement
# Device-resident Levenberg-Marquardt over many poses (nof.registration.refine_poses_fold): one fused evaluation of all
# running poses, the per-pose state machine and the SE(3) update as operators.  Reads no process-wide selector.
LM_STATE_DOUBLES = 64   # PCNERF_LM_STATE_DOUBLES: T_acc 12 | T_trial 12 | normal30 30 | lambda, status, evals, accepted | xi 6


def _ws(nbytes: int, dev) -> Tensor:
    return torch.empty((max(int(nbytes), 8),), dtype=torch.uint8, device=dev)


@torch.library.custom_op(f"{NS}::pose_normal_eq_fold", mutates_args=())
def pose_normal_eq_fold(points: Tensor, poses12: Optional[Tensor], state: Optional[Tensor], box6: Tensor,
                        fold_coarse: Tensor, fold_fine: Tensor, near: float, n_samples: int, n_importance: int,
                        eps: float, huber_delta: float, min_sumw: float,
                        want_beams: bool) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(normal30 (P, 30) float64 in gn_normal_eq's layout, depth (P, R), sumw (P, R), jac6 (P, R, 6) float32 or (0,)
    each) of one Gauss-Newton evaluation of the scan points (R, 3) under P poses: the states' T_trial (state (P, 64),
    lm_init / lm_update; poses with status != 0 are skipped: zero rows) or, without a state, the poses12 (P, 12) rows.
    scan_rays + render_scan(want_jac) + gn_normal_eq per pose, fused (pcnerf_pose_normal_eq_fold).  want_beams does
    not change a bit of normal30."""
    op = "pose_normal_eq_fold"
    _layout(op, "points", points, (None, 3))
    if state is None and poses12 is None:
        raise RuntimeError(f"pcnerf::{op}: one of poses12 and state is needed")
    if state is not None:
        _layout(op, "state", state, (None, LM_STATE_DOUBLES), torch.float64)
    else:
        _layout(op, "poses12", poses12, (None, 12), torch.float64)
    _layout(op, "box6", box6, (6,), torch.float64)
    _layout(op, "fold_coarse", fold_coarse, (64,), torch.float64)
    _layout(op, "fold_fine", fold_fine, (64,), torch.float64)
    check_score_samples(op, n_samples, n_importance)
    src = state if state is not None else poses12
    H.require_device(points, src, box6, fold_coarse, fold_fine)
    _one_device(op, points, src, box6, fold_coarse, fold_fine)
    R, Pn = points.shape[0], src.shape[0]
    dev = points.device
    n30 = torch.zeros((Pn, 30), dtype=torch.float64, device=dev)
    depth = torch.zeros((Pn, R) if want_beams else (0,), dtype=torch.float32, device=dev)
    sumw = torch.zeros((Pn, R) if want_beams else (0,), dtype=torch.float32, device=dev)
    jac = torch.zeros((Pn, R, 6) if want_beams else (0,), dtype=torch.float32, device=dev)
    nbytes = int(H.lib().pcnerf_pose_normal_eq_workspace_bytes(Pn, R))
    ws = _ws(nbytes, dev)
    H.check(H.lib().pcnerf_pose_normal_eq_fold(points.data_ptr(), R, None if state is not None else poses12.data_ptr(),
                                               Pn, state.data_ptr() if state is not None else None, box6.data_ptr(),
                                               float(near), int(n_samples), int(n_importance),
                                               fold_coarse.data_ptr(), fold_fine.data_ptr(), float(eps),
                                               float(huber_delta), float(min_sumw), ws.data_ptr(), nbytes,
                                               n30.data_ptr(), depth.data_ptr() if want_beams else None,
                                               sumw.data_ptr() if want_beams else None,
                                               jac.data_ptr() if want_beams else None, H.stream_of(points)))
    return n30, depth, sumw, jac


@pose_normal_eq_fold.register_fake
def _(points, poses12, state, box6, fold_coarse, fold_fine, near, n_samples, n_importance, eps, huber_delta, min_sumw,
      want_beams):
    R, Pn = points.shape[0], (state if state is not None else poses12).shape[0]
    return (points.new_empty((Pn, 30), dtype=torch.float64),
            points.new_empty((Pn, R) if want_beams else (0,), dtype=torch.float32),
            points.new_empty((Pn, R) if want_beams else (0,), dtype=torch.float32),
            points.new_empty((Pn, R, 6) if want_beams else (0,), dtype=torch.float32))


@torch.library.custom_op(f"{NS}::lm_init", mutates_args=())
def lm_init(poses12: Tensor, damping: float) -> Tensor:
    """state (P, 64) float64 of a refinement that starts at the poses12 (P, 12) rows: T_acc = T_trial = the start,
    lambda = damping, status, counters and xi zero (pcnerf_lm_init)."""
    op = "lm_init"
    _layout(op, "poses12", poses12, (None, 12), torch.float64)
    H.require_device(poses12)
    state = torch.empty((poses12.shape[0], LM_STATE_DOUBLES), dtype=torch.float64, device=poses12.device)
    H.check(H.lib().pcnerf_lm_init(poses12.data_ptr(), poses12.shape[0], float(damping), state.data_ptr(),
                                   H.stream_of(poses12)))
    return state


@lm_init.register_fake
def _(poses12, damping):
    return poses12.new_empty((poses12.shape[0], LM_STATE_DOUBLES), dtype=torch.float64)


@torch.library.custom_op(f"{NS}::lm_update", mutates_args=())
def lm_update(normal30: Tensor, state: Tensor, xi_tol: float) -> tuple[Tensor, Tensor, Tensor]:
    """(state' (P, 64), cost (P,) float64: the evaluation's cost, NaN for a pose that was not running, accepted (P,)
    uint8) of one Levenberg-Marquardt step of every running pose from its normal30 row: register_scan_fold's accept /
    reject rule, the damped 6 x 6 solve and T_trial = se3_exp(xi) T_acc in float64 (pcnerf_lm_update).  The input
    state is not modified."""
    op = "lm_update"
    _layout(op, "state", state, (None, LM_STATE_DOUBLES), torch.float64)
    _layout(op, "normal30", normal30, (state.shape[0], 30), torch.float64)
    H.require_device(normal30, state)
    _one_device(op, normal30, state)
    Pn = state.shape[0]
    out = state.clone()
    cost = torch.full((Pn,), float("nan"), dtype=torch.float64, device=state.device)
    acc = torch.zeros((Pn,), dtype=torch.uint8, device=state.device)
    H.check(H.lib().pcnerf_lm_update(normal30.data_ptr(), Pn, float(xi_tol), out.data_ptr(), cost.data_ptr(),
                                     acc.data_ptr(), 0, 1, H.stream_of(state)))
    return out, cost, acc


@lm_update.register_fake
def _(normal30, state, xi_tol):
    Pn = state.shape[0]
    return (state.new_empty((Pn, LM_STATE_DOUBLES), dtype=torch.float64),
            state.new_empty((Pn,), dtype=torch.float64), state.new_empty((Pn,), dtype=torch.uint8))


@torch.library.custom_op(f"{NS}::refine_poses_fold", mutates_args=())
def refine_poses_fold(points: Tensor, poses12: Tensor, box6: Tensor, fold_coarse: Tensor, fold_fine: Tensor,
                      near: float, n_samples: int, n_importance: int, eps: float, huber_delta: float,
                      min_sumw: float, damping: float, xi_tol: float,
                      iters: int) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(poses12_out (P, 12) float64, state (P, 64) float64, eval_costs (P, iters) float64 with NaN where a pose was
    not evaluated, accepted (P, iters) uint8) of lm_init and iters x (pose_normal_eq_fold, lm_update), enqueued without
    a host synchronisation (pcnerf_refine_poses_fold).  poses12_out is T_trial, or T_acc where status is 2 or 3."""
    op = "refine_poses_fold"
    _layout(op, "points", points, (None, 3))
    _layout(op, "poses12", poses12, (None, 12), torch.float64)
    _layout(op, "box6", box6, (6,), torch.float64)
    _layout(op, "fold_coarse", fold_coarse, (64,), torch.float64)
    _layout(op, "fold_fine", fold_fine, (64,), torch.float64)
    check_score_samples(op, n_samples, n_importance)
    if iters < 0:
        raise RuntimeError(f"pcnerf::{op}: iters = {iters} is negative")
    H.require_device(points, poses12, box6, fold_coarse, fold_fine)
    _one_device(op, points, poses12, box6, fold_coarse, fold_fine)
    R, Pn = points.shape[0], poses12.shape[0]
    dev = points.device
    out = torch.zeros((Pn, 12), dtype=torch.float64, device=dev)
    state = torch.zeros((Pn, LM_STATE_DOUBLES), dtype=torch.float64, device=dev)
    costs = torch.full((Pn, iters), float("nan"), dtype=torch.float64, device=dev)
    acc = torch.zeros((Pn, iters), dtype=torch.uint8, device=dev)
    n30 = torch.empty((max(Pn, 1), 30), dtype=torch.float64, device=dev)
    nbytes = int(H.lib().pcnerf_pose_normal_eq_workspace_bytes(Pn, R))
    ws = _ws(nbytes, dev)
    H.check(H.lib().pcnerf_refine_poses_fold(points.data_ptr(), R, poses12.data_ptr(), Pn, box6.data_ptr(),
                                             float(near), int(n_samples), int(n_importance),
                                             fold_coarse.data_ptr(), fold_fine.data_ptr(), float(eps),
                                             float(huber_delta), float(min_sumw), float(damping), float(xi_tol),
                                             int(iters), ws.data_ptr(), nbytes, n30.data_ptr(), state.data_ptr(),
                                             out.data_ptr(), costs.data_ptr(), acc.data_ptr(), H.stream_of(points)))
    return out, state, costs, acc


@refine_poses_fold.register_fake
def _(points, poses12, box6, fold_coarse, fold_fine, near, n_samples, n_importance, eps, huber_delta, min_sumw,
      damping, xi_tol, iters):
    Pn = poses12.shape[0]
    return (points.new_empty((Pn, 12), dtype=torch.float64),
            points.new_empty((Pn, LM_STATE_DOUBLES), dtype=torch.float64),
            points.new_empty((Pn, iters), dtype=torch.float64), points.new_empty((Pn, iters), dtype=torch.uint8))


@torch.library.custom_op(f"{NS}::se3_apply", mutates_args=())
def se3_apply(xi6: Tensor, poses12: Tensor) -> Tensor:
    """(P, 12) float64 rows of se3_exp(xi6[p]) @ T[p], xi = (rho, phi), on the poses12 (P, 12) rows [R row-major, t]
    (pcnerf_se3_apply: nof.registration.se3_exp's branches and series on the device)."""
    op = "se3_apply"
    _layout(op, "poses12", poses12, (None, 12), torch.float64)
    _layout(op, "xi6", xi6, (poses12.shape[0], 6), torch.float64)
    H.require_device(xi6, poses12)
    _one_device(op, xi6, poses12)
    out = torch.empty_like(poses12)
    H.check(H.lib().pcnerf_se3_apply(xi6.data_ptr(), poses12.data_ptr(), poses12.shape[0], out.data_ptr(),
                                     H.stream_of(poses12)))
    return out


@se3_apply.register_fake
def _(xi6, poses12):
    return poses12.new_empty(tuple(poses12.shape), dtype=torch.float64)


# ----------------------------------------------------------------------------------------------- maps of blocks
# score_poses_fold / pose_normal_eq_fold / refine_poses_fold with every pose rendered against its own block
# (nof.localization.BlockMap: folds (B, 64), boxes (B, 6)), and the particle-filter update of nof.mcl.  Read no
# process-wide selector.
def _need_on_device(op: str, *ts: Optional[Tensor]) -> None:
    """Every operand is a ROCm device tensor on one device (int32 block ids included)."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"pcnerf::{op}: pcnerf_hip kernels take ROCm device tensors (got {t.dtype} on "
                               f"{t.device}); this package has no CPU path")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"pcnerf::{op}: operands are on different devices")
        dev = t.device


def _check_map(op: str, boxes6: Tensor, folds_coarse: Tensor, folds_fine: Tensor) -> int:
    _layout(op, "boxes6", boxes6, (("min", 1), 6), torch.float64)
    B = boxes6.shape[0]
    _layout(op, "folds_coarse", folds_coarse, (B, 64), torch.float64)
    _layout(op, "folds_fine", folds_fine, (B, 64), torch.float64)
    return B


@torch.library.custom_op(f"{NS}::assign_blocks", mutates_args=())
def assign_blocks(poses12: Tensor, boxes6: Tensor, margin: float) -> Tensor:
    """(P,) int32: per poses12 (P, 12) row the block of boxes6 (B, 6) = [lo, hi] rows that contains the translation
    with ``margin`` to spare on every side and has the largest clearance (lowest index on ties); -1 for none or a NaN
    translation (pcnerf_assign_blocks)."""
    op = "assign_blocks"
    _layout(op, "poses12", poses12, (None, 12), torch.float64)
    _layout(op, "boxes6", boxes6, (("min", 1), 6), torch.float64)
    _need_on_device(op, poses12, boxes6)
    out = torch.empty((poses12.shape[0],), dtype=torch.int32, device=poses12.device)
    H.check(H.lib().pcnerf_assign_blocks(poses12.data_ptr(), poses12.shape[0], boxes6.data_ptr(), boxes6.shape[0],
                                         float(margin), out.data_ptr(), H.stream_of(poses12)))
    return out


@assign_blocks.register_fake
def _(poses12, boxes6, margin):
    return poses12.new_empty((poses12.shape[0],), dtype=torch.int32)


@torch.library.custom_op(f"{NS}::score_poses_map", mutates_args=())
def score_poses_map(points: Tensor, poses12: Tensor, block_of_pose: Tensor, boxes6: Tensor, folds_coarse: Tensor,
                    folds_fine: Tensor, near: float, n_samples: int, n_importance: int, eps: float,
                    huber_delta: float, min_sumw: float, want_depth: bool) -> tuple[Tensor, Tensor, Tensor]:
    """score_poses_fold with pose p rendered against block block_of_pose[p] (int32 (P,)) of the map boxes6 (B, 6),
    folds_coarse / folds_fine (B, 64): the same bits per pose as score_poses_fold with that block alone.  A pose with
    -1 (or any index outside 0 .. B - 1) gets a zero scores4 row, NaN depth and zero sumw (pcnerf_score_poses_map)."""
    op = "score_poses_map"
    _layout(op, "points", points, (None, 3))
    _layout(op, "poses12", poses12, (None, 12), torch.float64)
    _layout(op, "block_of_pose", block_of_pose, (poses12.shape[0],), torch.int32)
    B = _check_map(op, boxes6, folds_coarse, folds_fine)
    check_score_samples(op, n_samples, n_importance)
    _need_on_device(op, points, poses12, block_of_pose, boxes6, folds_coarse, folds_fine)
    R, Pn = points.shape[0], poses12.shape[0]
    dev = points.device
    scores = torch.empty((Pn, 4), dtype=torch.float64, device=dev)
    depth = torch.empty((Pn, R) if want_depth else (0,), dtype=torch.float32, device=dev)
    sumw = torch.empty((Pn, R) if want_depth else (0,), dtype=torch.float32, device=dev)
    nbytes = int(H.lib().pcnerf_score_poses_workspace_bytes(Pn, R))
    ws = _ws(nbytes, dev)
    H.check(H.lib().pcnerf_score_poses_map(points.data_ptr(), R, poses12.data_ptr(), Pn, block_of_pose.data_ptr(), B,
                                           boxes6.data_ptr(), float(near), int(n_samples), int(n_importance),
                                           folds_coarse.data_ptr(), folds_fine.data_ptr(), float(eps),
                                           float(huber_delta), float(min_sumw), ws.data_ptr(), nbytes,
                                           scores.data_ptr(), depth.data_ptr() if want_depth else None,
                                           sumw.data_ptr() if want_depth else None, H.stream_of(points)))
    return scores, depth, sumw


@score_poses_map.register_fake
def _(points, poses12, block_of_pose, boxes6, folds_coarse, folds_fine, near, n_samples, n_importance, eps,
      huber_delta, min_sumw, want_depth):
    R, Pn = points.shape[0], poses12.shape[0]
    return (points.new_empty((Pn, 4), dtype=torch.float64),
            points.new_empty((Pn, R) if want_depth else (0,), dtype=torch.float32),
            points.new_empty((Pn, R) if want_depth else (0,), dtype=torch.float32))


@torch.library.custom_op(f"{NS}::pose_normal_eq_map", mutates_args=())
def pose_normal_eq_map(points: Tensor, poses12: Optional[Tensor], state: Optional[Tensor], block_of_pose: Tensor,
                       boxes6: Tensor, folds_coarse: Tensor, folds_fine: Tensor, near: float, n_samples: int,
                       n_importance: int, eps: float, huber_delta: float, min_sumw: float,
                       want_beams: bool) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """pose_normal_eq_fold with pose p rendered against block block_of_pose[p] of the map: the same bits per pose.
    The rows of a pose without a block are zero, as a stopped pose's (pcnerf_pose_normal_eq_map)."""
    op = "pose_normal_eq_map"
    _layout(op, "points", points, (None, 3))
    if state is None and poses12 is None:
        raise RuntimeError(f"pcnerf::{op}: one of poses12 and state is needed")
    if state is not None:
        _layout(op, "state", state, (None, LM_STATE_DOUBLES), torch.float64)
    else:
        _layout(op, "poses12", poses12, (None, 12), torch.float64)
    src = state if state is not None else poses12
    _layout(op, "block_of_pose", block_of_pose, (src.shape[0],), torch.int32)
    B = _check_map(op, boxes6, folds_coarse, folds_fine)
    check_score_samples(op, n_samples, n_importance)
    _need_on_device(op, points, src, block_of_pose, boxes6, folds_coarse, folds_fine)
    R, Pn = points.shape[0], src.shape[0]
    dev = points.device
    n30 = torch.zeros((Pn, 30), dtype=torch.float64, device=dev)
    depth = torch.zeros((Pn, R) if want_beams else (0,), dtype=torch.float32, device=dev)
    sumw = torch.zeros((Pn, R) if want_beams else (0,), dtype=torch.float32, device=dev)
    jac = torch.zeros((Pn, R, 6) if want_beams else (0,), dtype=torch.float32, device=dev)
    nbytes = int(H.lib().pcnerf_pose_normal_eq_workspace_bytes(Pn, R))
    ws = _ws(nbytes, dev)
    H.check(H.lib().pcnerf_pose_normal_eq_map(points.data_ptr(), R, None if state is not None else poses12.data_ptr(),
                                              Pn, state.data_ptr() if state is not None else None,
                                              block_of_pose.data_ptr(), B, boxes6.data_ptr(), float(near),
                                              int(n_samples), int(n_importance), folds_coarse.data_ptr(),
                                              folds_fine.data_ptr(), float(eps), float(huber_delta), float(min_sumw),
                                              ws.data_ptr(), nbytes, n30.data_ptr(),
                                              depth.data_ptr() if want_beams else None,
                                              sumw.data_ptr() if want_beams else None,
                                              jac.data_ptr() if want_beams else None, H.stream_of(points)))
    return n30, depth, sumw, jac


@pose_normal_eq_map.register_fake
def _(points, poses12, state, block_of_pose, boxes6, folds_coarse, folds_fine, near, n_samples, n_importance, eps,
      huber_delta, min_sumw, want_beams):
    R, Pn = points.shape[0], (state if state is not None else poses12).shape[0]
    return (points.new_empty((Pn, 30), dtype=torch.float64),
            points.new_empty((Pn, R) if want_beams else (0,), dtype=torch.float32),
            points.new_empty((Pn, R) if want_beams else (0,), dtype=torch.float32),
            points.new_empty((Pn, R, 6) if want_beams else (0,), dtype=torch.float32))


@torch.library.custom_op(f"{NS}::refine_poses_map", mutates_args=())
def refine_poses_map(points: Tensor, poses12: Tensor, block_of_pose: Tensor, boxes6: Tensor, folds_coarse: Tensor,
                     folds_fine: Tensor, near: float, n_samples: int, n_importance: int, eps: float,
                     huber_delta: float, min_sumw: float, damping: float, xi_tol: float,
                     iters: int) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """refine_poses_fold with pose p refined against block block_of_pose[p] of the map, fixed for the call: the same
    bits per pose.  A pose without a block stops with status 2 at the first update and returns its input
    (pcnerf_refine_poses_map)."""
    op = "refine_poses_map"
    _layout(op, "points", points, (None, 3))
    _layout(op, "poses12", poses12, (None, 12), torch.float64)
    _layout(op, "block_of_pose", block_of_pose, (poses12.shape[0],), torch.int32)
    B = _check_map(op, boxes6, folds_coarse, folds_fine)
    check_score_samples(op, n_samples, n_importance)
    if iters < 0:
        raise RuntimeError(f"pcnerf::{op}: iters = {iters} is negative")
    _need_on_device(op, points, poses12, block_of_pose, boxes6, folds_coarse, folds_fine)
    R, Pn = points.shape[0], poses12.shape[0]
    dev = points.device
    out = torch.zeros((Pn, 12), dtype=torch.float64, device=dev)
    state = torch.zeros((Pn, LM_STATE_DOUBLES), dtype=torch.float64, device=dev)
    costs = torch.full((Pn, iters), float("nan"), dtype=torch.float64, device=dev)
    acc = torch.zeros((Pn, iters), dtype=torch.uint8, device=dev)
    n30 = torch.empty((max(Pn, 1), 30), dtype=torch.float64, device=dev)
    nbytes = int(H.lib().pcnerf_pose_normal_eq_workspace_bytes(Pn, R))
    ws = _ws(nbytes, dev)
    H.check(H.lib().pcnerf_refine_poses_map(points.data_ptr(), R, poses12.data_ptr(), Pn, block_of_pose.data_ptr(), B,
                                            boxes6.data_ptr(), float(near), int(n_samples), int(n_importance),
                                            folds_coarse.data_ptr(), folds_fine.data_ptr(), float(eps),
                                            float(huber_delta), float(min_sumw), float(damping), float(xi_tol),
                                            int(iters), ws.data_ptr(), nbytes, n30.data_ptr(), state.data_ptr(),
                                            out.data_ptr(), costs.data_ptr(), acc.data_ptr(), H.stream_of(points)))
    return out, state, costs, acc


@refine_poses_map.register_fake
def _(points, poses12, block_of_pose, boxes6, folds_coarse, folds_fine, near, n_samples, n_importance, eps,
      huber_delta, min_sumw, damping, xi_tol, iters):
    Pn = poses12.shape[0]
    return (points.new_empty((Pn, 12), dtype=torch.float64),
            points.new_empty((Pn, LM_STATE_DOUBLES), dtype=torch.float64),
            points.new_empty((Pn, iters), dtype=torch.float64), points.new_empty((Pn, iters), dtype=torch.uint8))


MCL_MAX_PARTICLES = 1 << 22   # pcnerf_mcl_weights / pcnerf_systematic_resample (re-reduced partials, serial chains)


@torch.library.custom_op(f"{NS}::mcl_weights", mutates_args=())
def mcl_weights(logw_prev: Tensor, scores4: Tensor, block_of_pose: Tensor, n_usable: Tensor, miss_cost: float,
                beta: float) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(w (P,), logw (P,), ess (1,) float64, best (1,), degenerate (1,) int32) of the particle weights
    logw = logw_prev - beta (cost + miss_cost (n_usable - n_valid)) / n_usable from the scores4 (P, 4) rows, -inf
    without a block or with a non-finite mean, normalised in float64 with fixed-order sums; ``n_usable`` is one
    float64 on the device.  No finite logw: uniform weights, logw 0, ess P, degenerate 1 (pcnerf_mcl_weights).
    Precondition: the ids are -1 .. B - 1 (assign_blocks' output); an id >= B is not known to be outside the map here
    and keeps the finite weight of a pose that missed every beam."""
    op = "mcl_weights"
    _layout(op, "logw_prev", logw_prev, (("min", 1),), torch.float64)
    Pn = logw_prev.shape[0]
    if Pn > MCL_MAX_PARTICLES:
        raise RuntimeError(f"pcnerf::{op}: {Pn} particles, at most {MCL_MAX_PARTICLES} are supported")
    _layout(op, "scores4", scores4, (Pn, 4), torch.float64)
    _layout(op, "block_of_pose", block_of_pose, (Pn,), torch.int32)
    _layout(op, "n_usable", n_usable, (1,), torch.float64)
    _need_on_device(op, logw_prev, scores4, block_of_pose, n_usable)
    dev = logw_prev.device
    w = torch.empty((Pn,), dtype=torch.float64, device=dev)
    logw = torch.empty((Pn,), dtype=torch.float64, device=dev)
    ess = torch.empty((1,), dtype=torch.float64, device=dev)
    best = torch.empty((1,), dtype=torch.int32, device=dev)
    deg = torch.empty((1,), dtype=torch.int32, device=dev)
    nbytes = int(H.lib().pcnerf_mcl_weights_workspace_bytes(Pn))
    ws = _ws(nbytes, dev)
    H.check(H.lib().pcnerf_mcl_weights(logw_prev.data_ptr(), scores4.data_ptr(), block_of_pose.data_ptr(), Pn,
                                       n_usable.data_ptr(), float(miss_cost), float(beta), ws.data_ptr(), nbytes,
                                       w.data_ptr(), logw.data_ptr(), ess.data_ptr(), best.data_ptr(), deg.data_ptr(),
                                       H.stream_of(logw_prev)))
    return w, logw, ess, best, deg


@mcl_weights.register_fake
def _(logw_prev, scores4, block_of_pose, n_usable, miss_cost, beta):
    Pn = logw_prev.shape[0]
    return (logw_prev.new_empty((Pn,)), logw_prev.new_empty((Pn,)), logw_prev.new_empty((1,)),
            logw_prev.new_empty((1,), dtype=torch.int32), logw_prev.new_empty((1,), dtype=torch.int32))


@torch.library.custom_op(f"{NS}::systematic_resample", mutates_args=())
def systematic_resample(w: Tensor, u0: Tensor, n_out: int, ess: Optional[Tensor], ess_threshold: float,
                        poses12: Optional[Tensor], block_of_pose: Optional[Tensor],
                        logw: Optional[Tensor]) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(ancestors (n_out,) int32, poses12_out (n_out, 12), blocks_out (n_out,) int32, logw_out (n_out,) float64; (0,)
    where the input is None) of systematic resampling of the weights w (P,) float64 with the offset u0 (1,) float64 in
    [0, 1) on the device: ancestor j is the first i whose inclusive prefix sum exceeds (j + u0) / n_out * sum(w),
    never an i with w_i == 0.  With ``ess`` (mcl_weights' (1,) output; the ESS switch, n_out == P) and
    ess >= ess_threshold, decided on the device, nothing is resampled: the identity, the log-weights kept; otherwise
    the new log-weights are 0 (pcnerf_systematic_resample)."""
    op = "systematic_resample"
    _layout(op, "w", w, (("min", 1),), torch.float64)
    Pn = w.shape[0]
    if Pn > MCL_MAX_PARTICLES:
        raise RuntimeError(f"pcnerf::{op}: {Pn} particles, at most {MCL_MAX_PARTICLES} are supported")
    _layout(op, "u0", u0, (1,), torch.float64)
    if n_out < 1:
        raise RuntimeError(f"pcnerf::{op}: n_out = {n_out}, at least one draw is needed")
    if ess is not None:
        _layout(op, "ess", ess, (1,), torch.float64)
        if n_out != Pn:
            raise RuntimeError(f"pcnerf::{op}: n_out = {n_out} != P = {Pn} with the ESS switch on (the identity needs "
                               "equal counts)")
    if poses12 is not None:
        _layout(op, "poses12", poses12, (Pn, 12), torch.float64)
    if block_of_pose is not None:
        _layout(op, "block_of_pose", block_of_pose, (Pn,), torch.int32)
    if logw is not None:
        _layout(op, "logw", logw, (Pn,), torch.float64)
    _need_on_device(op, w, u0, ess, poses12, block_of_pose, logw)
    dev = w.device
    anc = torch.empty((n_out,), dtype=torch.int32, device=dev)
    pout = torch.empty((n_out, 12) if poses12 is not None else (0,), dtype=torch.float64, device=dev)
    bout = torch.empty((n_out,) if block_of_pose is not None else (0,), dtype=torch.int32, device=dev)
    lout = torch.empty((n_out,) if logw is not None else (0,), dtype=torch.float64, device=dev)
    nbytes = int(H.lib().pcnerf_systematic_resample_workspace_bytes(Pn))
    ws = _ws(nbytes, dev)
    H.check(H.lib().pcnerf_systematic_resample(w.data_ptr(), Pn, u0.data_ptr(), int(n_out), H.ptr(ess),
                                               float(ess_threshold), H.ptr(poses12), H.ptr(block_of_pose),
                                               H.ptr(logw), ws.data_ptr(), nbytes, anc.data_ptr(),
                                               pout.data_ptr() if poses12 is not None else None,
                                               bout.data_ptr() if block_of_pose is not None else None,
                                               lout.data_ptr() if logw is not None else None, H.stream_of(w)))
    return anc, pout, bout, lout


@systematic_resample.register_fake
def _(w, u0, n_out, ess, ess_threshold, poses12, block_of_pose, logw):
    return (w.new_empty((n_out,), dtype=torch.int32),
            w.new_empty((n_out, 12) if poses12 is not None else (0,), dtype=torch.float64),
            w.new_empty((n_out,) if block_of_pose is not None else (0,), dtype=torch.int32),
            w.new_empty((n_out,) if logw is not None else (0,), dtype=torch.float64))


def map_op_names() -> list:
    """The operators of the map and particle-filter layer (tests)."""
    return ["assign_blocks", "score_poses_map", "pose_normal_eq_map", "refine_poses_map", "mcl_weights",
            "systematic_resample"]


# ----------------------------------------------------------------------------------------------- through the blocks
# score_poses_map with every beam carried on through the blocks it crosses (include/pcnerf_hip.h).  Reads no
# process-wide selector.
THROUGH_MAX_SEGMENTS = 16


def check_through_params(op: str, max_segments: int, seam_tol: float, min_transmittance: float) -> None:
    if not 1 <= max_segments <= THROUGH_MAX_SEGMENTS:
        raise RuntimeError(f"pcnerf::{op}: max_segments = {max_segments}, must be 1 .. {THROUGH_MAX_SEGMENTS}")
    if not seam_tol >= 0.0:
        raise RuntimeError(f"pcnerf::{op}: seam_tol = {seam_tol}, must be >= 0")
    if not 0.0 <= min_transmittance < 1.0:
        raise RuntimeError(f"pcnerf::{op}: min_transmittance = {min_transmittance}, must be in [0, 1)")


@torch.library.custom_op(f"{NS}::score_poses_through", mutates_args=())
def score_poses_through(points: Tensor, poses12: Tensor, block_of_pose: Tensor, boxes6: Tensor, folds_coarse: Tensor,
                        folds_fine: Tensor, near: float, n_samples: int, n_importance: int, eps: float,
                        huber_delta: float, min_sumw: float, max_segments: int, seam_tol: float,
                        min_transmittance: float,
                        want_beams: bool) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """score_poses_map with every beam carried through up to max_segments blocks, block_of_pose[p] first: (scores4,
    depth, sumw (P, R) float32, n_segments, last_block (P, R) int32), the four per-beam tensors (0,) unless
    want_beams.  A beam of one segment has score_poses_map's bits; a pose without a block gets a zero scores4 row, NaN
    depth, zero sumw, n_segments 0 and last_block -1 (pcnerf_score_poses_through)."""
    op = "score_poses_through"
    _layout(op, "points", points, (None, 3))
    _layout(op, "poses12", poses12, (None, 12), torch.float64)
    _layout(op, "block_of_pose", block_of_pose, (poses12.shape[0],), torch.int32)
    B = _check_map(op, boxes6, folds_coarse, folds_fine)
    check_score_samples(op, n_samples, n_importance)
    check_through_params(op, int(max_segments), float(seam_tol), float(min_transmittance))
    _need_on_device(op, points, poses12, block_of_pose, boxes6, folds_coarse, folds_fine)
    R, Pn = points.shape[0], poses12.shape[0]
    dev = points.device
    scores = torch.empty((Pn, 4), dtype=torch.float64, device=dev)
    shape = (Pn, R) if want_beams else (0,)
    depth = torch.empty(shape, dtype=torch.float32, device=dev)
    sumw = torch.empty(shape, dtype=torch.float32, device=dev)
    nseg = torch.empty(shape, dtype=torch.int32, device=dev)
    last = torch.empty(shape, dtype=torch.int32, device=dev)
    nbytes = int(H.lib().pcnerf_score_poses_workspace_bytes(Pn, R))
    ws = _ws(nbytes, dev)
    H.check(H.lib().pcnerf_score_poses_through(
        points.data_ptr(), R, poses12.data_ptr(), Pn, block_of_pose.data_ptr(), B, boxes6.data_ptr(), float(near),
        int(n_samples), int(n_importance), folds_coarse.data_ptr(), folds_fine.data_ptr(), float(eps),
        float(huber_delta), float(min_sumw), int(max_segments), float(seam_tol), float(min_transmittance),
        ws.data_ptr(), nbytes, scores.data_ptr(), depth.data_ptr() if want_beams else None,
        sumw.data_ptr() if want_beams else None, nseg.data_ptr() if want_beams else None,
        last.data_ptr() if want_beams else None, H.stream_of(points)))
    return scores, depth, sumw, nseg, last


@score_poses_through.register_fake
def _(points, poses12, block_of_pose, boxes6, folds_coarse, folds_fine, near, n_samples, n_importance, eps,
      huber_delta, min_sumw, max_segments, seam_tol, min_transmittance, want_beams):
    R, Pn = points.shape[0], poses12.shape[0]
    shape = (Pn, R) if want_beams else (0,)
    return (points.new_empty((Pn, 4), dtype=torch.float64), points.new_empty(shape, dtype=torch.float32),
            points.new_empty(shape, dtype=torch.float32), points.new_empty(shape, dtype=torch.int32),
            points.new_empty(shape, dtype=torch.int32))


def through_op_names() -> list:
    """The operator of the render carried through the blocks (tests)."""
    return ["score_poses_through"]
