"""Autograd bindings of the training path: loss.backward() of the reference's training step
(train_kitti.py:117-155, returned to Lightning) through the HIP kernels.

torch.autograd.Functions, each owning one forward kernel chain and its hand-written backward:
  * TrainPass -- one render pass of render_rays_train (render.py:38-163, 416-482): train-mode query + compositing
    + child losses.  Outputs (weights [non-differentiable], depth, child_free_loss, child_depth_loss); backward =
    pcnerf_composite_backward (dL/dlogit) -> pcnerf_nof_query_train_backward (parameter gradients, chunks
    recomputed).  The fine samples are detached from the coarse weights exactly as render.py:466 does.
  * TrainPassPoints -- the same pass on materialised sample positions (inference_train, render.py:38-163): the
    point-sourced fused query and its rematerialised backward (pcnerf_nof_points_train_fused_state /
    pcnerf_nof_points_train_backward_remat).  TrainPass's behaviour and saved tensors are untouched by it.
  * NofForward -- NOF.forward on an embedded batch (models.py:183-203): train mode, or eval mode with the frozen
    running statistics (pcnerf_nof_forward_eval_param_backward).
  * FrozenPass / FrozenPassPoints -- TrainPass / TrainPassPoints for an EVAL-mode module whose parameters require
    grad (frozen-BatchNorm training: model.eval() keeps the running statistics, every weight trains).  The eval
    network is a(theta) . e + c(theta), so the parameter gradients of a pass are those of one float64 pseudo-sample
    with input sum_s g_s e_s: backward = pcnerf_composite_backward -> pcnerf::eval_gmoments_* ->
    pcnerf::eval_param_grads.  No activations, state or rematerialisation; running statistics and
    num_batches_tracked are not touched; the Linear-bias and BatchNorm-shift gradients are not zero here.
  * EvalPass / EvalPassPoints -- one eval-mode pass of render_rays_val / inference_val (render.py:485-536, :13-36) on
    a FROZEN network, with the gradient of depth to rays[:, 0:6] / to samples_xy: backward =
    pcnerf_composite_backward -> pcnerf_nof_query_eval_backward / pcnerf_nof_points_eval_backward.
In the train-mode and the Frozen* Functions gradients flow to the 34 trainable tensors of the network and the inputs
(rays, positions) get none, as in the reference's training step where they never require grad; in EvalPass /
EvalPassPoints the geometry gets the gradient and the parameters none.
"""
from __future__ import annotations

import torch

from . import _ops


class TrainPass(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, rays, z, noise, noise_std, eps, chunk, with_losses, sub_num, *params):
        # a chunk larger than the pass is the same single BatchNorm chunk: size workspaces and store by the pass
        chunk = max(1, min(int(chunk), z.numel()))
        ctx.store = ctx.fold = ctx.state = None
        if _ops.train_fold_enabled():   # opt-in exact affine fold: per-chunk moments + layer maps, no activations
            ctx.fold = _ops.fold_state(z.device, z.numel(), chunk)
            p = _ops.query(model, rays, z, chunk, fold=ctx.fold)
        elif _ops.remat_enabled():
            # default: no activations kept -- the fused query's state (moments + layer maps, ~3 MB per chunk) only;
            # the backward rematerialises every layer input from the encoding
            ctx.state = _ops.fold_state(z.device, z.numel(), chunk)
            p = _ops.query(model, rays, z, chunk, keep=ctx.state)
        else:
            # keep the chunks' layer outputs for the backward in the HBM left after its workspace (+ 4 GiB margin)
            L = _ops.H.lib()
            reserve = int(L.pcnerf_nof_backward_workspace_bytes(int(chunk))) + (4 << 30)
            ctx.store = _ops.ActivationStore(z.device, z.numel(), chunk, reserve)
            p = _ops.query(model, rays, z, chunk, ctx.store)
        w, depth, fr, sl = _ops.composite(p, z, noise, noise_std, eps, rays if with_losses else None)
        if with_losses:
            free, dl = _ops.child_losses(fr, sl, rays, sub_num > 0, sub_num)
        else:
            free = dl = torch.zeros((), dtype=torch.float32, device=z.device)
        ctx.model, ctx.noise_std, ctx.eps, ctx.chunk = model, noise_std, eps, chunk
        ctx.with_losses, ctx.sub_num = with_losses, sub_num
        ctx.save_for_backward(rays, z, p, noise)
        ctx.mark_non_differentiable(w)
        return w, depth, free, dl

    @staticmethod
    def backward(ctx, g_w, g_depth, g_free, g_dl):
        rays, z, p, noise = ctx.saved_tensors
        if not ctx.with_losses:
            g_free = g_dl = None
        g_logit = _ops.composite_backward(p, z, noise, ctx.noise_std, ctx.eps, rays if ctx.with_losses else None,
                                          ctx.sub_num, g_depth, g_free, g_dl)
        if ctx.fold is not None:
            grads = _ops.nof_query_backward_fold(ctx.model, rays, z, ctx.chunk, g_logit, ctx.fold)
            ctx.fold = None
        elif ctx.state is not None:
            grads = _ops.nof_query_backward_remat(ctx.model, rays, z, ctx.chunk, g_logit, ctx.state)
            ctx.state = None
        else:
            grads = _ops.nof_query_backward(ctx.model, rays, z, ctx.chunk, g_logit, ctx.store)
            ctx.store.release()
        return (None,) * 9 + tuple(grads)


class TrainPassPoints(torch.autograd.Function):
    """TrainPass on explicit sample positions (inference_train, render.py:38-163): ``pts`` (R * S, 3) are the
    materialised samples, ``table`` the per-ray scalars the compositing and child-loss kernels read by column (child id
    9, near_far_child 10:12, range_readings 14; unused without the losses).  Default train math and backward only
    (nof._ops.query_points raises otherwise); no gradient flows to the positions."""

    @staticmethod
    def forward(ctx, model, pts, table, z, noise, noise_std, eps, chunk, with_losses, sub_num, *params):
        chunk = max(1, min(int(chunk), z.numel()))
        ctx.state = _ops.fold_state(z.device, z.numel(), chunk)
        p = _ops.query_points(model, pts, z.shape[0], z.shape[1], chunk, keep=ctx.state)
        w, depth, fr, sl = _ops.composite(p, z, noise, noise_std, eps, table if with_losses else None)
        if with_losses:
            free, dl = _ops.child_losses(fr, sl, table, sub_num > 0, sub_num)
        else:
            free = dl = torch.zeros((), dtype=torch.float32, device=z.device)
        ctx.model, ctx.noise_std, ctx.eps, ctx.chunk = model, noise_std, eps, chunk
        ctx.with_losses, ctx.sub_num = with_losses, sub_num
        ctx.save_for_backward(pts, table, z, p, noise)
        ctx.mark_non_differentiable(w)
        return w, depth, free, dl

    @staticmethod
    def backward(ctx, g_w, g_depth, g_free, g_dl):
        pts, table, z, p, noise = ctx.saved_tensors
        if not ctx.with_losses:
            g_free = g_dl = None
        g_logit = _ops.composite_backward(p, z, noise, ctx.noise_std, ctx.eps, table if ctx.with_losses else None,
                                          ctx.sub_num, g_depth, g_free, g_dl)
        if ctx.state is None:
            raise RuntimeError("the point query's state was consumed by an earlier backward")
        grads = _ops.nof_points_backward_remat(ctx.model, pts, ctx.chunk, g_logit, ctx.state)
        ctx.state = None
        return (None,) * 10 + tuple(grads)


def _eval_fold(model) -> torch.Tensor:
    """(a, c) of the frozen eval network (pcnerf::fold_eval): d logit / d encoding is the constant a."""
    from . import _torch_ops
    _ops._bn_config(model)
    return torch.ops.pcnerf.fold_eval([t.detach() for t in _torch_ops.eval_params(model)])


class EvalPass(torch.autograd.Function):
    """One eval-mode pass of render_rays_val (render.py:512-533) with the gradient of depth to the ray origins and
    directions: forward = the renderer's own eval query (``query``, whatever eval path is selected) + compositing,
    the calls and so the bits of the forward-only render; backward = pcnerf_composite_backward (dL/dlogit from
    dL/ddepth) -> pcnerf_nof_query_eval_backward.  The eval network is sigmoid(a . e + c), so its
    Jacobian to the encoding is the fold vector a whichever eval math computed p; it is composed once per pass and
    saved.  z is a constant of the pass; the parameters are frozen (no gradient to them); weights are
    non-differentiable (the compositing backward takes grad_depth only)."""

    @staticmethod
    def forward(ctx, query, model, rays, z, noise, noise_std, eps, chunk, want_weights):
        p = query(model, rays, z, chunk)
        w, depth, _, _ = torch.ops.pcnerf.composite(p, z, noise, noise_std, eps, None, 10, 11, 14, want_weights)
        ctx.noise_std, ctx.eps = noise_std, eps
        ctx.save_for_backward(rays, z, p, noise, _eval_fold(model))
        ctx.mark_non_differentiable(w)
        return w, depth

    @staticmethod
    def backward(ctx, g_w, g_depth):
        rays, z, p, noise, fold = ctx.saved_tensors
        g_logit = _ops.composite_backward(p, z, noise, ctx.noise_std, ctx.eps, None, 0, g_depth, None, None)
        g_rays = torch.zeros_like(rays)   # every column but the origin and the direction: zero
        g_rays[:, :6] = torch.ops.pcnerf.rays_grad_eval(rays, z, g_logit, fold)
        return (None, None, g_rays) + (None,) * 6


class EvalPassPoints(torch.autograd.Function):
    """EvalPass on explicit sample positions (inference_val, render.py:13-36): ``pts`` (R * S, 3) are the
    materialised samples, read verbatim; the gradient of depth goes to them (pcnerf_nof_points_eval_backward)."""

    @staticmethod
    def forward(ctx, query_points, model, pts, z, noise, noise_std, eps, chunk):
        p = query_points(model, pts, z.shape[0], z.shape[1], chunk)
        w, depth, _, _ = torch.ops.pcnerf.composite(p, z, noise, noise_std, eps, None, 10, 11, 14, True)
        ctx.noise_std, ctx.eps = noise_std, eps
        ctx.save_for_backward(pts, z, p, noise, _eval_fold(model))
        ctx.mark_non_differentiable(w)
        return w, depth

    @staticmethod
    def backward(ctx, g_w, g_depth):
        pts, z, p, noise, fold = ctx.saved_tensors
        g_logit = _ops.composite_backward(p, z, noise, ctx.noise_std, ctx.eps, None, 0, g_depth, None, None)
        return (None, None, torch.ops.pcnerf.points_grad_eval(pts, g_logit.view(-1), fold)) + (None,) * 5


def _frozen_param_grads(model, mom) -> tuple:
    """pcnerf::eval_param_grads on the module's tensors: the 34 gradients in grad_params order."""
    from . import _torch_ops
    _, bn_eps = _ops._bn_config(model)
    return tuple(torch.ops.pcnerf.eval_param_grads([t.detach() for t in _torch_ops.eval_params(model)], mom, bn_eps))


class FrozenPass(torch.autograd.Function):
    """One pass of render_rays_train (render.py:38-163, 416-482) on an EVAL-mode module whose parameters require grad
    (frozen BatchNorm: the running statistics normalise and are not touched).  forward = the renderer's own eval
    query (``query``, whatever eval path is selected) + compositing + child losses, the calls and so the bits of the
    no-grad render.  backward = pcnerf_composite_backward (dL/dlogit) -> pcnerf::eval_gmoments_rays (the pass's
    moments sum_s g_s e_s, sum_s g_s) -> pcnerf::eval_param_grads (one float64 pseudo-sample): the eval network is
    a(theta) . e + c(theta), so no activation, state or rematerialisation is needed -- it saves what
    TrainPass saves, minus the state.  Outputs as TrainPass; the rays get no gradient."""

    @staticmethod
    def forward(ctx, query, model, rays, z, noise, noise_std, eps, chunk, with_losses, divide, sub_num, *params):
        P = torch.ops.pcnerf
        p = query(model, rays, z, chunk)
        w, depth, fr, sl = P.composite(p, z, noise, noise_std, eps, rays if with_losses else None, 10, 11, 14, True)
        if with_losses:
            free, dl = P.child_losses(fr, sl, rays, divide, sub_num)
        else:
            free = dl = torch.zeros((), dtype=torch.float32, device=z.device)
        ctx.model, ctx.noise_std, ctx.eps = model, noise_std, eps
        ctx.with_losses, ctx.sub = with_losses, (sub_num if divide else 0)
        ctx.save_for_backward(rays, z, p, noise)
        ctx.mark_non_differentiable(w)
        return w, depth, free, dl

    @staticmethod
    def backward(ctx, g_w, g_depth, g_free, g_dl):
        rays, z, p, noise = ctx.saved_tensors
        if not ctx.with_losses:
            g_free = g_dl = None
        g_logit = _ops.composite_backward(p, z, noise, ctx.noise_std, ctx.eps, rays if ctx.with_losses else None,
                                          ctx.sub, g_depth, g_free, g_dl)
        mom = torch.ops.pcnerf.eval_gmoments_rays(rays, z, g_logit)
        return (None,) * 11 + _frozen_param_grads(ctx.model, mom)


class FrozenPassPoints(torch.autograd.Function):
    """FrozenPass on explicit sample positions (inference_train, render.py:38-163): ``pts`` (R * S, 3) read verbatim,
    ``table`` the per-ray scalars of TrainPassPoints; the moments come from pcnerf::eval_gmoments_points.  No
    gradient flows to the positions."""

    @staticmethod
    def forward(ctx, query_points, model, pts, table, z, noise, noise_std, eps, chunk, with_losses, divide, sub_num,
                *params):
        P = torch.ops.pcnerf
        p = query_points(model, pts, z.shape[0], z.shape[1], chunk)
        w, depth, fr, sl = P.composite(p, z, noise, noise_std, eps, table, 10, 11, 14, True)
        if with_losses:
            free, dl = P.child_losses(fr, sl, table, divide, sub_num)
        else:
            free = dl = torch.zeros((), dtype=torch.float32, device=z.device)
        ctx.model, ctx.noise_std, ctx.eps = model, noise_std, eps
        ctx.with_losses, ctx.sub = with_losses, (sub_num if divide else 0)
        ctx.save_for_backward(pts, table, z, p, noise)
        ctx.mark_non_differentiable(w)
        return w, depth, free, dl

    @staticmethod
    def backward(ctx, g_w, g_depth, g_free, g_dl):
        pts, table, z, p, noise = ctx.saved_tensors
        if not ctx.with_losses:
            g_free = g_dl = None
        g_logit = _ops.composite_backward(p, z, noise, ctx.noise_std, ctx.eps, table if ctx.with_losses else None,
                                          ctx.sub, g_depth, g_free, g_dl)
        mom = torch.ops.pcnerf.eval_gmoments_points(pts, g_logit.view(-1))
        return (None,) * 12 + _frozen_param_grads(ctx.model, mom)


def check_frozen_eval(model, what: str) -> None:
    """The geometry gradient exists for the frozen eval network only: train-mode BatchNorm takes its statistics from
    the batch, which couples every sample's output to every other sample's position."""
    if model.training:
        raise NotImplementedError(f"no gradient flows to {what} through a train-mode module: BatchNorm batch "
                                  "statistics couple the samples; call model.eval() (frozen parameters) or detach "
                                  f"{what}")


class NofForward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        ctx.frozen = not model.training
        if ctx.frozen:   # eval mode: the no-grad call itself (any eval path); nothing but x and p is kept
            p, ctx.fold = _ops.nof_forward_embedded(model, x), None
        else:
            p, ctx.fold = _ops.nof_forward_embedded(model, x, with_fold_state=True)
        ctx.model = model
        ctx.save_for_backward(x, p)
        return p

    @staticmethod
    def backward(ctx, g_p):
        x, p = ctx.saved_tensors
        if ctx.frozen:
            grads = _ops.nof_forward_eval_param_backward(ctx.model, x, p.reshape(-1), g_p.contiguous().reshape(-1))
        elif ctx.fold is not None:
            grads = _ops.nof_forward_backward_fold(ctx.model, x, p.reshape(-1), g_p.contiguous().reshape(-1),
                                                   ctx.fold)
            ctx.fold = None
        else:
            grads = _ops.nof_forward_backward(ctx.model, x, p.reshape(-1), g_p.contiguous().reshape(-1))
        return (None, None) + tuple(grads)


class ChildRangeLoss(torch.autograd.Function):
    """Per-child range loss of train_kitti.py:125-142 (divide branch) with d/dpred."""

    @staticmethod
    def forward(ctx, pred, target, rays, sub_num, kind, pre, post):
        out, ws = _ops.child_range_loss(pred, target, rays, sub_num, kind, pre, post)
        ctx.args = (sub_num, kind, pre, post)
        ctx.save_for_backward(pred, target, rays, ws)
        return out

    @staticmethod
    def backward(ctx, g):
        pred, target, rays, ws = ctx.saved_tensors
        gp = _ops.child_range_loss_backward(pred, target, rays, *ctx.args, ws, g.contiguous())
        return (gp.reshape(pred.shape),) + (None,) * 6


def needs_grad(model) -> bool:
    return torch.is_grad_enabled() and any(t.requires_grad for t in model.parameters())


def check_trainable(model) -> None:
    """Parameter gradients through the HIP NOF kernels exist in both BatchNorm modes, decided per module: train mode
    (batch statistics: TrainPass / TrainPassPoints / NofForward's rematerialised backward) and eval mode (frozen
    running statistics: FrozenPass / FrozenPassPoints / NofForward's eval branch).  What either needs is the uniform
    affine BatchNorm1d configuration with running statistics the kernels implement."""
    try:
        _ops._bn_config(model)
    except NotImplementedError as e:
        mode = "train-mode" if model.training else "eval-mode (frozen BatchNorm)"
        raise NotImplementedError(f"no {mode} parameter gradients through the HIP NOF kernels for this module: {e}; "
                                  "use torch.no_grad()") from e
