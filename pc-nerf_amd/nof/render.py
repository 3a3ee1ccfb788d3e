"""PC-NeRF LiDAR volume rendering -- drop-in for ``nof/render.py`` of the reference, on MI355X HIP kernels.

Same function names, signatures, result keys, shapes and dtypes as the reference.  Each stage is a kernel of
lib/libpcnerf_hip.so (see include/pcnerf_hip.h):

    coarse z sampling (+segmented merge)  pcnerf_sample_coarse      render.py:429-442
    stratified perturbation               pcnerf_perturb            render.py:449-454
    Embedding + NOF query (chunked BN)    pcnerf_nof_query_*        render.py:18-25 / 44-51, models.py
    compositing, child masks, loss terms  pcnerf_composite          render.py:51-61, 75-159
    sample_pdf + sort(cat(z, samples))    pcnerf_resample           render.py:371-412, 463-467
    child loss reductions                 pcnerf_child_loss_reduce  render.py:102-159
    query of materialised samples_xy      pcnerf_nof_points_*       render.py:13-25, 38-51, 166-201, 229-241
      (inference_val / inference_train / inference / inference_0525_2: the positions are read verbatim)

Differences from the reference, all deliberate:
  * everything stays on ``rays.device`` (the reference pins ``u`` to ``cuda:0``, render.py:397);
  * RNG: draws are taken from torch's generator on the device, and only when used (the reference also draws
    ``randn`` noise when ``noise_std == 0``).  Parity tests inject the draws with the keyword-only ``rng``
    dict: ``perturb_rand`` (R,S), ``noise`` (R,S), ``u`` (R,I), ``noise_fine`` (R,S+I);
  * gradients: ``render_rays_train`` is differentiable (train-mode networks): with autograd enabled and
    parameters requiring grad, each pass runs as ``nof._autograd.TrainPass`` whose backward is the HIP
    compositing backward + the NOF backward (chunks recomputed), so ``loss.backward()`` of train_kitti.py:155
    fills ``.grad`` of both networks.  An EVAL-mode module whose parameters require grad trains with frozen
    BatchNorm (running statistics used and left untouched), decided per module: its pass of ``render_rays_train`` /
    ``inference_train`` runs as ``nof._autograd.FrozenPass`` / ``FrozenPassPoints`` -- the eval query of the
    no-grad call (same output bits), then compositing backward + pcnerf::eval_gmoments_* +
    pcnerf::eval_param_grads.  ``render_rays_val`` and ``inference_val`` are differentiable with respect
    to their GEOMETRY on frozen eval-mode networks: when ``rays`` / ``samples_xy`` requires grad, each pass runs as
    ``nof._autograd.EvalPass`` / ``EvalPassPoints``, whose backward is the HIP compositing backward + the eval
    network's position gradient (pcnerf_nof_query_eval_backward / pcnerf_nof_points_eval_backward), so
    ``depth.backward()`` reaches ``rays[:, 0:6]`` / ``samples_xy`` as it does through the reference's eager eval
    render.  Sample depths are constants there.  The other renderers (``render_rays``, ``inference``,
    ``inference_0525_2``, the two-step view render) stay forward-only: their peak selection and ``depth2`` are not
    differentiable in any useful sense; parameters that require grad raise in every eval renderer.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _autograd, _ops
from . import _torch_ops
from .networks import NOF, Embedding, NOF_coarse, NOF_fine, NOF_plusfine  # noqa: F401  (reference exports)

__all__ = ['render_rays']

EPSILON = 1e-10  # render.py:456, :514, :656
# the tensor-level stages go through the registered operators (nof._torch_ops): torch's dispatcher, FakeTensor
# tracing and torch.compile see them as graph nodes
P = torch.ops.pcnerf


def _query(model, rays, z, chunk):
    """The NOF query of one pass: eval mode through pcnerf::pack_eval + pcnerf::query_eval (the module's tensors
    are operator inputs); train mode and the opt-in eval fold through nof._ops.query (module-level state: BatchNorm
    running statistics, chunk moments)."""
    if not model.training and not _ops.eval_fold_enabled():
        _ops._bn_config(model)
        return P.query_eval(rays, z, P.pack_eval(_torch_ops.eval_params(model)))
    return _ops.query(model, rays, z, chunk)


def _check_inputs(model, model_fine, embedding_xy, rays, n_cols, differentiable=False):
    if not rays.is_cuda:
        raise RuntimeError("nof.render (HIP) renders device-resident rays; move them with rays.to('cuda') -- there "
                           "is no CPU path")
    if rays.dim() != 2 or rays.shape[1] < n_cols:
        raise RuntimeError(f"rays must be (N_rays, >={n_cols}); got {tuple(rays.shape)}")
    if embedding_xy is not None and not embedding_xy.supported():
        raise NotImplementedError("HIP render supports Embedding(3, 10) (L_pos = 10)")
    for m in (model, model_fine):
        if not m.supported():
            raise NotImplementedError("HIP render supports NOF(feature_size=256, in_channels_xy=63, use_skip=True)")
        if _autograd.needs_grad(m):
            if not differentiable:
                raise NotImplementedError("this HIP renderer is forward-only (inference); call it under "
                                          "torch.no_grad()")
            _autograd.check_trainable(m)
    return rays.float().contiguous()


def _draw(rng, key, shape, device, fn):
    if rng is not None and key in rng:
        t = rng[key]
        return t.to(device=device, dtype=torch.float32).contiguous()
    return fn(shape, device=device)


def _coarse(rays, N_samples, segmented, ratio, perturb, rng):
    """render.py:429-454."""
    R = rays.shape[0]
    n_parent = int(N_samples * (1 - ratio)) if segmented else N_samples
    z = P.sample_coarse(rays, N_samples, n_parent, 6, 7, 10, 11, False)
    if perturb > 0:
        z = P.perturb(z, float(perturb), _draw(rng, "perturb_rand", (R, N_samples), rays.device, torch.rand))
    return z


def _noise(rng, key, z, noise_std):
    if noise_std == 0:
        return None
    return _draw(rng, key, tuple(z.shape), z.device, torch.randn)


def sample_pdf(bins, weights, N_samples, det=False, pytest=False, *, u=None):
    """render.py:371-412: inverse-CDF samples, unsorted, ``bins`` (R, B), ``weights`` (R, B-1) -> (R, N).
    ``u`` (keyword-only) injects the uniform draws when ``det`` is False.

    ``pytest=True`` is the reference's test hook (render.py:386-394): ``np.random.seed(0)`` (numpy's global
    generator, as the reference seeds it), then ``u`` = float32 of ``np.linspace(0, 1, N)`` (det) or of
    ``np.random.rand(R, N)``; the draws are made on the host and uploaded, the sampling itself runs on the device.
    With ``det`` False the reference first draws (and discards) ``torch.rand`` from torch's CPU generator
    (render.py:383); that draw is made here too, so torch's global RNG state afterwards is the reference's."""
    if pytest:
        R = bins.shape[0]
        if not det:   # render.py:383 draws u from torch's CPU generator before the numpy overwrite: consume it too
            torch.rand((R, N_samples))
        np.random.seed(0)
        if det:
            hu = np.broadcast_to(np.linspace(0., 1., N_samples), (R, N_samples))
        else:
            hu = np.random.rand(R, N_samples)
        u = torch.from_numpy(np.ascontiguousarray(hu, dtype=np.float32)).to(bins.device)
        det = False   # the uploaded draws are used as given (the linspace is numpy's, float64 rounded to float32)
    return P.sample_pdf(bins, weights, int(N_samples), bool(det), u)


# ----------------------------------------------------------------------------------------------- inference_*
# The reference's module-level helpers (render.py:13, :38, :166, :229): they take MATERIALISED sample positions
# samples_xy (R, S, 3) and a separate z_vals (R, S); the positions need not lie on any ray.  The query reads them
# verbatim through the point-sourced fused kernels (pcnerf_nof_points_*), everything after it is the renderers'
# kernels on a small per-ray table built on the device.
def _query_points(model, pts, R, S, chunk):
    """_query on explicit positions: eval mode through pcnerf::query_points_eval, train mode and the opt-in eval
    paths (fold, fp32 math: embed + embedded forward) through nof._ops.query_points."""
    if not model.training and not _ops.eval_fold_enabled() and _ops.get_eval_math() == "f16x2_3":
        _ops._bn_config(model)
        return P.query_points_eval(pts.view(R, S, 3), P.pack_eval(_torch_ops.eval_params(model)))
    return _ops.query_points(model, pts, R, S, chunk)


def _check_points_inputs(model, embedding_xy, samples_xy, z_vals, near_far_child=None, differentiable=False,
                         points_grad=False):
    """_check_inputs for the inference_* helpers -> (pts (R * S, 3), z (R, S)) contiguous float32.  ``points_grad``
    (inference_val): samples_xy may require grad; under autograd pts then stays attached to it."""
    for name, t in (("samples_xy", samples_xy), ("z_vals", z_vals), ("near_far_child", near_far_child)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f"nof.render (HIP) takes device-resident tensors; move {name} with .to('cuda') -- "
                               "there is no CPU path")
    if samples_xy.dim() != 3 or samples_xy.shape[2] != 3 or samples_xy.numel() == 0:
        raise RuntimeError(f"samples_xy must be (N_rays, N_samples, 3); got {tuple(samples_xy.shape)}")
    R, S = samples_xy.shape[:2]
    if tuple(z_vals.shape) != (R, S):
        raise RuntimeError(f"z_vals must be (N_rays, N_samples) = ({R}, {S}); got {tuple(z_vals.shape)}")
    if near_far_child is not None and tuple(near_far_child.shape) != (R, 2):
        raise RuntimeError(f"near_far_child must be (N_rays, 2) = ({R}, 2); got {tuple(near_far_child.shape)}")
    if embedding_xy is not None and not embedding_xy.supported():
        raise NotImplementedError("HIP render supports Embedding(3, 10) (L_pos = 10)")
    if not model.supported():
        raise NotImplementedError("HIP render supports NOF(feature_size=256, in_channels_xy=63, use_skip=True)")
    if _autograd.needs_grad(model):
        if not differentiable:
            raise NotImplementedError("this HIP inference helper is forward-only; call it under torch.no_grad()")
        _autograd.check_trainable(model)
    if samples_xy.requires_grad and not points_grad:
        raise NotImplementedError("no gradient flows to samples_xy through this HIP helper (inference_val alone "
                                  "differentiates its positions, on a frozen eval-mode module); detach it")
    if points_grad and torch.is_grad_enabled() and samples_xy.requires_grad:
        if z_vals.requires_grad:
            raise NotImplementedError("z_vals is a constant of the HIP eval render: no gradient flows to it; "
                                      "detach it (the gradient goes to samples_xy)")
        _autograd.check_frozen_eval(model, "samples_xy")
        return samples_xy.float().contiguous().view(-1, 3), z_vals.detach().float().contiguous()
    return samples_xy.detach().float().contiguous().view(-1, 3), z_vals.detach().float().contiguous()


def inference_val(model: NOF, embedding_xy: Embedding, samples_xy: torch.Tensor, rays: torch.Tensor,
                  z_vals: torch.Tensor, near_far_child: torch.Tensor, near_far_point: torch.Tensor,
                  range_readings: torch.Tensor, ray_class: torch.Tensor, chunk=1024 * 32, noise_std=1, epsilon=1e-10,
                  isval=False, sub_nerf_test_num=4, *, rng=None):
    """render.py:13-36 -> (depth_final (R,), weights_origin (R, S)).  ``rays``, ``near_far_point``,
    ``range_readings``, ``ray_class``, ``isval`` and ``sub_nerf_test_num`` are accepted and unused, as in the
    reference.  ``rng["noise"]`` (R, S) injects the randn draw (taken only when noise_std != 0).

    Differentiable with respect to ``samples_xy`` when it requires grad, on a frozen eval-mode module
    (``depth_final.backward()`` fills ``samples_xy.grad`` as the reference's eager render does): the pass runs as
    nof._autograd.EvalPassPoints.  ``weights_origin`` carries no gradient, ``z_vals`` is a constant (it raises if it
    requires grad), a train-mode module raises (batch statistics couple the samples) and parameters that require
    grad raise as before.  Without a tensor requiring grad the calls, and the outputs' bits, are the forward-only
    ones."""
    pts, z = _check_points_inputs(model, embedding_xy, samples_xy, z_vals, near_far_child, points_grad=True)
    if pts.requires_grad:
        w, depth = _autograd.EvalPassPoints.apply(_query_points, model, pts, z, _noise(rng, "noise", z, noise_std),
                                                  float(noise_std), float(epsilon), int(chunk))
        return depth, w
    p = _query_points(model, pts, z.shape[0], z.shape[1], chunk)
    w, depth, _, _ = P.composite(p, z, _noise(rng, "noise", z, noise_std), float(noise_std), float(epsilon), None,
                                 10, 11, 14, True)
    return depth, w


def _child_table(rays, near_far_child, range_readings, R, divide):
    """The (R, 15) per-ray table the compositing / child-loss kernels read by column: child id (rays[:, 9], divide
    branch only) in column 9, near_far_child in 10:12, range_readings in 14."""
    table = torch.zeros((R, 15), dtype=torch.float32, device=near_far_child.device)
    table[:, 10:12] = near_far_child
    if not (torch.is_tensor(range_readings) and range_readings.is_cuda):
        raise RuntimeError("nof.render (HIP) takes device-resident tensors; move range_readings with .to('cuda')")
    if range_readings.numel() != R:
        raise RuntimeError(f"range_readings must have one entry per ray ({R}); got {tuple(range_readings.shape)}")
    table[:, 14] = range_readings.reshape(-1)
    if divide:
        if not (torch.is_tensor(rays) and rays.is_cuda):
            raise RuntimeError("nof.render (HIP) takes device-resident tensors; move rays with .to('cuda')")
        if rays.dim() != 2 or rays.shape[0] != R or rays.shape[1] < 10:
            raise RuntimeError(f"rays must be (N_rays, >=10) = ({R}, >=10); got {tuple(rays.shape)}")
        table[:, 9] = rays[:, 9]
    return table


def inference_train(model: NOF, embedding_xy: Embedding, samples_xy: torch.Tensor, rays: torch.Tensor,
                    z_vals: torch.Tensor, near_far_child: torch.Tensor, near_far_point: torch.Tensor,
                    range_readings: torch.Tensor, ray_class: torch.Tensor, chunk=1024 * 32, noise_std=1,
                    epsilon=1e-10, isval=False, sub_nerf_test_num=4, use_child_nerf_divide=1, use_child_nerf_loss=0,
                    *, rng=None):
    """render.py:38-163 -> (child_free_loss, child_depth_loss, depth_final (R,), weights_origin (R, S)).  The losses
    are CPU ``torch.tensor(0.0)`` when use_child_nerf_loss != 1 and have shape (1,) in the divide branch.
    Differentiable under autograd with respect to the module's parameters, in train mode (batch statistics) or in
    eval mode (frozen BatchNorm, nof._autograd.FrozenPassPoints), as render_rays_train; no gradient flows to
    samples_xy.  ``near_far_point``, ``ray_class`` and ``isval`` are accepted and unused."""
    pts, z = _check_points_inputs(model, embedding_xy, samples_xy, z_vals, near_far_child, differentiable=True)
    R, S = z.shape
    with_losses = use_child_nerf_loss == 1
    divide = use_child_nerf_divide == 1
    table = _child_table(rays, near_far_child, range_readings, R, divide) if with_losses else None
    noise = _noise(rng, "noise", z, noise_std)
    if _autograd.needs_grad(model) and not model.training:   # frozen BatchNorm
        w, depth, free, dl = _autograd.FrozenPassPoints.apply(_query_points, model, pts, table, z, noise,
                                                              float(noise_std), float(epsilon), int(chunk),
                                                              with_losses, divide, int(sub_nerf_test_num),
                                                              *_ops.grad_params(model))
    elif _autograd.needs_grad(model):
        sub = int(sub_nerf_test_num) if divide else 0
        w, depth, free, dl = _autograd.TrainPassPoints.apply(model, pts, table, z, noise, float(noise_std),
                                                             float(epsilon), int(chunk), with_losses, sub,
                                                             *_ops.grad_params(model))
    else:
        p = _query_points(model, pts, R, S, chunk)
        w, depth, fr, sl = P.composite(p, z, noise, float(noise_std), float(epsilon), table, 10, 11, 14, True)
        if with_losses:
            free, dl = P.child_losses(fr, sl, table, divide, int(sub_nerf_test_num))
    if not with_losses:
        free, dl = torch.tensor(0.0), torch.tensor(0.0)   # render.py:123-125, 157-159 (CPU scalars)
    return free, dl, depth, w


def inference(model: NOF, embedding_xy: Embedding, samples_xy: torch.Tensor, z_vals: torch.Tensor,
              chunk=1024 * 32, noise_std=1, epsilon=1e-10, isval=False, *, rng=None):
    """render.py:166-226 -> (depth_final (R,), weights (R, S), opacity ()).  ``isval=True`` (un-normalised weights,
    render.py:219) is reached by no reference caller -- render_rays passes its isval into the ``epsilon`` slot -- and
    raises NotImplementedError here."""
    if not (isval == False):   # noqa: E712  (the reference's own test, render.py:219)
        raise NotImplementedError("inference(isval=True) (un-normalised weights) is not implemented: no reference "
                                  "caller reaches it (render_rays passes isval as epsilon)")
    pts, z = _check_points_inputs(model, embedding_xy, samples_xy, z_vals)
    p = _query_points(model, pts, z.shape[0], z.shape[1], chunk)
    w, depth, opac, _ = P.composite_extras(p, z, _noise(rng, "noise", z, noise_std), float(noise_std),
                                           float(epsilon))
    return depth, w, opac


def inference_0525_2(model: NOF, embedding_xy: Embedding, samples_xy: torch.Tensor, z_vals: torch.Tensor,
                     other_interest_sub_nerf_number: torch.Tensor, near_far_child: torch.Tensor, chunk=1024 * 32,
                     noise_std=1, epsilon=0, isval=False, is_fine=0, depth_inference_method=0, *, rng=None):
    """render.py:229-368 -> (depth_final (R,), weights (R, S), opacity (), rays_effective_flag (R, 1) bool).  Adds
    no noise (the reference does not) and never prints; ``noise_std``, ``isval`` and ``is_fine`` are accepted and
    unused."""
    pts, z = _check_points_inputs(model, embedding_xy, samples_xy, z_vals, near_far_child)
    R, S = z.shape
    other = other_interest_sub_nerf_number
    if not torch.is_tensor(other):
        other = torch.as_tensor(other)
    other = other.to(z.device)
    p = _query_points(model, pts, R, S, chunk)
    rows = torch.zeros((R, 8), dtype=torch.float32, device=z.device)   # view_rows reads the child bounds in 6:8
    rows[:, 6:8] = near_far_child
    w, depth, at_peak, csum, opac_row, _ = _ops.view_rows(p, z, rows, int(depth_inference_method), float(epsilon),
                                                          want_points=False)
    flags, opacity = P.view_walk(other, at_peak, csum, opac_row, int(S))
    return depth, w, opacity, flags


def render_rays_train(model: NOF, model_fine: NOF, embedding_xy: Embedding, rays: torch.Tensor, sub_nerf_test_num=4,
                      N_samples=64, N_importance=128, use_disp=False, perturb=0, noise_std=1, chunk=1024 * 3,
                      isval=False, issegmentated=0, childnerf_ratio=0.5, use_child_nerf_divide=0,
                      use_child_nerf_loss=0, *, rng=None):
    """render.py:416-482 -> {'child_free_loss_fine', 'child_depth_loss_fine', 'depth_fine', 'child_free_loss',
    'child_depth_loss', 'depth'}.  Under autograd each network takes the route of its own mode: train mode the
    rematerialised backward, eval mode the frozen-BatchNorm backward (coarse in train and fine in eval mode in one
    call is legal); no gradient goes to the rays."""
    rays = _check_inputs(model, model_fine, embedding_xy, rays, 15, differentiable=True)
    R = rays.shape[0]
    z = _coarse(rays, N_samples, issegmentated, childnerf_ratio, perturb, rng)
    with_losses = use_child_nerf_loss == 1

    def one_pass(m, z, noise_key):
        if _autograd.needs_grad(m) and not m.training:   # frozen BatchNorm: decided per module
            w, depth, free, dl = _autograd.FrozenPass.apply(
                _query, m, rays, z, _noise(rng, noise_key, z, noise_std), float(noise_std), EPSILON, int(chunk),
                with_losses, use_child_nerf_divide == 1, int(sub_nerf_test_num), *_ops.grad_params(m))
            if not with_losses:
                free, dl = torch.tensor(0.0), torch.tensor(0.0)
            return w, depth, free, dl
        if _autograd.needs_grad(m):
            noise = _noise(rng, noise_key, z, noise_std)
            sub = int(sub_nerf_test_num) if use_child_nerf_divide == 1 else 0
            w, depth, free, dl = _autograd.TrainPass.apply(m, rays, z, noise, float(noise_std), EPSILON, int(chunk),
                                                           with_losses, sub, *_ops.grad_params(m))
            if not with_losses:
                free, dl = torch.tensor(0.0), torch.tensor(0.0)
            return w, depth, free, dl
        p = _query(m, rays, z, chunk)
        w, depth, fr, sl = P.composite(p, z, _noise(rng, noise_key, z, noise_std), float(noise_std), EPSILON,
                                       rays if with_losses else None, 10, 11, 14, True)
        if with_losses:
            free, dl = P.child_losses(fr, sl, rays, use_child_nerf_divide == 1, int(sub_nerf_test_num))
        else:
            free, dl = torch.tensor(0.0), torch.tensor(0.0)   # render.py:123-125, 157-159 (CPU scalars)
        return w, depth, free, dl

    w, depth, free, dl = one_pass(model, z, "noise")
    u = None if perturb == 0 else _draw(rng, "u", (R, N_importance), rays.device, torch.rand)
    zf = P.resample(z, w, int(N_importance), u)
    _, depth_f, free_f, dl_f = one_pass(model_fine, zf, "noise_fine")
    return {'child_free_loss_fine': free_f, 'child_depth_loss_fine': dl_f, "depth_fine": depth_f,
            'child_free_loss': free, 'child_depth_loss': dl, 'depth': depth}


def render_rays_val(model: NOF, model_fine: NOF, embedding_xy: Embedding, rays: torch.Tensor, sub_nerf_test_num=4,
                    N_samples=64, N_importance=128, use_disp=False, perturb=0, noise_std=1, chunk=1024 * 3,
                    isval=False, *, rng=None):
    """render.py:485-536 -> {'depth_fine', 'depth'}.

    Differentiable with respect to the ray geometry when ``rays`` requires grad, on frozen eval-mode networks: both
    passes run as nof._autograd.EvalPass and the gradients of ``depth`` and of ``depth_fine`` reach ``rays[:, 0:3]``
    (origins) and ``rays[:, 3:6]`` (directions); every other column's gradient is zero.  Sample depths are constants
    of the render: the coarse z comes from the near / far columns of the detached rays, and the fine z is detached
    from the coarse weights, as the reference detaches it (render.py:523).  A train-mode module raises (batch
    statistics couple the samples); parameters that require grad raise as before.  Without a tensor requiring grad
    the calls, and the outputs' bits, are the forward-only ones."""
    rays = _check_inputs(model, model_fine, embedding_xy, rays, 8)
    R = rays.shape[0]
    if torch.is_grad_enabled() and rays.requires_grad:
        for m in (model, model_fine):
            _autograd.check_frozen_eval(m, "rays")
        rd = rays.detach()
        z = _coarse(rd, N_samples, False, 0.0, perturb, rng)
        w, depth = _autograd.EvalPass.apply(_query, model, rays, z, _noise(rng, "noise", z, noise_std),
                                            float(noise_std), EPSILON, int(chunk), True)
        u = None if perturb == 0 else _draw(rng, "u", (R, N_importance), rays.device, torch.rand)
        zf = P.resample(z, w, int(N_importance), u)
        _, depth_f = _autograd.EvalPass.apply(_query, model_fine, rays, zf, _noise(rng, "noise_fine", zf, noise_std),
                                              float(noise_std), EPSILON, int(chunk), False)
        return {"depth_fine": depth_f, 'depth': depth}
    z = _coarse(rays, N_samples, False, 0.0, perturb, rng)
    p = _query(model, rays, z, chunk)
    w, depth, _, _ = P.composite(p, z, _noise(rng, "noise", z, noise_std), float(noise_std), EPSILON, None, 10, 11,
                                 14, True)
    u = None if perturb == 0 else _draw(rng, "u", (R, N_importance), rays.device, torch.rand)
    zf = P.resample(z, w, int(N_importance), u)
    pf = _query(model_fine, rays, zf, chunk)
    _, depth_f, _, _ = P.composite(pf, zf, _noise(rng, "noise_fine", zf, noise_std), float(noise_std), EPSILON,
                                   None, 10, 11, 14, False)
    return {"depth_fine": depth_f, 'depth': depth}


def render_rays(model: NOF, model_fine: NOF, embedding_xy: Embedding, rays: torch.Tensor, N_samples=64,
                N_importance=128, use_disp=False, perturb=0, noise_std=1, chunk=1024 * 3, isval=False, *, rng=None):
    """render.py:538-611 (the generic NOF renderer, exported in the reference's __all__).  Reproduces the
    reference's call ``inference(..., chunk, noise_std, isval)``, which lands ``isval`` in inference's
    ``epsilon`` slot: weights are always normalised, by sum(w) + float(isval).  Returns {'depth_fine',
    'weights', 'opacity', 'z_vals', 'depth', 'depth2', 'opacity_fine'}; depth2 is the z at the position where
    the last sample falls in the descending weight order (render.py:598-600; ties broken stably)."""
    rays = _check_inputs(model, model_fine, embedding_xy, rays, 8)
    R = rays.shape[0]
    z = P.sample_coarse(rays, N_samples, N_samples, 6, 7, 0, 0, bool(use_disp))
    if perturb > 0:
        z = P.perturb(z, float(perturb), _draw(rng, "perturb_rand", (R, N_samples), rays.device, torch.rand))
    eps = float(isval)
    p = _query(model, rays, z, chunk)
    w, depth, opac, _ = P.composite_extras(p, z, _noise(rng, "noise", z, noise_std), float(noise_std), eps)
    u = None if perturb == 0 else _draw(rng, "u", (R, N_importance), rays.device, torch.rand)
    zf = P.resample(z, w, int(N_importance), u)
    pf = _query(model_fine, rays, zf, chunk)
    wf, depth_f, opac_f, depth2 = P.composite_extras(pf, zf, _noise(rng, "noise_fine", zf, noise_std),
                                                     float(noise_std), eps)
    return {'depth_fine': depth_f, 'weights': wf, 'opacity': opac, 'z_vals': zf, "depth": depth, "depth2": depth2,
            "opacity_fine": opac_f}


def _inference_view(model, rays, z, other, chunk, method):
    """inference_0525_2 (render.py:229-368) on the HIP kernels: query, per-row compositing / peak / child sums,
    then the ray-group walk."""
    p = _query(model, rays, z, chunk)
    w, depth, at_peak, csum, opac_row, pts = P.view_rows(p, z, rays, int(method), EPSILON)
    flags, opacity = P.view_walk(other, at_peak, csum, opac_row, int(z.shape[1]))
    return depth, w, opacity, flags, pts


def render_rays_view_0525_2_2(model: NOF, model_fine: NOF, embedding_xy: Embedding, rays: torch.Tensor,
                              other_interest_sub_nerf_number: torch.Tensor, N_samples=64, N_importance=128,
                              use_disp=False, perturb=0, noise_std=1, chunk=1024 * 3, isval=False,
                              depth_inference_method=0, *, rng=None):
    """render.py:614-699: two-step inference on 13-column rows grouped per ray.  Returns {'depth_fine', 'weights',
    'opacity', 'z_vals', 'depth', 'opacity_fine', 'points_inference_fine', 'points_inference',
    'rays_effective_flag', 'rays_effective_flag_fine'} (the reference's debug prints are not reproduced)."""
    rays = _check_inputs(model, model_fine, embedding_xy, rays, 11)
    other = other_interest_sub_nerf_number
    if not torch.is_tensor(other):
        other = torch.as_tensor(other)
    other = other.to(rays.device)
    R = rays.shape[0]
    z = P.sample_coarse(rays, N_samples, N_samples, 9, 10, 0, 0, False)   # parent bounds, render.py:622-628
    if perturb > 0:
        z = P.perturb(z, float(perturb), _draw(rng, "perturb_rand", (R, N_samples), rays.device, torch.rand))
    method = int(depth_inference_method)
    depth, w, opacity, flags, pts = _inference_view(model, rays, z, other, chunk, method)
    u = None if perturb == 0 else _draw(rng, "u", (R, N_importance), rays.device, torch.rand)
    zf = P.resample(z, w, int(N_importance), u)
    depth_f, wf, opacity_f, flags_f, pts_f = _inference_view(model_fine, rays, zf, other, chunk, method)
    return {'depth_fine': depth_f, 'weights': wf, 'opacity': opacity, 'z_vals': zf, "depth": depth,
            "opacity_fine": opacity_f, "points_inference_fine": pts_f, "points_inference": pts,
            "rays_effective_flag": flags, "rays_effective_flag_fine": flags_f}
