"""CPU oracle of the eval-mode geometry gradients (tests of nof._autograd.EvalPass / EvalPassPoints): torch autograd of
oracle.ref_cpu's embed / nof_forward(training=False) / composite, in float32 or float64.  test_eval_grad_cpu pins this
route to the reference's own autograd (tests/golden/eval_grads.npz); test_eval_grad_gpu uses it where the reference
has no fixture (render_rays_val end to end at the HIP path's own sample depths)."""
import torch

from nof import synthetic as syn
from oracle import ref_cpu as O


def frozen_params(seed, dtype):
    Q = O.params_from_numpy(syn.init_nof_params(seed))
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in Q.items()}


def points_grad(seed, pts, z, cot, dtype, noise=None, eps=1e-10):
    """d sum(cot * depth) / d pts of inference_val (render.py:13-36) on positions pts (R, S, 3), all float32 inputs
    cast to ``dtype``; ``noise`` is the already scaled draw."""
    x = pts.to(dtype).clone().requires_grad_(True)
    p = O.query(frozen_params(seed, dtype), x, False, 1 << 15)
    _, d = O.composite(p, z.to(dtype), eps, None if noise is None else noise.to(dtype))
    (d * cot.to(dtype)).sum().backward()
    return x.grad


def _ray_points(o, d, rays32, z32):
    """o + d z with the VALUE the float32 forward evaluates (fl(o + fl(d z)), one rounding per op, render.py:458) and
    the derivative of the exact expression: d x / d o = 1, d x / d d = z."""
    exact = o[:, None, :] + d[:, None, :] * z32.to(o.dtype)[..., None]
    rounded = (rays32[:, None, 0:3] + rays32[:, None, 3:6] * z32[..., None]).to(o.dtype)
    return exact + (rounded - exact).detach()


def rays_grad(seed_c, seed_f, rays32, z32, zf32, cot, dtype, eps=1e-10):
    """d sum(cot * (depth + depth_fine)) / d rays[:, 0:6] of render_rays_val (render.py:485-536, perturb = 0,
    noise_std = 0) at GIVEN coarse and fine sample depths (constants of the render) -> (R, 6)."""
    leaf = rays32[:, :6].to(dtype).clone().requires_grad_(True)
    total = 0
    for seed, z in ((seed_c, z32), (seed_f, zf32)):
        x = _ray_points(leaf[:, 0:3], leaf[:, 3:6], rays32, z)
        p = O.query(frozen_params(seed, dtype), x, False, 1 << 15)
        _, depth = O.composite(p, z.to(dtype), eps)
        total = total + (depth * cot.to(dtype)).sum()
    total.backward()
    return leaf.grad
