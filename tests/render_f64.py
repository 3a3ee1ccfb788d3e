"""Plain torch restatement of the compositing, child-loss and two-step row arithmetic, in float64 (the truth the
per-kernel tests compare k_composite, k_composite_bwd, k_child_loss_* and k_view_rows with) or float32 (the
yardstick: how far the reference's own number format is from that truth) -- test infrastructure only, CPU only.

It builds on oracle/ref_cpu.py: the child masks come from ``O.expand_mask`` on the float32 tensors (they are
discrete; the kernels reproduce the reference's float32 bound arithmetic bit for bit, so a mask is an INPUT of the
float64 evaluation and is never recomputed in float64), every other step is the reference's op in ``dtype``.
Line numbers are the reference's nof/render.py.
"""
import torch

from oracle import ref_cpu as O


def masks(z32, near32, far32):
    """-> (m0, m2, mv): the inclusive child masks of inference_train (render.py:77-84 thr0 = 0, :91-97 thr0 = 2)
    and the strict one of inference_view (render.py:252-263, thr0 = 0.01), all on the float32 tensors."""
    return (O.expand_mask(z32, near32, far32, 0.0), O.expand_mask(z32, near32, far32, 2),
            O.expand_mask(z32, near32, far32, 0.01, strict=True))


def _weights(p, z, noise, eps):
    """render.py:51-61: w~_i = p_i prod_{j<i}(1 - p_j) (+ noise), w = w~ / (sum w~ + eps)."""
    free = 1 - p
    trans = torch.cumprod(torch.cat([torch.ones_like(free[:, :1]), free], -1), -1)[:, :-1]
    w = trans * p
    if noise is not None:
        w = w + noise
    return w / (torch.sum(w, -1).reshape(-1, 1) + eps)


def opacity_rows(p):
    """render.py:224 (== :354) before the mean: sum_i log(0.1 + p_i) + log(0.1 + (1 - p_i)) + 2.20727 per ray.
    The two constants enter the reference's float32 arithmetic as fl32(0.1) and fl32(2.20727); they are taken as
    those values here too (like p and z, they are inputs of the evaluation): the terms cancel to ~2e-6 at p = 0, so
    the 5e-8 between 2.20727 and its float32 value would otherwise grow with S into the row sum."""
    c01, c22 = (float(torch.tensor(v, dtype=torch.float32)) for v in (0.1, 2.20727))
    return torch.sum(torch.log(c01 + p) + torch.log(c01 + (1 - p)) + c22, -1)


def child_reduce(free_ray, sl1_ray, child_id, divide, N):
    """The scalar losses from the per-ray terms: render.py:121 / :155 (plain: sum / R and 1/R * 0.1 * mean) and
    render.py:111-119 / :140-152 (divide: per child id c in 1..N owning >= 1 ray, sum / count and
    1/count * 0.1 * mean; ids outside (0.5, N + 0.5) belong to no child)."""
    R = free_ray.shape[0]
    if not divide:
        return torch.sum(free_ray) / R, 1 / R * 0.1 * torch.mean(sl1_ray)
    free = torch.zeros((), dtype=free_ray.dtype)
    depth = torch.zeros((), dtype=free_ray.dtype)
    ids = child_id.to(torch.float64)
    k = torch.floor(ids - 0.5).long()                 # candidate child slot: id in (k + 0.5, k + 1.5)
    ok = (k >= 0) & (k < N) & (ids > k + 0.5) & (ids < k + 1.5)
    if not bool(ok.any()):
        return free, depth
    k = k[ok]
    cnt = torch.zeros(N, dtype=free_ray.dtype).index_add_(0, k, torch.ones(len(k), dtype=free_ray.dtype))
    fs = torch.zeros(N, dtype=free_ray.dtype).index_add_(0, k, free_ray[ok])
    ss = torch.zeros(N, dtype=free_ray.dtype).index_add_(0, k, sl1_ray[ok])
    own = cnt >= 1
    c = cnt[own]
    return torch.sum(fs[own] / c), torch.sum(1 / c * 0.1 * (ss[own] / c))


def composite_losses(p, z, noise, eps, masks, ranges, child_id, divide, N, dtype):
    """render.py:51-61 (weights, depth), :75-159 (child free / depth losses) and :224 (opacity terms) in ``dtype``.
    ``noise`` is the term added to the raw weights (draws * noise_std) or None; ``masks`` is (m0, m2) from
    ``masks()`` or None for a render without the child losses.  Differentiable in ``p`` when it requires grad.
    -> dict(w, depth, opac_row[, free_ray, sl1_ray, dc, free, depth_loss])."""
    p, z = p.to(dtype), z.to(dtype)
    noise = None if noise is None else noise.to(dtype)
    w = _weights(p, z, noise, eps)
    out = {"w": w, "depth": torch.sum(w * z, -1), "opac_row": opacity_rows(p)}
    if masks is None:
        return out
    m0, m2 = (m.to(dtype) for m in masks)
    w_free = w * (1 - m0)                                        # render.py:85-86
    wc, zc = w * m2, z * m2                                      # render.py:98-99
    wc = wc / (torch.sum(wc, -1).reshape(-1, 1) + eps)           # render.py:129
    dc = torch.sum(wc * zc, -1)
    out["free_ray"] = torch.sum(torch.square(w_free), -1)
    out["dc"] = dc
    out["sl1_ray"] = torch.nn.functional.smooth_l1_loss(1e1 * dc, 1e1 * ranges.to(dtype), reduction="none")
    out["free"], out["depth_loss"] = child_reduce(out["free_ray"], out["sl1_ray"], child_id, divide, N)
    return out


def g_logit(p, z, noise, eps, masks, ranges, child_id, divide, N, dtype, g_depth=None, g_free=None, g_dl=None):
    """dL/dlogit for L = sum(g_depth * depth) + g_free * free + g_dl * depth_loss with p = sigmoid(logit):
    autograd.grad(L, p) * p (1 - p), everything in ``dtype``.  A gradient that is None leaves its term out."""
    pd = p.to(dtype).clone().requires_grad_(True)
    out = composite_losses(pd, z, noise, eps, masks, ranges, child_id, divide, N, dtype)
    L = torch.zeros((), dtype=dtype)
    if g_depth is not None:
        L = L + torch.sum(g_depth.to(dtype) * out["depth"])
    if masks is not None and g_free is not None:
        L = L + g_free.to(dtype).reshape(()) * out["free"]
    if masks is not None and g_dl is not None:
        L = L + g_dl.to(dtype).reshape(()) * out["depth_loss"]
    if not L.requires_grad:
        return torch.zeros_like(pd).detach()
    (g,) = torch.autograd.grad(L, pd)
    pd = pd.detach()
    return g * (pd * (1 - pd))


def view_rows(p, z, mv, method, eps, dtype):
    """inference_view (render.py:241-246 weights, :265 child weight sum, :346-351 depth: method 2 re-normalises the
    weights inside the strict child mask ``mv``, every other method keeps sum w z, :354 opacity terms) in ``dtype``.
    -> dict(w, depth, child_sum, opac_row)."""
    p, z, m = p.to(dtype), z.to(dtype), mv.to(dtype)
    w = _weights(p, z, None, eps)
    child_sum = torch.sum(w * m, -1)
    if method == 2:
        wc = w * m
        wc = wc / (torch.sum(wc, -1).reshape(-1, 1) + eps)
        depth = torch.sum(wc * z, -1)
    else:
        depth = torch.sum(w * z, -1)
    return {"w": w, "depth": depth, "child_sum": child_sum, "opac_row": opacity_rows(p)}


def err(x, q64):
    """e(x) = max |x - q64| / scale: scale the per-ray maximum of |q64| (|q64| itself for scalars and one-per-ray
    quantities).  An entry whose scale is 0 counts 0 when x is exactly 0 there and inf otherwise."""
    x = torch.as_tensor(x).detach().to(torch.float64).cpu()
    q = torch.as_tensor(q64).detach().to(torch.float64)
    x = x.reshape(q.shape)
    scale = q.abs().amax(-1, keepdim=True).expand_as(q) if q.dim() == 2 else q.abs()
    d = (x - q).abs()
    e = torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d),
                                                                         torch.full_like(d, float("inf"))))
    return float(e.max())
