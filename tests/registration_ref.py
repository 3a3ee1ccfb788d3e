"""Float64 restatement of the registration path (tests of nof.registration, pcnerf::render_jac_fold and
pcnerf::gn_normal_eq) -- test infrastructure only, torch CPU / numpy: the folded eval network as sigmoid(e @ a + c)
over oracle.ref_cpu's embed / composite / lin_z / sample_pdf, the per-ray Jacobian by autograd, the closed form of
d depth / d logit, the normal equations in numpy float64 and a complete float64 registration loop.

The analytic field (analytic_fold) is a closed cavity around the origin: ranges of 0.69 .. 2.06 m seen from the pose
se3_exp(XI_STAR)
with near 0.05; far is the exit from the parent box [-2.5, 2.5]^3 (2.40 .. 4.35 m over the test's directions, around
the 4.0 m of a constant bound: scan_rays takes its far from a box), which contains the cavity."""
import functools
import math

import numpy as np
import torch

from eval_grad_ref import _ray_points
from oracle import ref_cpu as O

EPS = 1e-10
S_FIELD = 10.0
XI_STAR = (0.1, -0.05, 0.08, 0.05, -0.03, 0.1)
XI_START = (0.12, -0.10, 0.10, math.radians(2.0), math.radians(-1.5), math.radians(2.0))
PARENT_LO, PARENT_HI = (-2.5, -2.5, -2.5), (2.5, 2.5, 2.5)
NEAR = 0.05


def analytic_fold(s=S_FIELD):
    """logit = s (2 - cos x - 0.8 cos y - 1.2 cos z - 0.3 sin 2x + 0.25 cos 2y + 0.2 sin y) in Embedding's column
    order (sin at 3 + 6k + m, cos at 6 + 6k + m) -> (64,) float64, c last."""
    a = torch.zeros(64, dtype=torch.float64)
    a[6], a[7], a[8] = -s, -0.8 * s, -1.2 * s
    a[9], a[16], a[4] = -0.3 * s, 0.25 * s, 0.2 * s
    a[63] = 2 * s
    return a


def fold_logit(fold, x):
    """a . Embedding(x) + c in x's dtype."""
    f = fold.to(x.dtype)
    return O.embed(x) @ f[:63] + f[63]


def unnormalised(p):
    """(T_s p_s, T_s): the weights before the normalisation and the transmittance."""
    free = 1 - p
    trans = torch.cumprod(torch.cat([torch.ones_like(free[:, :1]), free], -1), -1)[:, :-1]
    return trans * p, trans


def render(fold, rays, z, dtype, eps=EPS, want_jac=True):
    """One pass on rays (R, >= 6) at the depths z (R, S) in ``dtype`` -> (depth, weights, sumw, jac6 or None).  float32
    rows: positions take the VALUE the float32 forward evaluates and the derivative of the exact expression
    (eval_grad_ref._ray_points); float64 rows are used as they are.  jac6 = d depth / d rays[:, 0:6] by autograd."""
    leaf = rays[:, :6].to(dtype).clone().requires_grad_(want_jac)
    if rays.dtype == torch.float32:
        x = _ray_points(leaf[:, 0:3], leaf[:, 3:6], rays, z)
    else:
        x = leaf[:, None, 0:3] + leaf[:, None, 3:6] * z.to(dtype)[..., None]
    p = torch.sigmoid(fold_logit(fold, x))
    w, depth = O.composite(p, z.to(dtype), eps)
    sumw = unnormalised(p)[0].sum(-1)
    jac = None
    if want_jac:
        (jac,) = torch.autograd.grad(depth.sum(), leaf)
    return depth.detach(), w.detach(), sumw.detach(), jac


def logit_terms(fold, rays, z):
    """Per sample, in float64 at the float32 forward's positions: (g (R, S) = d depth / d logit by the closed form,
    grad logit (R, S, 3)) -- the terms of jac6 and of its scale sum_s |g_s grad logit_s| max(1, z_s)."""
    x = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).double().requires_grad_(True)
    logit = fold_logit(fold, x)
    (gl,) = torch.autograd.grad(logit.sum(), x)
    g = ddepth_dlogit(torch.sigmoid(logit.detach()), z.double())
    return g, gl


def ddepth_dlogit(p, z, eps=EPS):
    """d depth / d logit_s (R, S) in closed form, p = sigmoid(logit): with w~_j = T_j p_j, W = sum w~ + eps,
    g~_j = (z_j - depth) / W and U_{j-1} = g~_j p_j + (1 - p_j) U_j (U_{S-1} = 0):
    g_j = T_j (g~_j - U_j) (1 - p_j) p_j.  No division by 1 - p."""
    wt, trans = unnormalised(p)
    W = wt.sum(-1, keepdim=True) + eps
    depth = (wt / W * z).sum(-1, keepdim=True)
    gt = (z - depth) / W
    S = p.shape[1]
    U = torch.zeros_like(p[:, 0])
    out = torch.zeros_like(p)
    for j in range(S - 1, -1, -1):
        out[:, j] = trans[:, j] * (gt[:, j] - U) * (1 - p[:, j]) * p[:, j]
        U = gt[:, j] * p[:, j] + (1 - p[:, j]) * U
    return out


def ddepth_dlogit_autograd(logit, z, eps=EPS):
    leaf = logit.clone().requires_grad_(True)
    _, depth = O.composite(torch.sigmoid(leaf), z, eps)
    (g,) = torch.autograd.grad(depth.sum(), leaf)
    return g


def pose_jacobian(rays6, jac6):
    """[J_o, o x J_o + d x J_d] in numpy float64 (the kernel's order of operations)."""
    r, J = np.asarray(rays6, np.float64), np.asarray(jac6, np.float64)
    o, d, Jo, Jd = r[:, 0:3], r[:, 3:6], J[:, 0:3], J[:, 3:6]
    return np.concatenate([Jo, np.cross(o, Jo) + np.cross(d, Jd)], 1)


def normal_eq(rays, jac6, depth, sumw, target, huber_delta, min_sumw):
    """-> (out (30,), mag (30,)) in numpy float64 on the given (float32) inputs: the upper triangle of H, b, cost,
    n_valid, pad; mag the sum of the terms' absolute values (the scale of the 1e-12 comparison)."""
    depth, sumw, target = (np.asarray(v, np.float64) for v in (depth, sumw, target))
    tgt32 = np.asarray(target, np.float32)
    valid = (sumw >= min_sumw) & np.isfinite(depth) & np.isfinite(tgt32) & (target > 0)
    Jp = pose_jacobian(rays, jac6)[valid]
    r = (depth - target)[valid]
    ar = np.abs(r)
    lin = (huber_delta > 0) & (ar > huber_delta)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(lin, huber_delta / ar, 1.0)
    rho = np.where(lin, huber_delta * (ar - 0.5 * huber_delta), 0.5 * r * r)
    out, mag = np.zeros(30), np.zeros(30)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            t = (w * Jp[:, a]) * Jp[:, b]
            out[k], mag[k] = t.sum(), np.abs(t).sum()
            k += 1
    for a in range(6):
        t = (w * Jp[:, a]) * r
        out[21 + a], mag[21 + a] = t.sum(), np.abs(t).sum()
    out[27] = mag[27] = rho.sum()
    out[28] = mag[28] = float(valid.sum())
    return out, mag


# ----------------------------------------------------------------------------------------------- the float64 loop
def unit_directions(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return v / v.norm(dim=-1, keepdim=True)


def rays_f64(dirs_sensor, T, near=NEAR, lo=PARENT_LO, hi=PARENT_HI):
    """World rows [o, d, near, far] (float64) of unit sensor-frame directions under the pose T, far by the slab test."""
    T = torch.as_tensor(T, dtype=torch.float64)
    d = dirs_sensor @ T[:3, :3].T
    o = T[:3, 3].expand_as(d)
    lo, hi = torch.tensor(lo, dtype=torch.float64), torch.tensor(hi, dtype=torch.float64)
    t1, t2 = (lo - o) / d, (hi - o) / d
    far = torch.maximum(t1, t2).min(-1)[0]
    return torch.cat([o, d, torch.full_like(far, near)[:, None], far[:, None]], -1)


def render_two_pass(fold_c, fold_f, rays, n_samples, n_importance, want_jac=True):
    """render_rays_val's two passes (perturb = 0, noise_std = 0) in the rows' dtype (float64 rows: all float64) ->
    (depth_fine, sumw, jac6)."""
    dt = rays.dtype
    z = O.lin_z(rays[:, 6:7], rays[:, 7:8], n_samples).to(dt)
    _, w, _, _ = render(fold_c, rays, z, dt, want_jac=False)
    zmid = .5 * (z[..., 1:] + z[..., :-1])
    u = torch.linspace(0., 1., steps=n_importance, dtype=dt).expand(rays.shape[0], n_importance)
    zs = O.sample_pdf(zmid, w[..., 1:-1], n_importance, det=False, u=u)
    zf = torch.sort(torch.cat([z, zs], -1), -1)[0]
    depth, _, sumw, jac = render(fold_f, rays, zf, dt, want_jac=want_jac)
    return depth, sumw, jac


def pose_error(T, T_ref):
    """(translation distance, rotation angle) between two poses."""
    T, T_ref = np.asarray(T, np.float64), np.asarray(T_ref, np.float64)
    dR = T[:3, :3] @ T_ref[:3, :3].T
    ang = math.atan2(np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2,
                     (np.trace(dR) - 1) / 2)
    return float(np.linalg.norm(T[:3, 3] - T_ref[:3, 3])), float(ang)


def register_f64(fold_c, fold_f, dirs_sensor, ranges, init_pose, se3_exp, n_samples=64, n_importance=128, iters=20,
                 huber_delta=0.0, min_sumw=0.5, damping=1e-6, T_ref=None):
    """The registration loop of nof.registration.register_scan_fold in float64 throughout (rays, rendering, normal
    equations, solve) -> dict(pose, costs, n_valid, errors (per evaluation, against T_ref), all_costs)."""
    T = torch.as_tensor(init_pose, dtype=torch.float64).clone()
    lam, acc = damping, None
    costs, all_costs, errors = [], [], []
    for _ in range(iters):
        rays = rays_f64(dirs_sensor, T)
        depth, sumw, jac = render_two_pass(fold_c, fold_f, rays, n_samples, n_importance)
        out, _ = normal_eq(rays[:, :6].numpy(), jac.numpy(), depth.numpy(), sumw.numpy(), np.asarray(ranges),
                           huber_delta, min_sumw)
        H = np.zeros((6, 6))
        H[np.triu_indices(6)] = out[:21]
        H = H + np.triu(H, 1).T
        b, cost, n_valid = out[21:27], float(out[27]), int(out[28])
        all_costs.append(cost)
        if T_ref is not None:
            errors.append(pose_error(T, T_ref))
        if acc is None or cost <= acc[3]:
            if acc is not None:
                lam /= 10.0
            acc = (T, H, b, cost, n_valid)
            costs.append(cost)
        else:
            lam *= 10.0
        xi = np.linalg.solve(acc[1] + lam * np.diag(np.diag(acc[1])), -acc[2])
        T = se3_exp(xi) @ acc[0]
    return {"pose": T, "costs": costs, "all_costs": all_costs, "n_valid": acc[4], "errors": errors,
            "cond": float(np.linalg.cond(acc[1]))}


@functools.lru_cache(maxsize=None)
def scene():
    """The registration tests' scene, computed once per process: 2,048 unit directions (seed 0) seen from
    T* = se3_exp(XI_STAR) in the analytic field (the same fold for both passes), ranges from the float64 two-pass
    render at T*, the start se3_exp(XI_START) T*, and the float64 loop's 20 iterations at 64 + 128 samples."""
    from nof.registration import se3_exp
    fold = analytic_fold()
    T_star = se3_exp(XI_STAR)
    dirs = unit_directions(2048, 0)
    ranges, sumw, _ = render_two_pass(fold, fold, rays_f64(dirs, T_star), 64, 128, want_jac=False)
    T0 = se3_exp(XI_START) @ T_star
    run = register_f64(fold, fold, dirs, ranges.numpy(), T0, se3_exp, T_ref=T_star)
    return {"fold": fold, "T_star": T_star, "dirs": dirs, "ranges": ranges, "sumw": sumw, "T0": T0, "run": run}
