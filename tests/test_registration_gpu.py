"""pcnerf::render_jac_fold, pcnerf::gn_normal_eq and nof.registration on the MI355X against the float64 restatement
of tests/registration_ref.py.

Tolerance of the render pass, per quantity and case (the per-kernel tests' rule, parity_helpers.Tally): e(x) =
max |x - q64| / scale, e32 the same restatement run in float32 on the CPU, e_hip <= max(4 e32, 2.4e-7).  Scales: depth
and sumw their own float64 value per ray, weights the ray's largest weight, jac6 per component the ray's
sum_s |g_s d logit_s / d x_m| max(1, z_s) (the terms the component sums; the same scale for the origin and the
direction column of coordinate m).  No case is left out.  The normal equations are float64 sums of float64 products:
1e-12 of the sum of the terms' absolute values."""
import ctypes  # noqa: F401

import numpy as np
import pytest
import torch

import registration_ref as RR
from gradcheck import _report
from parity_helpers import Tally
from sampling_f64 import same_bits
from nof import _hip as H
from nof import _ops
from nof import _torch_ops as T
from nof import registration as G
from nof import synthetic as syn

pytestmark = pytest.mark.gpu
P = torch.ops.pcnerf
EPS = RR.EPS
NOCAP = float("inf")
SAMPLES = (1, 2, 63, 64, 65, 128, 129, 384, 1023, 1024)   # every block-size boundary, a partial last lane, the limit
RAYS = (1, 5, 67)
_CACHE = {}


def _dev(t):
    return t.cuda().contiguous()


def _random_fold():
    """The fold of a random init_nof_params network (composed on the device, pcnerf::fold_eval) -> (64,) float64 CPU."""
    if "fold" not in _CACHE:
        from nof.networks import NOF_fine
        m = syn.load_into(NOF_fine(), syn.init_nof_params(2)).cuda().eval()
        with torch.no_grad():
            _CACHE["fold"] = P.fold_eval(T.eval_params(m)).cpu()
    return _CACHE["fold"]


def _case(field, R, S):
    """(fold (CPU float64), rays (R, 8) float32, z (R, S) float32 ascending)."""
    g = torch.Generator().manual_seed(1000 * S + R)
    if field == "analytic":
        fold = RR.analytic_fold()
        rays = RR.rays_f64(RR.unit_directions(R, S), G.se3_exp(RR.XI_STAR)).float()
    else:
        fold = _random_fold()
        rays = torch.from_numpy(syn.make_rays(R, seed=S))[:, :8].contiguous()
        rays[:, 6] = 0.5
    near, far = rays[:, 6:7], rays[:, 7:8]
    z = torch.sort(near + (far - near) * torch.rand(R, S, generator=g), -1)[0].contiguous()
    return fold, rays, z


def _errs(x, q64, scale):
    """max |x - q64| / scale; where the scale is 0 the value must be exactly q64."""
    d = (x.double() - q64).abs()
    ok = scale > 0
    e = float((d[ok] / scale[ok]).max()) if bool(ok.any()) else 0.0
    return e if float(d[~ok].max() if bool((~ok).any()) else 0.0) == 0.0 else float("inf")


def _jac_scale(fold, rays, z):
    g, gl = RR.logit_terms(fold, rays, z)
    s = ((g[..., None] * gl).abs() * torch.clamp(z.double(), min=1.0)[..., None]).sum(1)   # (R, 3)
    return torch.cat([s, s], -1)


def _composed(rays, z, fold):
    """The composed route on the same fold: fold query -> composite -> composite_backward(grad_depth = 1) ->
    rays_grad_eval (four launches; p and g_logit through memory)."""
    R, S = z.shape
    p = torch.empty_like(z)
    H.check(H.lib().pcnerf_nof_query_eval_fold(rays.data_ptr(), R, rays.shape[1], z.data_ptr(), S, fold.data_ptr(),
                                               p.data_ptr(), H.stream_of(z)))
    w, depth, _, _ = P.composite(p, z, None, 0.0, EPS, None, 10, 11, 14, True)
    g = _ops.composite_backward(p, z, None, 0.0, EPS, None, 0, torch.ones(R, device=z.device), None, None)
    return depth, w, P.rays_grad_eval(rays, z, g, fold)


def _check_pass(t, case, fold, rays, z, composed=True):
    d64, w64, s64, j64 = RR.render(fold, rays, z, torch.float64)
    d32, w32, s32, j32 = RR.render(fold, rays, z, torch.float32)
    fd, rd, zd = _dev(fold), _dev(rays), _dev(z)
    depth, sumw, w, jac = (v.cpu() for v in P.render_jac_fold(rd, zd, fd, EPS, True, True))
    for v in (depth, sumw, w, jac):
        assert bool(torch.isfinite(v).all()), case
    wmax = w64.abs().amax(-1, keepdim=True).expand_as(w64)
    js = _jac_scale(fold, rays, z)
    for name, x, q32, q64, scale in (("depth", depth, d32, d64, d64.abs()), ("sumw", sumw, s32, s64, s64.abs()),
                                     ("weights", w, w32, w64, wmax), ("jac6", jac, j32, j64, js)):
        t.check_err(case, name, _errs(x, q64, scale), _errs(q32, q64, scale), NOCAP)
    if composed:
        cd, cw, cj = (v.cpu() for v in _composed(rd, zd, fd))
        _report({"test": t.test, "case": case, "quantity": "jac6 vs composed route",
                 "distance": _errs(jac, cj.double(), js), "depth_bits_equal": same_bits(depth, cd),
                 "weights_bits_equal": same_bits(w, cw)})
    return depth, sumw, w, jac


@pytest.mark.parametrize("field", ["analytic", "random"])
@pytest.mark.parametrize("S", SAMPLES)
def test_render_jac_fold_against_float64(S, field):
    """Measured on the MI355X: see DESIGN.md (registration) for the worst e_hip / max(4 e32, 2.4e-7)."""
    t = Tally("render_jac_fold")
    for R in RAYS:
        _check_pass(t, f"{field} R{R} S{S}", *_case(field, R, S))
    t.done()


def _line_rays(R):
    """Rays from the origin along +x (slightly fanned), near 0.1."""
    rays = torch.zeros(R, 8)
    rays[:, 3] = 1.0
    rays[:, 4] = 0.01 * torch.arange(R)
    rays[:, 3:6] /= rays[:, 3:6].norm(dim=-1, keepdim=True)
    rays[:, 6], rays[:, 7] = 0.1, 4.0
    return rays


def _plane_fold(k, x0):
    """logit = k (x - x0)."""
    a = torch.zeros(64, dtype=torch.float64)
    a[0], a[63] = k, -k * x0
    return a


@pytest.mark.parametrize("S", [3, 64, 130])
def test_saturation_and_emptiness(S):
    """Every p exactly 1 (a = 0, c = +40), sumw ~ 0 (c = -40), a plane whose first sample saturates (jac6 exactly 0:
    sample 0 carries the factor 1 - p = 0, every later one the transmittance 0 -- though grad logit = 400 there) and
    one whose third sample does; all finite, all under the float64 rule."""
    t = Tally("render_jac_fold_saturation")
    R = 5
    rays = _line_rays(R)
    z = (0.1 + 0.1 * torch.arange(S, dtype=torch.float32)).expand(R, S).contiguous()
    full, empty = torch.zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
    full[63], empty[63] = 40.0, -40.0
    depth, sumw, w, jac = _check_pass(t, f"full S{S}", full, rays, z)
    assert torch.equal(w[:, 0], torch.ones(R)) and float(w[:, 1:].abs().max()) == 0.0
    assert torch.equal(depth, z[:, 0]) and torch.equal(sumw, torch.ones(R)) and float(jac.abs().max()) == 0.0
    depth, sumw, w, jac = _check_pass(t, f"empty S{S}", empty, rays, z)
    assert float(sumw.max()) < 1e-14 and float(jac.abs().max()) == 0.0
    depth, sumw, w, jac = _check_pass(t, f"first S{S}", _plane_fold(400.0, -0.1), rays, z)
    assert torch.equal(w[:, 0], torch.ones(R)) and float(jac.abs().max()) == 0.0
    depth, sumw, w, jac = _check_pass(t, f"third S{S}", _plane_fold(400.0, 0.25), rays, z)
    assert torch.equal(w[:, 2], torch.ones(R)) and float(w[:, 3:].abs().sum()) == 0.0
    t.done()


@pytest.mark.parametrize("S", [48, 129, 1000])
def test_optional_outputs_and_repeatability(S):
    fold, rays, z = _case("analytic", 67, S)
    fd, rd, zd = _dev(fold), _dev(rays), _dev(z)
    full = P.render_jac_fold(rd, zd, fd, EPS, True, True)
    again = P.render_jac_fold(rd, zd, fd, EPS, True, True)
    assert all(same_bits(a, b) for a, b in zip(full, again))
    now = P.render_jac_fold(rd, zd, fd, EPS, False, True)
    noj = P.render_jac_fold(rd, zd, fd, EPS, True, False)
    none = P.render_jac_fold(rd, zd, fd, EPS, False, False)
    assert now[2].numel() == 0 and noj[3].numel() == 0 and none[2].numel() == 0 and none[3].numel() == 0
    for got, keep in ((now, (0, 1, 3)), (noj, (0, 1, 2)), (none, (0, 1))):
        for i in keep:
            assert same_bits(got[i], full[i]), (S, i)
    # wider rows (stride 15) read the same six columns
    wide = torch.rand(67, 15)
    wide[:, :8] = rays
    assert all(same_bits(a, b) for a, b in zip(P.render_jac_fold(_dev(wide), zd, fd, EPS, True, True), full))


def _gn_case(R, seed):
    g = torch.Generator().manual_seed(seed)
    rays = torch.rand(R, 8, generator=g) * 4 - 2
    rays[:, 3:6] /= rays[:, 3:6].norm(dim=-1, keepdim=True)
    jac = torch.randn(R, 6, generator=g)
    target = 0.7 + 1.4 * torch.rand(R, generator=g)
    depth = target + 0.2 * torch.randn(R, generator=g)
    sumw = 0.3 + 0.7 * torch.rand(R, generator=g)
    for k, (t, v) in enumerate(((depth, float("nan")), (target, 0.0), (target, float("inf")), (depth, float("inf")),
                                (target, -1.0), (target, float("nan")))):
        t[(5 + 7 * k) % R::41] = v   # spread through the rays (R = 1 takes the last one)
    return rays, jac, depth, sumw, target


@pytest.mark.parametrize("delta", [0.0, 0.05, 10.0])
@pytest.mark.parametrize("R", [1, 63, 64, 257, 100003])
def test_gn_normal_eq_against_numpy(R, delta):
    """delta 0.05: both Huber branches (|r| ~ 0.2 N(0, 1)); 10: the quadratic one alone; 0: least squares."""
    rays, jac, depth, sumw, target = _gn_case(R, R)
    if R == 1:
        depth[0], target[0], sumw[0] = 1.5, 1.25, 0.9   # one valid ray
    want, mag = RR.normal_eq(rays.numpy(), jac.numpy(), depth.numpy(), sumw.numpy(), target.numpy(), delta, 0.5)
    args = tuple(_dev(v) for v in (rays, jac, depth, sumw, target))
    got = P.gn_normal_eq(*args, delta, 0.5)
    assert got.dtype == torch.float64 and tuple(got.shape) == (30,)
    assert same_bits(got.view(torch.int32), P.gn_normal_eq(*args, delta, 0.5).view(torch.int32))
    got = got.cpu().numpy()
    assert got[28] == want[28] and got[29] == 0.0
    if R > 1:
        assert 0 < want[28] < R
    err = np.abs(got[:28] - want[:28])
    _report({"test": "gn_normal_eq", "case": f"R{R} d{delta}", "worst": float((err / np.maximum(mag[:28], 1e-300)).max())})
    assert (err <= 1e-12 * mag[:28]).all(), (err / np.maximum(mag[:28], 1e-300)).max()
    if delta == 0.05 and R >= 63:
        r = np.abs(depth.double().numpy() - target.double().numpy())
        assert (r[np.isfinite(r)] > delta).any() and (r[np.isfinite(r)] <= delta).any()


def test_gn_normal_eq_all_invalid_and_empty():
    rays, jac, depth, sumw, target = _gn_case(64, 1)
    out = P.gn_normal_eq(*(_dev(v) for v in (rays, jac, depth, torch.zeros(64), target)), 0.0, 0.5)
    assert float(out.abs().max()) == 0.0
    e = torch.empty(0, device="cuda")
    out = P.gn_normal_eq(torch.empty(0, 8, device="cuda"), torch.empty(0, 6, device="cuda"), e, e, e, 0.0, 0.5)
    assert tuple(out.shape) == (30,) and float(out.abs().max()) == 0.0


def test_register_scan_fold_end_to_end():
    """The CPU test's scene and start, 20 iterations; targets from the float64 helper at T*.  The final pose must lie
    within 2 (the float64 loop's final error) + 10 delta of T* in translation (delta = max |depth_hip - depth_f64|
    at T*: float32 rendering noise entering through 2,048 residuals; the factor 2: the differing LM path), and the
    same in rotation with delta over the mean range.  Measured on the MI355X: see DESIGN.md (registration)."""
    s = RR.scene()
    fold = _dev(s["fold"])
    pts = _dev((s["dirs"] * s["ranges"][:, None]).float())
    rays, rng = G.scan_rays(pts, s["T_star"], RR.PARENT_LO, RR.PARENT_HI, RR.NEAR)
    depth, sumw, _ = G.render_scan(fold, fold, rays, 64, 128, False)
    delta = float((depth.cpu().double() - s["ranges"]).abs().max())
    ht, hr = RR.pose_error(s["run"]["pose"], s["T_star"])
    res = G.register_scan_fold(fold, fold, pts, s["T0"], RR.PARENT_LO, RR.PARENT_HI, N_samples=64, N_importance=128,
                               iters=20, near=RR.NEAR)
    et, er = RR.pose_error(res.pose, s["T_star"])
    bt, br = 2 * ht + 10 * delta, 2 * hr + 10 * delta / float(s["ranges"].mean())
    line = {"test": "register_scan_fold", "delta": delta, "err_t": et, "err_r": er, "f64_err_t": ht, "f64_err_r": hr,
            "bound_t": bt, "bound_r": br, "n_valid": res.n_valid, "iterations": res.iterations,
            "accepted": len(res.costs), "cost_first": res.costs[0], "cost_last": res.costs[-1]}
    _report(line)
    print(line)
    assert et <= bt and er <= br, line
    assert all(b <= a for a, b in zip(res.costs, res.costs[1:]))
    assert res.n_valid == 2048 and res.iterations == 20 and res.pose.dtype == torch.float64


def test_register_scan_on_frozen_modules():
    """One iteration equals register_scan_fold on the modules' fold_eval vectors bit for bit; train-mode modules and
    parameters requiring grad raise; no process-wide selector moves."""
    from nof.networks import NOF_coarse, NOF_fine
    mc = syn.load_into(NOF_coarse(), syn.init_nof_params(1)).cuda().eval().requires_grad_(False)
    mf = syn.load_into(NOF_fine(), syn.init_nof_params(2)).cuda().eval().requires_grad_(False)
    rows = torch.from_numpy(syn.make_rays(512, seed=4))
    pts = _dev(rows[:, 3:6] * rows[:, 14:15])
    T0 = G.se3_exp([0.05, -0.02, 0.01, 0.0, 0.0, 0.01])
    kw = dict(N_samples=64, N_importance=128, iters=1, min_sumw=0.0)
    before = (_ops.get_eval_math(), _ops.eval_fold_enabled(), _ops.get_train_math())
    a = G.register_scan(mc, mf, pts, T0, syn.PARENT_LO, syn.PARENT_HI, **kw)
    with torch.no_grad():
        fc, ff = P.fold_eval(T.eval_params(mc)), P.fold_eval(T.eval_params(mf))
    b = G.register_scan_fold(fc, ff, pts, T0, syn.PARENT_LO, syn.PARENT_HI, **kw)
    assert torch.equal(a.pose, b.pose) and a.costs == b.costs and a.n_valid == b.n_valid == 512
    assert a.iterations == 1 and not torch.equal(a.pose, T0) and bool(torch.isfinite(a.pose).all())
    with pytest.raises(NotImplementedError, match="train-mode"):
        G.register_scan(mc, mf.train(), pts, T0, syn.PARENT_LO, syn.PARENT_HI, **kw)
    mf.eval()
    mc.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="require grad"):
        G.register_scan(mc, mf, pts, T0, syn.PARENT_LO, syn.PARENT_HI, **kw)
    assert (_ops.get_eval_math(), _ops.eval_fold_enabled(), _ops.get_train_math()) == before
