"""Eval-mode render: gradients to ray origins / directions and to explicit sample positions (nof._autograd.EvalPass /
EvalPassPoints over pcnerf_nof_query_eval_backward / pcnerf_nof_points_eval_backward).

1. point form vs the reference: inference_val(...)[0] backpropagated to samples_xy against the reference's own autograd
   (tests/golden/eval_grads.npz), gradcheck.check_grads_elem as it stands.
2. ray form vs point form: on pts = o + d z, rays_grad_eval against the float64 sums of points_grad_eval's output,
   within the DERIVED bound 2^-24 (sum_s |term_s| + |result|) per component: each float32 g_pts entry is one rounding
   of the exact term (relative 2^-24), the ray form rounds its float64 sum once (2^-24 |result|).
3. render_rays_val end to end against torch autograd of the oracle in float64 (float32: the envelope's second sample)
   at the HIP path's own coarse and fine sample depths.
4. determinism, 5. independence from the eval path (fold, fp32 math), 6. refusals."""
import numpy as np
import pytest
import torch

from conftest import golden
from eval_grad_ref import rays_grad
from gradcheck import check_grads_elem
from nof import _ops
from nof import render as R
from nof import synthetic as syn
from nof import _torch_ops as T
from nof.networks import Embedding, NOF_coarse, NOF_fine

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, SEED_F = 1234, 5678
P = torch.ops.pcnerf
SWITCHES = {"default": None, "eval_fold": (_ops.set_eval_fold, True), "eval_math_fp32": (_ops.set_eval_math, "fp32")}


def model(seed=SEED, cls=NOF_coarse, train=False, frozen=True):
    m = syn.load_into(cls(), syn.init_nof_params(seed)).to(DEV).train(train)
    for t in m.parameters():
        t.requires_grad_(not frozen)
    return m


class switched:
    """Run a block under one of the opt-in eval paths and restore the previous setting."""

    def __init__(self, name):
        self.sw = SWITCHES[name]

    def __enter__(self):
        if self.sw:
            self.prev = self.sw[0](self.sw[1])

    def __exit__(self, *exc):
        if self.sw:
            self.sw[0](self.prev)


@pytest.fixture(scope="module")
def g():
    return golden("eval_grads")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. point form
def hip_points_grad(g, case):
    k = case + "/"
    pts, z, cot = dev(g[k + "pts"]).requires_grad_(True), dev(g[k + "z"]), dev(g[k + "cot"])
    ns = float(g[k + "noise_std"])
    rng = {"noise": dev(g[k + "noise"])} if ns else None
    nfc = torch.zeros(pts.shape[0], 2, device=DEV)
    d, w = R.inference_val(model(), Embedding(3, 10), pts, None, z, nfc, None, None, None, noise_std=ns, rng=rng)
    assert d.requires_grad and not w.requires_grad and tuple(w.shape) == tuple(z.shape)
    (d * cot).sum().backward()
    assert pts.grad.dtype == torch.float32 and pts.grad.shape == pts.shape
    return d.detach(), pts.grad


def check_points_case(g, case, tag):
    d, grad = hip_points_grad(g, case)
    k = case + "/"
    if not float(g[k + "noise_std"]):
        np.testing.assert_allclose(d.cpu().numpy(), g[k + "depth"], rtol=1e-4, atol=1e-6)
    worst = check_grads_elem(lambda _: grad.cpu().numpy(), ["samples_xy"], g, k, f"eval_grad_points_{case}_{tag}")
    print(f"points case {case} [{tag}]: max err/tol {worst['samples_xy'][0]:.3g}, "
          f"max |err| / max |ref| {worst['samples_xy'][1]:.3g}")


@pytest.mark.parametrize("case", ["a", "b", "n"])
def test_inference_val_grad_vs_reference(case, g):
    check_points_case(g, case, "default")


# ------------------------------------------------------------------------------------------------ 2. ray vs point
@pytest.mark.parametrize("stride", [8, 15])
@pytest.mark.parametrize("S", [48, 65, 384])
@pytest.mark.parametrize("R_", [1, 5, 130])
def test_ray_form_equals_summed_point_form(R_, S, stride):
    gen = torch.Generator().manual_seed(100 * R_ + S + stride)
    rays = torch.from_numpy(syn.make_rays(R_, seed=R_ + S))[:, :stride].contiguous()
    z = torch.sort(rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * torch.rand(R_, S, generator=gen), dim=1).values
    gl = torch.randn(R_, S, generator=gen)
    rays, z, gl = rays.to(DEV), z.contiguous().to(DEV), gl.to(DEV)
    pts = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).contiguous()   # two torch ops: no contraction
    fold = P.fold_eval(T.eval_params(model()))
    g6 = P.rays_grad_eval(rays, z, gl, fold)
    gp = P.points_grad_eval(pts, gl, fold)
    assert tuple(g6.shape) == (R_, 6) and tuple(gp.shape) == (R_, S, 3)
    assert torch.equal(gp.view(-1, 3), P.points_grad_eval(pts.view(-1, 3), gl.view(-1), fold))
    terms = torch.cat([gp.double(), z.double()[..., None] * gp.double()], dim=2)   # (R, S, 6)
    want = terms.sum(1)
    bound = 2.0 ** -24 * (terms.abs().sum(1) + want.abs())
    err = (g6.double() - want).abs()
    assert torch.isfinite(g6).all() and float(want.abs().max()) > 0
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"ray vs point R={R_} S={S} stride={stride}: max err/bound {ratio:.3g}")
    assert bool((err <= bound).all()), ratio


# ------------------------------------------------------------------------------------------------ 3. render_rays_val
RAY_CASES = {"r130": (130, 64, 128, 11), "r24": (24, 128, 256, 12)}   # rays, N_samples, N_importance, seed
_RAY_REF = {}


def ray_case(name, switch="default"):
    """Inputs, the HIP path's own sample depths under ``switch`` and the oracle's gradients at them, once per case."""
    key = (name, switch)
    if key in _RAY_REF:
        return _RAY_REF[key]
    n, Ns, Ni, seed = RAY_CASES[name]
    rays = torch.from_numpy(syn.make_rays(n, seed=seed))
    cot = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    rd = rays.to(DEV)
    with torch.no_grad(), switched(switch):
        z = P.sample_coarse(rd, Ns, Ns, 6, 7, 10, 11, False)
        w = P.composite(R._query(model(), rd, z, 32768), z, None, 0.0, R.EPSILON, None, 10, 11, 14, True)[0]
        zf = P.resample(z, w, Ni, None)
    ref = {"rays6": rays_grad(SEED, SEED_F, rays, z.cpu(), zf.cpu(), cot, torch.float32).numpy(),
           "f64:rays6": rays_grad(SEED, SEED_F, rays, z.cpu(), zf.cpu(), cot, torch.float64).numpy()}
    # the float32 oracle itself under the same check against the float64 one, on these rays
    assert np.isfinite(ref["rays6"]).all() and np.isfinite(ref["f64:rays6"]).all()
    check_grads_elem(lambda _: ref["rays6"], ["rays6"], ref, "", f"eval_grad_oracle32_{name}")
    _RAY_REF[key] = dict(rays=rays, cot=cot, kw=dict(N_samples=Ns, N_importance=Ni, perturb=0, noise_std=0,
                                                     chunk=32768), ref=ref)
    return _RAY_REF[key]


def hip_rays_grad(c):
    mc, mf, emb = model(), model(SEED_F, NOF_fine), Embedding(3, 10)
    rays = c["rays"].to(DEV).requires_grad_(True)
    out = R.render_rays_val(mc, mf, emb, rays, **c["kw"])
    assert out["depth"].requires_grad and out["depth_fine"].requires_grad
    (c["cot"].to(DEV) * (out["depth"] + out["depth_fine"])).sum().backward()
    return out, rays.grad, (mc, mf, emb)


def check_rays_case(name, switch):
    with switched(switch):
        c = ray_case(name, switch)
        out, grad, (mc, mf, emb) = hip_rays_grad(c)
        with torch.no_grad():
            plain = R.render_rays_val(mc, mf, emb, c["rays"].to(DEV), **c["kw"])
    for k in ("depth", "depth_fine"):   # the differentiable call's forward is the forward-only call's, bit for bit
        assert torch.equal(out[k].detach(), plain[k]), k
    assert tuple(grad.shape) == tuple(c["rays"].shape) and grad.dtype == torch.float32
    assert not grad[:, 6:].any(), "columns >= 6 carry no gradient"
    worst = check_grads_elem(lambda _: grad[:, :6].cpu().numpy(), ["rays6"], c["ref"], "",
                             f"eval_grad_rays_{name}_{switch}")
    print(f"render_rays_val {name} [{switch}]: max err/tol {worst['rays6'][0]:.3g}, "
          f"max |err| / max |ref| {worst['rays6'][1]:.3g}")


@pytest.mark.parametrize("name", list(RAY_CASES))
def test_render_rays_val_grad_vs_oracle(name):
    check_rays_case(name, "default")


def test_only_one_depth_used():
    """Backward from depth_fine alone and from depth alone add up to the backward from both (each pass is its own
    node; the coarse pass's gradient does not depend on the fine one's)."""
    c = ray_case("r130")
    mc, mf, emb = model(), model(SEED_F, NOF_fine), Embedding(3, 10)
    grads = []
    for keys in (("depth",), ("depth_fine",)):
        rays = c["rays"].to(DEV).requires_grad_(True)
        out = R.render_rays_val(mc, mf, emb, rays, **c["kw"])
        sum((c["cot"].to(DEV) * out[k]).sum() for k in keys).backward()
        grads.append(rays.grad)
    both = hip_rays_grad(c)[1]
    assert grads[0].abs().max() > 0 and grads[1].abs().max() > 0
    assert torch.equal(grads[0] + grads[1], both)   # autograd accumulates the two nodes' float32 results


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_backward_is_bit_reproducible(g):
    a, b = hip_points_grad(g, "n")[1], hip_points_grad(g, "n")[1]
    assert torch.equal(a, b)
    c = ray_case("r130")
    assert torch.equal(hip_rays_grad(c)[1], hip_rays_grad(c)[1])


# ------------------------------------------------------------------------------------------------ 5. eval paths
@pytest.mark.parametrize("switch", ["eval_fold", "eval_math_fp32"])
def test_grads_independent_of_eval_path(switch, g):
    """The Jacobian is the fold vector whichever eval path computed p: the same checks pass under the opt-in paths."""
    with switched(switch):
        check_points_case(g, "a", switch)
    check_rays_case("r130", switch)


# ------------------------------------------------------------------------------------------------ 6. refusals
def val_args(g, **over):
    a = dict(pts=dev(g["a/pts"]), z=dev(g["a/z"]))
    a.update(over)
    nfc = torch.zeros(a["pts"].shape[0], 2, device=DEV)
    return (Embedding(3, 10), a["pts"], None, a["z"], nfc, None, None, None)


def test_train_mode_module_refuses_differentiable_geometry(g):
    c = ray_case("r130")
    rays = c["rays"].to(DEV).requires_grad_(True)
    for mc, mf in ((model(train=True), model(SEED_F, NOF_fine)), (model(), model(SEED_F, NOF_fine, train=True))):
        with pytest.raises(NotImplementedError, match="train-mode"):
            R.render_rays_val(mc, mf, Embedding(3, 10), rays, **c["kw"])
        assert [int(b.num_batches_tracked) for b in mc.norms() + mf.norms()] == [0] * 16
    with pytest.raises(NotImplementedError, match="train-mode"):
        R.inference_val(model(train=True), *val_args(g, pts=dev(g["a/pts"]).requires_grad_(True)), noise_std=0)


def test_z_vals_requiring_grad_refused(g):
    with pytest.raises(NotImplementedError, match="z_vals"):
        R.inference_val(model(), *val_args(g, pts=dev(g["a/pts"]).requires_grad_(True),
                                           z=dev(g["a/z"]).requires_grad_(True)), noise_std=0)


def test_parameters_requiring_grad_keep_their_error(g):
    c = ray_case("r130")
    with pytest.raises(NotImplementedError, match="forward-only"):
        R.render_rays_val(model(frozen=False), model(SEED_F, NOF_fine), Embedding(3, 10),
                          c["rays"].to(DEV).requires_grad_(True), **c["kw"])
    with pytest.raises(NotImplementedError, match="forward-only"):
        R.inference_val(model(frozen=False), *val_args(g, pts=dev(g["a/pts"]).requires_grad_(True)), noise_std=0)


def test_other_helpers_still_refuse_grad_on_positions(g):
    pts = dev(g["a/pts"]).requires_grad_(True)
    z = dev(g["a/z"])
    nfc = torch.zeros(pts.shape[0], 2, device=DEV)
    rr = torch.ones(pts.shape[0], 1, device=DEV)
    with pytest.raises(NotImplementedError, match="samples_xy"):
        R.inference_train(model(train=True, frozen=False), Embedding(3, 10), pts, None, z, nfc, None, rr, None,
                          chunk=500, noise_std=0)
    with pytest.raises(NotImplementedError, match="samples_xy"):
        R.inference(model(), Embedding(3, 10), pts, z, noise_std=0)


def test_no_grad_call_with_grad_requiring_inputs_is_forward_only(g):
    pts = dev(g["a/pts"]).requires_grad_(True)
    with torch.no_grad():
        d, w = R.inference_val(model(), *val_args(g, pts=pts), noise_std=0)
        d0, w0 = R.inference_val(model(), *val_args(g), noise_std=0)
    assert not d.requires_grad and torch.equal(d, d0) and torch.equal(w, w0)


def test_new_operators_operand_checks():
    fold = P.fold_eval(T.eval_params(model()))
    assert tuple(fold.shape) == (64,) and fold.dtype == torch.float64 and torch.isfinite(fold).all()
    assert torch.equal(fold, _ops.fold_eval(model(), torch.device(DEV)))
    pts, gl = torch.rand(35, 3, device=DEV), torch.rand(35, device=DEV)
    rays, z, glr = torch.rand(5, 8, device=DEV), torch.rand(5, 7, device=DEV), torch.rand(5, 7, device=DEV)
    assert tuple(P.points_grad_eval(pts, gl, fold).shape) == (35, 3)
    assert tuple(P.points_grad_eval(pts[:0], gl[:0], fold).shape) == (0, 3)   # empty: no launch
    assert tuple(P.rays_grad_eval(rays, z, glr, fold).shape) == (5, 6)
    for bad in (lambda: P.points_grad_eval(pts.cpu(), gl, fold), lambda: P.points_grad_eval(pts, gl.cpu(), fold),
                lambda: P.points_grad_eval(pts, gl, fold.cpu()), lambda: P.rays_grad_eval(rays.cpu(), z, glr, fold),
                lambda: P.rays_grad_eval(rays, z.cpu(), glr, fold), lambda: P.rays_grad_eval(rays, z, glr.cpu(), fold),
                lambda: P.fold_eval([t.cpu() for t in T.eval_params(model())])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            bad()
    for bad in (lambda: P.points_grad_eval(pts.double(), gl, fold), lambda: P.points_grad_eval(pts, gl.double(), fold),
                lambda: P.rays_grad_eval(rays.double(), z, glr, fold), lambda: P.rays_grad_eval(rays, z.double(), glr, fold),
                lambda: P.rays_grad_eval(rays, z, glr.double(), fold)):
        with pytest.raises(RuntimeError, match="float32"):
            bad()
    for bad in (lambda: P.points_grad_eval(pts, gl, fold.float()), lambda: P.rays_grad_eval(rays, z, glr, fold.float())):
        with pytest.raises(RuntimeError, match="float64"):
            bad()
    for bad in (lambda: P.points_grad_eval(torch.rand(3, 35, device=DEV).t(), gl, fold),
                lambda: P.rays_grad_eval(torch.rand(8, 5, device=DEV).t(), z, glr, fold),
                lambda: P.rays_grad_eval(rays, torch.rand(7, 5, device=DEV).t(), glr, fold),
                lambda: P.rays_grad_eval(rays, z, torch.rand(7, 5, device=DEV).t(), fold)):
        with pytest.raises(RuntimeError, match="contiguous"):
            bad()
    for bad in (lambda: P.points_grad_eval(torch.rand(35, 2, device=DEV), gl, fold),
                lambda: P.points_grad_eval(pts, gl[:34].contiguous(), fold),
                lambda: P.points_grad_eval(pts, gl, fold[:63].contiguous()),
                lambda: P.rays_grad_eval(rays[:, :5].contiguous(), z, glr, fold),
                lambda: P.rays_grad_eval(rays[:4].contiguous(), z, glr, fold),
                lambda: P.rays_grad_eval(rays, z, glr[:, :6].contiguous(), fold),
                lambda: P.rays_grad_eval(rays, z[:, :0].contiguous(), glr[:, :0].contiguous(), fold),
                lambda: P.rays_grad_eval(rays, z, glr, torch.zeros(65, dtype=torch.float64, device=DEV)),
                lambda: P.fold_eval(T.eval_params(model())[:49])):
        with pytest.raises(RuntimeError, match="expected|takes 50"):
            bad()
