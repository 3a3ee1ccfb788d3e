"""Scan-to-field registration, the parts that need no GPU: nof.registration's SE(3) maps, pose Jacobian and scan rays
against float64 restatements, the float64 helper of tests/registration_ref.py against autograd, its registration loop
on the analytic scene, and the two operators' fake shapes and host-side operand checks (layout first, device last, so
a wrong call is refused here as it is on the device)."""
import math

import numpy as np
import pytest
import torch

import registration_ref as RR
from nof import _torch_ops as T
from nof import registration as G

P = torch.ops.pcnerf
TWISTS = ([0.0] * 6, [0.3, -0.2, 0.1, 0.0, 0.0, 0.0], [0.1, 0.2, -0.3, 1e-9, -2e-9, 1e-9],
          [0.1, -0.05, 0.08, 0.05, -0.03, 0.1], [1.0, 2.0, -0.5, 0.3, 0.4, -0.2], [0.2, 0.1, 0.3, 1.2, -2.0, 1.5],
          [-0.4, 0.3, 0.2, 0.45, 0.1, -0.15])


def _twist_matrix(xi):
    """The 4 x 4 element of se(3) of xi = (rho, phi), differentiable."""
    z = xi.new_zeros(())
    rows = [torch.stack([z, -xi[5], xi[4], xi[0]]), torch.stack([xi[5], z, -xi[3], xi[1]]),
            torch.stack([-xi[4], xi[3], z, xi[2]]), torch.stack([z, z, z, z])]
    return torch.stack(rows)


@pytest.mark.parametrize("xi", TWISTS)
def test_se3_exp_log_round_trip_and_matrix_exp(xi):
    x = torch.tensor(xi, dtype=torch.float64)
    E = G.se3_exp(x)
    assert E.dtype == torch.float64 and tuple(E.shape) == (4, 4)
    assert (E - torch.linalg.matrix_exp(_twist_matrix(x))).abs().max() <= 1e-12
    back = G.se3_log(E)
    assert (back - x).abs().max() <= 1e-12
    assert (G.se3_exp(back) - E).abs().max() <= 1e-12


def test_pose_jacobian_matches_autograd_through_the_pose():
    """[J_o, o x J_o + d x J_d] against float64 autograd of depth through exp(xi) T at xi = 0: analytic field, 32
    rays, 48 samples at fixed depths."""
    fold = RR.analytic_fold()
    T_star = G.se3_exp(RR.XI_STAR)
    dirs = RR.unit_directions(32, 3)
    rays = RR.rays_f64(dirs, T_star)
    z = RR.O.lin_z(rays[:, 6:7], rays[:, 7:8], 48).double()
    _, _, _, jac6 = RR.render(fold, rays, z, torch.float64)
    got = G.pose_jacobian(rays[:, :6], jac6)

    def depth_of(xi):
        Tp = torch.linalg.matrix_exp(_twist_matrix(xi)) @ T_star
        o, d = Tp[:3, 3].expand_as(dirs), dirs @ Tp[:3, :3].T
        x = o[:, None, :] + d[:, None, :] * z[..., None]
        return RR.O.composite(torch.sigmoid(RR.fold_logit(fold, x)), z, RR.EPS)[1]

    want = torch.autograd.functional.jacobian(depth_of, torch.zeros(6, dtype=torch.float64))
    assert tuple(got.shape) == (32, 6) and float(want.abs().max()) > 1e-2
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())
    np.testing.assert_allclose(RR.pose_jacobian(rays[:, :6].numpy(), jac6.numpy()), got.numpy(), rtol=0, atol=1e-13)


def test_scan_rays_against_float64_slab_test():
    s = RR.scene()
    pts = (s["dirs"] * s["ranges"][:, None]).float()
    rays, rng = G.scan_rays(pts, s["T_star"], RR.PARENT_LO, RR.PARENT_HI, RR.NEAR)
    assert rays.dtype == torch.float32 and tuple(rays.shape) == (2048, 8) and rng.dtype == torch.float32
    p64 = pts.double()
    want = RR.rays_f64(p64 / p64.norm(dim=-1, keepdim=True), s["T_star"])
    assert torch.equal(rays[:, 6], torch.full((2048,), RR.NEAR, dtype=torch.float32))
    assert float((rays[:, 3:6].double().norm(dim=-1) - 1).abs().max()) <= 2e-7
    assert float((rays[:, :6].double() - want[:, :6]).abs().max()) <= 1e-7
    assert float(((rays[:, 7].double() - want[:, 7]) / want[:, 7]).abs().max()) <= 1.2e-7
    assert float((rng.double() - p64.norm(dim=-1)).abs().max()) <= 1.3e-7
    assert float(rays[:, 7].min()) > float(rng.max())   # the box contains the cavity
    # a ray parallel to two axes, from inside the box: those slabs do not limit it, no NaN
    r1, _ = G.scan_rays(torch.tensor([[0.0, 0.0, 2.0]]), torch.eye(4, dtype=torch.float64), RR.PARENT_LO,
                        RR.PARENT_HI, RR.NEAR)
    assert r1[0].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, np.float32(RR.NEAR), 2.5]
    # an origin outside the box in the ray's direction: far never falls below near
    out = torch.eye(4, dtype=torch.float64)
    out[2, 3] = 3.0
    r2, _ = G.scan_rays(torch.tensor([[0.0, 0.0, 2.0]]), out, RR.PARENT_LO, RR.PARENT_HI, RR.NEAR)
    assert float(r2[0, 7]) == float(np.float32(RR.NEAR))


def test_closed_form_ddepth_dlogit_matches_autograd():
    """To 1e-12 of each ray's largest entry; a ray whose first p is exactly 1 (every entry exactly zero: nothing
    divides by 1 - p) and a ray with every p < 1e-12."""
    g = torch.Generator().manual_seed(5)
    R, S = 8, 40
    logit = 3 * torch.randn(R, S, generator=g, dtype=torch.float64) - 2
    logit[1, 0] = 40.0
    logit[2] = -30.0 - torch.rand(S, generator=g, dtype=torch.float64)
    logit[3, 2] = 40.0   # saturates at the third sample
    z = torch.sort(0.5 + 3 * torch.rand(R, S, generator=g, dtype=torch.float64), -1)[0]
    p = torch.sigmoid(logit)
    assert float(p[1, 0]) == 1.0 and float(p[2].max()) < 1e-12 and float(p[3, 2]) == 1.0
    got, want = RR.ddepth_dlogit(p, z), RR.ddepth_dlogit_autograd(logit, z)
    assert torch.isfinite(got).all() and torch.isfinite(want).all()
    scale = want.abs().amax(-1, keepdim=True)
    assert float(((got - want).abs() - 1e-12 * scale).max()) <= 0
    assert float(got[1].abs().max()) == 0.0 and float(want[1].abs().max()) == 0.0
    assert float(got[3, 3:].abs().max()) == 0.0 and float(scale[2]) > 0


def test_float64_loop_converges_on_the_analytic_scene():
    """2,048 directions, start exp([0.12, -0.10, 0.10, 2 deg, -1.5 deg, 2 deg]) T*, 64 + 128 samples: within 20
    iterations the pose is < 1e-4 m and < 1e-4 rad from T*, and the cost never increases.  Measured: 0.185 m /
    0.0559 rad at the start, 4.5e-5 m / 1.0e-5 rad after 20 iterations, a factor ~0.66 per iteration (linear: the
    fine depths are constants of the Jacobian), cond(H) 26."""
    s = RR.scene()
    run = s["run"]
    assert 0.69 <= float(s["ranges"].min()) and float(s["ranges"].max()) <= 2.06 and float(s["sumw"].min()) > 0.99
    e0 = RR.pose_error(s["T0"], s["T_star"])
    assert abs(e0[0] - 0.1853) < 1e-3 and abs(e0[1] - 0.0559) < 1e-3
    et, er = RR.pose_error(run["pose"], s["T_star"])
    print("float64 loop:", run["errors"][0], "->", (et, er), "cond", run["cond"])
    assert et < 1e-4 and er < 1e-4
    assert len(run["all_costs"]) == 20 and run["n_valid"] == 2048
    assert all(b <= a for a, b in zip(run["all_costs"], run["all_costs"][1:]))
    assert run["costs"] == run["all_costs"]


def test_unpack_and_solve_match_numpy():
    rng = np.random.default_rng(0)
    J = rng.normal(size=(50, 6))
    r = rng.normal(size=50)
    out = np.zeros(30)
    Hm = J.T @ J
    out[:21] = Hm[np.triu_indices(6)]
    out[21:27] = J.T @ r
    out[27], out[28] = 0.5 * r @ r, 50
    H, b, cost, n = G.unpack_normal_eq(out)
    np.testing.assert_allclose(H, Hm, rtol=0, atol=0)
    assert n == 50 and cost == out[27]
    np.testing.assert_allclose(G.lm_step(H, b, 0.0), -np.linalg.lstsq(J, r, rcond=None)[0], rtol=1e-9)


# ----------------------------------------------------------------------------------------------- operators
def test_operators_registered_with_schemas():
    for name in ("render_jac_fold", "gn_normal_eq"):
        assert name in T.op_names()
        assert str(getattr(P, name).default._schema).startswith(f"pcnerf::{name}(")


@pytest.mark.parametrize("ww,wj", [(True, True), (True, False), (False, True), (False, False)])
def test_fake_shapes_and_dtypes(ww, wj):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        rays, z = torch.empty(5, 8, device="meta"), torch.empty(5, 48, device="meta")
        fold = torch.empty(64, dtype=torch.float64, device="meta")
        depth, sumw, w, jac = P.render_jac_fold(rays, z, fold, 1e-10, ww, wj)
        assert depth.shape == (5,) and sumw.shape == (5,)
        assert w.shape == ((5, 48) if ww else (0,)) and jac.shape == ((5, 6) if wj else (0,))
        assert {t.dtype for t in (depth, sumw, w, jac)} == {torch.float32}
        out = P.gn_normal_eq(rays, torch.empty(5, 6, device="meta"), depth, sumw, torch.empty(5, device="meta"),
                             0.1, 0.5)
        assert out.shape == (30,) and out.dtype == torch.float64


def _operands(R=4, S=8, cols=8):
    return torch.rand(R, cols), torch.rand(R, S), torch.zeros(64, dtype=torch.float64)


def test_render_jac_fold_rejects_bad_operands():
    rays, z, fold = _operands()
    with pytest.raises(RuntimeError, match="no CPU path"):   # right layouts, wrong place
        P.render_jac_fold(rays, z, fold, 1e-10, True, True)
    with pytest.raises(RuntimeError, match="rays must be a contiguous torch.float32"):
        P.render_jac_fold(rays.double(), z, fold, 1e-10, True, True)
    with pytest.raises(RuntimeError, match="z must be a contiguous torch.float32"):
        P.render_jac_fold(rays, z.half(), fold, 1e-10, True, True)
    with pytest.raises(RuntimeError, match="z must be a contiguous"):
        P.render_jac_fold(rays, torch.rand(8, 4).t(), fold, 1e-10, True, True)
    with pytest.raises(RuntimeError, match="fold must be a contiguous torch.float64"):
        P.render_jac_fold(rays, z, fold.float(), 1e-10, True, True)
    with pytest.raises(RuntimeError, match="fold has shape"):
        P.render_jac_fold(rays, z, fold[:63].contiguous(), 1e-10, True, True)
    with pytest.raises(RuntimeError, match="z has shape"):   # S = 0
        P.render_jac_fold(rays, torch.rand(4, 0), fold, 1e-10, True, True)
    with pytest.raises(RuntimeError, match="at most 1024"):
        P.render_jac_fold(rays, torch.rand(4, 1025), fold, 1e-10, True, True)
    with pytest.raises(RuntimeError, match="rays has shape"):   # 5 ray columns
        P.render_jac_fold(torch.rand(4, 5), z, fold, 1e-10, True, True)
    with pytest.raises(RuntimeError, match="rays has shape"):   # rows differ
        P.render_jac_fold(torch.rand(3, 8), z, fold, 1e-10, True, True)


def test_gn_normal_eq_rejects_bad_operands():
    rays = torch.rand(4, 8)
    jac, d, sw, tg = torch.rand(4, 6), torch.rand(4), torch.rand(4), torch.rand(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.gn_normal_eq(rays, jac, d, sw, tg, 0.0, 0.5)
    with pytest.raises(RuntimeError, match="jac6 has shape"):
        P.gn_normal_eq(rays, torch.rand(4, 5), d, sw, tg, 0.0, 0.5)
    with pytest.raises(RuntimeError, match="rays has shape"):
        P.gn_normal_eq(torch.rand(4, 5), jac, d, sw, tg, 0.0, 0.5)
    with pytest.raises(RuntimeError, match="target has shape"):
        P.gn_normal_eq(rays, jac, d, sw, torch.rand(3), 0.0, 0.5)
    with pytest.raises(RuntimeError, match="sumw must be a contiguous"):
        P.gn_normal_eq(rays, jac, d, sw.double(), tg, 0.0, 0.5)
    with pytest.raises(RuntimeError, match="depth has shape"):
        P.gn_normal_eq(rays, jac, d[:, None], sw, tg, 0.0, 0.5)


def test_registration_refuses_host_scans_and_unfrozen_modules():
    from nof import _ops
    from nof import synthetic as syn
    from nof.networks import NOF_coarse, NOF_fine
    pts = torch.rand(16, 3) + 0.5
    eye = torch.eye(4, dtype=torch.float64)
    fold = RR.analytic_fold()
    with pytest.raises(RuntimeError, match="no CPU path"):
        G.register_scan_fold(fold, fold, pts, eye, RR.PARENT_LO, RR.PARENT_HI)
    mc = syn.load_into(NOF_coarse(), syn.init_nof_params(1))
    mf = syn.load_into(NOF_fine(), syn.init_nof_params(2))
    math_before, fold_before = _ops.get_eval_math(), _ops.eval_fold_enabled()
    with pytest.raises(NotImplementedError, match="train-mode"):
        G.register_scan(mc.train(), mf.eval(), pts, eye, RR.PARENT_LO, RR.PARENT_HI)
    with pytest.raises(NotImplementedError, match="require grad"):
        G.register_scan(mc.eval(), mf.eval(), pts, eye, RR.PARENT_LO, RR.PARENT_HI)
    assert (_ops.get_eval_math(), _ops.eval_fold_enabled()) == (math_before, fold_before)
    with pytest.raises(RuntimeError, match="exceeds"):
        G.render_scan(fold, fold, torch.rand(4, 8), 512, 513)
    assert math.isclose(float(G.EPSILON), 1e-10)
