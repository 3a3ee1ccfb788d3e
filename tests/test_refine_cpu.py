"""Batched pose refinement, the parts that need no GPU: the five operators' schemas, fake shapes and host-side operand
checks (layout first, then the sample limits, the device last), the C entries' declaration, binding and argument
errors, nof.registration's refusals, localize_scan_fold's new keyword, and the restatement of the per-pose state machine
(tests/refine_ref.py) against registration_ref.register_f64 on the 256-beam scene."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import localization_ref as LR
import refine_ref as FR
import registration_ref as RR
from nof import _hip
from nof import _torch_ops as T
from nof import localization as L
from nof import registration as G

P = torch.ops.pcnerf
OPS = ("pose_normal_eq_fold", "lm_init", "lm_update", "refine_poses_fold", "se3_apply")
NEW = {"pcnerf_pose_normal_eq_workspace_bytes": 2, "pcnerf_pose_normal_eq_fold": 21, "pcnerf_lm_init": 5,
       "pcnerf_lm_update": 9, "pcnerf_refine_poses_fold": 24, "pcnerf_se3_apply": 5}


# ----------------------------------------------------------------------------------------------- operators
def test_operators_registered_with_schemas():
    names = T.op_names()
    assert names[-5:] == list(OPS)   # appended: the earlier names keep their places
    for op in OPS:
        assert str(getattr(P, op).default._schema).startswith(f"pcnerf::{op}("), op
    assert T.LM_STATE_DOUBLES == 64


@pytest.mark.parametrize("want_beams", [False, True])
def test_fake_shapes_and_dtypes(want_beams):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        pts = torch.empty(7, 3, device="meta")
        poses = torch.empty(5, 12, dtype=torch.float64, device="meta")
        box = torch.empty(6, dtype=torch.float64, device="meta")
        fold = torch.empty(64, dtype=torch.float64, device="meta")
        state = P.lm_init(poses, 1e-6)
        assert state.shape == (5, 64) and state.dtype == torch.float64
        for src in ((poses, None), (None, state)):
            n30, depth, sumw, jac = P.pose_normal_eq_fold(pts, src[0], src[1], box, fold, fold, 0.05, 64, 128, 1e-10,
                                                          0.0, 0.5, want_beams)
            assert n30.shape == (5, 30) and n30.dtype == torch.float64
            assert depth.shape == sumw.shape == ((5, 7) if want_beams else (0,))
            assert jac.shape == ((5, 7, 6) if want_beams else (0,))
            assert depth.dtype == sumw.dtype == jac.dtype == torch.float32
        st2, cost, acc = P.lm_update(n30, state, 1e-9)
        assert st2.shape == (5, 64) and st2.dtype == torch.float64
        assert cost.shape == acc.shape == (5,) and cost.dtype == torch.float64 and acc.dtype == torch.uint8
        out, st3, costs, mask = P.refine_poses_fold(pts, poses, box, fold, fold, 0.05, 64, 128, 1e-10, 0.0, 0.5, 1e-6,
                                                    1e-9, 20)
        assert out.shape == (5, 12) and st3.shape == (5, 64) and out.dtype == st3.dtype == torch.float64
        assert costs.shape == mask.shape == (5, 20) and costs.dtype == torch.float64 and mask.dtype == torch.uint8
        moved = P.se3_apply(torch.empty(5, 6, dtype=torch.float64, device="meta"), poses)
        assert moved.shape == (5, 12) and moved.dtype == torch.float64


def _operands(R=4, Pn=3):
    return (torch.rand(R, 3) + 0.5, torch.rand(Pn, 12, dtype=torch.float64), torch.rand(6, dtype=torch.float64),
            torch.zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64))


def _eval(pts, poses, box, fc, ff, S=64, I=128, state=None):
    return P.pose_normal_eq_fold(pts, poses, state, box, fc, ff, 0.05, S, I, 1e-10, 0.0, 0.5, False)


def _refine(pts, poses, box, fc, ff, S=64, I=128, iters=2):
    return P.refine_poses_fold(pts, poses, box, fc, ff, 0.05, S, I, 1e-10, 0.0, 0.5, 1e-6, 1e-9, iters)


@pytest.mark.parametrize("call", [_eval, _refine])
def test_render_operators_reject_bad_operands_and_sample_limits(call):
    pts, poses, box, fc, ff = _operands()
    with pytest.raises(RuntimeError, match="no CPU path"):   # right layouts, wrong place
        call(pts, poses, box, fc, ff)
    with pytest.raises(RuntimeError, match="points must be a contiguous torch.float32"):
        call(pts.double(), poses, box, fc, ff)
    with pytest.raises(RuntimeError, match="points has shape"):
        call(torch.rand(4, 4), poses, box, fc, ff)
    with pytest.raises(RuntimeError, match="points must be a contiguous"):
        call(torch.rand(3, 4).t(), poses, box, fc, ff)
    with pytest.raises(RuntimeError, match="poses12 must be a contiguous torch.float64"):
        call(pts, poses.float(), box, fc, ff)
    with pytest.raises(RuntimeError, match="poses12 has shape"):
        call(pts, torch.rand(3, 16, dtype=torch.float64), box, fc, ff)
    with pytest.raises(RuntimeError, match="box6 has shape"):
        call(pts, poses, box[:5].contiguous(), fc, ff)
    with pytest.raises(RuntimeError, match="fold_coarse must be a contiguous torch.float64"):
        call(pts, poses, box, fc.float(), ff)
    with pytest.raises(RuntimeError, match="fold_fine has shape"):
        call(pts, poses, box, fc, ff[:63].contiguous())
    # the sample limits, before anything looks for a device
    with pytest.raises(RuntimeError, match="at most 1024"):
        call(pts, poses, box, fc, ff, 512, 513)
    with pytest.raises(RuntimeError, match="at least 3"):
        call(pts, poses, box, fc, ff, 2, 8)
    with pytest.raises(RuntimeError, match="at least 1 "):
        call(pts, poses, box, fc, ff, 8, 0)


def test_state_operators_reject_bad_operands():
    pts, poses, box, fc, ff = _operands()
    state, n30 = torch.zeros(3, 64, dtype=torch.float64), torch.zeros(3, 30, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="one of poses12 and state"):
        _eval(pts, None, box, fc, ff)
    with pytest.raises(RuntimeError, match="state has shape"):
        _eval(pts, None, box, fc, ff, state=torch.zeros(3, 63, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="state must be a contiguous torch.float64"):
        _eval(pts, None, box, fc, ff, state=state.float())
    with pytest.raises(RuntimeError, match="no CPU path"):
        _eval(pts, None, box, fc, ff, state=state)
    with pytest.raises(RuntimeError, match="negative"):
        _refine(pts, poses, box, fc, ff, iters=-1)
    # lm_init
    with pytest.raises(RuntimeError, match="poses12 has shape"):
        P.lm_init(torch.zeros(3, 16, dtype=torch.float64), 1e-6)
    with pytest.raises(RuntimeError, match="poses12 must be a contiguous torch.float64"):
        P.lm_init(poses.float(), 1e-6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.lm_init(poses, 1e-6)
    # lm_update
    with pytest.raises(RuntimeError, match="state has shape"):
        P.lm_update(n30, torch.zeros(3, 60, dtype=torch.float64), 1e-9)
    with pytest.raises(RuntimeError, match="normal30 has shape"):
        P.lm_update(torch.zeros(2, 30, dtype=torch.float64), state, 1e-9)
    with pytest.raises(RuntimeError, match="normal30 must be a contiguous torch.float64"):
        P.lm_update(n30.float(), state, 1e-9)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.lm_update(n30, state, 1e-9)
    # se3_apply
    xi = torch.zeros(3, 6, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="xi6 has shape"):
        P.se3_apply(xi[:2].contiguous(), poses)
    with pytest.raises(RuntimeError, match="xi6 must be a contiguous torch.float64"):
        P.se3_apply(xi.float(), poses)
    with pytest.raises(RuntimeError, match="poses12 has shape"):
        P.se3_apply(xi, torch.zeros(3, 4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.se3_apply(xi, poses)


# ----------------------------------------------------------------------------------------------- C ABI
def test_symbols_declared_bound_and_exported():
    header = (Path(__file__).resolve().parents[1] / "include" / "pcnerf_hip.h").read_text()
    lib = _hip.lib()
    for name, arity in NEW.items():
        decl = re.search(r"\b(size_t|int)\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in _hip.exported_symbols() and hasattr(lib, name), name
        assert len(decl.group(2).split(",")) == len(_hip._SIGS[name][1]) == arity, name
    assert re.search(r"#define\s+PCNERF_LM_STATE_DOUBLES\s+64\b", header)
    assert lib.pcnerf_abi_version() == 1


def test_workspace_bytes_follow_the_counts_alone():
    f = _hip.lib().pcnerf_pose_normal_eq_workspace_bytes   # 32 doubles per four beams of a pose
    assert f(0, 5) == 0 and f(5, 0) == 0 and f(-1, 8) == 0
    assert f(1, 1) == 256 and f(1, 4) == 256 and f(1, 5) == 512 and f(3, 5) == 1536
    assert f(1024, 2048) == 1024 * 512 * 256


def test_argument_errors_reach_no_device():
    lib = _hip.lib()

    def ev(R, Pn, S, I):
        return lib.pcnerf_pose_normal_eq_fold(None, R, None, Pn, None, None, 0.05, S, I, None, None, 1e-10, 0.0, 0.5,
                                              None, 0, None, None, None, None, None)

    def rf(R, Pn, S, I, iters=2):
        return lib.pcnerf_refine_poses_fold(None, R, None, Pn, None, 0.05, S, I, None, None, 1e-10, 0.0, 0.5, 1e-6,
                                            1e-9, iters, None, 0, None, None, None, None, None, None)

    for call in (ev, rf):
        assert call(8, 0, 64, 128) == 0   # no poses: a no-op
        for args, word in (((8, 4, 2, 8), b"n_samples < 3"), ((8, 4, 8, 0), b"n_importance < 1"),
                           ((8, 4, 512, 513), b"> 1024"), ((8, 0, 1024, 1), b"> 1024"),
                           ((-1, 4, 64, 128), b"negative"), ((8, -1, 64, 128), b"negative"),
                           ((8, 4, 64, 128), b"null"), ((0, 4, 64, 128), b"null")):
            assert call(*args) == -1, word
            assert word in lib.pcnerf_last_error(), (word, lib.pcnerf_last_error())
    assert rf(8, 4, 64, 128, iters=-1) == -1 and b"iters < 0" in lib.pcnerf_last_error()
    assert lib.pcnerf_lm_init(None, 0, 1e-6, None, None) == 0
    assert lib.pcnerf_lm_init(None, 3, 1e-6, None, None) == -1 and b"null" in lib.pcnerf_last_error()
    assert lib.pcnerf_lm_init(None, -1, 1e-6, None, None) == -1 and b"negative" in lib.pcnerf_last_error()
    assert lib.pcnerf_lm_update(None, 0, 1e-9, None, None, None, 0, 1, None) == 0
    assert lib.pcnerf_lm_update(None, 3, 1e-9, None, None, None, 0, 1, None) == -1
    assert b"null" in lib.pcnerf_last_error()
    assert lib.pcnerf_lm_update(None, -2, 1e-9, None, None, None, 0, 1, None) == -1
    assert b"negative" in lib.pcnerf_last_error()
    assert lib.pcnerf_se3_apply(None, None, 0, None, None) == 0
    assert lib.pcnerf_se3_apply(None, None, 2, None, None) == -1 and b"null" in lib.pcnerf_last_error()
    assert lib.pcnerf_se3_apply(None, None, -2, None, None) == -1 and b"negative" in lib.pcnerf_last_error()


# ----------------------------------------------------------------------------------------------- public module
def test_refinement_refuses_host_scans_unfrozen_modules_and_bad_limits():
    from nof import _ops
    from nof import synthetic as syn
    from nof.networks import NOF_coarse, NOF_fine
    pts = torch.rand(16, 3) + 0.5
    poses = torch.eye(4, dtype=torch.float64)[None]
    fold = RR.analytic_fold()
    with pytest.raises(RuntimeError, match="no CPU path"):
        G.refine_poses_fold(fold, fold, pts, poses, RR.PARENT_LO, RR.PARENT_HI)
    with pytest.raises(RuntimeError, match="no CPU path"):
        G.apply_twists(poses, torch.zeros(1, 6, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.localize_scan_fold(fold, fold, pts, poses, RR.PARENT_LO, RR.PARENT_HI, refine="batched")
    with pytest.raises(ValueError, match="sequential"):
        L.localize_scan_fold(fold, fold, pts, poses, RR.PARENT_LO, RR.PARENT_HI, refine="both")
    mc = syn.load_into(NOF_coarse(), syn.init_nof_params(1))
    mf = syn.load_into(NOF_fine(), syn.init_nof_params(2))
    before = (_ops.get_eval_math(), _ops.eval_fold_enabled(), _ops.get_train_math())
    with pytest.raises(NotImplementedError, match="train-mode"):
        G.refine_poses(mc.train(), mf.eval(), pts, poses, RR.PARENT_LO, RR.PARENT_HI)
    with pytest.raises(NotImplementedError, match="require grad"):
        G.refine_poses(mc.eval(), mf.eval(), pts, poses, RR.PARENT_LO, RR.PARENT_HI)
    with pytest.raises(RuntimeError, match="no CPU path"):
        G.refine_poses(mc.eval().requires_grad_(False), mf.eval().requires_grad_(False), pts, poses, RR.PARENT_LO,
                       RR.PARENT_HI)
    assert (_ops.get_eval_math(), _ops.eval_fold_enabled(), _ops.get_train_math()) == before
    fields = G.RefineResult._fields
    assert fields[:8] == ("poses", "cost", "n_valid", "iterations", "accepted", "status", "eval_costs",
                          "accepted_mask")


# ----------------------------------------------------------------------------------------------- the state machine
def _n30(H, b, cost, n_valid):
    row = np.zeros(30)
    row[:21], row[21:27], row[27], row[28] = H[np.triu_indices(6)], b, cost, n_valid
    return row


def test_restatement_walks_every_branch():
    """Synthetic rows: first accept, accept (lambda / 10), reject (lambda x 10, the pose rewound), a NaN cost, a step
    below xi_tol (status 1), fewer than 6 valid beams (status 2) and a singular system (status 3)."""
    g = np.random.default_rng(0)
    A = g.standard_normal((12, 6))
    H, b = A.T @ A, g.standard_normal(6) * 0.01
    T0 = G.se3_exp(RR.XI_STAR)
    st = FR.lm_init(T0, 1e-3)
    assert FR.lm_update(st, _n30(H, b, 2.0, 40), 0.0, G.se3_exp) == (2.0, True)
    assert st["lam"] == 1e-3 and st["nacc"] == 1 and st["evals"] == 1 and torch.equal(st["T_acc"], T0)
    first = st["T_trial"].clone()
    assert FR.lm_update(st, _n30(H, 0.5 * b, 1.0, 41), 0.0, G.se3_exp) == (1.0, True)
    assert st["lam"] == 1e-3 / 10.0 and torch.equal(st["T_acc"], first) and st["n30"][28] == 41
    kept = st["T_acc"].clone()
    assert FR.lm_update(st, _n30(H, b, 1.5, 42), 0.0, G.se3_exp) == (1.5, False)
    assert st["lam"] == 1e-3 / 10.0 * 10.0 and torch.equal(st["T_acc"], kept) and st["n30"][28] == 41
    cost, acc = FR.lm_update(st, _n30(H, b, float("nan"), 42), 0.0, G.se3_exp)
    assert math.isnan(cost) and not acc and st["nacc"] == 2 and st["evals"] == 4 and st["status"] == 0
    assert FR.lm_update(st, _n30(H, 1e-12 * b, 0.5, 42), 1e-9, G.se3_exp) == (0.5, True)
    assert st["status"] == 1 and torch.equal(FR.pose_out(st), st["T_trial"])
    cost, acc = FR.lm_update(st, _n30(H, b, 0.1, 42), 0.0, G.se3_exp)   # stopped: nothing moves
    assert math.isnan(cost) and not acc and st["evals"] == 5
    few = FR.lm_init(T0, 1e-3)
    assert FR.lm_update(few, _n30(H, b, 2.0, 5), 0.0, G.se3_exp) == (2.0, False)
    assert few["status"] == 2 and few["evals"] == 1 and few["nacc"] == 0 and few["lam"] == 1e-3
    assert torch.equal(FR.pose_out(few), T0)
    sing = FR.lm_init(T0, 1e-3)
    Hs = H.copy()
    Hs[3, :] = Hs[:, 3] = 0.0
    assert FR.lm_update(sing, _n30(Hs, b, 2.0, 40), 0.0, G.se3_exp) == (2.0, True)
    assert sing["status"] == 3 and torch.equal(sing["T_trial"], T0) and sing["nacc"] == 1
    row = FR.to_row(st)
    back = FR.from_row(row)
    assert np.array_equal(FR.to_row(back), row) and row.shape == (64,)


def test_restatement_is_the_float64_loop_on_the_256_beam_scene():
    """Driven by registration_ref's float64 evaluations, the restatement reproduces register_f64's poses and accepted
    costs exactly from the four converging starts (all 20 evaluations accepted, final error within 4.6e-5 m /
    1.2e-5 rad, cond(H) about 23) and from the rejection start (10 of 20 accepted, not converged)."""
    s = LR.grid_scene()
    good, bad = FR.f64_runs()
    starts, bad_start = FR.starts()
    ev = FR.evaluate_f64(s["fold"], s["dirs"], s["ranges"].numpy())
    for T0, want in zip(starts + [bad_start], good + [bad]):
        got = FR.run(ev, T0, G.se3_exp)
        assert torch.equal(torch.as_tensor(got["pose"]), torch.as_tensor(want["pose"]))
        assert got["costs"] == want["costs"] and got["eval_costs"] == want["all_costs"]
        assert got["state"]["evals"] == 20 and got["state"]["status"] == 0
    for run in good:
        et, er = RR.pose_error(run["pose"], s["T_star"])
        print("float64 loop:", len(run["costs"]), et, er, run["cond"])
        assert len(run["costs"]) == 20 and et <= 4.6e-5 and er <= 1.2e-5 and 15 < run["cond"] < 35
    et, er = RR.pose_error(bad["pose"], s["T_star"])
    print("float64 loop, rejection start:", len(bad["costs"]), et, er)
    assert len(bad["costs"]) == 10 and max(et, er) > 1e-3
