"""Pose-hypothesis scoring, the parts that need no GPU: pose_grid, the operator's schema, fake shapes and host-side
operand checks (layout first, then the sample limits, the device last), the two C entries' binding and argument
errors, nof.localization's refusals, and the ranking fact of the float64 restatement (tests/localization_ref.py) that
the GPU end-to-end test relies on."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import localization_ref as LR
import registration_ref as RR
from nof import _hip
from nof import _torch_ops as T
from nof import localization as L
from nof import registration as G

P = torch.ops.pcnerf
NEW = ("pcnerf_score_poses_workspace_bytes", "pcnerf_score_poses_fold")


# ----------------------------------------------------------------------------------------------- pose_grid
def test_pose_grid_shape_order_centre_and_se3_exp():
    C = G.se3_exp([0.3, -0.2, 0.1, 0.05, -0.02, 0.7])
    g = L.pose_grid(C, 0.4, 0.2, math.radians(10.0), math.radians(5.0))
    assert g.dtype == torch.float64 and tuple(g.shape) == (125, 4, 4)
    assert torch.equal(g[62], C)   # the centre is hypothesis (2, 2, 0, 2)
    offs = [-0.4, -0.2, 0.0, 0.2, 0.4]
    yaws = [math.radians(v) for v in (-10.0, -5.0, 0.0, 5.0, 10.0)]
    for ix, iy, iw in ((0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (4, 3, 1), (2, 2, 2), (4, 4, 4)):
        want = G.se3_exp([ix * 0.2 - 0.4, iy * 0.2 - 0.4, 0.0, 0.0, 0.0, iw * math.radians(5.0) - math.radians(10.0)]) @ C
        assert float((g[(ix * 5 + iy) * 5 + iw] - want).abs().max()) <= 1e-15, (ix, iy, iw)
    # yaw fastest, x slowest: the translations offsets read back through the left perturbation
    eye = L.pose_grid(torch.eye(4, dtype=torch.float64), 0.4, 0.2, math.radians(10.0), math.radians(5.0))
    assert [round(float(eye[25 * i + 2, 0, 3]), 12) for i in range(5)] == [round(v, 12) for v in offs]
    yaw_of = [math.atan2(float(eye[k, 1, 0]), float(eye[k, 0, 0])) for k in range(5)]
    assert np.allclose(yaw_of, yaws, atol=1e-15)
    # z offsets sit between y and yaw; a half extent below one step leaves the centre alone
    gz = L.pose_grid(C, 0.2, 0.2, 0.0, 1.0, z_offsets=(-0.1, 0.0, 0.3))
    assert tuple(gz.shape) == (27, 4, 4) and torch.equal(gz[13], C)
    assert abs(float(gz[14, 2, 3] - C[2, 3]) - 0.3) <= 1e-15
    assert tuple(L.pose_grid(C, 0.1, 0.2, 0.01, 0.02).shape) == (1, 4, 4)
    with pytest.raises(ValueError):
        L.pose_grid(C, 0.4, 0.0, 0.1, 0.1)


# ----------------------------------------------------------------------------------------------- operator
def test_operator_registered_with_schema():
    assert "score_poses_fold" in T.op_names()
    assert str(P.score_poses_fold.default._schema).startswith("pcnerf::score_poses_fold(")


@pytest.mark.parametrize("want_depth", [False, True])
def test_fake_shapes_and_dtypes(want_depth):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        pts = torch.empty(7, 3, device="meta")
        poses = torch.empty(5, 12, dtype=torch.float64, device="meta")
        box = torch.empty(6, dtype=torch.float64, device="meta")
        fold = torch.empty(64, dtype=torch.float64, device="meta")
        s4, depth, sumw = P.score_poses_fold(pts, poses, box, fold, fold, 0.05, 64, 128, 1e-10, 0.0, 0.5, want_depth)
        assert s4.shape == (5, 4) and s4.dtype == torch.float64
        assert depth.shape == sumw.shape == ((5, 7) if want_depth else (0,))
        assert depth.dtype == sumw.dtype == torch.float32


def _operands(R=4, Pn=3):
    return (torch.rand(R, 3) + 0.5, torch.rand(Pn, 12, dtype=torch.float64), torch.rand(6, dtype=torch.float64),
            torch.zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64))


def _call(pts, poses, box, fc, ff, S=64, I=128):
    return P.score_poses_fold(pts, poses, box, fc, ff, 0.05, S, I, 1e-10, 0.0, 0.5, False)


def test_operator_rejects_bad_operands_and_sample_limits():
    pts, poses, box, fc, ff = _operands()
    with pytest.raises(RuntimeError, match="no CPU path"):   # right layouts, wrong place
        _call(pts, poses, box, fc, ff)
    with pytest.raises(RuntimeError, match="points must be a contiguous torch.float32"):
        _call(pts.double(), poses, box, fc, ff)
    with pytest.raises(RuntimeError, match="points has shape"):
        _call(torch.rand(4, 4), poses, box, fc, ff)
    with pytest.raises(RuntimeError, match="points must be a contiguous"):
        _call(torch.rand(3, 4).t(), poses, box, fc, ff)
    with pytest.raises(RuntimeError, match="poses12 must be a contiguous torch.float64"):
        _call(pts, poses.float(), box, fc, ff)
    with pytest.raises(RuntimeError, match="poses12 has shape"):
        _call(pts, torch.rand(3, 16, dtype=torch.float64), box, fc, ff)
    with pytest.raises(RuntimeError, match="box6 has shape"):
        _call(pts, poses, box[:5].contiguous(), fc, ff)
    with pytest.raises(RuntimeError, match="fold_coarse must be a contiguous torch.float64"):
        _call(pts, poses, box, fc.float(), ff)
    with pytest.raises(RuntimeError, match="fold_fine has shape"):
        _call(pts, poses, box, fc, ff[:63].contiguous())
    # the sample limits, before anything looks for a device
    with pytest.raises(RuntimeError, match="at most 1024"):
        _call(pts, poses, box, fc, ff, 512, 513)
    with pytest.raises(RuntimeError, match="at least 3"):
        _call(pts, poses, box, fc, ff, 2, 8)
    with pytest.raises(RuntimeError, match="at least 1 "):
        _call(pts, poses, box, fc, ff, 8, 0)


# ----------------------------------------------------------------------------------------------- C ABI
def test_symbols_declared_bound_and_exported():
    header = (Path(__file__).resolve().parents[1] / "include" / "pcnerf_hip.h").read_text()
    lib = _hip.lib()
    for name in NEW:
        assert re.search(r"\b(size_t|int)\s+%s\s*\(" % name, header), name
        assert name in _hip.exported_symbols() and hasattr(lib, name), name
    # the binding's arity is the declaration's
    decl = re.search(r"int\s+pcnerf_score_poses_fold\s*\(([^;]*)\);", header).group(1)
    assert len(decl.split(",")) == len(_hip._SIGS["pcnerf_score_poses_fold"][1]) == 19
    assert lib.pcnerf_abi_version() == 1


def test_workspace_bytes_follow_the_counts_alone():
    lib = _hip.lib()
    f = lib.pcnerf_score_poses_workspace_bytes   # 4 doubles per four beams of a pose
    assert f(0, 5) == 0 and f(5, 0) == 0 and f(-1, 8) == 0
    assert f(1, 1) == 32 and f(1, 4) == 32 and f(1, 5) == 64 and f(3, 5) == 192
    assert f(1024, 2048) == 1024 * 512 * 32


def test_score_poses_fold_argument_errors_reach_no_device():
    lib = _hip.lib()
    f = lib.pcnerf_score_poses_fold

    def call(R, Pn, S, I):
        return f(None, R, None, Pn, None, 0.05, S, I, None, None, 1e-10, 0.0, 0.5, None, 0, None, None, None, None)

    assert call(8, 0, 64, 128) == 0   # no poses: a no-op
    for args, word in (((8, 4, 2, 8), b"n_samples < 3"), ((8, 4, 8, 0), b"n_importance < 1"),
                       ((8, 4, 512, 513), b"> 1024"), ((8, 0, 1024, 1), b"> 1024"), ((-1, 4, 64, 128), b"negative"),
                       ((8, 4, 64, 128), b"null"), ((0, 4, 64, 128), b"null")):
        assert call(*args) == -1, word
        assert word in lib.pcnerf_last_error(), (word, lib.pcnerf_last_error())


# ----------------------------------------------------------------------------------------------- public module
def test_localization_refuses_host_scans_unfrozen_modules_and_bad_limits():
    from nof import _ops
    from nof import synthetic as syn
    from nof.networks import NOF_coarse, NOF_fine
    pts = torch.rand(16, 3) + 0.5
    poses = torch.eye(4, dtype=torch.float64)[None]
    fold = RR.analytic_fold()
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.score_poses_fold(fold, fold, pts, poses, RR.PARENT_LO, RR.PARENT_HI)
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.localize_scan_fold(fold, fold, pts, poses, RR.PARENT_LO, RR.PARENT_HI)
    mc = syn.load_into(NOF_coarse(), syn.init_nof_params(1))
    mf = syn.load_into(NOF_fine(), syn.init_nof_params(2))
    before = (_ops.get_eval_math(), _ops.eval_fold_enabled(), _ops.get_train_math())
    for fn in (L.score_poses, L.localize_scan):
        with pytest.raises(NotImplementedError, match="train-mode"):
            fn(mc.train(), mf.eval(), pts, poses, RR.PARENT_LO, RR.PARENT_HI)
        with pytest.raises(NotImplementedError, match="require grad"):
            fn(mc.eval(), mf.eval(), pts, poses, RR.PARENT_LO, RR.PARENT_HI)
    assert (_ops.get_eval_math(), _ops.eval_fold_enabled(), _ops.get_train_math()) == before


def test_default_miss_cost_is_rho_of_the_box_diagonal():
    D = math.sqrt(75.0)
    assert math.isclose(L.default_miss_cost(RR.PARENT_LO, RR.PARENT_HI), 0.5 * D * D, rel_tol=1e-15)
    assert math.isclose(L.default_miss_cost(RR.PARENT_LO, RR.PARENT_HI, 0.05), 0.05 * (D - 0.025), rel_tol=1e-15)
    assert L.rho(0.03, 0.05) == 0.5 * 0.03 * 0.03 and L.rho(-0.2, 0.05) == 0.05 * (0.2 - 0.025)


def test_reduce_scores_applies_the_validity_rule():
    depth = np.array([[1.0, 2.0, np.nan, 1.5, 1.0, 3.0]])
    sumw = np.array([[0.9, 0.4, 0.9, 0.9, 0.9, 0.9]])
    target = np.array([1.2, 2.0, 1.0, np.inf, 0.0, 2.0], np.float32)
    out, mag = LR.reduce_scores(depth, sumw, target, 0.5, 0.5)
    t0 = float(np.float32(1.2))
    # valid: beams 0 (quadratic) and 5 (linear); usable: 0, 1, 2, 5
    assert out[0, 1] == 2 and math.isclose(out[0, 0], 0.5 * (1.0 - t0) ** 2 + 0.5 * (1.0 - 0.25))
    assert math.isclose(out[0, 2], (t0 - 1.0) + 1.0) and math.isclose(out[0, 3], 0.9 + 0.4 + 0.9 + 0.9)
    assert np.array_equal(out, mag)


# ----------------------------------------------------------------------------------------------- the ranking fact
def test_float64_ranking_of_the_grid_puts_the_centre_first():
    """The analytic cavity, 256 directions, targets at T*, the 125 hypotheses around se3_exp((0.07, -0.06, 0.03, 0, 0,
    0)) T*: every ray is valid at every hypothesis, the lowest float64 mean cost is the grid centre (0.00291) and the
    runner-up 0.00422 -- a margin of 45 %, against float32 rendering noise of 1e-6 relative."""
    s = LR.grid_scene()
    assert tuple(s["poses"].shape) == (125, 4, 4) and torch.equal(s["poses"][62], s["center"])
    assert (s["out"][:, 1] == 256).all()
    order = np.argsort(s["scores"], kind="stable")
    print("float64 grid scores:", s["scores"][order[:3]], order[:3])
    assert order[0] == 62
    assert abs(s["scores"][62] - 0.00291) < 5e-6 and abs(s["scores"][order[1]] - 0.00422) < 5e-6
    assert np.array_equal(s["scores"], s["out"][:, 0] / 256)   # nothing missed: the miss cost plays no part
