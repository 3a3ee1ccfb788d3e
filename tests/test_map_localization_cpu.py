"""The numpy restatement of the map / particle-filter layer on its own (tests/map_ref.py), the two-block analytic scene
the GPU end-to-end tests depend on, and the public signatures -- no GPU."""
import inspect
import math

import numpy as np
import pytest
import torch

import localization_ref as LR
import map_ref as MR
import registration_ref as RR


# ----------------------------------------------------------------------------------------------- assign_blocks
def test_assign_blocks_nested_overlapping_face_margin_and_nan():
    boxes = np.array([[-4, -4, -4, 4, 4, 4],          # 0: the outer box
                      [-1, -1, -1, 1, 1, 1],          # 1: nested in 0
                      [0.5, -1, -1, 3, 1, 1],         # 2: overlaps 1
                      [-4, -4, -4, 4, 4, 4]], float)  # 3: a copy of 0 (ties go to the lower index)
    t = np.array([[0, 0, 0],            # clearance 4 in block 0, 1 in block 1 -> 0
                  [3.5, 0, 0],          # only 0 / 3 -> 0
                  [0.9, 0, 0],          # 0: 3.1 -> 0
                  [9, 0, 0],            # outside everything
                  [4, 0, 0],            # on the outer face: contained (clearance 0)
                  [np.nan, 0, 0],
                  [0, np.inf, 0]], float)
    assert MR.assign_blocks(boxes, t).tolist() == [0, 0, 0, -1, 0, -1, -1]
    inner = boxes[1:3]
    assert MR.assign_blocks(inner, t[:3]).tolist() == [0, -1, 1]   # 0.9: clearance 0.1 in block 1, 0.4 in block 2
    assert MR.assign_blocks(inner, np.array([[0.75, 0, 0]])).tolist() == [0]   # equal clearance 0.25: lower index
    # margin: the face point needs margin 0; 3.5 is 0.5 from the face
    assert MR.assign_blocks(boxes[:1], t[[1, 4]], margin=0.5).tolist() == [0, -1]
    assert MR.assign_blocks(boxes[:1], t[[1, 4]], margin=0.5 + 1e-12).tolist() == [-1, -1]
    assert MR.assign_blocks(boxes[:1], t[[4]], margin=0.0).tolist() == [0]
    assert MR.assign_blocks(boxes, t).dtype == np.int32


# ----------------------------------------------------------------------------------------------- mcl_weights
def test_mcl_weights_restatement():
    n = 9
    s4 = np.zeros((n, 4))
    s4[:, 0] = np.linspace(0.0, 800.0, n) * 16     # mean costs 0 .. 800 apart at n_usable = 16, beta = 1
    s4[:, 1] = 16
    blocks = np.zeros(n, np.int32)
    blocks[2] = -1
    s4[5, 0] = np.nan
    r = MR.mcl_weights(np.zeros(n), s4, blocks, 16, 3.0, 1.0)
    assert r["best"] == 0 and r["degenerate"] == 0
    assert np.isneginf(r["logw"][[2, 5]]).all() and np.isfinite(np.delete(r["logw"], [2, 5])).all()
    assert r["w"][2] == 0 and r["w"][5] == 0 and r["w"][-1] == 0      # exp underflows at 800 apart
    assert abs(r["w"].sum() - 1) <= 1e-15 and 1.0 <= r["ess"] <= n
    assert abs(np.exp(r["logw"][0]) - r["w"][0]) <= 1e-15
    # a miss is charged miss_cost: n_valid = 0 -> mean = miss_cost
    s = np.array([[0.0, 0.0, 0, 0], [0.0, 16.0, 0, 0]])
    r = MR.mcl_weights(np.zeros(2), s, np.zeros(2, np.int32), 16, 3.0, 2.0)
    assert math.isclose(r["logw"][0] - r["logw"][1], -6.0, rel_tol=1e-15)
    # the lowest index attaining the maximum
    r = MR.mcl_weights(np.zeros(4), np.tile([[1.0, 16.0, 0, 0]], (4, 1)), np.array([-1, 0, 0, 0], np.int32), 16, 3.0,
                       1.0)
    assert r["best"] == 1 and math.isclose(r["ess"], 3.0, rel_tol=1e-15)
    # no finite logw: uniform
    r = MR.mcl_weights(np.zeros(5), np.zeros((5, 4)), np.full(5, -1, np.int32), 16, 3.0, 1.0)
    assert r["degenerate"] == 1 and r["best"] == 0 and r["ess"] == 5.0
    assert (r["w"] == 0.2).all() and (r["logw"] == 0).all()


# ----------------------------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("n", [1, 3, 64, 65, 1025, 4099])
def test_systematic_resample_restatement_exact_weights(n):
    w = MR.exact_weights(n, n)
    for u0 in (0.0, 0.5, 1.0 - 2.0 ** -20):
        for n_out in sorted({n, 1, 2 * n + 1}):
            anc, resampled = MR.systematic_resample(w, u0, n_out)
            assert resampled and anc.shape == (n_out,) and (np.diff(anc) >= 0).all()
            assert (w[anc] > 0).all() and MR.count_property(anc, w, n_out)
            # every prefix sum is exact, so the kernels' summation order gives the same ancestors
            assert np.array_equal(anc, MR.ancestors_of(MR.hierarchical_prefix(w), w, u0, n_out))


@pytest.mark.parametrize("seed", MR.RESAMPLE_SEEDS)
@pytest.mark.parametrize("n", [1, 3, 64, 65, 1025, 4099])
def test_the_tolerant_seeds_agree_between_summation_orders(n, seed):
    """numpy's sequential cumsum and the hierarchical (kernel-order) prefix give the same ancestors except for draws
    within 1e-12 C of a prefix edge, and those are at most 1 % of the case's draws."""
    w = MR.random_weights(n, seed)
    c_seq, c_h = np.cumsum(w), MR.hierarchical_prefix(w)
    assert np.abs(c_seq - c_h).max() <= (n + 4) * 2.0 ** -53
    for n_out in sorted({n, 2 * n + 1}):
        a_seq, a_h = MR.ancestors_of(c_seq, w, 0.37, n_out), MR.ancestors_of(c_h, w, 0.37, n_out)
        excepted = MR.near_an_edge(c_seq, MR.draws(c_seq[-1], 0.37, n_out))
        assert excepted.sum() <= MR.EDGE_CAP * n_out
        assert np.array_equal(a_seq[~excepted], a_h[~excepted])
        assert (np.diff(a_h) >= 0).all() and MR.count_property(a_h, w, n_out) and MR.count_property(a_seq, w, n_out)


def test_the_hierarchical_prefix_repeats_itself_over_a_zero_weight():
    """What keeps a zero weight from ever being an ancestor: c_i == c_{i-1} exactly, also across run and group
    boundaries, and c never decreases."""
    w = MR.random_weights(2500, 5)
    zeros = [3, 4, 8, 1023, 1024, 1025, 2047, 2048, 2499]
    w[zeros] = 0.0
    c = MR.hierarchical_prefix(w)
    assert all(c[i] == c[i - 1] for i in zeros) and (np.diff(c) >= 0).all()
    anc = MR.ancestors_of(c, w, 0.25, 5001)
    assert (w[anc] > 0).all()


def test_ess_switch_of_the_restatement():
    w = MR.random_weights(65, 3)
    ess = 1.0 / float((w * w).sum())
    anc, resampled = MR.systematic_resample(w, 0.5, 65, ess=ess, ess_threshold=ess)
    assert not resampled and np.array_equal(anc, np.arange(65))
    anc, resampled = MR.systematic_resample(w, 0.5, 65, ess=ess, ess_threshold=ess * (1 + 1e-12))
    assert resampled and not np.array_equal(anc, np.arange(65))


def test_bad_weights_count_as_zero():
    w = np.array([0.25, np.nan, -1.0, 0.5, np.inf, 0.25, 0.0])
    anc, _ = MR.systematic_resample(w, 0.5, 8)
    assert set(anc.tolist()) <= {0, 3, 5} and anc.max() == 5


# ----------------------------------------------------------------------------------------------- the two-block scene
def test_every_beam_of_the_two_block_scene_is_a_hit():
    """BLOCK1_COS_Y = -0.5: from T*_1 every one of the 256 beams ends inside block 1's box with sumw >= 0.5 in float64
    (the GPU end-to-end tests depend on it); block 1 is a different cavity from block 0, not a copy."""
    s = MR.two_block_scene()
    assert MR.BLOCK1_COS_Y == -0.5
    print("two-block scene: sumw min", float(s["sumw"].min()), "ranges", float(s["ranges"].min()),
          float(s["ranges"].max()))
    assert bool((s["sumw"] >= 0.5).all()) and bool(torch.isfinite(s["ranges"]).all())
    assert tuple(s["poses"].shape) == (250, 4, 4)
    # the same beams seen in block 0 from T*_0 have other ranges: the scan tells the blocks apart
    r0, s0 = LR.render_poses(s["folds"][0], s["folds"][0], s["dirs"], [s["T0"]], 64, 128)
    assert bool((s0[0] >= 0.5).all()) and float((r0[0] - s["ranges"]).abs().max()) > 0.1
    # block 1's field is block 0's function of x - 2 pi up to the changed coefficient
    x = torch.tensor([[0.3, -0.4, 0.2]], dtype=torch.float64)
    f0 = RR.fold_logit(s["folds"][0], x)
    f0s = RR.fold_logit(s["folds"][0], x + torch.tensor([[MR.TWO_PI, 0, 0]], dtype=torch.float64))
    assert abs(float(f0 - f0s)) <= 1e-12 * RR.S_FIELD * 6
    # the hypotheses fall into their blocks
    ids = MR.assign_blocks(s["boxes"], s["poses"][:, :3, 3].numpy())
    assert ids[:125].tolist() == [0] * 125 and ids[125:].tolist() == [1] * 125


# ----------------------------------------------------------------------------------------------- signatures
def _kw_defaults(fn, skip=()):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items()
            if p.kind is inspect.Parameter.KEYWORD_ONLY and k not in skip}


def test_signatures_follow_the_single_block_functions():
    from nof import localization as L
    from nof import mcl as M
    from nof import registration as G
    assert _kw_defaults(L.score_poses_map) == _kw_defaults(L.score_poses_fold)
    assert _kw_defaults(G.refine_poses_map) == _kw_defaults(G.refine_poses_fold)
    assert _kw_defaults(L.localize_scan_map, skip=("blocks",)) == _kw_defaults(L.localize_scan_fold, skip=("refine",))
    names = lambda fn: list(inspect.signature(fn).parameters)   # noqa: E731
    assert names(L.assign_blocks) == ["block_map", "poses", "margin"]
    assert inspect.signature(L.assign_blocks).parameters["margin"].default == 0.0
    assert names(L.score_poses_map)[:4] == ["block_map", "points_sensor", "poses", "blocks"]
    assert names(G.refine_poses_map)[:4] == ["block_map", "points_sensor", "poses", "blocks"]
    assert inspect.signature(L.score_poses_map).parameters["blocks"].default is None
    assert inspect.signature(G.refine_poses_map).parameters["blocks"].default is None
    assert names(L.localize_scan_map)[:3] == ["block_map", "points_sensor", "poses"]
    assert L.MapLocalizationResult._fields[:5] == L.LocalizationResult._fields
    assert "block" in L.MapLocalizationResult._fields and "block" not in L.LocalizationResult._fields
    assert inspect.signature(M.ParticleFilter.resample).parameters["ess_frac"].default == 0.5
    assert inspect.signature(M.ParticleFilter.resample).parameters["u0"].default is None
    assert names(M.ParticleFilter.step)[:4] == ["self", "points_sensor", "twist", "sigma"]
    for name in ("predict", "update", "resample", "step", "estimate"):
        assert callable(getattr(M.ParticleFilter, name))


def test_the_operators_are_registered_with_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from nof import _torch_ops as T
    P = torch.ops.pcnerf
    for name in T.map_op_names():
        assert name not in T.op_names()   # (op_names keeps the earlier operators' places; these have their own list)
        assert str(getattr(P, name).default._schema).startswith(f"pcnerf::{name}(")
    with FakeTensorMode():
        f64 = lambda *s: torch.empty(s, dtype=torch.float64)   # noqa: E731
        i32 = lambda *s: torch.empty(s, dtype=torch.int32)     # noqa: E731
        pts = torch.empty((7, 3))
        assert tuple(P.assign_blocks(f64(5, 12), f64(3, 6), 0.0).shape) == (5,)
        s4, d, w = P.score_poses_map(pts, f64(5, 12), i32(5), f64(3, 6), f64(3, 64), f64(3, 64), 0.05, 64, 128, 1e-10,
                                     0.0, 0.5, True)
        assert tuple(s4.shape) == (5, 4) and tuple(d.shape) == tuple(w.shape) == (5, 7)
        n30, d, w, j = P.pose_normal_eq_map(pts, f64(5, 12), None, i32(5), f64(3, 6), f64(3, 64), f64(3, 64), 0.05, 64,
                                            128, 1e-10, 0.0, 0.5, True)
        assert tuple(n30.shape) == (5, 30) and tuple(j.shape) == (5, 7, 6)
        out, st, c, a = P.refine_poses_map(pts, f64(5, 12), i32(5), f64(3, 6), f64(3, 64), f64(3, 64), 0.05, 64, 128,
                                           1e-10, 0.0, 0.5, 1e-6, 1e-9, 4)
        assert tuple(out.shape) == (5, 12) and tuple(st.shape) == (5, 64) and tuple(c.shape) == (5, 4)
        w, lw, ess, best, deg = P.mcl_weights(f64(5), f64(5, 4), i32(5), f64(1), 3.0, 1.0)
        assert tuple(w.shape) == tuple(lw.shape) == (5,) and best.dtype == torch.int32 and tuple(ess.shape) == (1,)
        anc, po, bo, lo = P.systematic_resample(f64(5), f64(1), 11, None, 0.0, f64(5, 12), i32(5), f64(5))
        assert tuple(anc.shape) == (11,) and tuple(po.shape) == (11, 12) and tuple(bo.shape) == tuple(lo.shape) == (11,)
        assert anc.dtype == bo.dtype == torch.int32


def test_twist_and_sigma_forms():
    """A twist has six components; only sigma may be one number for all six."""
    from nof import mcl as M
    assert M._six(0.5, "sigma", scalar_ok=True) == [0.5] * 6
    assert M._six((1, 2, 3, 4, 5, 6), "twist") == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert M._six(torch.arange(6.0), "twist") == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    with pytest.raises(RuntimeError, match="six components"):
        M._six(0.5, "twist")
    with pytest.raises(RuntimeError, match="six components"):
        M._six((1, 2, 3), "sigma", scalar_ok=True)
