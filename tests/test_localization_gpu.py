"""pcnerf::score_poses_fold and nof.localization on the MI355X against the float64 restatement of
tests/localization_ref.py.

Per-beam tolerance (the per-kernel tests' rule, parity_helpers.Tally): e(x) = max |x - q64| / |q64| over the usable
beams, e32 the same restatement run on rays.float() on the CPU, e_hip <= max(4 e32, 2.4e-7); depth and sumw of the
fine pass, no case left out.  The four scores are float64 sums of float64 terms of the kernel's own float32 depth and
sumw: 1e-12 of the sum of the terms' absolute values, n_valid exact."""
import functools

import numpy as np
import pytest
import torch

import localization_ref as LR
import registration_ref as RR
from gradcheck import _report
from parity_helpers import FLOOR, Tally
from sampling_f64 import same_bits
from nof import _ops
from nof import _torch_ops as T
from nof import localization as L
from nof import registration as G
from nof import synthetic as syn

pytestmark = pytest.mark.gpu
P = torch.ops.pcnerf
NOCAP = float("inf")
SAMPLES = ((3, 1), (4, 7), (63, 65), (64, 128), (65, 64), (128, 256), (129, 895), (512, 512))
BEAMS = (1, 5, 67, 259)
# three poses within 0.4 m / 10 degrees of T* (the first is T* itself)
NEAR_TWISTS = ((0.0,) * 6, (0.2, -0.15, 0.1, 0.05, -0.03, 0.08), (-0.25, 0.2, -0.1, -0.06, 0.04, -0.12))
BOX = (RR.PARENT_LO, RR.PARENT_HI)
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


def _fold(field):
    return RR.analytic_fold() if field == "analytic" else _random_fold()


def _near_poses():
    T_star = G.se3_exp(RR.XI_STAR)
    return torch.stack([G.se3_exp(x) @ T_star for x in NEAR_TWISTS])


def _points(R, seed):
    """R float32 sensor-frame points: unit directions (seeded) at ranges 0.7 .. 2.0 m."""
    g = torch.Generator().manual_seed(7000 + seed)
    return (RR.unit_directions(R, seed) * (0.7 + 1.3 * torch.rand(R, 1, generator=g, dtype=torch.float64))).float()


@functools.lru_cache(maxsize=None)
def _reference(field, S, I, R):
    """The case's float64 and float32 restatements for the three poses, computed once: (points, d64, s64, d32, s32)."""
    fold = _fold(field)
    pts = _points(R, S)
    dirs = LR.dirs_of(pts)[0]
    d64, s64 = LR.render_poses(fold, fold, dirs, _near_poses(), S, I)
    d32, s32 = LR.render_poses(fold, fold, dirs, _near_poses(), S, I, dtype=torch.float32)
    return pts, d64, s64, d32, s32


def _err(x, q64):
    """max |x - q64| / |q64|; where q64 is 0 the value must be exactly 0."""
    d, scale = (x.double() - q64).abs(), q64.abs()
    ok = scale > 0
    e = float((d[ok] / scale[ok]).max()) if bool(ok.any()) else 0.0
    return e if float(d[~ok].max() if bool((~ok).any()) else 0.0) == 0.0 else float("inf")


def _score(fold, pts, poses, S, I, **kw):
    f = _dev(fold)
    return L.score_poses_fold(f, f, _dev(pts), poses, *BOX, N_samples=S, N_importance=I, near=RR.NEAR, **kw)


# ----------------------------------------------------------------------------------------------- 1. per-beam accuracy
@pytest.mark.parametrize("field", ["analytic", "random"])
@pytest.mark.parametrize("S,I", SAMPLES)
def test_depth_and_sumw_against_float64(S, I, field):
    """Measured on the MI355X: see DESIGN.md (localisation) for the worst e_hip / max(4 e32, 2.4e-7)."""
    t = Tally("score_poses_fold")
    fold, poses = _fold(field), _near_poses()
    for R in BEAMS:
        pts, d64, s64, d32, s32 = _reference(field, S, I, R)
        for Pn in (1, 3):
            s = _score(fold, pts, poses[:Pn], S, I, want_depth=True)
            assert tuple(s.depth.shape) == tuple(s.sumw.shape) == (Pn, R) and s.depth.dtype == torch.float32
            depth, sumw = s.depth.cpu(), s.sumw.cpu()
            assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(sumw).all())
            case = f"{field} P{Pn} R{R} S{S} I{I}"
            t.check_err(case, "depth", _err(depth, d64[:Pn]), _err(d32[:Pn], d64[:Pn]), NOCAP)
            t.check_err(case, "sumw", _err(sumw, s64[:Pn]), _err(s32[:Pn], s64[:Pn]), NOCAP)
    t.done()


# ----------------------------------------------------------------------------------------------- 2. misses, bad beams
def test_misses_and_bad_beams_are_not_counted():
    """The open plane field logit = 40 (x - 1), 259 directions (seed 0), five poses, box [-2.5, 2.5]^3, 64 + 128
    samples.  In float64 442 of the 1,295 rays hit (sumw >= 0.5) and the closest sumw lies 0.030 from the threshold, so
    n_valid must be exact.  Then beams with a range of 0 (an all-zero point), inf and NaN are planted through the
    scan: not counted, every score finite.  (A range is a norm: a negative target cannot be expressed through
    points_sensor; the kernel's ``target > 0`` test covers it all the same.)"""
    fold = LR.plane_fold()
    poses = torch.stack([G.se3_exp(x) for x in LR.PLANE_POSES])
    pts = _points(259, 0)
    dirs, rng = LR.dirs_of(pts)
    d64, s64 = LR.render_poses(fold, fold, dirs, poses, 64, 128)
    gap = float((s64 - 0.5).abs().min())
    want, _ = LR.reduce_scores(d64.numpy(), s64.numpy(), rng.numpy(), 0.0, 0.5)
    _report({"test": "score_poses_fold_misses", "hits": int(want[:, 1].sum()), "gap": gap})
    assert gap >= 1e-3 and int(want[:, 1].sum()) == 442
    s = _score(fold, pts, poses, 64, 128, want_depth=True)
    assert s.n_valid.dtype == torch.int64 and s.n_valid.cpu().tolist() == [int(v) for v in want[:, 1]]
    assert ((s.sumw.cpu() >= 0.5) == (s64 >= 0.5)).all()
    # bad beams, spread through the scan
    bad = pts.clone()
    bad[3] = 0.0
    bad[64, 1] = float("inf")
    bad[130, 2] = float("nan")
    bad[131] = torch.tensor([float("-inf"), 0.0, 1.0])
    bad[258] = 0.0
    idx = [3, 64, 130, 131, 258]
    keep = np.ones(259, bool)
    keep[idx] = False
    sb = _score(fold, bad, poses, 64, 128, want_depth=True)
    for v in (sb.cost, sb.abs_residual, sb.hit):
        assert bool(torch.isfinite(v).all())
    assert sb.n_valid.cpu().tolist() == [int((s64[p].numpy() >= 0.5)[keep].sum()) for p in range(5)]
    # the good beams keep their bits; the scores are those of the good beams alone
    assert same_bits(sb.depth[:, torch.from_numpy(keep)], s.depth[:, torch.from_numpy(keep)])
    tgt = rng.numpy().copy()
    tgt[idx] = np.nan
    ref, mag = LR.reduce_scores(s.depth.cpu().numpy(), s.sumw.cpu().numpy(), tgt, 0.0, 0.5)
    got = np.stack([v.cpu().double().numpy() for v in (sb.cost, sb.n_valid, sb.abs_residual, sb.hit)], 1)
    assert (np.abs(got - ref) <= 1e-12 * mag).all()


# ----------------------------------------------------------------------------------------------- 3. the reduction
def _noisy_scan(R):
    """R points in the analytic cavity whose ranges are the kernel's own depths at T* plus 0.05 N(0, 1) of noise:
    residuals on both sides of huber_delta = 0.05 at T*, larger ones at the second pose."""
    if ("scan", R) not in _CACHE:
        dirs = RR.unit_directions(R, 11).float()
        d0 = _score(RR.analytic_fold(), dirs, _near_poses()[:1], 64, 128, want_depth=True).depth[0].cpu()
        g = torch.Generator().manual_seed(R)
        _CACHE["scan", R] = (dirs * (d0 + 0.05 * torch.randn(R, generator=g))[:, None]).contiguous()
    return _CACHE["scan", R]


@pytest.mark.parametrize("delta", [0.0, 0.05, 10.0])
@pytest.mark.parametrize("R", [1, 63, 64, 257, 4099])
def test_scores_are_the_float64_sums_of_the_per_beam_outputs(R, delta):
    pts = _noisy_scan(R)
    s = _score(RR.analytic_fold(), pts, _near_poses()[:2], 64, 128, huber_delta=delta, want_depth=True)
    tgt = LR.dirs_of(pts)[1].numpy()
    want, mag = LR.reduce_scores(s.depth.cpu().numpy(), s.sumw.cpu().numpy(), tgt, delta, 0.5)
    got = np.stack([v.cpu().double().numpy() for v in (s.cost, s.n_valid, s.abs_residual, s.hit)], 1)
    assert (got[:, 1] == want[:, 1]).all() and (want[:, 1] > 0).all()
    err = np.abs(got - want)
    _report({"test": "score_poses_fold_sums", "case": f"R{R} d{delta}",
             "worst": float((err / np.maximum(mag, 1e-300)).max())})
    assert (err <= 1e-12 * mag).all(), (err / np.maximum(mag, 1e-300)).max()
    if delta == 0.05 and R >= 63:
        r = np.abs(s.depth[0].cpu().double().numpy() - tgt)
        assert (r > delta).any() and (r <= delta).any()


# ----------------------------------------------------------------------------------------------- 4. bits
def test_bits_do_not_depend_on_the_batch_the_outputs_or_where_the_poses_live():
    fold, pts = RR.analytic_fold(), _points(67, 4)
    poses = L.pose_grid(G.se3_exp(RR.XI_STAR), 0.2, 0.2, 0.1, 0.1)[::6]   # 5 of 27
    assert poses.shape[0] == 5
    full = _score(fold, pts, poses, 64, 128, huber_delta=0.05, want_depth=True)
    again = _score(fold, pts, poses, 64, 128, huber_delta=0.05, want_depth=True)
    bare = _score(fold, pts, poses, 64, 128, huber_delta=0.05)
    on_dev = _score(fold, pts, poses.cuda(), 64, 128, huber_delta=0.05)
    assert bare.depth is None and bare.sumw is None

    def bits(s):
        return torch.stack([s.cost, s.n_valid.double(), s.abs_residual, s.hit], 1).view(torch.int32)

    assert same_bits(bits(full), bits(again)) and same_bits(full.depth, again.depth)
    assert same_bits(full.sumw, again.sumw)
    assert same_bits(bits(full), bits(bare)) and same_bits(bits(full), bits(on_dev))
    for p in (0, 2, 4):
        one = _score(fold, pts, poses[p:p + 1], 64, 128, huber_delta=0.05, want_depth=True)
        assert same_bits(bits(one)[0], bits(full)[p]) and same_bits(one.depth[0], full.depth[p])


# ----------------------------------------------------------------------------------------------- 5. the composed route
@pytest.mark.parametrize("S,I", [(4, 7), (64, 128), (129, 895)])
def test_against_the_composed_route(S, I):
    """scan_rays + render_scan + gn_normal_eq per pose.  Both routes meet the float64 rule with the case's tolerance
    tol = max(4 e32, 2.4e-7), so their depths differ by at most 2 tol |depth64| (the triangle inequality), and with
    e = 2 tol max |depth64| the costs by at most sum (|r| e + e^2 / 2) = e sum |r| + n e^2 / 2."""
    R = 67
    pts, d64, s64, d32, s32 = _reference("analytic", S, I, R)
    tol = max(4 * _err(d32, d64), FLOOR)
    fold, poses = _dev(RR.analytic_fold()), _near_poses()
    s = _score(RR.analytic_fold(), pts, poses, S, I, want_depth=True)
    pd = _dev(pts)
    shared = []
    for p in range(3):
        rays, rng = G.scan_rays(pd, poses[p], *BOX, RR.NEAR)
        depth, sumw, jac = G.render_scan(fold, fold, rays, S, I, True)
        out = P.gn_normal_eq(rays, jac, depth, sumw, rng, 0.0, 0.5).cpu().numpy()
        dist = (s.depth[p].cpu().double() - depth.cpu().double()).abs()
        assert bool((dist <= 2 * tol * d64[p].abs()).all()), float((dist / d64[p].abs()).max())
        assert int(s.n_valid[p]) == int(out[28]) == R
        e = 2 * tol * float(d64[p].abs().max())
        assert abs(float(s.cost[p]) - out[27]) <= e * float(s.abs_residual[p]) + 0.5 * R * e * e
        shared.append(same_bits(s.depth[p], depth) and same_bits(s.sumw[p], sumw))
    _report({"test": "score_poses_fold_vs_composed", "case": f"S{S} I{I}", "tol": tol, "depth_bits_equal": shared})
    print("depths share bits with the composed route:", shared)


# ----------------------------------------------------------------------------------------------- 6. end to end
def test_localize_scan_fold_end_to_end():
    """The CPU test's scene and grid: the winner must be the grid centre, and its refined pose must lie within
    2 (the float64 loop's final error from the same start on these 256 directions) + 10 delta of T*, delta =
    max |depth_hip - depth_f64| at T* (rotation: delta over the mean range), as test_register_scan_fold_end_to_end.
    Measured on the MI355X: see DESIGN.md (localisation)."""
    s = LR.grid_scene()
    fold, pts = _dev(s["fold"]), _dev(s["points"])
    dirs, rng = LR.dirs_of(s["points"])
    d64, _ = LR.render_poses(s["fold"], s["fold"], dirs, [s["T_star"]], 64, 128)
    at_star = L.score_poses_fold(fold, fold, pts, s["T_star"][None], *BOX, near=RR.NEAR, want_depth=True)
    delta = float((at_star.depth[0].cpu().double() - d64[0]).abs().max())
    run = RR.register_f64(s["fold"], s["fold"], dirs, rng.double().numpy(), s["center"], G.se3_exp,
                          T_ref=s["T_star"])
    ht, hr = RR.pose_error(run["pose"], s["T_star"])
    res = L.localize_scan_fold(fold, fold, pts, s["poses"], *BOX, top_k=4, refine_iters=20, near=RR.NEAR)
    et, er = RR.pose_error(res.pose, s["T_star"])
    bt, br = 2 * ht + 10 * delta, 2 * hr + 10 * delta / float(rng.mean())
    got = res.scores.cpu().numpy()
    line = {"test": "localize_scan_fold", "index": res.index, "score": res.score, "delta": delta, "err_t": et,
            "err_r": er, "f64_err_t": ht, "f64_err_r": hr, "bound_t": bt, "bound_r": br,
            "grid_best": float(got.min()), "grid_runner_up": float(np.sort(got)[1]),
            "scores_vs_f64": float(np.abs(got - s["scores"]).max())}
    _report(line)
    print(line)
    assert res.index == 62 and int(np.argmin(got)) == 62
    assert et <= bt and er <= br, line
    assert tuple(res.scores.shape) == (125,) and res.scores.dtype == torch.float64 and res.scores.is_cuda
    assert len(res.refined) == 4 and all(isinstance(r, G.RegistrationResult) for r in res.refined)
    assert res.pose.dtype == torch.float64 and tuple(res.pose.shape) == (4, 4)
    # the four best hypotheses are neighbours of one basin: the later ones find the centre's pose again (within the
    # default 1 mm / 1 mrad) and do not compete, whatever the last digits of their final costs
    first = res.refined[0]
    assert torch.equal(res.pose, first.pose) and res.score == (first.costs[-1] + s["miss_cost"] * (256 - first.n_valid)) / 256
    assert all(max(L.pose_distance(r.pose, first.pose)) <= 1e-3 for r in res.refined)


def test_localize_scan_on_frozen_modules_equals_the_fold_form():
    """Bit for bit, and no process-wide selector moves."""
    from nof.networks import NOF_coarse, NOF_fine
    mc = syn.load_into(NOF_coarse(), syn.init_nof_params(1)).cuda().eval().requires_grad_(False)
    mf = syn.load_into(NOF_fine(), syn.init_nof_params(2)).cuda().eval().requires_grad_(False)
    rows = torch.from_numpy(syn.make_rays(512, seed=4))
    pts = _dev(rows[:, 3:6] * rows[:, 14:15])
    poses = L.pose_grid(G.se3_exp([0.05, -0.02, 0.01, 0.0, 0.0, 0.01]), 0.1, 0.1, 0.0, 1.0)
    kw = dict(top_k=2, refine_iters=1, N_samples=64, N_importance=128, min_sumw=0.0)
    before = (_ops.get_eval_math(), _ops.eval_fold_enabled(), _ops.get_train_math())
    a = L.localize_scan(mc, mf, pts, poses, syn.PARENT_LO, syn.PARENT_HI, **kw)
    with torch.no_grad():
        fc, ff = P.fold_eval(T.eval_params(mc)), P.fold_eval(T.eval_params(mf))
    b = L.localize_scan_fold(fc, ff, pts, poses, syn.PARENT_LO, syn.PARENT_HI, **kw)
    assert torch.equal(a.pose, b.pose) and a.index == b.index and a.score == b.score
    assert same_bits(a.scores.view(torch.int32), b.scores.view(torch.int32)) and tuple(a.scores.shape) == (9,)
    assert [r.costs for r in a.refined] == [r.costs for r in b.refined] and len(a.refined) == 2
    sa = L.score_poses(mc, mf, pts, poses, syn.PARENT_LO, syn.PARENT_HI, min_sumw=0.0)
    sb = L.score_poses_fold(fc, ff, pts, poses, syn.PARENT_LO, syn.PARENT_HI, min_sumw=0.0)
    assert same_bits(sa.cost.view(torch.int32), sb.cost.view(torch.int32)) and torch.equal(sa.n_valid, sb.n_valid)
    assert int(sa.n_valid.min()) == 512 and bool(torch.isfinite(sa.cost).all())
    assert (_ops.get_eval_math(), _ops.eval_fold_enabled(), _ops.get_train_math()) == before


# ----------------------------------------------------------------------------------------------- 7. errors, empties
def test_sample_limits_raise_and_empty_inputs_give_zeros():
    fold, pts, poses = RR.analytic_fold(), _points(5, 1), _near_poses()
    for S, I in ((512, 513), (2, 8), (8, 0)):
        with pytest.raises(RuntimeError, match="at most 1024|at least"):
            _score(fold, pts, poses, S, I)
    s = _score(fold, pts, torch.empty(0, 4, 4, dtype=torch.float64), 64, 128, want_depth=True)
    assert tuple(s.cost.shape) == tuple(s.n_valid.shape) == (0,) and tuple(s.depth.shape) == (0, 5)
    s = _score(fold, torch.empty(0, 3), poses, 64, 128, want_depth=True)
    assert tuple(s.depth.shape) == tuple(s.sumw.shape) == (3, 0) and s.n_valid.dtype == torch.int64
    for v in (s.cost, s.n_valid, s.abs_residual, s.hit):
        assert tuple(v.shape) == (3,) and float(v.double().abs().max()) == 0.0
