"""pcnerf::pose_normal_eq_fold, lm_init, lm_update, refine_poses_fold, se3_apply and nof.registration.refine_poses_fold
on the MI355X, against the composed route of the earlier operators (scan_rays -> render_scan -> gn_normal_eq, bit for
bit per beam), the float64 restatement of tests/registration_ref.py / localization_ref.py and the restatement of the
state machine in tests/refine_ref.py.

Per-beam tolerance (parity_helpers.Tally): e(x) = max |x - q64| / scale, e32 the same restatement run on rays.float()
on the CPU, e_hip <= max(4 e32, 2.4e-7), no case left out; depth and sumw against their own float64 value, jac6 against
test_registration_gpu._jac_scale.  Sums: 1e-12 of the sum of the terms' absolute values, n_valid exact.  The solve:
|xi_dev - xi_np| <= 64 cond_2(A) 2^-53 |xi_np| (the backward-error scale of a 6 x 6 LU), pose entries that plus
64 2^-53 max(1, max |T|) (a sin / cos pair and some twenty rounded float64 operations behind an entry)."""
import functools
import math

import numpy as np
import pytest
import torch

import localization_ref as LR
import refine_ref as FR
import registration_ref as RR
from gradcheck import _report
from parity_helpers import Tally
from sampling_f64 import same_bits
from test_localization_gpu import BEAMS, NEAR_TWISTS, SAMPLES, _fold, _points
from test_registration_cpu import TWISTS
from test_registration_gpu import _jac_scale
from nof import localization as L
from nof import registration as G

pytestmark = pytest.mark.gpu
P = torch.ops.pcnerf
NOCAP = float("inf")
BOX = (RR.PARENT_LO, RR.PARENT_HI)
EPS = G.EPSILON
U = 2.0 ** -53
_CACHE = {}


def _dev(t):
    return t.cuda().contiguous()


def _same(a, b):
    """Bit for bit (a NaN equal to any NaN); integer and bool tensors by value."""
    if a.is_floating_point():
        return same_bits(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))


def _box():
    if "box" not in _CACHE:
        _CACHE["box"] = _dev(torch.tensor(list(RR.PARENT_LO) + list(RR.PARENT_HI), dtype=torch.float64))
    return _CACHE["box"]


def _near_poses():
    T_star = G.se3_exp(RR.XI_STAR)
    return torch.stack([G.se3_exp(x) @ T_star for x in NEAR_TWISTS])


def _evaluate(fold, pts, poses, S, I, delta=0.0, min_sumw=0.5, want_beams=True, state=None):
    """One evaluation through the operator -> (normal30, depth, sumw, jac6) on the device."""
    f = _dev(fold)
    rows = None if state is not None else G._pose_rows(poses, "cuda")
    return P.pose_normal_eq_fold(_dev(pts), rows, state, _box(), f, f, RR.NEAR, S, I, EPS, delta, min_sumw,
                                 want_beams)


def _composed(fold, pts, pose, S, I):
    """The parent route of one pose: scan_rays -> sample_coarse / render_jac_fold / resample / render_jac_fold ->
    (rays, ranges, depth, sumw, jac6, zf) on the device."""
    f = _dev(fold)
    rays, rng = G.scan_rays(_dev(pts), pose, *BOX, RR.NEAR)
    z = P.sample_coarse(rays, S, S, 6, 7, 0, 0, False)
    _, _, w, _ = P.render_jac_fold(rays, z, f, EPS, True, False)
    zf = P.resample(z, w, I, None)
    depth, sumw, _, jac = P.render_jac_fold(rays, zf, f, EPS, False, True)
    return rays, rng, depth, sumw, jac, zf


@functools.lru_cache(maxsize=None)
def _reference(field, S, I, R):
    """The case's float64 and float32 restatements with the Jacobian for the three near poses, computed once:
    (points, (d64, s64, j64), (d32, s32, j32))."""
    fold = _fold(field)
    pts = _points(R, S)
    dirs = LR.dirs_of(pts)[0]
    out = []
    for dt in (torch.float64, torch.float32):
        rows = [RR.render_two_pass(fold, fold, LR.rays_f64(dirs, T).to(dt), S, I, want_jac=True)
                for T in _near_poses()]
        out.append(tuple(torch.stack([r[k] for r in rows]) for k in range(3)))
    return pts, out[0], out[1]


def _err(x, q64, scale):
    """max |x - q64| / scale; where the scale is 0 the value must be exactly q64."""
    d = (x.double() - q64).abs()
    ok = scale > 0
    e = float((d[ok] / scale[ok]).max()) if bool(ok.any()) else 0.0
    return e if float(d[~ok].max() if bool((~ok).any()) else 0.0) == 0.0 else float("inf")


# ----------------------------------------------------------------------------------------------- 1. per-beam outputs
@pytest.mark.parametrize("field", ["analytic", "random"])
@pytest.mark.parametrize("S,I", SAMPLES)
def test_per_beam_outputs_against_the_composed_route_and_float64(S, I, field):
    """depth, sumw and jac6 of one evaluation equal the composed route's bits; against float64 the project's rule.
    Measured on the MI355X: see DESIGN.md (batched refinement) for the worst e_hip / max(4 e32, 2.4e-7)."""
    t = Tally("pose_normal_eq_fold")
    fold, poses = _fold(field), _near_poses()
    for R in BEAMS:
        pts, (d64, s64, j64), (d32, s32, j32) = _reference(field, S, I, R)
        comp = [_composed(fold, pts, poses[p], S, I) for p in range(3)]
        scale = torch.stack([_jac_scale(fold, c[0].cpu(), c[5].cpu()) for c in comp])
        for Pn in (1, 3):
            n30, depth, sumw, jac = _evaluate(fold, pts, poses[:Pn], S, I)
            assert tuple(depth.shape) == tuple(sumw.shape) == (Pn, R) and tuple(jac.shape) == (Pn, R, 6)
            assert depth.dtype == sumw.dtype == jac.dtype == torch.float32 and tuple(n30.shape) == (Pn, 30)
            case = f"{field} P{Pn} R{R} S{S} I{I}"
            for p in range(Pn):
                assert _same(depth[p], comp[p][2]), (case, p, "depth")
                assert _same(sumw[p], comp[p][3]), (case, p, "sumw")
                assert _same(jac[p], comp[p][4]), (case, p, "jac6")
            depth, sumw, jac = depth.cpu(), sumw.cpu(), jac.cpu()
            for v in (depth, sumw, jac):
                assert bool(torch.isfinite(v).all()), case
            t.check_err(case, "depth", _err(depth, d64[:Pn], d64[:Pn].abs()),
                        _err(d32[:Pn], d64[:Pn], d64[:Pn].abs()), NOCAP)
            t.check_err(case, "sumw", _err(sumw, s64[:Pn], s64[:Pn].abs()),
                        _err(s32[:Pn], s64[:Pn], s64[:Pn].abs()), NOCAP)
            t.check_err(case, "jac6", _err(jac, j64[:Pn], scale[:Pn]), _err(j32[:Pn], j64[:Pn], scale[:Pn]), NOCAP)
    t.done()


# ----------------------------------------------------------------------------------------------- 2. the sums
def _noisy_scan(R):
    """R points in the analytic cavity whose ranges are the kernel's own depths at T* plus 0.05 N(0, 1) of noise:
    residuals on both sides of huber_delta = 0.05 at T*, larger ones at the second pose."""
    if ("scan", R) not in _CACHE:
        dirs = RR.unit_directions(R, 11).float()
        d0 = _evaluate(RR.analytic_fold(), dirs, _near_poses()[:1], 64, 128)[1][0].cpu()
        g = torch.Generator().manual_seed(R)
        _CACHE["scan", R] = (dirs * (d0 + 0.05 * torch.randn(R, generator=g))[:, None]).contiguous()
    return _CACHE["scan", R]


def _sums_of_the_beams(rays, jac, depth, sumw, target, delta, min_sumw=0.5):
    return RR.normal_eq(rays.cpu().numpy()[:, :6], jac.cpu().numpy(), depth.cpu().numpy(), sumw.cpu().numpy(),
                        target.cpu().numpy(), delta, min_sumw)


@pytest.mark.parametrize("delta", [0.0, 0.05])
@pytest.mark.parametrize("R", [1, 3, 4, 5, 63, 64, 257])
def test_normal30_is_the_float64_sum_of_the_per_beam_terms(R, delta):
    """normal30 against numpy float64 sums of the 29 terms formed from the kernel's own float32 outputs (and the
    float32 ray rows of scan_rays), and against pcnerf::gn_normal_eq on the composed route's arrays."""
    fold, pts, poses = RR.analytic_fold(), _noisy_scan(R), _near_poses()[:2]
    n30, depth, sumw, jac = _evaluate(fold, pts, poses, 64, 128, delta=delta)
    got = n30.cpu().numpy()
    worst = 0.0
    for p in range(2):
        rays, rng, cd, cs, cj, _ = _composed(fold, pts, poses[p], 64, 128)
        want, mag = _sums_of_the_beams(rays, jac[p], depth[p], sumw[p], rng, delta)
        assert got[p, 28] == want[28] and 0 < want[28] <= R and got[p, 29] == 0.0
        err = np.abs(got[p, :28] - want[:28])
        worst = max(worst, float((err / np.maximum(mag[:28], 1e-300)).max()))
        assert (err <= 1e-12 * mag[:28]).all(), (p, (err / np.maximum(mag[:28], 1e-300)).max())
        ref = P.gn_normal_eq(rays, cj, cd, cs, rng, delta, 0.5).cpu().numpy()
        err = np.abs(got[p, :28] - ref[:28])
        assert ref[28] == got[p, 28] and (err <= 1e-12 * mag[:28]).all(), (p, "gn_normal_eq")
        if delta == 0.05 and R >= 63:
            r = np.abs(depth[p].cpu().double().numpy() - rng.cpu().double().numpy())
            assert (r > delta).any() and (r <= delta).any()
    _report({"test": "pose_normal_eq_fold_sums", "case": f"R{R} d{delta}", "worst": worst})


# ----------------------------------------------------------------------------------------------- 3. misses, bad beams
def test_misses_and_bad_beams_are_not_counted():
    """test_localization_gpu's plane scene: in float64 442 of the 1,295 rays hit, the closest sumw 0.030 from the
    threshold, so n_valid must be exact.  Then beams with a range of 0, inf and NaN are planted through the scan: not
    counted, every sum finite, and the other beams keep their bits."""
    fold = LR.plane_fold()
    poses = torch.stack([G.se3_exp(x) for x in LR.PLANE_POSES])
    pts = _points(259, 0)
    dirs, rng = LR.dirs_of(pts)
    d64, s64 = LR.render_poses(fold, fold, dirs, poses, 64, 128)
    want, _ = LR.reduce_scores(d64.numpy(), s64.numpy(), rng.numpy(), 0.0, 0.5)
    assert int(want[:, 1].sum()) == 442
    n30, depth, sumw, jac = _evaluate(fold, pts, poses, 64, 128)
    assert n30[:, 28].cpu().tolist() == [float(v) for v in want[:, 1]]
    assert ((sumw.cpu() >= 0.5) == (s64 >= 0.5)).all()
    bad = pts.clone()
    bad[3] = 0.0
    bad[64, 1] = float("inf")
    bad[130, 2] = float("nan")
    bad[131] = torch.tensor([float("-inf"), 0.0, 1.0])
    bad[258] = 0.0
    idx = [3, 64, 130, 131, 258]
    keep = np.ones(259, bool)
    keep[idx] = False
    kt = torch.from_numpy(keep)
    b30, bdepth, bsumw, bjac = _evaluate(fold, bad, poses, 64, 128)
    assert bool(torch.isfinite(b30).all())
    assert b30[:, 28].cpu().tolist() == [float((s64[p].numpy() >= 0.5)[keep].sum()) for p in range(5)]
    assert _same(bdepth[:, kt], depth[:, kt]) and _same(bsumw[:, kt], sumw[:, kt])
    assert _same(bjac[:, kt], jac[:, kt])
    # the sums are those of the good beams alone
    got = b30.cpu().numpy()
    for p in range(5):
        rays, _ = G.scan_rays(_dev(pts), poses[p], *BOX, RR.NEAR)
        tgt = rng.clone()
        tgt[idx] = float("nan")
        ref, mag = _sums_of_the_beams(rays, jac[p], depth[p], sumw[p], tgt, 0.0)
        assert (np.abs(got[p, :29] - ref[:29]) <= 1e-12 * mag[:29]).all(), p


# ----------------------------------------------------------------------------------------------- 4. batch independence
def _refine(fold, pts, poses, **kw):
    f = _dev(fold)
    kw.setdefault("near", RR.NEAR)
    return G.refine_poses_fold(f, f, _dev(pts), poses, *BOX, **kw)


def _result_bits(r, p):
    return [r.poses[p], r.state[p], r.eval_costs[p],
            r.accepted_mask[p], r.cost[p:p + 1], r.n_valid[p:p + 1], r.status[p:p + 1]]


def test_bits_do_not_depend_on_the_batch_the_outputs_or_where_the_poses_live():
    fold, pts, poses = RR.analytic_fold(), _noisy_scan(67), _near_poses()
    full = _evaluate(fold, pts, poses, 64, 128, delta=0.05)
    again = _evaluate(fold, pts, poses, 64, 128, delta=0.05)
    bare = _evaluate(fold, pts, poses, 64, 128, delta=0.05, want_beams=False)
    assert all(_same(a, b) for a, b in zip(full, again))
    assert _same(full[0], bare[0])
    assert bare[1].numel() == bare[2].numel() == bare[3].numel() == 0
    state = P.lm_init(G._pose_rows(poses, "cuda"), 1e-6)
    via_state = _evaluate(fold, pts, None, 64, 128, delta=0.05, state=state)
    assert all(_same(a, b) for a, b in zip(full, via_state))
    for p in range(3):
        one = _evaluate(fold, pts, poses[p:p + 1], 64, 128, delta=0.05)
        assert all(_same(a[0], b[p]) for a, b in zip(one, full)), p
    kw = dict(iters=4, huber_delta=0.05)
    r = _refine(fold, pts, poses, **kw)
    r2 = _refine(fold, pts, poses, **kw)
    on_dev = _refine(fold, pts, poses.cuda(), **kw)
    assert r.poses.is_cuda and tuple(r.poses.shape) == (3, 4, 4) and r.poses.dtype == torch.float64
    assert tuple(r.eval_costs.shape) == tuple(r.accepted_mask.shape) == (3, 4)
    assert r.iterations.tolist() == [4, 4, 4]
    for p in range(3):
        one = _refine(fold, pts, poses[p:p + 1], **kw)
        for a, b, c, d in zip(_result_bits(r, p), _result_bits(r2, p), _result_bits(on_dev, p), _result_bits(one, 0)):
            assert _same(a, b) and _same(a, c) and _same(a, d), p


@pytest.mark.parametrize("status", [1, 2, 3])
def test_a_stopped_pose_keeps_every_word_and_its_neighbours_theirs(status):
    fold, pts, poses = RR.analytic_fold(), _noisy_scan(67), _near_poses()
    state = P.lm_init(G._pose_rows(poses, "cuda"), 1e-6)
    planted = state.clone()
    planted[1, FR.STATUS] = float(status)
    planted[1, FR.XI:FR.XI + 6] = 0.25   # any words: they must survive
    a, b = state, planted
    for _ in range(2):
        na = _evaluate(fold, pts, None, 64, 128, state=a, want_beams=False)[0]
        nb, depth, _, _ = _evaluate(fold, pts, None, 64, 128, state=b)
        assert float(nb[1].abs().max()) == 0.0 and float(depth[1].abs().max()) == 0.0
        assert _same(na[::2], nb[::2])
        a, ca, _ = P.lm_update(na, a, 1e-9)
        b, cb, acc = P.lm_update(nb, b, 1e-9)
        assert _same(b[1], planted[1])
        assert _same(a[::2], b[::2])
        assert math.isnan(float(cb[1])) and int(acc[1]) == 0 and _same(ca[::2],
                                                                           cb[::2])
    assert b[:, FR.EVALS].tolist() == [2.0, 0.0, 2.0]


# ----------------------------------------------------------------------------------------------- 5. lm_update
def _n30(H, b, cost, n_valid):
    row = np.zeros(30)
    row[:21], row[21:27], row[27], row[28] = H[np.triu_indices(6)], b, cost, n_valid
    return row


def _scripts():
    """Per pose a list of normal30 rows: every branch of the state machine."""
    g = np.random.default_rng(5)

    def spd(cond):
        Q, _ = np.linalg.qr(g.standard_normal((6, 6)))
        return Q @ np.diag(np.geomspace(1.0, cond, 6)) @ Q.T * 50.0

    H1, H2, H3 = spd(23.0), spd(1e4), spd(1e8)
    b = g.standard_normal(6)
    sing = H1.copy()
    sing[2, :] = sing[:, 2] = 0.0
    nan = float("nan")
    return [
        # first accept, accept (lambda / 10), reject (lambda x 10, rewound), NaN cost (a rejection), accept again
        [_n30(H1, b, 2.0, 40), _n30(H2, 0.5 * b, 1.0, 41), _n30(H1, b, 1.5, 42), _n30(H1, b, nan, 42),
         _n30(H3, 0.1 * b, 0.5, 43)],
        # an equal cost is accepted; then a step below xi_tol: status 1; the rest is not looked at
        [_n30(H2, b, 1.0, 30), _n30(H1, b, 1.0, 30), _n30(H1, 1e-13 * b, 0.9, 30), _n30(H1, b, 0.1, 30),
         _n30(H1, b, 0.1, 30)],
        # five valid beams at once: status 2
        [_n30(H1, b, 2.0, 5)] * 5,
        # accepted once, then five valid beams: status 2 with the accepted evaluation kept
        [_n30(H1, b, 2.0, 40), _n30(H1, b, 1.0, 5)] + [_n30(H1, b, 1.0, 40)] * 3,
        # a singular H: status 3
        [_n30(sing, b, 2.0, 40)] * 5,
        # a NaN cost first is accepted (nothing to compare with), everything after it rejected
        [_n30(H1, b, nan, 40), _n30(H1, b, 1.0, 40), _n30(H2, b, 0.5, 40), _n30(H2, b, 0.5, 40),
         _n30(H2, b, 0.5, 40)],
        # an all-zero row (no beams): status 2
        [np.zeros(30)] * 5,
    ]


def _solve_bounds(row):
    """(xi_np, |xi| bound, pose-entry bound) of the restatement's state row after a step that solved."""
    A = FR.damped(row[FR.N30:FR.N30 + 30], row[FR.LAMBDA])
    xi = row[FR.XI:FR.XI + 6]
    bx = 64.0 * np.linalg.cond(A, 2) * U * np.linalg.norm(xi)
    tmax = max(1.0, float(np.abs(row[:24]).max()))
    return xi, bx, bx + 64.0 * U * tmax


def test_lm_update_walks_every_branch_like_the_restatement():
    xi_tol = 1e-9
    scripts = _scripts()
    starts = [G.se3_exp(np.asarray(RR.XI_STAR) * (1 + 0.3 * k)) for k in range(len(scripts))]
    state = P.lm_init(G._pose_rows(torch.stack(starts), "cuda"), 1e-3)
    assert _same(state.cpu(),
                     torch.from_numpy(np.stack([FR.to_row(FR.lm_init(T, 1e-3)) for T in starts])))
    seen, worst = set(), {"xi": 0.0, "pose": 0.0}
    for step in range(5):
        rows = np.stack([s[step] for s in scripts])
        before = state.cpu().numpy()
        state, cost, acc = P.lm_update(_dev(torch.from_numpy(rows)), state, xi_tol)
        after, cost, acc = state.cpu().numpy(), cost.cpu().numpy(), acc.cpu().numpy()
        for p in range(len(scripts)):
            st = FR.from_row(before[p])
            was = st["status"]
            c, a = FR.lm_update(st, rows[p], xi_tol, G.se3_exp)
            want = FR.to_row(st)
            if was != 0:   # a stopped pose keeps every word
                assert np.array_equal(after[p].view(np.int64), before[p].view(np.int64)) and math.isnan(cost[p])
                assert acc[p] == 0
                continue
            assert (math.isnan(c) and math.isnan(cost[p])) or cost[p] == c, (step, p)
            assert bool(acc[p]) == a, (step, p)
            # lambda, status and the counters exactly; the accepted evaluation and pose are copies
            for f in (FR.LAMBDA, FR.STATUS, FR.EVALS, FR.NACC):
                assert after[p, f] == want[f], (step, p, f)
            assert np.array_equal(after[p, FR.N30:FR.N30 + 30].view(np.int64), want[FR.N30:FR.N30 + 30].view(np.int64))
            assert np.array_equal(after[p, :12].view(np.int64), want[:12].view(np.int64)), (step, p)
            seen.add(("status", st["status"]))
            seen.add(("accept", a, st["nacc"] > 1))
            if st["status"] in (2, 3):
                if st["status"] == 3:   # the pose stays at the last accepted one
                    assert np.array_equal(after[p, 12:24].view(np.int64), after[p, :12].view(np.int64))
                else:                   # nothing else moves
                    assert np.array_equal(after[p, 12:24].view(np.int64), before[p, 12:24].view(np.int64))
                    assert np.array_equal(after[p, FR.XI:].view(np.int64), before[p, FR.XI:].view(np.int64))
                continue
            xi, bx, bt = _solve_bounds(want)
            ex = float(np.linalg.norm(after[p, FR.XI:FR.XI + 6] - xi))
            et = float(np.abs(after[p, 12:24] - want[12:24]).max())
            worst["xi"], worst["pose"] = max(worst["xi"], ex / max(bx, 1e-300)), max(worst["pose"], et / bt)
            assert ex <= bx, (step, p, ex, bx)
            assert et <= bt, (step, p, et, bt)
    _report({"test": "lm_update_branches", "worst_xi_over_bound": worst["xi"], "worst_pose_over_bound": worst["pose"]})
    print(worst, sorted(seen))
    for need in (("status", 1), ("status", 2), ("status", 3), ("accept", True, False), ("accept", True, True),
                 ("accept", False, False), ("accept", False, True)):
        assert need in seen, need
    final = state.cpu().numpy()
    assert final[:, FR.STATUS].tolist() == [0.0, 1.0, 2.0, 2.0, 3.0, 0.0, 2.0]
    assert final[:, FR.EVALS].tolist() == [5.0, 3.0, 1.0, 2.0, 1.0, 5.0, 1.0]
    assert final[:, FR.NACC].tolist() == [3.0, 3.0, 0.0, 1.0, 1.0, 1.0, 0.0]


# ----------------------------------------------------------------------------------------------- 6. se3_apply
def test_se3_apply_against_the_host_exponential():
    """test_registration_cpu.TWISTS (theta = 0, about 1e-9, both sides of the 0.5 series switch) and one twist with
    theta within 1e-3 of pi, on three poses each.  Measured on the MI355X: see DESIGN.md (batched refinement)."""
    axis = np.array([0.6, -0.48, 0.64])
    twists = [list(x) for x in TWISTS] + [[0.2, -0.1, 0.3] + list(axis * (math.pi - 5e-4))]
    poses = [torch.eye(4, dtype=torch.float64), G.se3_exp(RR.XI_STAR), G.se3_exp([2.0, -1.5, 0.7, 0.9, -1.4, 2.1])]
    xs = torch.tensor([x for x in twists for _ in poses], dtype=torch.float64)
    Ts = torch.stack([T for _ in twists for T in poses])
    got = G.apply_twists(Ts.cuda(), xs.cuda())
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (len(twists) * 3, 4, 4)
    got = got.cpu()
    worst = 0.0
    for k in range(xs.shape[0]):
        want = G.se3_exp(xs[k]) @ Ts[k]
        bound = 64.0 * U * max(1.0, float(want.abs().max()), float(Ts[k].abs().max()))
        e = float((got[k] - want).abs().max())
        worst = max(worst, e / bound)
        assert e <= bound, (k, xs[k].tolist(), e, bound)
        assert got[k, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
    _report({"test": "se3_apply", "worst_over_bound": worst, "worst_ulps": worst * 64.0})
    print("se3_apply worst error / bound:", worst)
    assert tuple(G.apply_twists(Ts[:0].cuda(), xs[:0].cuda()).shape) == (0, 4, 4)


# ----------------------------------------------------------------------------------------------- 7. one step in lockstep
def _scene():
    s = LR.grid_scene()
    good, bad = FR.starts()
    return s, torch.stack(good), bad


def test_one_step_equals_register_scan_fold_and_the_operator_loop_equals_the_entry():
    s, starts, _ = _scene()
    fold, pts = _dev(s["fold"]), _dev(s["points"])
    r = _refine(s["fold"], s["points"], starts, iters=1)
    assert r.iterations.tolist() == [1] * 4 and r.accepted.tolist() == [1] * 4 and r.status.tolist() == [0] * 4
    worst = 0.0
    for p in range(4):
        one = G.register_scan_fold(fold, fold, pts, starts[p], *BOX, iters=1, near=RR.NEAR)
        cost = float(r.cost[p])
        assert int(r.n_valid[p]) == one.n_valid == 256
        assert abs(cost - one.costs[0]) <= 1e-12 * abs(one.costs[0]) and float(r.eval_costs[p, 0]) == cost
        row = r.state[p].cpu().numpy()
        _, bx, bt = _solve_bounds(row)
        e = float((r.poses[p].cpu() - one.pose).abs().max())
        worst = max(worst, e / bt)
        assert e <= bt, (p, e, bt)
    _report({"test": "refine_one_step_vs_register_scan_fold", "worst_pose_over_bound": worst})
    rows = G._pose_rows(starts, "cuda")
    for k in (1, 3):
        want = P.refine_poses_fold(pts, rows, _box(), fold, fold, RR.NEAR, 64, 128, EPS, 0.0, 0.5, 1e-6, 1e-9, k)
        state = P.lm_init(rows, 1e-6)
        costs, accs = [], []
        for _ in range(k):
            n30 = P.pose_normal_eq_fold(pts, None, state, _box(), fold, fold, RR.NEAR, 64, 128, EPS, 0.0, 0.5,
                                        False)[0]
            state, c, a = P.lm_update(n30, state, 1e-9)
            costs.append(c)
            accs.append(a)
        assert _same(state, want[1]), k
        assert _same(state[:, 12:24], want[0]), k
        assert _same(torch.stack(costs, 1), want[2]), k
        assert _same(torch.stack(accs, 1), want[3]), k


# ----------------------------------------------------------------------------------------------- 8. end to end
def _delta_at_T_star(s):
    depth = _evaluate(s["fold"], s["points"], s["T_star"][None], 64, 128)[1][0].cpu().double()
    return float((depth - s["ranges"]).abs().max())


def test_refine_poses_fold_end_to_end():
    """The 256-beam scene, the four converging starts in one call, 20 evaluations: per pose the final error against T*
    is at most 2 (the float64 loop's error from that start) + 10 delta in translation (delta = max |depth_hip -
    depth_f64| at T*) and the same in rotation with delta over the mean range -- test_register_scan_fold_end_to_end's
    rule.  Measured on the MI355X: see DESIGN.md (batched refinement)."""
    s, starts, _ = _scene()
    runs, _ = FR.f64_runs()
    delta = _delta_at_T_star(s)
    r = _refine(s["fold"], s["points"], starts, iters=20)
    assert r.n_valid.tolist() == [256] * 4 and r.iterations.tolist() == [20] * 4 and r.status.tolist() == [0] * 4
    poses, ec, mask = r.poses.cpu(), r.eval_costs.cpu(), r.accepted_mask.cpu()
    for p in range(4):
        ht, hr = RR.pose_error(runs[p]["pose"], s["T_star"])
        et, er = RR.pose_error(poses[p], s["T_star"])
        bt, br = 2 * ht + 10 * delta, 2 * hr + 10 * delta / float(s["ranges"].mean())
        costs = ec[p][mask[p]].tolist()
        line = {"test": "refine_poses_fold", "start": p, "delta": delta, "err_t": et, "err_r": er, "f64_err_t": ht,
                "f64_err_r": hr, "bound_t": bt, "bound_r": br, "accepted": len(costs), "cost_first": costs[0],
                "cost_last": costs[-1]}
        _report(line)
        print(line)
        assert et <= bt and er <= br, line
        assert all(b <= a for a, b in zip(costs, costs[1:])) and costs[-1] == float(r.cost[p])
        assert int(r.accepted[p]) == len(costs) and bool(torch.isfinite(ec[p]).all())


def test_xi_tol_stops_a_pose_where_the_restatement_stops():
    """xi_tol = the geometric mean of the float64 loop's |xi| at its 8th and 9th evaluation: status 1, and as many
    evaluations as the float64 restatement makes with that threshold."""
    s, starts, _ = _scene()
    ev = FR.evaluate_f64(s["fold"], s["dirs"], s["ranges"].numpy())
    for p in (0, 3):
        free = FR.run(ev, starts[p], G.se3_exp)
        tol = math.sqrt(free["xi_norms"][7] * free["xi_norms"][8])
        want = FR.run(ev, starts[p], G.se3_exp, xi_tol=tol)
        assert want["state"]["status"] == 1 and want["state"]["evals"] == 9
        r = _refine(s["fold"], s["points"], starts[p:p + 1], iters=20, xi_tol=tol)
        print("xi_tol", tol, "evaluations", r.iterations.tolist(), "status", r.status.tolist())
        assert r.status.tolist() == [1] and r.iterations.tolist() == [want["state"]["evals"]]
        ec = r.eval_costs[0].cpu()
        assert bool(torch.isfinite(ec[:9]).all()) and bool(torch.isnan(ec[9:]).all())
        assert not bool(r.accepted_mask[0, 9:].any())
        assert float(r.state[0, FR.XI:FR.XI + 6].norm()) < tol


def test_the_rejection_start_keeps_the_invariants():
    s, _, bad = _scene()
    damping = 1e-6
    r = _refine(s["fold"], s["points"], bad[None], iters=20, damping=damping)
    ec, mask = r.eval_costs[0].cpu(), r.accepted_mask[0].cpu()
    assert r.iterations.tolist() == [20] and bool(torch.isfinite(r.poses).all()) and r.status.tolist() == [0]
    costs = ec[mask].tolist()
    accepts, rejects = len(costs), 20 - len(costs)
    print("rejection start: accepted", accepts, "of 20; lambda", float(r.lam[0]))
    assert bool(mask[0]) and int(r.accepted[0]) == accepts and costs[-1] == float(r.cost[0])
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    # the mask is the accept rule applied to eval_costs, and lambda its replay
    lam, best = damping, None
    for k in range(20):
        c = float(ec[k])
        ok = best is None or c <= best
        assert ok == bool(mask[k]), k
        if ok:
            lam, best = (lam / 10.0 if best is not None else lam), c
        else:
            lam = lam * 10.0
    assert float(r.lam[0]) == lam
    assert math.isclose(lam, damping * 10.0 ** (rejects - (accepts - 1)), rel_tol=1e-12)


def test_five_beams_leave_every_pose_undetermined_and_empty_inputs_give_empties():
    s, starts, _ = _scene()
    r = _refine(s["fold"], s["points"][:5], starts, iters=20)
    assert r.status.tolist() == [2] * 4 and r.iterations.tolist() == [1] * 4 and r.accepted.tolist() == [0] * 4
    assert torch.equal(r.poses.cpu(), starts) and r.n_valid.tolist() == [0] * 4
    assert bool(torch.isfinite(r.eval_costs[:, 0]).all()) and bool(torch.isnan(r.eval_costs[:, 1:]).all())
    none = _refine(s["fold"], s["points"][:0], starts, iters=3)   # no beams: nothing is valid
    assert none.status.tolist() == [2] * 4 and torch.equal(none.poses.cpu(), starts)
    empty = _refine(s["fold"], s["points"], starts[:0], iters=3)
    assert tuple(empty.poses.shape) == (0, 4, 4) and tuple(empty.eval_costs.shape) == (0, 3)
    zero = _refine(s["fold"], s["points"], starts, iters=0)
    assert torch.equal(zero.poses.cpu(), starts) and tuple(zero.eval_costs.shape) == (4, 0)
    for S, I in ((512, 513), (2, 8), (8, 0)):
        with pytest.raises(RuntimeError, match="at most 1024|at least"):
            _refine(s["fold"], s["points"], starts, N_samples=S, N_importance=I)


# ----------------------------------------------------------------------------------------------- 9. localisation
def test_localize_scan_fold_batched():
    """LR.grid_scene(): the winner is the centre hypothesis, within check 8's bound of T*; refine="sequential" is the
    call without the keyword, bit for bit."""
    s = LR.grid_scene()
    fold, pts = _dev(s["fold"]), _dev(s["points"])
    delta = _delta_at_T_star(s)
    from nof.registration import se3_exp
    run = RR.register_f64(s["fold"], s["fold"], s["dirs"], s["ranges"].numpy(), s["center"], se3_exp,
                          T_ref=s["T_star"])
    ht, hr = RR.pose_error(run["pose"], s["T_star"])
    kw = dict(top_k=4, refine_iters=20, near=RR.NEAR)
    res = L.localize_scan_fold(fold, fold, pts, s["poses"], *BOX, refine="batched", **kw)
    et, er = RR.pose_error(res.pose, s["T_star"])
    bt, br = 2 * ht + 10 * delta, 2 * hr + 10 * delta / float(s["ranges"].mean())
    line = {"test": "localize_scan_fold_batched", "index": res.index, "score": res.score, "delta": delta, "err_t": et,
            "err_r": er, "bound_t": bt, "bound_r": br}
    _report(line)
    print(line)
    assert res.index == 62 and et <= bt and er <= br, line
    assert len(res.refined) == 4 and all(isinstance(q, G.RegistrationResult) for q in res.refined)
    assert res.pose.dtype == torch.float64 and tuple(res.pose.shape) == (4, 4) and not res.pose.is_cuda
    first = res.refined[0]
    assert torch.equal(res.pose, first.pose)
    assert res.score == (first.costs[-1] + s["miss_cost"] * (256 - first.n_valid)) / 256
    seq = L.localize_scan_fold(fold, fold, pts, s["poses"], *BOX, refine="sequential", **kw)
    plain = L.localize_scan_fold(fold, fold, pts, s["poses"], *BOX, **kw)
    assert torch.equal(seq.pose, plain.pose) and seq.score == plain.score and seq.index == plain.index == 62
    assert [q.costs for q in seq.refined] == [q.costs for q in plain.refined]
    assert all(torch.equal(a.pose, b.pose) for a, b in zip(seq.refined, plain.refined))
    assert max(L.pose_distance(res.pose, plain.pose)) <= 1e-3


def test_localize_batched_raises_when_no_candidate_is_left():
    s = LR.grid_scene()
    fold = _dev(s["fold"])
    with pytest.raises(RuntimeError, match="no candidate is left"):
        L.localize_scan_fold(fold, fold, _dev(s["points"][:5]), s["poses"][60:65], *BOX, top_k=2, refine_iters=3,
                             near=RR.NEAR, refine="batched")
