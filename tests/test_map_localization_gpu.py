"""pcnerf::score_poses_map / pose_normal_eq_map / refine_poses_map and nof.localization's map functions on the MI355X.

The contract is equality: for a pose with block b every output has the bits the single-block operator gives for that
pose with block b's folds and box alone; a pose without a block (-1, or an index outside the map) renders nothing.  The
end-to-end check is test_refine_gpu's: the final error against the truth is at most 2 (the float64 loop's error from
the same start) + 10 delta, delta = max |depth_hip - depth_f64| at the truth pose."""
import functools
import math

import numpy as np
import pytest
import torch

import localization_ref as LR
import map_ref as MR
import registration_ref as RR
from gradcheck import _report
from sampling_f64 import same_bits
from test_localization_gpu import NEAR_TWISTS, _points
from nof import _torch_ops as T
from nof import localization as L
from nof import registration as G
from nof import synthetic as syn

pytestmark = pytest.mark.gpu
P = torch.ops.pcnerf
EPS = G.EPSILON
DELTA = 0.05
_CACHE = {}


def _dev(t):
    return t.cuda().contiguous()


def _same(a, b):
    if a.is_floating_point():
        return same_bits(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))


def _random_folds():
    """Three folds of random init_nof_params networks (seeds 1, 2, 3), composed on the device -> (3, 64) float64 CPU."""
    if "random" not in _CACHE:
        from nof.networks import NOF_fine
        rows = []
        for seed in (1, 2, 3):
            m = syn.load_into(NOF_fine(), syn.init_nof_params(seed)).cuda().eval()
            with torch.no_grad():
                rows.append(P.fold_eval(T.eval_params(m)).cpu())
        _CACHE["random"] = torch.stack(rows)
    return _CACHE["random"]


def _map(field, B):
    """(folds_c, folds_f, boxes) on the device: B blocks whose coarse and fine folds and boxes all differ."""
    if field == "analytic":
        F = torch.stack([RR.analytic_fold(), MR.block1_fold(), MR.block1_fold(-0.65)])
    else:
        F = _random_folds()
    boxes = torch.tensor([[-2.5, -2.5, -2.5, 2.5, 2.5, 2.5], [-2.4, -2.6, -2.5, 2.6, 2.4, 2.7],
                          [-3.0, -3.0, -3.0, 3.0, 3.0, 3.0]], dtype=torch.float64)
    return _dev(F[:B]), _dev(F.roll(-1, 0)[:B]), _dev(boxes[:B])


def _poses(Pn):
    T_star = G.se3_exp(RR.XI_STAR)
    near = [G.se3_exp(x) @ T_star for x in NEAR_TWISTS]
    return torch.stack((near + [near[1], near[2]])[:Pn])


def _ids(B, Pn):
    if Pn == 1:
        return [[B - 1], [-1]]
    return [[0, B - 1, -1, min(1, B - 1), 7], [-5, 0, B - 1, 0, 0]]


def _planted(R, seed):
    pts = _points(R, seed).clone()
    if R >= 5:
        pts[1] = 0.0
        pts[3, 1] = float("nan")
    return pts


def _score_map(pts, rows, ids, m, S, I, want=True):
    return P.score_poses_map(pts, rows, ids, m[2], m[0], m[1], RR.NEAR, S, I, EPS, DELTA, 0.5, want)


def _neq_map(pts, rows, ids, m, S, I, want=True, state=None):
    return P.pose_normal_eq_map(pts, None if state is not None else rows, state, ids, m[2], m[0], m[1], RR.NEAR, S, I,
                                EPS, DELTA, 0.5, want)


# ----------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("field", ["analytic", "random"])
@pytest.mark.parametrize("S,I", [(3, 1), (64, 128), (129, 895)])
def test_every_pose_has_the_bits_of_its_block_alone(S, I, field):
    """B in {1, 3} x P in {1, 5} x R in {1, 5, 67} (MAXB 1, 4 and 16 over the three sample counts, a partial last
    workgroup, the 1,024 limit), mixed block ids with -1 and out-of-range ones, a zero and a NaN point."""
    checked, valid_seen = 0, 0.0
    for B in (1, 3):
        m = _map(field, B)
        for R in (1, 5, 67):
            pts = _dev(_planted(R, S))
            for Pn in (1, 5):
                poses = _poses(Pn)
                rows = G._pose_rows(poses, "cuda")
                for ids_list in _ids(B, Pn):
                    ids = torch.tensor(ids_list, dtype=torch.int32).cuda()
                    case = f"{field} B{B} P{Pn} R{R} S{S} I{I} ids{ids_list}"
                    s4, depth, sumw = _score_map(pts, rows, ids, m, S, I)
                    n30, nd, nsw, jac = _neq_map(pts, rows, ids, m, S, I)
                    valid_seen = max(valid_seen, float(s4[:, 1].max()))
                    # the same bits over two runs, without the per-beam outputs, and with the poses from the host
                    again = _score_map(pts, rows, ids, m, S, I)
                    assert all(_same(a, b) for a, b in zip((s4, depth, sumw), again)), case
                    assert _same(_score_map(pts, rows, ids, m, S, I, want=False)[0], s4), case
                    assert _same(_neq_map(pts, rows, ids, m, S, I, want=False)[0], n30), case
                    via = L.score_poses_map(L.BlockMap(m[0], m[1], m[2]), pts, poses.cuda(), ids, N_samples=S,
                                            N_importance=I, huber_delta=DELTA, near=RR.NEAR, want_depth=True)
                    host = L.score_poses_map(L.BlockMap(m[0], m[1], m[2]), pts, poses, ids_list, N_samples=S,
                                             N_importance=I, huber_delta=DELTA, near=RR.NEAR, want_depth=True)
                    for r in (via, host):
                        assert _same(r.cost, s4[:, 0].contiguous()) and _same(r.depth, depth), case
                        assert _same(r.hit, s4[:, 3].contiguous()) and _same(r.sumw, sumw), case
                    for p, b in enumerate(ids_list):
                        if not 0 <= b < B:
                            assert bool((s4[p] == 0).all()) and bool((n30[p] == 0).all()), case
                            assert bool(torch.isnan(depth[p]).all()) and bool((sumw[p] == 0).all()), case
                            assert bool((nd[p] == 0).all()) and bool((nsw[p] == 0).all()), case
                            assert bool((jac[p] == 0).all()), case
                            continue
                        one = P.score_poses_fold(pts, rows[p:p + 1], m[2][b], m[0][b], m[1][b], RR.NEAR, S, I, EPS,
                                                 DELTA, 0.5, True)
                        assert _same(s4[p:p + 1], one[0]) and _same(depth[p:p + 1], one[1]), (case, p)
                        assert _same(sumw[p:p + 1], one[2]), (case, p)
                        neq = P.pose_normal_eq_fold(pts, rows[p:p + 1], None, m[2][b], m[0][b], m[1][b], RR.NEAR, S, I,
                                                    EPS, DELTA, 0.5, True)
                        assert _same(n30[p:p + 1], neq[0]) and _same(nd[p:p + 1], neq[1]), (case, p)
                        assert _same(nsw[p:p + 1], neq[2]) and _same(jac[p:p + 1], neq[3]), (case, p)
                        assert _same(nd[p], depth[p]) and _same(nsw[p], sumw[p]), (case, p)
                        checked += 1
    assert checked >= 20 and (field == "random" or valid_seen > 0)   # (analytic: the comparison is not of zeros alone)


def test_blocks_differ_so_the_bits_tell_them_apart():
    """The same pose scored against each of the three blocks gives three different rows: a kernel that staged the
    wrong block's folds or box would not pass the test above by accident."""
    for field in ("analytic", "random"):
        m = _map(field, 3)
        pts = _dev(_planted(67, 64))
        rows = G._pose_rows(_poses(1).repeat(3, 1, 1), "cuda")
        ids = torch.tensor([0, 1, 2], dtype=torch.int32).cuda()
        s4, depth, _ = _score_map(pts, rows, ids, m, 64, 128)
        assert not _same(depth[0], depth[1]) and not _same(depth[1], depth[2]) and not _same(depth[0], depth[2])


# ----------------------------------------------------------------------------------------------- 2. refinement
def _two_block_map():
    s = MR.two_block_scene()
    f = _dev(s["folds"])
    return L.BlockMap(f, f, _dev(torch.as_tensor(s["boxes"])))


def test_refine_poses_map_equals_refine_poses_fold_per_block():
    """3 poses in 2 blocks and one without a block, 259 beams, 64 + 128, 5 evaluations: poses, the 64-word state,
    eval_costs and accepted equal refine_poses_fold per block bit for bit; the pose without a block stops with status 2
    at the first update and returns its input bits."""
    bm = _two_block_map()
    near = _poses(3)
    poses = torch.stack([near[0], MR.shifted(near[1]), near[2], MR.shifted(near[1])])
    ids = [0, 1, 0, -1]
    pts = _dev(_points(259, 64))
    kw = dict(iters=5, huber_delta=DELTA, near=RR.NEAR)
    r = G.refine_poses_map(bm, pts, poses, ids, **kw)
    again = G.refine_poses_map(bm, pts, poses.cuda(), torch.tensor(ids).cuda(), **kw)
    for a, b in zip(r, again):
        assert _same(a, b)
    boxes = MR.two_block_scene()["boxes"]
    for b in (0, 1):
        sel = [p for p, v in enumerate(ids) if v == b]
        one = G.refine_poses_fold(bm.folds_c[b], bm.folds_f[b], pts, poses[sel], boxes[b, :3], boxes[b, 3:], **kw)
        for name in ("poses", "state", "eval_costs", "accepted_mask", "status", "n_valid", "cost", "lam"):
            assert _same(getattr(r, name)[sel], getattr(one, name)), (b, name)
        assert one.iterations.tolist() == [5] * len(sel) and int(one.n_valid.min()) >= 6
    assert r.status.tolist()[3] == 2 and r.iterations.tolist()[3] == 1 and r.accepted.tolist()[3] == 0
    assert torch.equal(r.poses[3].cpu(), poses[3]) and int(r.n_valid[3]) == 0
    assert bool(torch.isnan(r.eval_costs[3, 1:]).all()) and float(r.eval_costs[3, 0]) == 0.0
    # blocks=None assigns them from the start poses: the pose without a block falls into block 1
    auto = G.refine_poses_map(bm, pts, poses, **kw)
    assert _same(auto.state[:3], r.state[:3]) and _same(auto.state[3], r.state[1])
    # the operator loop through the state equals the entry
    rows = G._pose_rows(poses, "cuda")
    idt = torch.tensor(ids, dtype=torch.int32).cuda()
    state = P.lm_init(rows, 1e-6)
    for _ in range(5):
        n30 = P.pose_normal_eq_map(pts, None, state, idt, bm.boxes, bm.folds_c, bm.folds_f, RR.NEAR, 64, 128, EPS,
                                   DELTA, 0.5, False)[0]
        state, _, _ = P.lm_update(n30, state, 1e-9)
    assert _same(state, r.state)


def test_assign_blocks_equals_the_restatement():
    rng = np.random.default_rng(3)
    for B in (1, 3, 17):
        lo = rng.uniform(-4, 2, size=(B, 3))
        boxes = np.concatenate([lo, lo + rng.uniform(0.5, 5, size=(B, 3))], 1)
        if B >= 3:
            boxes[2] = boxes[0]                       # equal clearance: the lower index
            boxes[1, :3], boxes[1, 3:] = boxes[0, :3] + 0.25, boxes[0, 3:] - 0.25   # nested
        for Pn in (1, 64, 65, 4099):
            t = rng.uniform(-5, 7, size=(Pn, 3))
            t[0] = boxes[0, :3]                       # a corner: on three faces
            if Pn > 4:
                t[1, 1] = np.nan
                t[2] = boxes[B - 1, 3:]
                t[3, 0] = np.inf
            poses = torch.eye(4, dtype=torch.float64).repeat(Pn, 1, 1)
            poses[:, :3, 3] = torch.as_tensor(t)
            for margin in (0.0, 0.25):
                want = MR.assign_blocks(boxes, t, margin)
                got = P.assign_blocks(G._pose_rows(poses, "cuda"), _dev(torch.as_tensor(boxes)), margin)
                assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (B, Pn, margin)
            if Pn == 4099:
                assert (want >= 0).any() and (want < 0).any()
    bm = _two_block_map()
    s = MR.two_block_scene()
    ids = L.assign_blocks(bm, s["poses"])
    assert ids.tolist() == [0] * 125 + [1] * 125 and _same(ids, L.assign_blocks(bm, s["poses"].cuda()))


# ----------------------------------------------------------------------------------------------- 3. end to end
@functools.lru_cache(maxsize=None)
def _delta_at_truth():
    s = MR.two_block_scene()
    bm = _two_block_map()
    r = L.score_poses_map(bm, _dev(s["points"]), s["T1"][None], [1], near=RR.NEAR, want_depth=True)
    return float((r.depth[0].cpu().double() - s["ranges"]).abs().max())


def test_localize_scan_map_end_to_end():
    """The two-block scene, the scan rendered in float64 from block 1's truth pose, 125 + 125 hypotheses around both
    blocks' (offset) truths: the winner is a hypothesis of block 1, the result names block 1 and ends within
    2 (the float64 loop's error from the same start) + 10 delta of T*_1.  The float64 loop runs in block 0's
    coordinates (the start and the truth shifted by -2 pi: the field has that period), where its box is."""
    s = MR.two_block_scene()
    bm = _two_block_map()
    pts = _dev(s["points"])
    delta = _delta_at_truth()
    res = L.localize_scan_map(bm, pts, s["poses"], top_k=4, refine_iters=20, near=RR.NEAR)
    assert isinstance(res, L.MapLocalizationResult) and res.index >= 125 and res.block == 1
    assert res.blocks.tolist() == [0] * 125 + [1] * 125 and tuple(res.scores.shape) == (250,)
    f1 = s["folds"][1]
    run = RR.register_f64(f1, f1, s["dirs"], s["ranges"].numpy(), MR.shifted(s["poses"][res.index], -MR.TWO_PI),
                          G.se3_exp, T_ref=s["T0"])
    ht, hr = RR.pose_error(run["pose"], s["T0"])
    et, er = RR.pose_error(res.pose, s["T1"])
    bt, br = 2 * ht + 10 * delta, 2 * hr + 10 * delta / float(s["ranges"].mean())
    line = {"test": "localize_scan_map", "index": res.index, "block": res.block, "score": res.score, "delta": delta,
            "err_t": et, "err_r": er, "f64_err_t": ht, "f64_err_r": hr, "bound_t": bt, "bound_r": br}
    _report(line)
    print(line)
    assert et <= bt and er <= br, line
    assert len(res.refined) == 4 and res.pose.dtype == torch.float64 and not res.pose.is_cuda
    # every block-1 hypothesis scores below every block-0 hypothesis' miss-charged mean?  Not required; the best does
    assert int(torch.argmin(res.scores)) >= 125


def test_default_miss_cost_is_the_largest_over_the_blocks():
    m = _map("analytic", 3)
    bm = L.BlockMap(m[0], m[1], m[2])
    boxes = m[2].cpu().numpy()
    each = [L.default_miss_cost(b[:3], b[3:], 0.05) for b in boxes]
    assert bm.default_miss_cost(0.05) == max(each) == each[2] and bm.n_blocks == 3


# ----------------------------------------------------------------------------------------------- 4. rejection
def test_map_operators_reject_bad_operands():
    m = _map("analytic", 3)
    pts = _dev(_points(5, 1))
    rows = G._pose_rows(_poses(5), "cuda")
    ids = torch.zeros(5, dtype=torch.int32).cuda()
    ok = lambda **k: None   # noqa: E731
    args = dict(pts=pts, rows=rows, ids=ids, boxes=m[2], fc=m[0], ff=m[1], S=64, I=128)

    def score(**k):
        a = {**args, **k}
        return P.score_poses_map(a["pts"], a["rows"], a["ids"], a["boxes"], a["fc"], a["ff"], RR.NEAR, a["S"], a["I"],
                                 EPS, 0.0, 0.5, False)

    def neq(**k):
        a = {**args, **k}
        return P.pose_normal_eq_map(a["pts"], a["rows"], None, a["ids"], a["boxes"], a["fc"], a["ff"], RR.NEAR, a["S"],
                                    a["I"], EPS, 0.0, 0.5, False)

    def refine(**k):
        a = {**args, **k}
        return P.refine_poses_map(a["pts"], a["rows"], a["ids"], a["boxes"], a["fc"], a["ff"], RR.NEAR, a["S"],
                                  a["I"], EPS, 0.0, 0.5, 1e-6, 1e-9, 2)

    score(), neq(), refine(), ok()
    bad = [dict(pts=pts.cpu()), dict(rows=rows.cpu()), dict(ids=ids.cpu()), dict(boxes=m[2].cpu()),
           dict(ids=ids.long()), dict(rows=rows.float()), dict(fc=m[0].float()), dict(pts=pts.double()),
           dict(fc=m[0][:, :63].contiguous()), dict(ff=m[1][:2]), dict(boxes=m[2][:, :5].contiguous()),
           dict(ids=ids[:4]), dict(rows=rows[:, :11].contiguous()), dict(fc=m[0].t().contiguous().t()),
           dict(S=512, I=513), dict(S=2, I=8), dict(S=8, I=0)]
    for fn in (score, neq, refine):
        for k in bad:
            with pytest.raises(RuntimeError):
                fn(**k)
    with pytest.raises(RuntimeError):
        P.assign_blocks(rows.cpu(), m[2], 0.0)
    with pytest.raises(RuntimeError):
        P.assign_blocks(rows, m[2][:, :5].contiguous(), 0.0)
    with pytest.raises(RuntimeError):
        P.assign_blocks(rows.float(), m[2], 0.0)
    with pytest.raises(RuntimeError, match="device"):
        L.BlockMap(m[0].cpu(), m[1].cpu(), m[2].cpu())
    with pytest.raises(RuntimeError, match="boxes"):
        L.BlockMap(m[0], m[1], m[2][:2])
    with pytest.raises(RuntimeError, match="blocks must be"):
        L.score_poses_map(L.BlockMap(*m), pts, _poses(5), [0, 1])
