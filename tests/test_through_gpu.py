"""pcnerf::score_poses_through, nof.localization.score_poses_through / synthesize_scan and ParticleFilter(through=True)
on the MI355X, against the single-block operator composed on the host and against the float64 restatement of
tests/through_ref.py.

1. a beam of one segment has score_poses_map's bits; 2. a chain is score_poses_fold's segments, composed by the
restatement's rule and chain arithmetic on the float32 results, bit for bit; 3. depth and sumw against float64 by the
per-kernel rule e_hip <= max(4 e32, 2.4e-7) (parity_helpers.Tally); 4. the bits do not depend on the batch, the
outputs asked for or where the poses live; 5. the particle filter; 6. operand checks."""
import functools

import numpy as np
import pytest
import torch

import localization_ref as LR
import map_ref as MR
import registration_ref as RR
import through_ref as TR
from gradcheck import _report
from parity_helpers import Tally
from sampling_f64 import same_bits
from nof import localization as L
from nof import mcl as M
from nof import registration as G

pytestmark = pytest.mark.gpu
P = torch.ops.pcnerf
EPS = G.EPSILON
DELTA = 0.05
NOCAP = float("inf")
SAMPLES = [(3, 1), (64, 128), (129, 895)]
NEAR_TWISTS = ((0.0,) * 6, (0.2, -0.15, 0.1, 0.05, -0.03, 0.08), (-0.25, 0.2, -0.1, -0.06, 0.04, -0.12))


def _dev(t):
    return torch.as_tensor(t).cuda().contiguous()


def _same(a, b):
    if a.is_floating_point():
        return same_bits(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))


def _through(pts, rows, ids, m, S, I, K, tol=1e-3, tmin=1e-3, want=True, delta=DELTA):
    """m = (folds_c, folds_f, boxes) on the device."""
    return P.score_poses_through(pts, rows, ids, m[2], m[0], m[1], RR.NEAR, S, I, EPS, delta, 0.5, K, tol, tmin, want)


def _map_of(scene):
    return _dev(scene["folds_c"]), _dev(scene["folds_f"]), _dev(torch.from_numpy(scene["boxes"]))


# ----------------------------------------------------------------------------------------------- 1. one segment
OFFSETS = torch.tensor([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0]], dtype=torch.float64)


def _three_blocks(B, disjoint):
    """B blocks whose coarse and fine folds and boxes all differ; overlapping around the origin, or 10 m apart."""
    F = torch.stack([RR.analytic_fold(), MR.block1_fold(), MR.block1_fold(-0.65)])
    boxes = torch.tensor([[-2.5, -2.5, -2.5, 2.5, 2.5, 2.5], [-2.4, -2.6, -2.5, 2.6, 2.4, 2.7],
                          [-3.0, -3.0, -3.0, 3.0, 3.0, 3.0]], dtype=torch.float64)
    if disjoint:
        boxes = boxes + torch.cat([OFFSETS, OFFSETS], 1)
    return _dev(F[:B]), _dev(F.roll(-1, 0)[:B]), _dev(boxes[:B])


def _poses(Pn, ids, B, disjoint):
    """Poses within 0.4 m / 10 degrees of T*, each moved into its own block of the disjoint map."""
    T_star = G.se3_exp(RR.XI_STAR)
    near = [G.se3_exp(x) @ T_star for x in NEAR_TWISTS]
    poses = torch.stack((near + [near[1], near[2]])[:Pn]).clone()
    if disjoint:
        for p, b in enumerate(ids):
            if 0 <= b < B:
                poses[p, :3, 3] += OFFSETS[b]
    return poses


def _ids(B, Pn):
    if Pn == 1:
        return [[B - 1], [-1]]
    return [[0, B - 1, -1, min(1, B - 1), 7], [-5, 0, B - 1, 0, 0]]


def _planted(R, seed):
    g = torch.Generator().manual_seed(7000 + seed)
    pts = (RR.unit_directions(R, seed) * (0.7 + 1.3 * torch.rand(R, 1, generator=g, dtype=torch.float64))).float()
    if R >= 5:
        pts[1] = 0.0
        pts[3, 1] = float("nan")
    return pts


@pytest.mark.parametrize("S,I", SAMPLES)
def test_one_segment_is_the_clipped_render(S, I):
    """max_segments = 1 on overlapping boxes, and max_segments = 4 on boxes 10 m apart (no beam finds a second block):
    scores4, depth and sumw are score_poses_map's bit for bit.  B in {1, 3} x P in {1, 5} x R in {1, 5, 67}, block ids
    mixed with -1, 7 and -5, a zero and a NaN point."""
    checked = 0
    for K, disjoint in ((1, False), (4, True)):
        for B in (1, 3):
            m = _three_blocks(B, disjoint)
            for R in (1, 5, 67):
                pts = _dev(_planted(R, S))
                for Pn in (1, 5):
                    for ids_list in _ids(B, Pn):
                        rows = G._pose_rows(_poses(Pn, ids_list, B, disjoint), "cuda")
                        ids = torch.tensor(ids_list, dtype=torch.int32).cuda()
                        case = f"K{K} B{B} P{Pn} R{R} S{S} I{I} ids{ids_list}"
                        want = P.score_poses_map(pts, rows, ids, m[2], m[0], m[1], RR.NEAR, S, I, EPS, DELTA, 0.5, True)
                        s4, depth, sumw, nseg, last = _through(pts, rows, ids, m, S, I, K)
                        assert _same(s4, want[0]) and _same(depth, want[1]) and _same(sumw, want[2]), case
                        has = torch.tensor([0 <= b < B for b in ids_list]).cuda()
                        assert bool((nseg == has[:, None].to(torch.int32)).all()), case
                        assert bool((last == torch.where(has, ids, torch.full_like(ids, -1))[:, None]).all()), case
                        checked += int(has.sum()) * R
    torch.cuda.synchronize()
    assert checked > 0


# ----------------------------------------------------------------------------------------------- 2. the composed chain
SCENES = {"split": TR.split_cavity, "row": TR.row_of_three, "gap_joined": lambda: TR.row_of_three(gap=5e-4),
          "gap_open": lambda: TR.row_of_three(gap=5e-3), "overlap": lambda: TR.row_of_three(overlap=1.0),
          "blocks65": TR.sixty_five_blocks}


def _scene_pose_dirs(name, R):
    if name == "split":
        return TR.cavity_pose(), RR.unit_directions(R, 0)
    return TR.row_pose(), TR.row_directions(R, 0)


@functools.lru_cache(maxsize=None)
def _scan(name, R):
    """The scene, its pose and R float32 points whose ranges are the float64 through depths at 64 + 128 samples (1.5 m
    where the beam sees nothing), computed once."""
    scene = SCENES[name]()
    pose, dirs = _scene_pose_dirs(name, R)
    r64 = TR.through_render(scene, pose, TR.scan_points(dirs), 0, 64, 128, 4, 1e-3, 0.0)
    ranges = np.where(r64["sumw"] >= 0.5, r64["depth"], np.nan)
    return scene, pose, TR.scan_points(dirs, ranges)


_SEGMENTS = {}


def _composed_segments(name, R, S, I):
    """walk_many's segment render by the shipped single-block operator: one score_poses_fold call per (beam, segment)
    with that one point, the pose, the block's box and folds and near = near_k.  Results are kept per (beam, block,
    near_k): they do not depend on max_segments or min_transmittance."""
    scene, pose, pts = _scan(name, R)
    m = _map_of(scene)
    rows = G._pose_rows(pose[None], "cuda")
    pd = _dev(pts)
    row12 = TR.pose_rows(pose[None])[0]
    beam_of = {tuple(TR.ray_od(row12, p)[1]): i for i, p in enumerate(pts.numpy())}
    assert len(beam_of) == R
    kept = _SEGMENTS.setdefault((name, R, S, I), {})

    def segments(block, o, d, near_k, te):
        keys = [(beam_of[tuple(di)], block, float(nk)) for di, nk in zip(d, near_k)]
        todo = [k for k in keys if k not in kept]
        outs = [P.score_poses_fold(pd[i:i + 1], rows, m[2][b], m[0][b], m[1][b], nk, S, I, EPS, 0.0, 0.5, True)
                for i, b, nk in todo]
        if outs:
            dep = torch.cat([o_[1].reshape(1) for o_ in outs]).cpu().numpy()
            sw = torch.cat([o_[2].reshape(1) for o_ in outs]).cpu().numpy()
            for k, v, s in zip(todo, dep, sw):
                kept[k] = (v, s)
        return np.array([kept[k][0] for k in keys], np.float32), np.array([kept[k][1] for k in keys], np.float32)

    return segments


def _check_composed(name, R, S, I, K, tmin, tol=1e-3):
    scene, pose, pts = _scan(name, R)
    m = _map_of(scene)
    rows = G._pose_rows(pose[None], "cuda")
    ids = torch.zeros(1, dtype=torch.int32).cuda()
    s4, depth, sumw, nseg, last = _through(_dev(pts), rows, ids, m, S, I, K, tol, tmin)
    torch.cuda.synchronize()
    walks = TR.walk_many(scene["boxes"], TR.pose_rows(pose[None])[0], pts.numpy(), 0, K, tol, tmin,
                         _composed_segments(name, R, S, I))
    case = f"{name} R{R} S{S} I{I} K{K} tmin{tmin}"
    want_d = torch.from_numpy(np.array([w["depth"] for w in walks], np.float32))[None]
    want_s = torch.from_numpy(np.array([w["sumw"] for w in walks], np.float32))[None]
    want_n = [w["n_segments"] for w in walks]
    want_b = [w["last_block"] for w in walks]
    assert nseg.cpu()[0].tolist() == want_n and last.cpu()[0].tolist() == want_b, case
    assert same_bits(depth.cpu(), want_d), (case, (depth.cpu() != want_d).sum())
    assert same_bits(sumw.cpu(), want_s), (case, (sumw.cpu() != want_s).sum())
    # scores4: the float64 sums of the operator's own per-beam outputs
    tgt = LR.dirs_of(pts)[1].numpy()
    ref, mag = LR.reduce_scores(depth.cpu().numpy(), sumw.cpu().numpy(), tgt, DELTA, 0.5)
    got = s4.cpu().numpy()
    assert (got[:, 1] == ref[:, 1]).all(), case
    assert (np.abs(got - ref) <= 1e-12 * mag).all(), (case, np.abs(got - ref) / np.maximum(mag, 1e-300))
    return want_n


@pytest.mark.parametrize("S,I", SAMPLES)
@pytest.mark.parametrize("R", [5, 67])
@pytest.mark.parametrize("name", ["split", "row"])
def test_the_chain_is_the_single_block_operator_composed(name, R, S, I):
    """Every beam: depth, sumw, n_segments and last_block equal the host walk over score_poses_fold's segments bit for
    bit, at max_segments 2 and 4 and min_transmittance 0 and 1e-3."""
    for K in (2, 4):
        for tmin in (0.0, 1e-3):
            n = _check_composed(name, R, S, I, K, tmin)
            assert max(n) == (2 if name == "split" else min(K, 3)), (name, K, n)
    if name == "split" and R == 67 and (S, I) == (64, 128):   # the transmittance stop takes part
        a = _check_composed(name, R, S, I, 2, 0.0)
        b = _check_composed(name, R, S, I, 2, 0.5)
        assert sum(b) < sum(a)


@pytest.mark.parametrize("name", ["gap_joined", "gap_open", "overlap", "blocks65"])
def test_gaps_overlap_and_sixty_five_blocks_composed(name):
    n = _check_composed(name, 67, 64, 128, 4, 1e-3)
    assert max(n) == (1 if name == "gap_open" else 3)
    assert sorted(set(n)) == ([1] if name == "gap_open" else [1, 2, 3])


# ----------------------------------------------------------------------------------------------- 3. float64
def _err(x, q64):
    """max |x - q64| / |q64|; where q64 is 0 the value must be exactly 0."""
    x, q64 = np.asarray(x, np.float64), np.asarray(q64, np.float64)
    d, scale = np.abs(x - q64), np.abs(q64)
    ok = scale > 0
    e = float((d[ok] / scale[ok]).max()) if ok.any() else 0.0
    return e if (d[~ok] == 0).all() else float("inf")


@pytest.mark.parametrize("S,I", [(64, 128), (129, 895)])
@pytest.mark.parametrize("name", ["split", "row"])
def test_depth_and_sumw_against_float64(name, S, I):
    """min_transmittance = 0, max_segments = 4.  e32: the same restatement on float32 rows.  Split cavity: all 256
    beams, and the operator counts 256 valid beams where score_poses_map counts fewer.  Row of three: sumw on all 96
    beams, depth on those with float64 sumw >= 0.5, which are exactly the 52 that reach the third box."""
    R = 256 if name == "split" else 96
    scene, pose, pts = _scan(name, R)
    r64 = TR.through_render(scene, pose, pts, 0, S, I, 4, 1e-3, 0.0)
    r32 = TR.through_render(scene, pose, pts, 0, S, I, 4, 1e-3, 0.0, dtype=torch.float32)
    m = _map_of(scene)
    rows = G._pose_rows(pose[None], "cuda")
    ids = torch.zeros(1, dtype=torch.int32).cuda()
    s4, depth, sumw, nseg, last = _through(_dev(pts), rows, ids, m, S, I, 4, 1e-3, 0.0, delta=0.0)
    torch.cuda.synchronize()
    depth, sumw = depth.cpu().numpy()[0], sumw.cpu().numpy()[0]
    hit = r64["sumw"] >= 0.5
    if name == "split":
        assert int(hit.sum()) == 256
        clipped = P.score_poses_map(_dev(pts), rows, ids, m[2], m[0], m[1], RR.NEAR, S, I, EPS, 0.0, 0.5, False)[0]
        print("split cavity: valid beams through", float(s4[0, 1]), "clipped", float(clipped[0, 1]))
        assert float(s4[0, 1]) == 256.0 and float(clipped[0, 1]) < 256.0
    else:
        reach = r64["n_segments"] == 3
        assert int(hit.sum()) == 52 and (hit == reach).all() and (r64["last_block"][reach] == 2).all()
        assert float(s4[0, 1]) == 52.0
    t = Tally("score_poses_through")
    case = f"{name} S{S} I{I}"
    e_d, e32_d = _err(depth[hit], r64["depth"][hit]), _err(r32["depth"][hit], r64["depth"][hit])
    e_s, e32_s = _err(sumw, r64["sumw"]), _err(r32["sumw"], r64["sumw"])
    print(case, "depth e_hip", e_d, "e32", e32_d, "sumw e_hip", e_s, "e32", e32_s)
    t.check_err(case, "depth", e_d, e32_d, NOCAP)
    t.check_err(case, "sumw", e_s, e32_s, NOCAP)
    t.done()


# ----------------------------------------------------------------------------------------------- 4. order independence
def _bits4(s):
    return torch.stack([s.cost, s.n_valid.double(), s.abs_residual, s.hit], 1)


def test_bits_do_not_depend_on_the_batch_the_outputs_or_where_the_poses_live():
    scene, pose, pts = _scan("split", 67)
    bm = L.BlockMap(*_map_of(scene))
    pd = _dev(pts)
    poses = torch.stack([G.se3_exp(x) @ pose for x in NEAR_TWISTS] + [pose, G.se3_exp(NEAR_TWISTS[1]) @ pose])
    kw = dict(N_samples=64, N_importance=128, huber_delta=DELTA, near=RR.NEAR, max_segments=4)
    ids = [0, 0, 0, 0, 0]
    full = L.score_poses_through(bm, pd, poses, ids, want_depth=True, **kw)
    again = L.score_poses_through(bm, pd, poses, ids, want_depth=True, **kw)
    bare = L.score_poses_through(bm, pd, poses, ids, **kw)
    on_dev = L.score_poses_through(bm, pd, poses.cuda(), torch.tensor(ids, dtype=torch.int32).cuda(), **kw)
    assigned = L.score_poses_through(bm, pd, poses, None, **kw)   # assign_blocks puts them all into block 0
    torch.cuda.synchronize()
    assert bare.depth is None and bare.sumw is None and bare.n_segments is None and bare.last_block is None
    assert int(full.n_segments.max()) == 2 and int(full.n_segments.min()) == 1
    for other in (again, bare, on_dev, assigned):
        assert same_bits(_bits4(full), _bits4(other))
    for f in ("depth", "sumw", "n_segments", "last_block"):
        assert _same(getattr(full, f), getattr(again, f)), f
    for p in (0, 2, 3):
        one = L.score_poses_through(bm, pd, poses[p:p + 1], ids[p:p + 1], want_depth=True, **kw)
        assert same_bits(_bits4(one)[0], _bits4(full)[p])
        for f in ("depth", "sumw", "n_segments", "last_block"):
            assert _same(getattr(one, f)[0], getattr(full, f)[p]), (p, f)
    # a pose without a block: zero sums, NaN depth, no segment; its neighbours keep their bits
    holes = L.score_poses_through(bm, pd, poses, [0, -1, 0, 9, 0], want_depth=True, **kw)
    for p in (1, 3):
        assert bool((_bits4(holes)[p] == 0).all()) and bool(torch.isnan(holes.depth[p]).all())
        assert bool((holes.sumw[p] == 0).all()) and bool((holes.n_segments[p] == 0).all())
        assert bool((holes.last_block[p] == -1).all())
    for p in (0, 2, 4):
        assert same_bits(_bits4(holes)[p], _bits4(full)[p]) and same_bits(holes.depth[p], full.depth[p])
        assert _same(holes.n_segments[p], full.n_segments[p])


# ----------------------------------------------------------------------------------------------- 5. the filter
def _particles(pose):
    grid = L.pose_grid(G.se3_exp(LR.GRID_OFFSET) @ pose, 0.2, 0.2, np.radians(5.0), np.radians(5.0))
    return torch.cat([pose[None], grid])   # particle 0 is the true pose


def test_particle_filter_through_and_synthesize_scan():
    scene, pose, pts = _scan("split", 256)
    bm = L.BlockMap(*_map_of(scene))
    pd = _dev(pts)
    kw = dict(beta=50.0, near=RR.NEAR)
    pf = M.ParticleFilter(bm, _particles(pose), through=True, **kw)
    clipped = M.ParticleFilter(bm, _particles(pose), **kw)
    assert pf.through and not clipped.through and pf.n_particles == 28
    pf.update(pd)
    clipped.update(pd)
    s4 = P.score_poses_through(pd, pf.poses12, pf.blocks, bm.boxes, bm.folds_c, bm.folds_f, RR.NEAR, 64, 128, EPS, 0.0,
                               0.5, 4, 1e-3, 1e-3, False)[0]
    assert same_bits(pf.scores4, s4)
    s4m = P.score_poses_map(pd, clipped.poses12, clipped.blocks, bm.boxes, bm.folds_c, bm.folds_f, RR.NEAR, 64, 128,
                            EPS, 0.0, 0.5, False)[0]
    assert same_bits(clipped.scores4, s4m)   # the default is the clipped path
    mean = lambda f: float((f.scores4[0, 0] + f.miss_cost * (256 - f.scores4[0, 1])) / 256)   # noqa: E731
    print("mean cost at the true pose: through", mean(pf), "clipped", mean(clipped), "valid",
          float(pf.scores4[0, 1]), float(clipped.scores4[0, 1]))
    assert float(pf.scores4[0, 1]) == 256.0 and mean(pf) < mean(clipped)
    # three steps make no host synchronisation
    gen = torch.Generator(device="cuda").manual_seed(5)
    sums = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            pf.step(pd, (0.0,) * 6, 1e-3, generator=gen)
            sums.append(pf.w.sum())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(abs(float(v) - 1.0) <= 1e-12 for v in sums) and bool(torch.isfinite(pf.scores4).all())
    # the scan the map predicts from the true pose: its ranges are the operator's depths
    dirs = _dev(RR.unit_directions(256, 0).float() * 3.0)   # (any length)
    scan = L.synthesize_scan(bm, dirs, pose, near=RR.NEAR)
    rows = G._pose_rows(pose[None], "cuda")
    ids = torch.zeros(1, dtype=torch.int32).cuda()
    _, depth, sumw, nseg, last = P.score_poses_through(dirs, rows, ids, bm.boxes, bm.folds_c, bm.folds_f, RR.NEAR, 64,
                                                       128, EPS, 0.0, 0.5, 4, 1e-3, 1e-3, True)
    assert same_bits(scan.depth, depth[0]) and same_bits(scan.hit, sumw[0])
    assert _same(scan.n_segments, nseg[0]) and _same(scan.last_block, last[0])
    assert tuple(scan.points_sensor.shape) == (256, 3) and scan.points_sensor.dtype == torch.float32
    rng = torch.linalg.norm(scan.points_sensor.double(), dim=-1)
    assert float(((rng - depth[0].double()).abs() / depth[0].double()).max()) <= 4 * 2.0 ** -24
    assert bool((scan.hit >= 0.5).all()) and int(scan.n_segments.max()) == 2


# ----------------------------------------------------------------------------------------------- 6. operand checks
def test_operand_checks_raise_before_launch():
    scene, pose, pts = _scan("split", 5)
    m = _map_of(scene)
    rows = G._pose_rows(pose[None], "cuda")
    ids = torch.zeros(1, dtype=torch.int32).cuda()
    pd = _dev(pts)
    for K in (0, 17):
        with pytest.raises(RuntimeError, match="max_segments"):
            _through(pd, rows, ids, m, 64, 128, K)
    with pytest.raises(RuntimeError, match="seam_tol"):
        _through(pd, rows, ids, m, 64, 128, 4, tol=-1.0)
    with pytest.raises(RuntimeError, match="min_transmittance"):
        _through(pd, rows, ids, m, 64, 128, 4, tmin=1.0)
    with pytest.raises(RuntimeError, match="at most 1024"):
        _through(pd, rows, ids, m, 512, 513, 4)
    with pytest.raises(RuntimeError, match="block_of_pose"):
        _through(pd, rows, ids.long(), m, 64, 128, 4)
    with pytest.raises(RuntimeError, match="block_of_pose has shape"):
        _through(pd, rows, torch.zeros(2, dtype=torch.int32).cuda(), m, 64, 128, 4)
    with pytest.raises(RuntimeError, match="folds_fine has shape"):
        _through(pd, rows, ids, (m[0], m[1][:1].contiguous(), m[2]), 64, 128, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _through(pd, rows, ids.cpu(), m, 64, 128, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.score_poses_through(L.BlockMap(*m), pts, pose[None])
    bm = L.BlockMap(*m)
    with pytest.raises(RuntimeError, match="max_segments"):
        L.score_poses_through(bm, pd, pose[None], max_segments=0)
    with pytest.raises(RuntimeError, match="max_segments"):
        M.ParticleFilter(bm, pose[None], through=True, max_segments=17)
    # empty inputs give empty or zero outputs
    s = L.score_poses_through(bm, pd, torch.empty(0, 4, 4, dtype=torch.float64), [], want_depth=True)
    assert tuple(s.cost.shape) == (0,) and tuple(s.n_segments.shape) == (0, 5)
    torch.cuda.synchronize()
