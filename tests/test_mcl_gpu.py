"""pcnerf::mcl_weights, pcnerf::systematic_resample and nof.mcl.ParticleFilter on the MI355X against the numpy float64
restatement of tests/map_ref.py.

Decisions are compared for equality (the -inf pattern, best, degenerate, the ancestors of exactly representable
weights, the gather).  Sums are compared within 1e-12 relative: (P + 4) 2^-53 < 1e-12 for P <= 4,099, one rounding
per added term plus the exp; a subnormal value carries the absolute error of a few subnormal ulps instead (TINY)."""
import math

import numpy as np
import pytest
import torch

import map_ref as MR
import registration_ref as RR
from sampling_f64 import same_bits
from nof import localization as L
from nof import mcl as M
from nof import registration as G

pytestmark = pytest.mark.gpu
P = torch.ops.pcnerf
SIZES = (1, 3, 64, 65, 1025, 4099)
REL = 1e-12
TINY = 8 * 2.0 ** -1074   # subnormal results have no relative precision: a few of their own ulps


def _f64(a):
    return torch.as_tensor(np.asarray(a, np.float64)).cuda().contiguous()


def _i32(a):
    return torch.as_tensor(np.asarray(a, np.int32)).cuda().contiguous()


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    inf = np.isinf(want)
    if not np.array_equal(inf, np.isinf(got)) or not np.array_equal(got[inf], want[inf]):
        return False
    return bool(np.all(np.abs(got[~inf] - want[~inf]) <= REL * np.abs(want[~inf]) + TINY))


# ----------------------------------------------------------------------------------------------- mcl_weights
def _weights_case(n, seed, beta):
    """Mean costs 0 .. 700 beta apart (exp underflows for some particles), some particles without a block, one NaN
    cost, log-weights of a previous step."""
    rng = np.random.default_rng(seed)
    n_usable, miss = 16.0, 3.0
    s4 = np.zeros((n, 4))
    s4[:, 1] = rng.integers(0, 17, size=n)
    mean = rng.permutation(np.linspace(0.0, 700.0 * beta, n)) if n > 1 else np.array([1.5])
    s4[:, 0] = mean * n_usable - miss * (n_usable - s4[:, 1])
    blocks = rng.integers(0, 4, size=n).astype(np.int32)
    if n >= 3:
        blocks[rng.integers(0, n, size=max(1, n // 7))] = -1
        s4[n // 2, 0] = np.nan
    logw_prev = -rng.random(n)
    return logw_prev, s4, blocks, n_usable, miss


@pytest.mark.parametrize("n", SIZES)
def test_mcl_weights_against_the_restatement(n):
    beta = 2.0
    logw_prev, s4, blocks, n_usable, miss = _weights_case(n, n, beta)
    want = MR.mcl_weights(logw_prev, s4, blocks, n_usable, miss, beta)
    args = (_f64(logw_prev), _f64(s4), _i32(blocks), _f64([n_usable]), miss, beta)
    w, logw, ess, best, deg = P.mcl_weights(*args)
    again = P.mcl_weights(*args)
    assert all(same_bits(a, b) if a.is_floating_point() else torch.equal(a, b)
               for a, b in zip((w, logw, ess, best, deg), again))
    w, logw = w.cpu().numpy(), logw.cpu().numpy()
    line = {"n": n, "ess": float(ess), "want_ess": want["ess"], "best": int(best), "sum_w": float(w.sum()),
            "zeros": int((w == 0).sum()), "neg_inf": int(np.isneginf(logw).sum())}
    print(line)
    assert int(best) == want["best"] and int(deg) == want["degenerate"] == 0, line
    assert np.array_equal(np.isneginf(logw), np.isneginf(want["logw"])), line
    assert np.array_equal(np.isneginf(logw), (blocks < 0) | np.isnan(s4[:, 0])), line
    assert _close(w, want["w"]) and _close(logw, want["logw"]) and _close([float(ess)], [want["ess"]]), line
    assert abs(float(w.sum()) - 1.0) <= REL and (w[np.isneginf(logw)] == 0).all(), line
    if n >= 64:
        assert (w[~np.isneginf(logw)] == 0).any(), line   # exp underflowed for some particle with a block


@pytest.mark.parametrize("n", SIZES)
def test_mcl_weights_without_a_finite_weight_is_uniform(n):
    logw_prev, s4, blocks, n_usable, miss = _weights_case(n, 100 + n, 1.0)
    blocks[:] = -1
    w, logw, ess, best, deg = P.mcl_weights(_f64(logw_prev), _f64(s4), _i32(blocks), _f64([n_usable]), miss, 1.0)
    assert int(deg) == 1 and int(best) == 0 and float(ess) == float(n)
    assert bool((w == 1.0 / n).all()) and bool((logw == 0).all())
    # a NaN previous weight and an n_usable of zero carry no weight either
    lp = np.zeros(n)
    lp[0] = np.nan
    out = P.mcl_weights(_f64(lp), _f64(np.zeros((n, 4))), _i32(np.zeros(n)), _f64([16.0]), miss, 1.0)
    assert bool(torch.isneginf(out[1][0])) if n > 1 else int(out[4]) == 1
    out = P.mcl_weights(_f64(np.zeros(n)), _f64(np.zeros((n, 4))), _i32(np.zeros(n)), _f64([0.0]), miss, 1.0)
    assert int(out[4]) == 1


# ----------------------------------------------------------------------------------------------- resampling
def _resample(w, u0, n_out, ess=None, thr=0.0, poses=None, blocks=None, logw=None):
    return P.systematic_resample(_f64(w), _f64([u0]), int(n_out), None if ess is None else _f64([ess]), float(thr),
                                 poses, blocks, logw)


@pytest.mark.parametrize("n", SIZES)
def test_systematic_resample_exact_weights(n):
    """Weights that are integer multiples of 2^-20: every prefix sum is exact in any order, so the ancestors equal the
    restatement's exactly; no zero-weight ancestor appears."""
    w = MR.exact_weights(n, n)
    for u0 in (0.0, 0.5, 1.0 - 2.0 ** -20):
        for n_out in sorted({n, 1, 2 * n + 1}):
            want, _ = MR.systematic_resample(w, u0, n_out)
            anc = _resample(w, u0, n_out)[0]
            assert anc.dtype == torch.int32 and tuple(anc.shape) == (n_out,)
            got = anc.cpu().numpy()
            assert np.array_equal(got, want), (n, u0, n_out, np.nonzero(got != want)[0][:5])
            assert (w[got] > 0).all() and MR.count_property(got, w, n_out)
            assert torch.equal(_resample(w, u0, n_out)[0], anc)


@pytest.mark.parametrize("seed", MR.RESAMPLE_SEEDS)
@pytest.mark.parametrize("n", SIZES)
def test_systematic_resample_random_weights(n, seed):
    w = MR.random_weights(n, seed)
    c = np.cumsum(w)
    for n_out in sorted({n, 2 * n + 1}):
        want, _ = MR.systematic_resample(w, 0.37, n_out)
        got = _resample(w, 0.37, n_out)[0].cpu().numpy()
        excepted = MR.near_an_edge(c, MR.draws(c[-1], 0.37, n_out))
        line = {"n": n, "seed": seed, "n_out": n_out, "excepted": int(excepted.sum()),
                "differ": int((got != want).sum())}
        print(line)
        assert (np.diff(got) >= 0).all() and got.min() >= 0 and got.max() < n, line
        assert excepted.sum() <= MR.EDGE_CAP * n_out, line
        assert np.array_equal(got[~excepted], want[~excepted]), line
        assert MR.count_property(got, w, n_out), line


def test_bad_and_zero_weights_are_never_ancestors():
    w = MR.random_weights(2500, 5)
    zeros = [3, 4, 8, 1023, 1024, 1025, 2047, 2048, 2499]
    w[zeros] = 0.0
    w[7], w[100], w[2000] = np.nan, -1.0, np.inf
    got = _resample(w, 0.25, 5001)[0].cpu().numpy()
    assert (MR.clamp_weights(w)[got] > 0).all() and (np.diff(got) >= 0).all() and got.max() <= 2498
    want, _ = MR.systematic_resample(w, 0.25, 5001)
    c = np.cumsum(MR.clamp_weights(w))
    excepted = MR.near_an_edge(c, MR.draws(c[-1], 0.25, 5001))
    assert np.array_equal(got[~excepted], want[~excepted]) and excepted.sum() <= 50
    # a u0 outside [0, 1) counts as 0; all-zero weights give ancestor 0
    assert torch.equal(_resample(w, 1.5, 64)[0], _resample(w, 0.0, 64)[0])
    assert _resample(np.zeros(5), 0.5, 7)[0].tolist() == [0] * 7


@pytest.mark.parametrize("n", [1, 65, 4099])
def test_the_ess_switch_and_the_gather(n):
    """(c) ess >= the threshold: the identity and the log-weights kept, decided on the device from the (1,) ess tensor;
    below: a redraw and zero log-weights.  (d) the gathered poses and block ids are poses[ancestors] bit for bit."""
    rng = np.random.default_rng(n)
    w = MR.random_weights(n, 7)
    ess = 1.0 / float((w * w).sum())
    poses = _f64(rng.standard_normal((n, 12)))
    blocks = _i32(rng.integers(-1, 5, size=n))
    logw = _f64(np.log(w))
    keep = _resample(w, 0.5, n, ess=ess, thr=ess, poses=poses, blocks=blocks, logw=logw)
    assert keep[0].tolist() == list(range(n))
    assert same_bits(keep[1], poses) and torch.equal(keep[2], blocks) and same_bits(keep[3], logw)
    for redo in (_resample(w, 0.5, n, ess=ess, thr=ess * (1 + 1e-9) + 1e-9, poses=poses, blocks=blocks, logw=logw),
                 _resample(w, 0.5, n, poses=poses, blocks=blocks, logw=logw)):
        anc = redo[0].long()
        want, _ = MR.systematic_resample(w, 0.5, n)
        excepted = MR.near_an_edge(np.cumsum(w), MR.draws(np.cumsum(w)[-1], 0.5, n))
        assert np.array_equal(anc.cpu().numpy()[~excepted], want[~excepted])
        assert same_bits(redo[1], poses[anc]) and torch.equal(redo[2], blocks[anc])
        assert bool((redo[3] == 0).all()) and tuple(redo[3].shape) == (n,)
    # more draws than particles, only some of the inputs
    more = _resample(w, 0.5, 2 * n + 1, poses=poses)
    assert same_bits(more[1], poses[more[0].long()]) and tuple(more[2].shape) == tuple(more[3].shape) == (0,)


def test_filter_operators_reject_bad_operands():
    n = 5
    w, u0, ess = _f64(np.full(n, 0.2)), _f64([0.5]), _f64([5.0])
    poses, blocks, logw = _f64(np.zeros((n, 12))), _i32(np.zeros(n)), _f64(np.zeros(n))
    P.systematic_resample(w, u0, n, ess, 2.5, poses, blocks, logw)
    bad = [(w.cpu(), u0, n, ess, 2.5, poses, blocks, logw), (w, u0.cpu(), n, ess, 2.5, poses, blocks, logw),
           (w.float(), u0, n, ess, 2.5, poses, blocks, logw), (w, u0, n, ess, 2.5, poses, blocks.long(), logw),
           (w, u0, n + 1, ess, 2.5, None, None, None),            # n_out != P with the ESS switch on
           (w, u0, 2 * n + 1, ess, 2.5, poses, blocks, logw),
           (w, u0, 0, None, 0.0, None, None, None), (w, u0, n, None, 0.0, poses[:4], None, None),
           (w, u0, n, None, 0.0, None, blocks[:4], None), (w, u0, n, None, 0.0, None, None, logw[:4]),
           (w, _f64([0.5, 0.5]), n, None, 0.0, None, None, None), (w[:0], u0, n, None, 0.0, None, None, None),
           (w, u0, n, ess.cpu(), 2.5, None, None, None)]
    for args in bad:
        with pytest.raises(RuntimeError):
            P.systematic_resample(*args)
    from nof import _torch_ops as T
    big = torch.zeros(T.MCL_MAX_PARTICLES + 1, dtype=torch.float64, device="cuda")   # the serial chains' limit
    with pytest.raises(RuntimeError, match="at most"):
        P.systematic_resample(big, u0, 4, None, 0.0, None, None, None)
    s4, nu = _f64(np.zeros((n, 4))), _f64([16.0])
    P.mcl_weights(logw, s4, blocks, nu, 3.0, 1.0)
    bad = [(logw.cpu(), s4, blocks, nu, 3.0, 1.0), (logw, s4.cpu(), blocks, nu, 3.0, 1.0),
           (logw, s4, blocks.cpu(), nu, 3.0, 1.0), (logw, s4, blocks, nu.cpu(), 3.0, 1.0),
           (logw.float(), s4, blocks, nu, 3.0, 1.0), (logw, s4, blocks.long(), nu, 3.0, 1.0),
           (logw, s4[:4], blocks, nu, 3.0, 1.0), (logw, s4, blocks[:4], nu, 3.0, 1.0),
           (logw, s4[:, :3].contiguous(), blocks, nu, 3.0, 1.0), (logw, s4, blocks, _f64([16.0, 1.0]), 3.0, 1.0),
           (logw[:0], s4[:0], blocks[:0], nu, 3.0, 1.0)]
    for args in bad:
        with pytest.raises(RuntimeError):
            P.mcl_weights(*args)


# ----------------------------------------------------------------------------------------------- the filter
def _filter(**kw):
    s = MR.two_block_scene()
    f = s["folds"].cuda()
    bm = L.BlockMap(f, f, torch.as_tensor(s["boxes"]).cuda())
    return s, bm, M.ParticleFilter(bm, s["poses"], near=RR.NEAR, **kw)


def test_particle_filter_converges_into_block_1_without_a_host_synchronisation():
    """The two-block scene, 250 particles at the hypotheses of both blocks, the scan of block 1's truth pose: three
    steps with zero twist, a small sigma and a fixed generator make no host synchronisation (torch's sync debug mode
    raises on one); after each the weights sum to 1, after the third more than half of the weight lies in block 1 and
    the best particle is there."""
    s, bm, pf = _filter(beta=200.0)
    pts = s["points"].cuda()
    assert pf.blocks.tolist() == [0] * 125 + [1] * 125 and pf.n_particles == 250
    gen = torch.Generator(device="cuda").manual_seed(0)
    sums, in_block_1, ess = [], [], []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            pf.step(pts, (0.0,) * 6, 1e-3, generator=gen)
            sums.append(pf.w.sum())
            in_block_1.append((pf.w * (pf.blocks == 1)).sum())
            ess.append(pf.ess.clone())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    sums, in_block_1 = [float(v) for v in sums], [float(v) for v in in_block_1]
    print({"sum_w": sums, "weight_in_block_1": in_block_1, "ess": [float(e) for e in ess]})
    assert all(abs(v - 1.0) <= REL for v in sums)
    assert in_block_1[-1] > 0.5
    est = pf.estimate()
    assert int(est.best_block) == 1 and int(pf.blocks[int(est.best_index)]) == 1
    assert tuple(est.pose.shape) == tuple(est.best_pose.shape) == (4, 4) and est.pose.is_cuda
    R = est.pose[:3, :3]
    assert float((R @ R.T - torch.eye(3, dtype=torch.float64, device=R.device)).abs().max()) <= 1e-12
    assert abs(float(torch.linalg.det(R)) - 1.0) <= 1e-12
    et, er = RR.pose_error(est.best_pose.cpu(), s["T1"])
    print({"best_err_t": et, "best_err_r": er})
    assert et <= 0.7 and er <= math.radians(15.0)   # (the grid around block 1's truth: 0.4 sqrt 2 + the offset; 10 degrees)


def test_particle_filter_pieces():
    """update and resample on their own: the weights are mcl_weights' of score_poses_map's rows, a forced redraw
    gathers the particles, a high threshold keeps them."""
    s, bm, pf = _filter(beta=50.0)
    pts = s["points"].cuda()
    before = pf.poses12.clone()
    pf.update(pts)
    sc = L.score_poses_map(bm, pts, s["poses"], near=RR.NEAR)
    assert same_bits(pf.scores4[:, 0].contiguous(), sc.cost)
    want = MR.mcl_weights(np.zeros(250), pf.scores4.cpu().numpy(), pf.blocks.cpu().numpy(), 256.0, pf.miss_cost, 50.0)
    assert int(pf.best) == want["best"] and abs(float(pf.ess) - want["ess"]) <= REL * want["ess"]
    assert pf.miss_cost == bm.default_miss_cost(0.0)
    w = pf.w.clone()
    pf.resample(ess_frac=0.0, u0=0.25)                      # ess >= 0: nothing moves
    assert same_bits(pf.poses12, before) and pf.ancestors.tolist() == list(range(250))
    assert float((pf.w - w).abs().max()) <= 1e-14
    pf.resample(ess_frac=1.0 + 1e-9, u0=0.25)               # ess < P (1 + 1e-9): a redraw
    anc, _ = MR.systematic_resample(w.cpu().numpy(), 0.25, 250)
    excepted = MR.near_an_edge(np.cumsum(w.cpu().numpy()), MR.draws(float(np.cumsum(w.cpu().numpy())[-1]), 0.25, 250))
    got = pf.ancestors.cpu().numpy()
    assert np.array_equal(got[~excepted], anc[~excepted])
    assert same_bits(pf.poses12, before[pf.ancestors.long()]) and bool((pf.logw == 0).all())
    assert bool((pf.w == 1.0 / 250).all())
    # predict with zero noise and a twist moves every particle by se3_exp(twist)
    pf.predict((0.1, 0, 0, 0, 0, 0.05), 0.0)
    moved = G.apply_twists(G._rows_to_poses(before[pf.ancestors.long()]),
                           torch.tensor([[0.1, 0, 0, 0, 0, 0.05]], dtype=torch.float64).cuda().repeat(250, 1))
    assert same_bits(pf.poses, moved)
    assert torch.equal(pf.blocks, L.assign_blocks(bm, pf.poses))
