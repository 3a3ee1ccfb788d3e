"""tests/render_f64.py against the oracle (which reference-generated goldens pin), and the conditions the per-kernel
GPU tests' inputs (tests/render_inputs.py) must meet -- all on the CPU."""
import numpy as np
import pytest
import torch

from nof import synthetic as syn
from oracle import ref_cpu as O

import render_f64 as F
import render_inputs as I

RTOL = 1e-6   # the same float32 ops in another grouping (per-ray sums first)


def _rows(R, S, seed):
    gen = torch.Generator().manual_seed(seed)
    rays = torch.from_numpy(syn.make_rays(R, seed=seed))
    z = torch.sort(rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * torch.rand(R, S, generator=gen), -1)[0]
    return gen, rays, z, torch.rand(R, S, generator=gen) ** 4


@pytest.mark.parametrize("divide", [False, True])
@pytest.mark.parametrize("R,S,noisy", [(33, 96, False), (64, 192, True)])
def test_float32_restatement_matches_oracle_train(R, S, noisy, divide):
    gen, rays, z, p = _rows(R, S, 11 + S)
    noise = 1e-3 * torch.randn(R, S, generator=gen) if noisy else None
    w, depth = O.composite(p, z, 1e-10, noise)
    free, dl = O.child_losses(w, z, rays, rays[:, 10:12], rays[:, 14], divide, 32)
    m0, m2, _ = F.masks(z, rays[:, 10], rays[:, 11])
    got = F.composite_losses(p, z, noise, 1e-10, (m0, m2), rays[:, 14], rays[:, 9], divide, 32, torch.float32)
    np.testing.assert_allclose(got["w"].numpy(), w.numpy(), rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(got["depth"].numpy(), depth.numpy(), rtol=RTOL)
    np.testing.assert_allclose(float(got["free"]), float(free), rtol=RTOL)
    np.testing.assert_allclose(float(got["depth_loss"]), float(dl), rtol=RTOL)
    assert float(free) > 0 and float(dl) > 0
    opac = torch.mean(torch.log(0.1 + p) + torch.log(0.1 + (1 - p)) + 2.20727)       # render.py:224
    np.testing.assert_allclose(float(got["opac_row"].sum() / (R * S)), float(opac), rtol=RTOL)


@pytest.mark.parametrize("method", [0, 2])
def test_float32_restatement_matches_oracle_view(method):
    rows, other, _ = syn.make_view_rows(24, seed=5)
    rows, other = torch.from_numpy(rows), torch.from_numpy(other)
    R, S = rows.shape[0], 160
    gen = torch.Generator().manual_seed(3)
    z = torch.sort(rows[:, 9:10] + (rows[:, 10:11] - rows[:, 9:10]) * torch.rand(R, S, generator=gen), -1)[0]
    p = torch.rand(R, S, generator=gen) ** 4
    depth, w, opac, _ = O.inference_view(p, z, other, rows[:, 6:8], method)
    mv = F.masks(z, rows[:, 6], rows[:, 7])[2]
    got = F.view_rows(p, z, mv, method, 1e-10, torch.float32)
    np.testing.assert_allclose(got["w"].numpy(), w.numpy(), rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(got["depth"].numpy(), depth.numpy(), rtol=RTOL)
    np.testing.assert_allclose(float(got["opac_row"].sum() / (R * S)), float(opac), rtol=RTOL)
    np.testing.assert_allclose(got["child_sum"].numpy(), torch.sum(w * mv.float(), -1).numpy(), rtol=RTOL)


def test_gradient_restatement_is_the_derivative():
    """g_logit is autograd of the restatement; check it against central differences of the float64 loss in the
    logits (one plain, one divide case), so a slip in how the terms are put together cannot hide."""
    c = I.composite_case(65)
    for branch in ("plain", "divide"):
        br = c[branch]
        gd, gf, gl = I.upstream(c, branch, True, True, True)

        def loss(logit):
            o = F.composite_losses(torch.sigmoid(logit), c["z"], br["noise"], I.EPS, c["masks"], br["rays"][:, 14],
                                   br["rays"][:, 9], br["divide"], I.N_CHILD, torch.float64)
            return float(torch.sum(gd.double() * o["depth"]) + gf.double() * o["free"] + gl.double() * o["depth_loss"])
        p64 = c["p"].double().clamp(1e-12, 1 - 1e-12)
        logit = torch.log(p64) - torch.log1p(-p64)
        g = F.g_logit(torch.sigmoid(logit), c["z"], br["noise"], I.EPS, c["masks"], br["rays"][:, 14],
                      br["rays"][:, 9], br["divide"], I.N_CHILD, torch.float64, gd, gf, gl)
        for r, j in ((0, 3), (1, 40), (4, 2), (6, 64)):
            h = 1e-5
            lp, lm = logit.clone(), logit.clone()
            lp[r, j] += h
            lm[r, j] -= h
            fd = (loss(lp) - loss(lm)) / (2 * h)
            assert abs(fd - float(g[r, j])) <= 1e-6 * float(g[r].abs().max()) + 1e-12, (branch, r, j, fd, float(g[r, j]))


@pytest.mark.parametrize("S", I.FB_S + I.FWD_ONLY_S)
def test_composite_inputs_meet_their_conditions(S):
    """Conditions on the GPU tests' inputs, checked on the references alone: no ray's 10 dc - 10 range is near the
    SmoothL1 kink at 1 (all are +-0.5 or +-3), both regimes occur when there are >= 3 rays, and the float32
    restatement stays within 2e-5 of the float64 one (I.E32_CAP; for the quantities that are functions of the
    cancelling difference 10 dc - 10 range alone the cap is on dc, carried through that cancellation:
    I.e32_cap)."""
    c = I.composite_case(S)
    for branch in ("plain", "divide"):
        br = c[branch]
        x = (10 * br["f64"]["dc"] - 10 * br["rays"][:, 14].double()).abs()
        assert bool(((x - 0.5).abs() < 1e-3).logical_or((x - 3).abs() < 1e-3).all()), x
        if c["R"] >= 3:
            assert bool((x < 1).any()) and bool((x > 1).any())
        for k in ("w", "depth", "free_ray", "sl1_ray", "opac_row", "free", "depth_loss"):
            e32 = F.err(br["f32"][k], br["f64"][k])
            assert e32 <= I.e32_cap(br, k), (branch, k, e32, I.e32_cap(br, k))
    if c["R"] >= 5:   # the edge rows are what they claim to be
        m0, m2 = c["masks"]
        k = min(S // 3, 3)
        assert bool(m0[4, k]) and int(m0[4].sum()) == 1 and float(c["plain"]["f64"]["w"][4, k]) > 1e-3
        assert int(m0[2].sum()) >= 1 and int(m0[3].sum()) >= 1
    if S > 1:
        # the rows reach the end: in some row the weights in the last thread's samples and on either side of each wave
        # boundary are >= 1e-3 of the row's maximum, 1000 x the tolerance -- a kernel that dropped a cross-lane or
        # cross-wave term, or wrote zeros there, cannot pass.  (One ray: its saturated last sample holds 30 % of the
        # weight and the others ~1 / S each, so 1e-4 there; every instantiation also has a case with >= 5 rays)
        for branch in ("plain", "divide"):
            reach = I.lane_reach(S, c[branch]["f64"]["w"])
            assert min(reach.values()) >= (1e-4 if c["R"] == 1 else 1e-3), (branch, reach)
    if S in I.FB_S and S > 1:
        for name, branch, has_d, has_f, *_ in I.BWD_COMBOS:
            gd, gf, gl, g64, g32 = I.backward_refs(S)[name]
            # and so does dL/dlogit: >= 1e-3 of the row's maximum at each of those places where both the depth and
            # the free-loss gradient are given.  Without the first the child losses' in-mask entries tower over the
            # rest of a row, without the second a one-ray row ends on dL/ddepth ~ z[S-2] - z[S-1]: there the places
            # still hold 100 x the tolerance's floor
            reach = I.lane_reach(S, g64, last_is_zero=c["R"] == 1)
            assert min(reach.values()) >= (1e-3 if has_d and has_f else 2.4e-5), (name, reach)
            cap = I.E32_CAP if has_d else I.e32_cap(c[branch], "sl1_ray")
            assert F.err(g32, g64) <= cap, (name, F.err(g32, g64), cap)
            if has_d and gl is not None:
                # float32's rounding of 10 dc - 10 range cannot move this gradient by more than an ulp, and the
                # depth-loss term is still far above the tolerance in the rows it acts on most
                assert I.x_noise(c, branch, g64, gl) <= I.ULP32 and abs(float(gl)) >= 0.25 / 2 ** 12, (name, float(gl))


@pytest.mark.parametrize("S", I.VIEW_S)
def test_view_inputs_meet_their_conditions(S):
    """The two-step rows: the float32 restatement within 2e-5 of float64, the sample on the first strict bound left
    out of the mask, the gap row's mask non-empty only after expansion, and no row's smoothed peak unclear."""
    c = I.view_case(S)
    for method in (0, 2):
        for k in ("w", "depth", "child_sum", "opac_row"):
            assert F.err(c[method]["f32"][k], c[method]["f64"][k]) <= 2e-5, (method, k)
    lo1 = c["rows"][1, 6] - torch.tensor(0.01)
    assert float(c["z"][1, c["k1"]]) == float(lo1)
    if S >= 2:   # a sample lies inside the child interval, the loop stops at thr 0.01: the bound itself is outside
        assert not bool(c["mv"][1, c["k1"]]) and int(c["mv"][1].sum()) >= 1
    assert not bool(((c["z"][3] > c["rows"][3, 6] - 0.4) & (c["z"][3] < c["rows"][3, 7] + 0.4)).any())
    at, unclear = I.peak_reference(c[0]["f32"]["w"], c["mv"])
    assert not bool(unclear.any())
    if S >= 64:   # (shorter rows: the reflected ends can move the smoothed peak off the dominant sample)
        peak = torch.argmax(O.gaussian_smooth(c[0]["f32"]["w"]), dim=1)
        assert peak.tolist() == torch.argmax(c["p"], dim=1).tolist()      # one dominant sample per row


def test_strict_bound_case_bites_somewhere():
    """Row 1's sample on the bound is the dominant one, so an inclusive mask would flip at_peak and child_sum at
    every size from 2 on; and at_peak is True for row 0 (its peak is inside the child interval) at many sizes."""
    for S in I.VIEW_S[1:]:
        c = I.view_case(S)
        assert int(torch.argmax(c["p"][1])) == c["k1"] and not bool(c["mv"][1, c["k1"]]), S
    hit = sum(int(I.peak_reference(I.view_case(S)[0]["f32"]["w"], I.view_case(S)["mv"])[0][0]) for S in I.VIEW_S)
    assert hit >= 5, hit
