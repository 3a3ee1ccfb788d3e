"""k_composite, k_composite_bwd, the child-loss reduce kernels and k_view_rows, each against a float64 restatement
of the same operation (tests/render_f64.py), at the sample counts where their templates, lanes and block shapes
change (tests/render_inputs.py: inputs and references, computed once per case and shared).

Tolerance, per quantity q and case: e(x) = max |x - q64| / scale, scale the per-ray maximum of |q64| (|q64| itself
for scalars and one-per-ray values); e32 is e of the same restatement run in float32 on the CPU.  The kernel must
keep e_hip <= max(4 e32, 2.4e-7): its sums are float64 rounded once where torch's are float32, so its error is
another draw of the same size, not the same number; 2.4e-7 is two float32 ulps for the final rounding.  A
structural error (a dropped term, an off-by-one lane, a wrong mask operator) shows at 1e-3 or more.  The inputs
keep e32 itself <= 2e-5 (render_inputs.e32_cap; checked here and, without a GPU, in test_render_f64_cpu.py).
Every e_hip / e32 pair goes to the parity report (gradcheck._report).
"""
import numpy as np
import pytest
import torch

from nof import _hip as H
from nof import _ops

import render_f64 as F
import render_inputs as I
from parity_helpers import FLOOR, Tally

pytestmark = pytest.mark.gpu
DEV = "cuda"

@pytest.fixture
def group(request):
    prev = _ops.set_composite_group(0)
    try:
        _ops.set_composite_group(request.param)
        yield request.param
    finally:
        _ops.set_composite_group(prev)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _composite(p, z, noise, rays):
    """pcnerf_composite with every output at once (weights, depth, free_ray, sl1_ray, per-ray opacity sums, depth2);
    noise_std is 1 when noise is given."""
    R, S = z.shape
    new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=DEV)
    w, depth, opac, depth2 = new((R, S)), new((R,)), new((R,), torch.float64), new((R,))
    fr = sl = None
    if rays is not None:
        fr, sl = new((R,)), new((R,))
    H.check(H.lib().pcnerf_composite(p.data_ptr(), z.data_ptr(), R, S, H.ptr(noise), 1.0 if noise is not None else 0.0,
                                     I.EPS, H.ptr(rays), rays.shape[1] if rays is not None else 0, 10, 11, 14,
                                     w.data_ptr(), depth.data_ptr(), H.ptr(fr), H.ptr(sl), opac.data_ptr(),
                                     depth2.data_ptr(), H.stream_of(z)))
    return {"w": w, "depth": depth, "free_ray": fr, "sl1_ray": sl, "opac_row": opac, "depth2": depth2}


def _forward(t, case, tag):
    """Both branches of one case through k_composite and the child-loss reduce; -> {branch: outputs on the CPU}."""
    z, p = _dev(case["z"]), _dev(case["p"])
    S = case["S"]
    res = {}
    for branch in ("plain", "divide"):
        br = case[branch]
        rays = _dev(br["rays"])
        out = _composite(p, z, _dev(br["noise"]), rays)
        # the scalar losses: the reduce kernels on the float32 restatement's per-ray terms, so that what is compared
        # is the reduction alone (k_composite's own free_ray / sl1_ray are checked per ray above; fed with those,
        # the scalar would carry their admitted deviations -- for sl1_ray up to 4 e32 of a value that cancels
        # ~400:1 -- against the one float32 draw that e32 of a scalar is)
        free, dl = _ops.child_losses(_dev(br["f32"]["free_ray"]), _dev(br["f32"]["sl1_ray"]), rays, br["divide"],
                                     I.N_CHILD)
        assert free.shape == dl.shape == ((1,) if br["divide"] else ())
        out["free"], out["depth_loss"] = free.reshape(()), dl.reshape(())
        # and the chain as a whole: the reduce kernels on k_composite's own per-ray terms, against the float64 /
        # float32 reduce of those same terms
        kf, kd = _ops.child_losses(out["free_ray"], out["sl1_ray"], rays, br["divide"], I.N_CHILD)
        out = {k: v.cpu() for k, v in out.items()}
        q32, q64 = (F.child_reduce(out["free_ray"].to(dt), out["sl1_ray"].to(dt), br["rays"][:, 9], br["divide"],
                                   I.N_CHILD) for dt in (torch.float32, torch.float64))
        for i, (k, x) in enumerate((("free", kf), ("depth_loss", kd))):
            t.check(f"{tag}:{branch}", k + " of the kernel's terms", x.cpu().reshape(()), q32[i], q64[i])
        for k in ("w", "depth", "free_ray", "sl1_ray", "opac_row", "free", "depth_loss"):
            t.check(f"{tag}:{branch}", k, out[k], br["f32"][k], br["f64"][k], I.e32_cap(br, k))
        # the project's existing bound on the forward (test_composite_workgroup_per_ray)
        np.testing.assert_allclose(out["w"].numpy(), br["f32"]["w"].numpy(), rtol=1e-5, atol=1e-7, err_msg=tag)
        np.testing.assert_allclose(out["depth"].numpy(), br["f32"]["depth"].numpy(), rtol=1e-5, atol=1e-6, err_msg=tag)
        # depth2 (render.py:598-600): z at the position of sample S-1 in the stable descending argsort of the
        # kernel's own weights, bit for bit (the rule of test_depth2_tie_order)
        order = torch.argsort(out["w"], dim=-1, descending=True, stable=True)
        pos = (order == S - 1).nonzero()[:, 1]
        assert torch.equal(out["depth2"], case["z"][torch.arange(case["R"]), pos]), (tag, branch, "depth2")
        res[branch] = out
    return res


def _backward(t, case, refs, tag):
    z, p = _dev(case["z"]), _dev(case["p"])
    for name, branch, has_d, has_f, has_l, has_r in I.BWD_COMBOS:
        if name not in refs:
            continue
        br = case[branch]
        gd, gf, gl, g64, g32 = refs[name]
        g = _ops.composite_backward(p, z, _dev(br["noise"]), 1.0 if br["noise"] is not None else 0.0, I.EPS,
                                    _dev(br["rays"]) if has_r else None, I.N_CHILD if br["divide"] else 0,
                                    _dev(gd), _dev(gf), _dev(gl)).cpu()
        if case["S"] == 1:
            # one sample: w = w~ / (w~ + eps), every derivative carries eps / (w~ + eps) ~ 1e-9 -- zero up to eps.
            # No relative error of a 1e-9-sized value: the gradient is within 1e-6 of the upstream gradient's reach
            reach = (gd.abs()[:, None] if has_d else sum(x.abs() for x in (gf, gl) if x is not None)) * case["z"].abs()
            assert bool((g.abs() <= 1e-6 * reach).all()) and bool((g64.abs() <= 1e-6 * reach).all()), (tag, name)
            continue
        t.check(tag, "g_logit:" + name, g, g32, g64, I.E32_CAP if has_d else I.e32_cap(br, "sl1_ray"))


@pytest.mark.parametrize("group", [64, 256], indirect=True)
@pytest.mark.parametrize("S", I.FB_S + I.FWD_ONLY_S)
def test_composite_forward_vs_f64(S, group):
    """weights, depth, free_ray, sl1_ray, the per-ray opacity sums, the two scalar child losses (plain and divide,
    the divide branch with noise) and depth2, for every k_composite<MAXB, G> instantiation on both sides of each
    boundary, with ragged and empty last lanes, 1 / 3 / 5 / 7 rays and the edge rows of render_inputs.edge_rows.
    The scalar losses come from the reduce kernels fed with the float32 restatement's per-ray terms, and once more
    from k_composite's own terms against the reduce of those (see _forward).  With logf in the opacity terms (before
    k_composite took the float64 log rounded once, as k_view_rows) opac_row missed at 28 of the 40 cases: S 4096
    e_hip 3.0e-5, e32 5.4e-6.
    Measured on the MI355X: worst e_hip / max(4 e32, 2.4e-7) 0.52 (S 4095, wave per ray, free_ray: e_hip 1.9e-7,
    e32 9.1e-8); worst e_hip / e32 among errors above the floor 1.46 (S 63, sl1_ray)."""
    t = Tally("composite_forward")
    _forward(t, I.composite_case(S), f"S{S}g{group}")
    t.done()


@pytest.mark.parametrize("group", [64, 256], indirect=True)
@pytest.mark.parametrize("S", I.FB_S)
def test_composite_backward_vs_f64(S, group):
    """dL/dlogit per element against float64 autograd of the restatement: plain and divide, with and without the
    depth gradient, the free / depth-loss gradient each absent once, and rays=None (depth only).  Upstream
    gradients: render_inputs.upstream.  The faint rows of render_inputs.faint_rows keep every lane and wave boundary
    in play (checked on the CPU: render_inputs.lane_reach).  Measured on the MI355X: worst e_hip /
    max(4 e32, 2.4e-7) 0.62 (S 1025, wave per ray, divide without depth gradient: e_hip 4.7e-6, e32 1.9e-6), worst
    e_hip / e32 above the floor 2.48."""
    t = Tally("composite_backward")
    _backward(t, I.composite_case(S), I.backward_refs(S), f"S{S}g{group}")
    t.done()


def test_composite_auto_group_rule():
    """The automatic group (pcnerf_set_composite_group(0)): 512 samples with 2,048 rays (a wave per ray) and with
    the first 2,047 of the same rays (a workgroup per ray), and 511 samples with 64 rays (a wave per ray); forward
    and backward against float64 on all rows, and the shared rows agree across the two sides to the forward
    tolerance.  No noise here (the per-size tests carry it): among 2,048 rays it leaves a few with a depth or an
    in-mask weight sum that cancels to ~0, where float32 itself has no relative accuracy (e32 1.6e-3 for depth) and
    that one ray's e32 would set the tolerance of all.  Measured: worst e_hip / max(4 e32, 2.4e-7) 0.36, worst e_hip / e32 above the floor 1.06."""
    prev = _ops.set_composite_group(0)
    try:
        t = Tally("composite_auto_group")
        big = I.composite_case(512, 2048, 90512, False)
        sub = I.first_rows(big, 2047)
        names = ("plain", "divide")
        a = _forward(t, big, "S512R2048")
        b = _forward(t, sub, "S512R2047")
        _backward(t, big, I.backward_refs_of(big, names), "S512R2048")
        _backward(t, sub, I.backward_refs_of(sub, names), "S512R2047")
        for branch in names:
            for k in ("w", "depth", "free_ray", "sl1_ray", "opac_row"):
                q64, q32 = sub[branch]["f64"][k], sub[branch]["f32"][k]
                tol = max(4 * F.err(q32, q64), FLOOR)
                scale = q64.abs().amax(-1, keepdim=True) if q64.dim() == 2 else q64.abs()
                d = (a[branch][k][:2047].double() - b[branch][k].double()).abs()
                assert bool((d <= tol * scale).all()), (branch, k, float((d / scale.clamp_min(1e-300)).max()), tol)
        small = I.composite_case(511, 64, 90511, False)
        _forward(t, small, "S511R64")
        _backward(t, small, I.backward_refs_of(small, names), "S511R64")
        t.done()
    finally:
        _ops.set_composite_group(prev)


@pytest.mark.parametrize("group", [0, 64, 256], indirect=True)
def test_composite_limits_refused_before_launch(group):
    """More samples per ray than the largest instantiation holds: an error naming the limit, no launch."""
    for S, limit, call in ((16385, "16384", "fwd"), (4097, "4096", "bwd")):
        z = torch.sort(torch.rand(2, S, device=DEV), -1)[0]
        p = torch.rand(2, S, device=DEV)
        with pytest.raises(RuntimeError, match=limit):
            if call == "fwd":
                _ops.composite(p, z)
            else:
                _ops.composite_backward(p, z, None, 0.0, I.EPS, None, 0, torch.ones(2, device=DEV), None, None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("divide", [False, True])
@pytest.mark.parametrize("R,N", [(1, 4), (257, 3), (1000, 15333), (4096, 16)])
def test_child_loss_reduce_direct(R, N, divide):
    """pcnerf_child_loss_reduce alone on given per-ray terms: ids 0 and N + 1 (no child), children owning no ray
    (most of them when N > R), one ray, more rays than one block reduces at once.  Measured: worst e_hip /
    max(4 e32, 2.4e-7) 0.37 (every error below the floor)."""
    fr, sl, rays = I.child_reduce_case(R, N, 31 * R + N)
    got = _ops.child_losses(_dev(fr), _dev(sl), _dev(rays), divide, N)
    q64 = F.child_reduce(fr.double(), sl.double(), rays[:, 9], divide, N)
    q32 = F.child_reduce(fr, sl, rays[:, 9], divide, N)
    t = Tally("child_loss_reduce")
    for k, g, a, b in zip(("free", "depth_loss"), got, q32, q64):
        t.check(f"R{R}N{N}{'div' if divide else ''}", k, g.cpu().reshape(()), a, b)
    t.done()


@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("S", I.VIEW_S)
def test_view_rows_vs_f64(S, method):
    """k_view_rows on five rows (render_inputs.view_case): weights, depth, child_sum and the opacity sums against
    float64; points bit for bit o + depth d in float32; at_peak the strict mask at the argmax of scipy's Gaussian
    filter of the kernel's own weights.  Rows shorter than the 41-tap filter, every MAXB form, 3 / 2 / 1 waves per
    block, a sample exactly on the first strict bound, an interval in a gap of z.  Measured on the MI355X: worst
    e_hip / max(4 e32, 2.4e-7) 0.43, worst e_hip / e32 above the floor 1.5 -- with logf in the opacity terms
    (before k_view_rows took the float64 log rounded once) opac_row missed at 13 of the 26 cases, e_hip growing with
    S to 2.3e-5 against e32 4.2e-6 at S 8193."""
    c = I.view_case(S)
    rows = _dev(c["rows"])
    w, depth, at_peak, csum, opac, pts = (x.cpu() for x in _ops.view_rows(_dev(c["p"]), _dev(c["z"]), rows, method,
                                                                            I.EPS))
    t = Tally("view_rows")
    ref = c[method]
    for k, x in (("w", w), ("depth", depth), ("child_sum", csum), ("opac_row", opac)):
        t.check(f"S{S}m{method}", k, x, ref["f32"][k], ref["f64"][k])
    r = c["rows"].numpy()
    want = r[:, 0:3] + depth.numpy()[:, None] * r[:, 3:6]           # float32, one rounding per op
    assert want.dtype == np.float32 and np.array_equal(pts.numpy(), want)
    at, unclear = I.peak_reference(w, c["mv"])
    assert not bool(unclear.any())                                   # the inputs leave no row out
    assert at_peak.bool().tolist() == at.tolist()
    t.done()
