"""Frozen-BatchNorm training on the GPU: parameter gradients of EVAL-mode networks (nof._autograd.FrozenPass /
FrozenPassPoints / NofForward's eval branch; kernels k_eval_gmoments and k_eval_param_grads).

1. the moments kernel against the float64 sum of g_s E(x_s), its three sources against one another, zeros, bits;
2. the algebra kernel against tests/frozen_bn_ref.py on a random mom; accumulation and NULL entries through the C entry;
3. inference_train on an eval-mode module against the reference's own autograd (tests/golden/frozen_bn_grads.npz);
4. render_rays_train end to end against torch float64 autograd of the oracle at the HIP path's own sample depths;
5. coarse in train mode + fine in eval mode in one call, and the eval switches (fold, fp32 math);
6. NOF.forward on an embedded batch;  7. the refusals that stay;  8. the driver's freeze_bn.

Gradient envelope (check_grads_elem's f64 rule, without the train-mode noise-level list -- no gradient is zero here):
|hip - f64| <= max(1e-4 |f64|, 1.5 spread + 6 RMS(spread)) per entry, spread = the larger of the float32 reference
runs' distances from the float64 run; the norm of a sampled matrix within 1e-4 + 1.5 x the reference's own norm
distance; with two float32 runs, the tensor's RMS error within 1.5 x the noisier run's RMS distance."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import frozen_bn_ref as FR
from conftest import golden
from gradcheck import _report
from nof import _hip, _ops
from nof import _torch_ops as T
from nof import render as R
from nof import synthetic as syn
from nof.networks import Embedding, NOF_coarse, NOF_fine
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
P = torch.ops.pcnerf
EPS32 = float(np.float32(1e-5))   # BatchNorm's eps as the C ABI carries it (a float)


def module(cls, seed, train=False, grad=True):
    m = syn.load_into(cls(), syn.init_nof_params(seed)).cuda().train(train)
    for t in m.parameters():
        t.requires_grad_(grad)
    return m


def running(m):
    return [t.clone() for b in m.norms() for t in (b.running_mean, b.running_var, b.num_batches_tracked)]


def hip_grads(m):
    return {k: t.grad.detach().cpu().numpy() for k, t in m.named_parameters()}


# ------------------------------------------------------------------------------------------------ the envelope
def envelope(hip, f64, ref, ref2=None, idx=None, norms=None, rtol=1e-4, spread_k=1.5, floor_k=6.0):
    """-> max err / tol of one tensor (asserting the norm / RMS conditions); ``idx``: compare the sampled entries of
    ``hip`` with the stored ones, ``norms`` = (ref, [ref2,] f64) norms of the full matrix."""
    hip = np.asarray(hip, dtype=np.float64)
    if idx is not None:
        nr, nf = float(norms[0]), float(norms[-1])
        assert abs(np.linalg.norm(hip) - nf) <= rtol * nf + spread_k * abs(nr - nf), ("norm", np.linalg.norm(hip), nf)
        hip = hip.reshape(-1)[idx]
    hip, f64, ref = hip.ravel(), np.asarray(f64, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    spread = np.abs(ref - f64)
    if ref2 is not None:
        ref2 = np.asarray(ref2, dtype=np.float64).ravel()
        spread = np.maximum(spread, np.abs(ref2 - f64))
    tol = np.maximum(rtol * np.abs(f64), spread_k * spread + floor_k * np.sqrt(np.mean(spread ** 2)))
    err = np.abs(hip - f64)
    if ref2 is not None:
        rms_ref = max(np.sqrt(np.mean((ref - f64) ** 2)), np.sqrt(np.mean((ref2 - f64) ** 2)))
        assert np.sqrt(np.mean(err ** 2)) <= spread_k * rms_ref + rtol * np.sqrt(np.mean(f64 ** 2)), "rms"
    return float((err / np.maximum(tol, 1e-300)).max())


def check_envelope(case, got, f64, ref):
    """Full tensors: {key: array} of the HIP path, the float64 oracle and its float32 run."""
    worst, bad = {}, []
    for k in FR.GRAD_KEYS:
        worst[k] = envelope(got[k], f64[k], ref[k])
        if worst[k] > 1.0:
            bad.append((k, worst[k]))
    kw = max(worst, key=worst.get)
    print(case, "worst err/tol", worst[kw], kw)
    _report({"case": case, "tensors": len(worst), "max_err_over_tol": worst[kw], "worst_tensor": kw,
             "failed": len(bad)})
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 1. moments
def ray_case(R_, S, stride, seed):
    g = torch.Generator().manual_seed(seed)
    rays = torch.zeros(R_, stride)
    rays[:, 0:3] = (torch.rand(R_, 3, generator=g) - 0.5) * 4
    d = torch.randn(R_, 3, generator=g)
    rays[:, 3:6] = d / d.norm(dim=1, keepdim=True)
    rays[:, 6:] = torch.rand(R_, stride - 6, generator=g)
    z = torch.sort(torch.rand(R_, S, generator=g) * 24 + 0.5, dim=1).values.contiguous()
    gl = torch.randn(R_, S, generator=g)
    dz = rays[:, None, 3:6] * z[..., None]          # two torch ops: no contraction
    pts = (rays[:, None, 0:3] + dz).contiguous()
    return rays, z, gl, pts


def moments_bound(E, gl):
    """(ref, bound) per component for E (N, 63) float64 and g (N,): 2e-6 sum|g| (the float32 encoding's stated
    agreement, DESIGN row a9; not for the exact raw-coordinate terms and mom[63]) + 1e-12 sum|term|."""
    g64 = gl.double().reshape(-1, 1)
    terms = torch.cat([g64 * E, g64], 1)
    absum = terms.abs().sum(0)
    enc = torch.full((64,), 2e-6, dtype=torch.float64) * g64.abs().sum()
    enc[0:3] = 0
    enc[63] = 0
    return terms.sum(0), enc + 1e-12 * absum, absum


@pytest.mark.parametrize("R_", [1, 5, 130])
@pytest.mark.parametrize("S", [48, 65, 384])
@pytest.mark.parametrize("stride", [8, 15])
def test_moments_kernel(R_, S, stride):
    rays, z, gl, pts = ray_case(R_, S, stride, 100 * R_ + S + stride)
    N = R_ * S
    ref, bound, absum = moments_bound(O.embed(pts.double().reshape(-1, 3)), gl)
    rd, zd, gd, pd = rays.cuda(), z.cuda(), gl.cuda(), pts.cuda()
    mr = P.eval_gmoments_rays(rd, zd, gd)
    assert mr.shape == (64,) and mr.dtype == torch.float64
    err = (mr.cpu() - ref).abs()
    print("rays: worst err/bound", float((err / bound).max()))
    assert bool((err <= bound).all()), (err / bound).max()
    order = 2 * (N - 1) * 2.0 ** -53 * absum     # the same float64 terms in another order
    mp = P.eval_gmoments_points(pd.view(R_, S, 3), gd)
    assert bool(((mp - mr).abs().cpu() <= order).all())
    assert torch.equal(P.eval_gmoments_points(pd.view(-1, 3), gd.view(-1)), mp)
    emb = P.embed(pd.view(-1, 3))
    me = P.eval_gmoments_embedded(emb, gd.view(-1))
    assert bool(((me - mp).abs().cpu() <= order).all())
    assert bool(((me.cpu() - ref).abs() <= bound).all())
    assert torch.equal(P.eval_gmoments_rays(rd, zd, gd), mr)                       # two runs: equal bits
    zero = P.eval_gmoments_rays(rd, zd, torch.zeros_like(gd))
    assert torch.equal(zero, torch.zeros(64, dtype=torch.float64, device="cuda"))  # g = 0: exact zeros


def test_moments_single_point_and_empty():
    pts = torch.tensor([[3.25, -17.5, 24.0625]])
    gl = torch.tensor([0.37])
    ref, bound, _ = moments_bound(O.embed(pts.double()), gl)
    m = P.eval_gmoments_points(pts.cuda(), gl.cuda())
    assert bool(((m.cpu() - ref).abs() <= bound).all())
    assert float(m[63]) == float(gl.double()) and float(m[0]) == float(gl.double() * pts[0, 0].double())
    m0 = P.eval_gmoments_points(torch.empty(0, 3, device="cuda"), torch.empty(0, device="cuda"))
    assert torch.equal(m0, torch.zeros(64, dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------------------------------------ 2. algebra
def random_mom(seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(64) * np.concatenate([np.full(3, 20.0), np.ones(60), [3.0]])


def test_algebra_kernel_against_restatement():
    """|hip - ref| <= 2^-24 |ref| + 1e-10 max|ref| per entry: one float32 rounding + float64 reordering."""
    mom = random_mom(5)
    ref = FR.param_grads(FR.params64(1234), mom, EPS32)
    m = module(NOF_coarse, 1234)
    got = P.eval_param_grads([t.detach() for t in T.eval_params(m)], torch.from_numpy(mom).cuda(), 1e-5)
    assert len(got) == 34
    worst = 0.0
    for k, t in zip(FR.GRAD_KEYS, got):
        assert t.dtype == torch.float32 and tuple(t.shape) == ref[k].shape, k
        tol = 2.0 ** -24 * np.abs(ref[k]) + 1e-10 * np.abs(ref[k]).max()
        err = np.abs(t.cpu().numpy().astype(np.float64) - ref[k])
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (k, float((err / tol).max()))
    print("algebra: worst err/tol", worst)
    again = P.eval_param_grads([t.detach() for t in T.eval_params(m)], torch.from_numpy(mom).cuda(), 1e-5)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_algebra_entry_accumulates_and_skips_null():
    """Through the C entry: non-zero buffers receive old + fl32(value) exactly; NULL entries are skipped."""
    m = module(NOF_coarse, 1234)
    mom = torch.from_numpy(random_mom(6)).cuda()
    val = P.eval_param_grads([t.detach() for t in T.eval_params(m)], mom, 1e-5)
    g = torch.Generator(device="cuda").manual_seed(1)
    old = [torch.randn(t.shape, device="cuda", generator=g) * float(t.abs().max()) for t in val]
    buf = [t.clone() for t in old]
    skip = {0, 4, 9, 17, 30, 33}   # lin_w[0], lin_w[4], lin_b[1], bn_w[1], bn_b[6], out_b stay NULL
    s, keep = _ops._params(m)
    gs = _hip.NofGrads()
    ptr = [None if i in skip else b.data_ptr() for i, b in enumerate(buf)]
    for i in range(8):
        gs.lin_w[i], gs.lin_b[i], gs.bn_w[i], gs.bn_b[i] = ptr[i], ptr[8 + i], ptr[16 + i], ptr[24 + i]
    gs.out_w, gs.out_b = ptr[32], ptr[33]
    _hip.check(_hip.lib().pcnerf_nof_eval_param_grads(ctypes.byref(s), 1e-5, mom.data_ptr(), ctypes.byref(gs),
                                                      _hip.stream_of(mom)))
    torch.cuda.synchronize()
    for i, (b, o, v) in enumerate(zip(buf, old, val)):
        assert torch.equal(b, o if i in skip else o + v), FR.GRAD_KEYS[i]


# ------------------------------------------------------------------------------------------------ 3. reference
def load_golden():
    """frozen_bn_grads.npz with gradcheck's alt: / f64: keys rebuilt (make_frozen_bn_golden.py stores them relative
    to the float32 run: ulp: = int32 bit-pattern difference, res: = float32(f64 - ref))."""
    g = dict(golden("frozen_bn_grads"))
    for k in [k for k in g if k.startswith("ulp:")]:
        base = k[4:]
        bits = (g[base].view(np.uint32).astype(np.uint64) + g[k].view(np.uint32).astype(np.uint64)) & 0xffffffff
        g["alt:" + base] = bits.astype(np.uint32).view(np.float32)
        g["f64:" + base] = g[base].astype(np.float64) + g["res:" + base].astype(np.float64)
    return g


@pytest.fixture(scope="module")
def gold():
    return load_golden()


@pytest.mark.parametrize("case", ["a", "b", "d"])
def test_inference_train_frozen_vs_reference(case, gold):
    g, k = gold, case + "/"
    rays, pts, z, cot = (torch.from_numpy(g[k + n]).cuda() for n in ("rays", "pts", "z", "cot"))
    losses, divide, noise_std = int(g[k + "losses"]), int(g[k + "divide"]), float(g[k + "noise_std"])
    rng = {"noise": torch.from_numpy(g[k + "noise"])} if noise_std else None
    m = module(NOF_coarse, int(g["seed"]))
    before = running(m)
    kw = dict(noise_std=noise_std, sub_nerf_test_num=int(g["sub_nerf_test_num"]), use_child_nerf_divide=divide,
              use_child_nerf_loss=losses, rng=rng)
    args = (m, Embedding(3, 10), pts, rays, z, rays[:, 10:12].contiguous(), rays[:, 12:14].contiguous(),
            rays[:, -1:].contiguous(), rays[:, 8:9].contiguous())
    fl, dl, d, w = R.inference_train(*args, **kw)
    with torch.no_grad():
        fl0, dl0, d0, w0 = R.inference_train(*args, **kw)
    assert torch.equal(d, d0) and torch.equal(w, w0) and torch.equal(fl.cpu(), fl0.cpu()) and \
        torch.equal(dl.cpu(), dl0.cpu())
    tol = dict(rtol=1e-4, atol=1e-6)   # test_inference_fns_gpu's forward tolerances
    np.testing.assert_allclose(d.detach().cpu().numpy(), g[k + "depth"], err_msg="depth", **tol)
    if losses:
        np.testing.assert_allclose(fl.detach().cpu().numpy(), g[k + "free"], err_msg="free", **tol)
        np.testing.assert_allclose(dl.detach().cpu().numpy(), g[k + "depth_loss"], err_msg="depth_loss", **tol)
    total = (d * cot).sum()
    if losses:
        total = total + float(g[k + "c1"]) * fl.sum() + float(g[k + "c2"]) * dl.sum()
    total.backward()
    assert all(torch.equal(a, b) for a, b in zip(before, running(m)))
    got, worst, bad = hip_grads(m), {}, []
    for key in FR.GRAD_KEYS:
        sfx = "" if k + key in g else "@val"
        idx = g["idx/" + key] if sfx else None
        norms = [g[p + k + key + "@norm"] for p in ("", "alt:", "f64:")] if sfx else None
        try:
            worst[key] = envelope(got[key], g["f64:" + k + key + sfx], g[k + key + sfx], g["alt:" + k + key + sfx],
                                  idx, norms)
            assert worst[key] <= 1.0, worst[key]
        except AssertionError as e:
            bad.append((key, str(e)[:200]))
    kw_ = max(worst, key=worst.get)
    print("golden", case, "worst err/tol", worst[kw_], kw_)
    _report({"case": "frozen_bn_golden_" + case, "tensors": len(worst), "max_err_over_tol": worst[kw_],
             "worst_tensor": kw_, "failed": len(bad)})
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 4. end to end
def oracle_params(seed, dtype):
    Q = O.params_from_numpy(syn.init_nof_params(seed))
    return {k: (v.to(dtype).requires_grad_(k in FR.GRAD_KEYS) if v.is_floating_point() else v) for k, v in Q.items()}


def oracle_pass(Q, rays32, z32, dtype, losses, divide, sub):
    """One eval-mode pass of render_rays_train (render.py:38-163) at GIVEN float32 depths: positions fl(o + fl(d z))
    and the child masks from the float32 values, the arithmetic after them in ``dtype``."""
    pts = (rays32[:, None, 0:3] + rays32[:, None, 3:6] * z32[..., None]).to(dtype)
    z = z32.to(dtype)
    p = O.query(Q, pts, False, 1 << 20)
    w, depth = O.composite(p, z, 1e-10)
    if not losses:
        return depth, 0.0, 0.0
    m0 = O.expand_mask(z32, rays32[:, 10], rays32[:, 11], 0.0)
    m2 = O.expand_mask(z32, rays32[:, 10], rays32[:, 11], 2)
    w_free = w * (~m0).to(dtype)
    wc, zc = w * m2.to(dtype), z * m2.to(dtype)
    dc = torch.sum(wc / (torch.sum(wc, -1).reshape(-1, 1) + 1e-10) * zc, -1)
    sl1 = torch.nn.SmoothL1Loss(reduction="mean")
    rr, n = rays32[:, 14].to(dtype), rays32.shape[0]
    if not divide:
        return depth, torch.sum(torch.square(w_free)) / n, 1 / n * 0.1 * sl1(1e1 * dc, 1e1 * rr)
    free = depth_loss = 0.0
    for i in range(sub):
        m = (rays32[:, 9] > (i + 0.5)) & (rays32[:, 9] < (i + 1.5))
        c = float(m.sum())
        if c >= 1:
            free = free + torch.sum(torch.square(w_free[m])) / c
            depth_loss = depth_loss + 1 / c * 0.1 * sl1(1e1 * dc[m], 1e1 * rr[m])
    return depth, free, depth_loss


C1, C2 = 7.0, 11.0


def oracle_grads(seed, rays32, z32, cot, dtype, divide, sub):
    Q = oracle_params(seed, dtype)
    depth, free, dl = oracle_pass(Q, rays32, z32, dtype, True, divide, sub)
    ((depth * cot.to(dtype)).sum() + C1 * free + C2 * dl).backward()
    return {k: Q[k].grad.numpy() for k in FR.GRAD_KEYS}


def hip_depths(mc, rays, Ns, Ni, chunk):
    """The coarse and fine sample depths render_rays_train takes (perturb = 0, noise_std = 0: deterministic)."""
    with torch.no_grad():
        z = R._coarse(rays, Ns, 1, 0.1, 0, None)
        mcc = copy.deepcopy(mc)   # a train-mode module's statistics move in a forward
        w = P.composite(R._query(mcc, rays, z, chunk), z, None, 0.0, 1e-10, None, 10, 11, 14, True)[0]
        return z, P.resample(z, w, Ni, None)


def e2e(n_rays, Ns, Ni, divide, seed, coarse_train=False):
    """-> (modules, rays, cot, (z, zf), kwargs): one render_rays_train + backward with the fine (and, unless
    ``coarse_train``, the coarse) network in eval mode."""
    rays = torch.from_numpy(syn.make_rays(n_rays, seed=seed)).cuda()
    cot = torch.randn(n_rays, generator=torch.Generator().manual_seed(seed))
    mc, mf = module(NOF_coarse, 1234, train=coarse_train), module(NOF_fine, 5678)
    kw = dict(sub_nerf_test_num=32, N_samples=Ns, N_importance=Ni, perturb=0, noise_std=0, chunk=8192,
              issegmentated=1, childnerf_ratio=0.1, use_child_nerf_divide=divide, use_child_nerf_loss=1)
    zs = hip_depths(mc, rays, Ns, Ni, 8192)
    return (mc, mf), rays, cot, zs, kw


def total_loss(res, cot):
    return ((res["depth"] + res["depth_fine"]) * cot).sum() + \
        C1 * (res["child_free_loss"].sum() + res["child_free_loss_fine"].sum()) + \
        C2 * (res["child_depth_loss"].sum() + res["child_depth_loss_fine"].sum())


@pytest.mark.parametrize("n_rays,Ns,Ni", [(130, 64, 128), (24, 128, 256)])
@pytest.mark.parametrize("divide", [0, 1])
def test_render_rays_train_frozen_end_to_end(n_rays, Ns, Ni, divide):
    (mc, mf), rays, cot, (z, zf), kw = e2e(n_rays, Ns, Ni, divide, 300 + n_rays)
    before = running(mc) + running(mf)
    emb = Embedding(3, 10)
    res = R.render_rays_train(mc, mf, emb, rays, **kw)
    with torch.no_grad():
        res0 = R.render_rays_train(mc, mf, emb, rays, **kw)
    for k in res:
        assert torch.equal(res[k], res0[k]), k          # the no_grad call's bits
    total_loss(res, cot.cuda()).backward()
    assert all(torch.equal(a, b) for a, b in zip(before, running(mc) + running(mf)))
    first = [t.grad.clone() for m in (mc, mf) for t in m.parameters()]
    for m in (mc, mf):
        m.zero_grad(set_to_none=True)
    total_loss(R.render_rays_train(mc, mf, emb, rays, **kw), cot.cuda()).backward()
    assert all(torch.equal(a, t.grad) for a, t in zip(first, [t for m in (mc, mf) for t in m.parameters()]))
    r32 = rays.cpu()
    for name, m, seed, zz in (("coarse", mc, 1234, z), ("fine", mf, 5678, zf)):
        f64 = oracle_grads(seed, r32, zz.cpu(), cot, torch.float64, divide, 32)
        f32 = oracle_grads(seed, r32, zz.cpu(), cot, torch.float32, divide, 32)
        check_envelope(f"frozen_e2e_{n_rays}x{Ns}+{Ni}_div{divide}_{name}", hip_grads(m), f64, f32)


# ------------------------------------------------------------------------------------------------ 5. mixed, switches
def test_mixed_modes_in_one_call():
    """Coarse in train mode (the existing rematerialised backward, statistics move) and fine in eval mode (frozen,
    statistics stay): the fine gradients are the frozen backward's at this call's own fine depths."""
    (mc, mf), rays, cot, (z, zf), kw = e2e(130, 64, 128, 0, 430, coarse_train=True)
    twin = copy.deepcopy(mc)
    bc, bf = running(mc), running(mf)
    total_loss(R.render_rays_train(mc, mf, Embedding(3, 10), rays, **kw), cot.cuda()).backward()
    assert all(torch.equal(a, b) for a, b in zip(bf, running(mf)))
    assert not torch.equal(bc[0], running(mc)[0]) and int(running(mc)[2]) > int(bc[2])
    f64 = oracle_grads(5678, rays.cpu(), zf.cpu(), cot, torch.float64, 0, 32)
    f32 = oracle_grads(5678, rays.cpu(), zf.cpu(), cot, torch.float32, 0, 32)
    check_envelope("frozen_mixed_fine", hip_grads(mf), f64, f32)
    # the coarse gradients are TrainPass's: those of the call with both networks in train mode
    mf2 = module(NOF_fine, 5678, train=True)
    total_loss(R.render_rays_train(twin, mf2, Embedding(3, 10), rays, **kw), cot.cuda()).backward()
    for (k, a), b in zip(mc.named_parameters(), twin.parameters()):
        assert torch.equal(a.grad, b.grad), k


@pytest.mark.parametrize("switch", ["fold", "fp32"])
def test_eval_switches(switch):
    (mc, mf), rays, cot, _, kw = e2e(130, 64, 128, 0, 430)
    prev = _ops.set_eval_fold(True) if switch == "fold" else _ops.set_eval_math("fp32")
    try:
        zs = hip_depths(mc, rays, 64, 128, 8192)
        res = R.render_rays_train(mc, mf, Embedding(3, 10), rays, **kw)
        with torch.no_grad():
            res0 = R.render_rays_train(mc, mf, Embedding(3, 10), rays, **kw)
        assert all(torch.equal(res[k], res0[k]) for k in res)
        total_loss(res, cot.cuda()).backward()
    finally:
        _ops.set_eval_fold(prev) if switch == "fold" else _ops.set_eval_math(prev)
    for name, m, seed, zz in (("coarse", mc, 1234, zs[0]), ("fine", mf, 5678, zs[1])):
        f64 = oracle_grads(seed, rays.cpu(), zz.cpu(), cot, torch.float64, 0, 32)
        f32 = oracle_grads(seed, rays.cpu(), zz.cpu(), cot, torch.float32, 0, 32)
        check_envelope(f"frozen_switch_{switch}_{name}", hip_grads(m), f64, f32)


# ------------------------------------------------------------------------------------------------ 6. NOF.forward
def test_nof_forward_frozen():
    g = torch.Generator().manual_seed(21)
    x = (torch.rand(257, 3, generator=g) - 0.5) * 50
    emb = O.embed(x)
    gp = torch.randn(257, 1, generator=g)
    m = module(NOF_coarse, 1234)
    before = running(m)
    p = m(emb.cuda())
    with torch.no_grad():
        assert torch.equal(p, m(emb.cuda()))
    p.backward(gp.cuda())
    assert all(torch.equal(a, b) for a, b in zip(before, running(m)))
    refs = []
    for dtype in (torch.float64, torch.float32):
        Q = oracle_params(1234, dtype)
        (O.nof_forward(Q, emb.to(dtype), False) * gp.to(dtype)).sum().backward()
        refs.append({k: Q[k].grad.numpy() for k in FR.GRAD_KEYS})
    check_envelope("frozen_nof_forward", hip_grads(m), refs[0], refs[1])


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_kept():
    rays = torch.from_numpy(syn.make_rays(16, seed=3)).cuda()
    mc, mf, emb = module(NOF_coarse, 1), module(NOF_fine, 2), Embedding(3, 10)
    with pytest.raises(NotImplementedError, match="forward-only"):
        R.render_rays_val(mc, mf, emb, rays, N_samples=16, N_importance=16, perturb=0, noise_std=0)
    z = torch.linspace(1, 20, 8, device="cuda").expand(16, 8).contiguous()
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).contiguous()
    args = (rays, z, rays[:, 10:12].contiguous(), rays[:, 12:14].contiguous(), rays[:, 14:15].contiguous(),
            rays[:, 8:9].contiguous())
    with pytest.raises(NotImplementedError, match="forward-only"):
        R.inference_val(mc, emb, pts, *args, noise_std=0)
    with pytest.raises(NotImplementedError, match="samples_xy"):
        R.inference_train(mc, emb, pts.clone().requires_grad_(True), *args, noise_std=0)


def test_operator_operand_checks():
    rays, z, gl, pts = (t.cuda() for t in ray_case(5, 48, 8, 1))
    params = [t.detach() for t in T.eval_params(module(NOF_coarse, 1))]
    mom = P.eval_gmoments_rays(rays, z, gl)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.eval_gmoments_rays(rays.cpu(), z, gl)
    with pytest.raises(RuntimeError, match="contiguous"):
        P.eval_gmoments_rays(rays, z, gl.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        P.eval_gmoments_rays(rays, z, gl.t().contiguous().t())
    with pytest.raises(RuntimeError, match="expected"):
        P.eval_gmoments_rays(rays[:4].contiguous(), z, gl)
    with pytest.raises(RuntimeError, match="expected"):
        P.eval_gmoments_points(pts.view(-1, 3), gl.view(-1)[:-1].contiguous())
    with pytest.raises(RuntimeError, match="expected"):
        P.eval_gmoments_points(pts.view(-1, 3)[:, :2].contiguous(), gl.view(-1))
    emb = P.embed(pts.view(-1, 3))
    with pytest.raises(RuntimeError, match="expected"):
        P.eval_gmoments_embedded(emb[:, :62].contiguous(), gl.view(-1))
    with pytest.raises(RuntimeError, match="expected"):
        P.eval_gmoments_embedded(emb, gl.view(-1)[:-1].contiguous())
    with pytest.raises(RuntimeError, match="50 parameter tensors"):
        P.eval_param_grads(params[:49], mom, 1e-5)
    with pytest.raises(RuntimeError, match="contiguous"):
        P.eval_param_grads(params, mom.float(), 1e-5)
    with pytest.raises(RuntimeError, match="expected"):
        P.eval_param_grads(params, mom[:63].contiguous(), 1e-5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.eval_param_grads(params, mom.cpu(), 1e-5)


# ------------------------------------------------------------------------------------------------ 8. driver
def _fit(tmp_path, name, **kw):
    import train_kitti as TK
    from nof.nof_utils import get_opts
    from test_dataset import write_scene
    root, pose_path, _ = write_scene(str(tmp_path / name))
    args = f"""--datasettype kitti_dataload --root_dir {root} --pose_path {pose_path} --data_start 1150 --data_end 1155
     --re_loaddata 1 --result_path {tmp_path / name / "run"} --N_samples 32 --N_importance 64 --perturb 1 --noise_std 0
     --chunk 8192 --batch_size 128 --batch_size_val 64 --cloud_size_val 128 --num_epochs 2 --optimizer adam --lr 5e-4
     --weight_decay 1e-3 --decay_gamma 0.2 --use_child_nerf_divide 0 --use_child_nerf_loss 1
     --use_segmentated_sample 1 --segmentated_child_nerf_ratio 0.1 --lambda_loss 1 --lambda_loss_fine 1
     --lambda_child_free_loss 1000000 --lambda_child_depth_loss 100000 --range_delete_x 3 --range_delete_y 2
     --range_delete_z 1.25 --surface_expand 0.05 --interest_x 20 --interest_y 20 --visualize 0 --seed 42"""
    h = get_opts(args.split())
    assert h.freeze_bn is False and get_opts(args.split() + ["--freeze_bn"]).freeze_bn is True
    torch.manual_seed(0)
    system = TK.NOFSystem(h)
    system.prepare_data()
    h.sub_nerf_test_num = system.train_dataset.sub_nerf_test_num
    nets = (system.nof_coarse, system.nof_fine)
    start = [{k: v.clone() for k, v in m.state_dict().items()} for m in nets]
    res = TK.fit(system, max_steps=3, **kw)
    assert res["steps"] == 3
    return start, [m.state_dict() for m in nets]


def test_driver_freeze_bn(tmp_path):
    (tmp_path / "frozen").mkdir()
    (tmp_path / "plain").mkdir()
    (tmp_path / "plain2").mkdir()
    start, end = _fit(tmp_path, "frozen", freeze_bn=True)
    for s, e in zip(start, end):
        for k in s:
            if "running" in k or "num_batches" in k:
                assert torch.equal(s[k], e[k]), k          # every running statistic bit-unchanged
            else:
                assert not torch.equal(s[k], e[k]), k      # every parameter moves
    start2, plain = _fit(tmp_path, "plain")
    _, plain2 = _fit(tmp_path, "plain2", freeze_bn=False)
    for s, s2, a, b, f in zip(start, start2, plain, plain2, end):
        for k in a:
            assert torch.equal(s[k], s2[k]), k
            assert torch.equal(a[k], b[k]), k              # without the flag: the existing trajectory
        assert not torch.equal(a["layer1.1.running_mean"], s["layer1.1.running_mean"])
        assert not torch.equal(a["layer1.0.weight"], f["layer1.0.weight"])
