"""The point-sourced fused NOF query (pcnerf_nof_points_*, k_nof_eval_h3<..., PT = true> and the PT forms of the
moment / rematerialisation kernels) and nof.render's inference_val / inference_train / inference / inference_0525_2
on top of it.

1. eval and 2. train: on pts = fl(o + fl(d z)) formed by separate torch ops the point source must give the ray source's
   BITS (same arithmetic after the position fetch), in every query geometry, at sample totals that hit every block
   tail, and -- train mode -- with BatchNorm chunk boundaries inside 32-sample tiles; running statistics and the
   per-chunk statistics records included.
3. the four functions against the reference's own outputs on jittered (off-ray) positions
   (tests/golden/inference_fns.npz), at test_parity_gpu's tolerances.
4. loss.backward() through inference_train against the oracle's autograd (two thread counts + float64), the envelope
   of test_backward_gpu.test_train_grads_vs_oracle_small_chunks.
5. refusals and the opt-in eval paths' fallback."""
import numpy as np
import pytest
import torch

from conftest import golden
from gradcheck import check_grads_elem
from nof import _ops
from nof import render as R
from nof import synthetic as syn
from nof import _torch_ops as T
from nof.networks import Embedding, NOF_coarse
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 1234
NOISE = 1e-4   # test_backward_gpu's level for the mathematically-zero gradients
P = torch.ops.pcnerf


def model(train):
    return syn.load_into(NOF_coarse(), syn.init_nof_params(SEED)).to(DEV).train(train)


@pytest.fixture(scope="module")
def g():
    return golden("inference_fns")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ray_inputs(R_, S, seed):
    rays = torch.from_numpy(syn.make_rays(R_, seed=seed)).to(DEV)
    gen = torch.Generator().manual_seed(seed)
    z = (rays[:, 7:8].cpu() * torch.rand(R_, S, generator=gen)).to(DEV).contiguous()
    pts = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).contiguous()   # two torch ops: no contraction
    return rays, z, pts


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.isfinite(a).all(), what
    assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                       b.view(torch.int32) if b.dtype == torch.float32 else b), \
        f"{what}: {(a != b).sum().item()} of {a.numel()} values differ"


# ------------------------------------------------------------------------------------------------ 1. eval bits
# 7 samples: less than one block; 185: three 48-blocks + 41, one 96-block + 89; 3,072: whole blocks of both sizes
@pytest.mark.parametrize("geometry", [0, 1, 2, 3])
@pytest.mark.parametrize("R_,S", [(1, 7), (5, 37), (64, 48)])
def test_eval_points_bit_equal_to_rays(R_, S, geometry):
    rays, z, pts = ray_inputs(R_, S, 3)
    m = model(False)
    prev = _ops.set_query_geometry(geometry)
    try:
        with torch.no_grad():
            packed = P.pack_eval(T.eval_params(m))
            a = P.query_points_eval(pts, packed)
            flat = P.query_points_eval(pts.view(-1, 3), packed)
            b = P.query_eval(rays, z, packed)
    finally:
        _ops.set_query_geometry(prev)
    same_bits(a, b, f"eval {R_}x{S} geometry {geometry}")
    same_bits(flat.view(R_, S), b, f"eval {R_}x{S} flat geometry {geometry}")


# ------------------------------------------------------------------------------------------------ 2. train bits
def bn_state(m):
    return ([b.running_mean.clone() for b in m.norms()] + [b.running_var.clone() for b in m.norms()],
            [int(b.num_batches_tracked) for b in m.norms()])


@pytest.mark.parametrize("geometry", [-1, 0, 2, 3])   # (-1: the train query's default, geometry 1)
@pytest.mark.parametrize("keep", [True, False])
def test_train_points_bit_equal_to_rays(keep, geometry):
    """4,608 samples in chunks of 1,000: 5 chunks, the last 608, every boundary inside a 32-sample tile."""
    R_, S, chunk = 96, 48, 1000
    rays, z, pts = ray_inputs(R_, S, 4)
    N = R_ * S
    prev = _ops.set_query_geometry(geometry)
    try:
        with torch.no_grad():
            ma, mb = model(True), model(True)
            sa = _ops.fold_state(DEV, N, chunk) if keep else None
            sb = _ops.fold_state(DEV, N, chunk) if keep else None
            pa = _ops.query_points(ma, pts.view(-1, 3), R_, S, chunk, keep=sa)
            pb = _ops.query(mb, rays, z, chunk, keep=sb)
            if keep:
                ra, rb = _ops.bn_chunk_stats(sa, N, chunk), _ops.bn_chunk_stats(sb, N, chunk)
    finally:
        _ops.set_query_geometry(prev)
    same_bits(pa, pb, "train p")
    (ta, na), (tb, nb) = bn_state(ma), bn_state(mb)
    assert len(ta) == 16 and na == nb == [5] * 8
    for i, (x, y) in enumerate(zip(ta, tb)):
        same_bits(x, y, f"running statistic {i}")
    if keep:
        assert tuple(ra.shape) == (5, 8, 2, 256)
        assert torch.isfinite(ra).all() and torch.equal(ra, rb), "per-chunk BatchNorm records"


# ------------------------------------------------------------------------------------------------ 3. the fixture
def close(a, b, what, rtol=1e-4, atol=1e-6):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b, rtol=rtol, atol=atol, err_msg=what)


def table_a(g):
    rays = dev(g["a_rays"])
    return dict(rays=rays, nfc=rays[:, 10:12].contiguous(), nfp=rays[:, 12:14].contiguous(),
                ranges=rays[:, -1].view(-1, 1), rclass=rays[:, 8].view(-1, 1), pts=dev(g["a_pts"]), z=dev(g["a_z"]))


def check_val_and_inference(g):
    a, emb = table_a(g), Embedding(3, 10)
    with torch.no_grad():
        out = R.inference_val(model(False), emb, a["pts"], a["rays"], a["z"], a["nfc"], a["nfp"], a["ranges"],
                              a["rclass"], noise_std=0)
        assert len(out) == 2
        d, w = out
        assert tuple(d.shape) == (40,) and tuple(w.shape) == (40, 37) and d.dtype == w.dtype == torch.float32
        close(d, g["val_depth"], "inference_val depth")
        close(w, g["val_weights"], "inference_val weights")
        out = R.inference(model(False), emb, a["pts"], a["z"], noise_std=0)
        assert len(out) == 3
        d, w, o = out
        assert tuple(d.shape) == (40,) and tuple(w.shape) == (40, 37) and tuple(o.shape) == ()
        assert o.dtype == torch.float32 and o.is_cuda
        close(d, g["inf_depth"], "inference depth")
        close(w, g["inf_weights"], "inference weights")
        close(o, g["inf_opacity"], "inference opacity", atol=0)


def check_view(g, cases=((0, 0), (0, 1), (2, 0), (2, 1))):
    emb = Embedding(3, 10)
    rows, other = dev(g["v_rows"]), dev(g["v_other"])
    pts, z, nfc = dev(g["v_pts"]), dev(g["v_z"]), rows[:, 6:8].contiguous()
    for method, ei in cases:
        with torch.no_grad():
            out = R.inference_0525_2(model(False), emb, pts, z, other, nfc, noise_std=0,
                                     epsilon=float(g["view_eps"][ei]), depth_inference_method=method)
        assert len(out) == 4
        d, w, o, f = out
        k = f"view_m{method}_e{ei}_"
        assert tuple(d.shape) == (82,) and tuple(w.shape) == (82, 96) and tuple(o.shape) == ()
        assert tuple(f.shape) == (82, 1) and f.dtype == torch.bool
        close(d, g[k + "depth"], k + "depth")
        close(w, g[k + "weights"], k + "weights")
        close(o, g[k + "opacity"], k + "opacity", atol=0)
        assert np.array_equal(f.cpu().numpy(), g[k + "flag"]), k + "flag"


def test_inference_val_and_inference_vs_reference(g):
    check_val_and_inference(g)


def test_inference_0525_2_vs_reference(g, capsys):
    check_view(g)
    assert capsys.readouterr().out == ""   # the reference's prints are not reproduced


@pytest.mark.parametrize("divide", [0, 1])
def test_inference_train_vs_reference(divide, g):
    a, emb = table_a(g), Embedding(3, 10)
    m = model(True)
    with torch.no_grad():
        out = R.inference_train(m, emb, a["pts"], a["rays"], a["z"], a["nfc"], a["nfp"], a["ranges"], a["rclass"],
                                chunk=int(g["train_chunk"]), noise_std=0,
                                sub_nerf_test_num=int(g["train_sub_nerf_test_num"]), use_child_nerf_divide=divide,
                                use_child_nerf_loss=1)
    assert len(out) == 4
    fl, dl, d, w = out
    k = f"train{divide}_"
    assert tuple(fl.shape) == tuple(dl.shape) == ((1,) if divide else ())
    assert fl.dtype == dl.dtype == torch.float32 and fl.is_cuda and dl.is_cuda
    assert tuple(d.shape) == (40,) and tuple(w.shape) == (40, 37)
    close(fl, g[k + "free"], "child_free_loss")
    close(dl, g[k + "depth_loss"], "child_depth_loss")
    close(d, g[k + "depth"], "depth")
    close(w, g[k + "weights"], "weights")
    running = torch.stack([torch.stack([b.running_mean, b.running_var]) for b in m.norms()])
    close(running, g[k + "running"], "running statistics", atol=0)
    assert [int(b.num_batches_tracked) for b in m.norms()] == g[k + "batches"].tolist()


def test_inference_train_without_losses_returns_cpu_zeros(g):
    a, emb = table_a(g), Embedding(3, 10)
    with torch.no_grad():
        fl, dl, d, w = R.inference_train(model(True), emb, a["pts"], a["rays"], a["z"], a["nfc"], a["nfp"],
                                         a["ranges"], a["rclass"], chunk=500, noise_std=0)
    for t in (fl, dl):
        assert not t.is_cuda and tuple(t.shape) == () and float(t) == 0.0
    close(d, g["train0_depth"], "depth")


def test_noise_is_injected_and_used(g):
    a, emb = table_a(g), Embedding(3, 10)
    noise = torch.randn(40, 37, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        d, w = R.inference_val(model(False), emb, a["pts"], a["rays"], a["z"], a["nfc"], a["nfp"], a["ranges"],
                               a["rclass"], noise_std=1e-3, rng={"noise": noise})
        p = O.query(O.params_from_numpy(syn.init_nof_params(SEED)), torch.from_numpy(g["a_pts"]), False, 1 << 15)
        wr, dr = O.composite(p, torch.from_numpy(g["a_z"]), 1e-10, noise * 1e-3)
    close(d, dr.numpy(), "noisy depth", rtol=1e-4, atol=1e-5)
    close(w, wr.numpy(), "noisy weights", rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 4. gradients
def oracle_params(dtype=torch.float32):
    Q = O.params_from_numpy(syn.init_nof_params(SEED))
    Q = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in Q.items()}
    for k in Q:
        if k.endswith(".weight") or k.endswith(".bias"):
            Q[k].requires_grad_(True)
    return Q


def oracle_summary(Q, seed, prefix=""):
    """test_backward_gpu.oracle_summary's layout: small tensors in full, weight matrices by 2048 entries + norm."""
    out = {}
    rng = np.random.default_rng(seed)
    for k, t in Q.items():
        if not (k.endswith(".weight") or k.endswith(".bias")) or t.grad is None:
            continue
        gr = t.grad.numpy()
        if gr.size <= 512:
            out[prefix + k] = gr
        else:
            idx = rng.choice(gr.size, size=2048, replace=False)
            out[prefix + k + "@idx"], out[prefix + k + "@val"] = idx, gr.reshape(-1)[idx]
            out[prefix + k + "@norm"] = np.linalg.norm(gr.astype(np.float64))
    return out


def grad_case(R_, S, chunk, divide, seed):
    """Inputs and the oracle's gradients (float32 at two thread counts, ``alt:``; float64, ``f64:``) of
    sum(depth * wgt) + 1e6 free + 1e5 depth_loss through the train-mode point query, computed once per case."""
    rays = torch.from_numpy(syn.make_rays(R_, seed=seed))
    z = O.coarse_z(rays, S, True, 0.1)
    gen = torch.Generator().manual_seed(seed + 1)
    pts = (O.points(rays, z) + (torch.rand(R_, S, 3, generator=gen) - 0.5) * 0.1).contiguous()
    wgt = torch.rand(R_, generator=gen)

    def run(Q, dt):
        p = O.query(Q, pts.to(dt), True, chunk)
        w, d = O.composite(p, z.to(dt), 1e-10)
        r = rays.to(dt)
        fl, dl = O.child_losses(w, z.to(dt), r, r[:, 10:12], r[:, 14], divide, 32)
        ((d * wgt.to(dt)).sum() + 1e6 * fl.sum() + 1e5 * dl.sum()).backward()

    n0 = torch.get_num_threads()
    gr = {}
    for j, threads in enumerate((n0, 3 if n0 != 3 else 4)):
        torch.set_num_threads(threads)
        Q = oracle_params()
        run(Q, torch.float32)
        gr.update(oracle_summary(Q, 5, "alt:" if j else ""))
    torch.set_num_threads(n0)
    Q = oracle_params(torch.float64)
    run(Q, torch.float64)
    gr.update(oracle_summary(Q, 5, "f64:"))
    return dict(rays=rays, z=z, pts=pts, wgt=wgt, grads=gr, chunk=chunk, divide=divide)


_CASES = {}


def cached_case(*key):
    if key not in _CASES:
        _CASES[key] = grad_case(*key)
    return _CASES[key]


def run_hip_grads(c, case):
    m, emb = model(True), Embedding(3, 10)
    rays, z, pts = c["rays"].to(DEV), c["z"].to(DEV), c["pts"].to(DEV)
    fl, dl, d, w = R.inference_train(m, emb, pts, rays, z, rays[:, 10:12].contiguous(), None, rays[:, 14:15], None,
                                     chunk=c["chunk"], noise_std=0, sub_nerf_test_num=32,
                                     use_child_nerf_divide=c["divide"], use_child_nerf_loss=1)
    assert not w.requires_grad and d.requires_grad
    ((d * c["wgt"].to(DEV)).sum() + 1e6 * fl.sum() + 1e5 * dl.sum()).backward()
    named = dict(m.named_parameters())
    check_grads_elem(lambda k: named[k].grad.cpu().numpy(), list(named), c["grads"], "", case, noise=NOISE)


def test_inference_train_grads_small_chunks():
    """(96, 48) jittered samples in chunks of 1,000 (5 chunks, the last 608)."""
    run_hip_grads(cached_case(96, 48, 1000, 0, 31), "inference_train_chunk1000_remat4")


def test_inference_train_grads_ragged_second_chunk():
    """(256, 192) = 49,152 samples in chunks of 30,000: a ragged second chunk of 19,152; the divide branch."""
    run_hip_grads(cached_case(256, 192, 30000, 1, 37), "inference_train_chunk30000")


def test_inference_train_refuses_grad_on_positions(g):
    a, emb = table_a(g), Embedding(3, 10)
    with pytest.raises(NotImplementedError, match="samples_xy"):
        R.inference_train(model(True), emb, a["pts"].clone().requires_grad_(True), a["rays"], a["z"], a["nfc"],
                          a["nfp"], a["ranges"], a["rclass"], chunk=500, noise_std=0)


# ------------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("switch", ["train_math_fp32", "train_backward_store", "train_fold"])
def test_train_point_query_refused_under_opt_in_paths(switch, g):
    a, emb = table_a(g), Embedding(3, 10)
    if switch == "train_math_fp32":
        prev, restore = _ops.set_train_math("fp32"), _ops.set_train_math
    elif switch == "train_backward_store":
        prev, restore = _ops.set_train_backward("store"), _ops.set_train_backward
    else:
        prev, restore = _ops.set_train_fold(True), _ops.set_train_fold
    try:
        m = model(True)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="set_train_"):
            R.inference_train(m, emb, a["pts"], a["rays"], a["z"], a["nfc"], a["nfp"], a["ranges"], a["rclass"],
                              chunk=500, noise_std=0)
        assert [int(b.num_batches_tracked) for b in m.norms()] == [0] * 8
    finally:
        restore(prev)


@pytest.mark.parametrize("switch", ["eval_math_fp32", "eval_fold"])
def test_eval_fallback_matches_reference(switch, g):
    if switch == "eval_math_fp32":
        prev, restore = _ops.set_eval_math("fp32"), _ops.set_eval_math
    else:
        prev, restore = _ops.set_eval_fold(True), _ops.set_eval_fold
    try:
        check_val_and_inference(g)
        check_view(g, cases=((2, 1),))
    finally:
        restore(prev)


def test_query_points_eval_operand_checks():
    m = model(False)
    with torch.no_grad():
        packed = P.pack_eval(T.eval_params(m))
        pts = torch.rand(35, 3, device=DEV)
        out = P.query_points_eval(pts, packed)
        assert tuple(out.shape) == (35,) and out.dtype == torch.float32
        assert tuple(P.query_points_eval(pts.view(5, 7, 3), packed).shape) == (5, 7)
        with pytest.raises(RuntimeError, match="contiguous"):
            P.query_points_eval(torch.rand(3, 35, device=DEV).t(), packed)
        with pytest.raises(RuntimeError, match="float32"):
            P.query_points_eval(pts.double(), packed)
        with pytest.raises(RuntimeError, match=r"\(N, 3\)"):
            P.query_points_eval(torch.rand(35, 2, device=DEV), packed)
        with pytest.raises(RuntimeError, match="packed"):
            P.query_points_eval(pts, packed[:-1].contiguous())
        with pytest.raises(RuntimeError, match="no CPU path"):
            P.query_points_eval(pts.cpu(), packed)


def test_wrong_shapes_raise(g):
    a, emb = table_a(g), Embedding(3, 10)
    m = model(False)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="samples_xy"):
            R.inference(m, emb, a["pts"].view(-1, 3), a["z"])
        with pytest.raises(RuntimeError, match="z_vals"):
            R.inference(m, emb, a["pts"], a["z"][:, :-1])
        with pytest.raises(RuntimeError, match="near_far_child"):
            R.inference_val(m, emb, a["pts"], a["rays"], a["z"], a["rays"][:, 10:13], a["nfp"], a["ranges"],
                            a["rclass"])
