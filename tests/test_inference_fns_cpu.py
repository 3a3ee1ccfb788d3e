"""nof.render's inference_val / inference_train / inference / inference_0525_2 (reference render.py:13, :38, :166,
:229) without a GPU: the public signatures against the reference's (recorded in tests/golden/inference_fns.npz by
make_inference_golden.py), the fixture against the CPU oracle's pieces, the new C-ABI entries' argument checks, and
the host-side refusals."""
import ctypes
import inspect
import json

import numpy as np
import pytest
import torch

from conftest import golden
from nof import synthetic as syn
from oracle import ref_cpu as O

FUNCTIONS = ("inference_val", "inference_train", "inference", "inference_0525_2")


@pytest.fixture(scope="module")
def g():
    return golden("inference_fns")


@pytest.mark.parametrize("name", FUNCTIONS)
def test_signatures_match_reference(name, g):
    """Same parameter names, order and defaults (value and type) as the reference; only keyword-only parameters
    may follow."""
    from nof import render
    want = json.loads(str(g["sig_" + name]))
    params = list(inspect.signature(getattr(render, name)).parameters.values())
    assert len(params) >= len(want)
    for p, (pname, has, default) in zip(params, want):
        assert p.name == pname
        assert p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert (p.default is not inspect.Parameter.empty) == has, pname
        if has:
            assert p.default == default and type(p.default) is type(default), (pname, p.default, default)
    for p in params[len(want):]:
        assert p.kind == inspect.Parameter.KEYWORD_ONLY, p.name
    assert "rng" in [p.name for p in params[len(want):]]


@pytest.fixture(autouse=True)
def one_thread():
    """The fixture was generated at one torch thread (make_inference_golden.py); another thread count blocks the
    matrix products differently and moves float32 results by a few ulp."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def oracle_params():
    return O.params_from_numpy(syn.init_nof_params(1234))


def close(a, b, what):
    np.testing.assert_allclose(a.numpy() if torch.is_tensor(a) else a, b, rtol=1e-6, atol=0, err_msg=what)


def test_oracle_reproduces_val_and_inference(g):
    pts, z = torch.from_numpy(g["a_pts"]), torch.from_numpy(g["a_z"])
    with torch.no_grad():
        p = O.query(oracle_params(), pts, False, 1024 * 32)
        w, d = O.composite(p, z, 1e-10)
        opac = torch.mean(torch.log(0.1 + p) + torch.log(0.1 + (1 - p)) + 2.20727)
    close(d, g["val_depth"], "val depth")
    close(w, g["val_weights"], "val weights")
    close(d, g["inf_depth"], "inference depth")
    close(w, g["inf_weights"], "inference weights")
    close(opac, g["inf_opacity"], "inference opacity")


@pytest.mark.parametrize("divide", [0, 1])
def test_oracle_reproduces_inference_train(divide, g):
    rays = torch.from_numpy(g["a_rays"])
    pts, z = torch.from_numpy(g["a_pts"]), torch.from_numpy(g["a_z"])
    P = oracle_params()
    with torch.no_grad():
        p = O.query(P, pts, True, int(g["train_chunk"]))
        w, d = O.composite(p, z, 1e-10)
        fl, dl = O.child_losses(w, z, rays, rays[:, 10:12], rays[:, 14], divide, int(g["train_sub_nerf_test_num"]))
    k = f"train{divide}_"
    close(d, g[k + "depth"], "depth")
    close(w, g[k + "weights"], "weights")
    close(fl, g[k + "free"], "free loss")
    close(dl, g[k + "depth_loss"], "depth loss")
    assert tuple(fl.shape) == tuple(g[k + "free"].shape) == ((1,) if divide else ())
    running = torch.stack([torch.stack([P[b + ".running_mean"], P[b + ".running_var"]]) for b in O.BN])
    close(running, g[k + "running"], "running statistics")
    assert [int(P[b + ".num_batches_tracked"]) for b in O.BN] == g[k + "batches"].tolist() == [3] * 8


@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("ei", [0, 1])
def test_oracle_reproduces_inference_0525_2(method, ei, g):
    rows, other = torch.from_numpy(g["v_rows"]), torch.from_numpy(g["v_other"])
    pts, z = torch.from_numpy(g["v_pts"]), torch.from_numpy(g["v_z"])
    with torch.no_grad():
        p = O.query(oracle_params(), pts, False, 1024 * 32)
        d, w, opac, flag = O.inference_view(p, z, other, rows[:, 6:8], method, eps=float(g["view_eps"][ei]))
    k = f"view_m{method}_e{ei}_"
    close(d, g[k + "depth"], "depth")
    close(w, g[k + "weights"], "weights")
    close(opac, g[k + "opacity"], "opacity")
    assert np.array_equal(flag.numpy(), g[k + "flag"])
    assert np.isfinite(g[k + "depth"]).all()


def test_positions_are_off_the_rays(g):
    """The fixture's samples are o + d*z plus jitter: a query that rebuilds them from rays and z gives other
    weights (the oracle on the un-jittered points is far outside the 1e-6 the tests above hold)."""
    rays, z = torch.from_numpy(g["a_rays"]), torch.from_numpy(g["a_z"])
    on_ray = O.points(rays, z)
    off = np.abs(g["a_pts"] - on_ray.numpy())
    assert 0.04 < off.max() <= float(g["jitter"]) + 1e-5
    with torch.no_grad():
        w, _ = O.composite(O.query(oracle_params(), on_ray, False, 1024 * 32), z, 1e-10)
    assert np.abs(w.numpy() - g["val_weights"]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ C ABI
def test_point_entries_report_argument_errors_before_launch():
    """Null / empty / too-small-state arguments come back through pcnerf_last_error() (no GPU is touched: every
    check precedes the first launch)."""
    from nof import _hip
    L = _hip.lib()
    buf = ctypes.create_string_buffer(4096)   # a non-null stand-in pointer: never dereferenced by the checks
    a = ctypes.addressof(buf)
    params = _hip.NofParams()
    grads = _hip.NofGrads()
    pp, gp = ctypes.byref(params), ctypes.byref(grads)

    def err(rc, word):
        assert rc != 0
        assert word in L.pcnerf_last_error().decode(), L.pcnerf_last_error()

    err(L.pcnerf_nof_points_eval(None, 8, a, a, None), "null")
    err(L.pcnerf_nof_points_eval(a, 8, None, a, None), "null")
    err(L.pcnerf_nof_points_eval(a, 0, a, a, None), "empty")
    for fn in (L.pcnerf_nof_points_train_fused, L.pcnerf_nof_points_train_fused_state):
        err(fn(None, 1000, 500, pp, 0.1, 1e-5, a, 4096, a, None), "null")
        err(fn(a, 1000, 500, None, 0.1, 1e-5, a, 4096, a, None), "null")
        err(fn(a, 1000, 500, pp, 0.1, 1e-5, None, 4096, a, None), "null")
        err(fn(a, 0, 500, pp, 0.1, 1e-5, a, 4096, a, None), "empty")
        err(fn(a, 1000, 0, pp, 0.1, 1e-5, a, 4096, a, None), "empty")
        err(fn(a, 1000, 500, pp, 0.1, 1e-5, a, 16, a, None), "state buffer too small")
        err(fn(a, 1001, 500, pp, 0.1, 1e-5, a, 1 << 40, a, None), "more than 1 value per channel")
    assert L.pcnerf_nof_train_fused_bytes(1000, 500) > 16
    bw = L.pcnerf_nof_points_train_backward_remat
    err(bw(None, 1000, 500, pp, 1e-5, a, a, 4096, a, 4096, gp, None), "null")
    err(bw(a, 1000, 500, pp, 1e-5, None, a, 4096, a, 4096, gp, None), "null")
    err(bw(a, 1000, 500, pp, 1e-5, a, a, 4096, a, 4096, None, None), "null")
    err(bw(a, 0, 500, pp, 1e-5, a, a, 4096, a, 4096, gp, None), "empty")
    err(bw(a, 1000, 500, pp, 1e-5, a, a, 4096, a, 16, gp, None), "workspace too small")


# ------------------------------------------------------------------------------------------------ refusals
def _cpu_args(R=4, S=5):
    return dict(samples_xy=torch.zeros(R, S, 3), z_vals=torch.zeros(R, S), rays=torch.zeros(R, 15),
                nfc=torch.zeros(R, 2), nfp=torch.zeros(R, 2), ranges=torch.zeros(R, 1), rclass=torch.zeros(R, 1),
                other=torch.zeros(R, dtype=torch.int64))


def test_cpu_tensors_raise():
    from nof import render
    from nof.networks import Embedding, NOF_coarse
    m, emb, a = NOF_coarse().eval(), Embedding(3, 10), _cpu_args()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU path"):
            render.inference_val(m, emb, a["samples_xy"], a["rays"], a["z_vals"], a["nfc"], a["nfp"], a["ranges"],
                                 a["rclass"])
        with pytest.raises(RuntimeError, match="no CPU path"):
            render.inference_train(m, emb, a["samples_xy"], a["rays"], a["z_vals"], a["nfc"], a["nfp"], a["ranges"],
                                   a["rclass"])
        with pytest.raises(RuntimeError, match="no CPU path"):
            render.inference(m, emb, a["samples_xy"], a["z_vals"])
        with pytest.raises(RuntimeError, match="no CPU path"):
            render.inference_0525_2(m, emb, a["samples_xy"], a["z_vals"], a["other"], a["nfc"])


def test_inference_isval_true_is_not_implemented():
    from nof import render
    from nof.networks import Embedding, NOF_coarse
    a = _cpu_args()
    with pytest.raises(NotImplementedError, match="isval"):
        render.inference(NOF_coarse().eval(), Embedding(3, 10), a["samples_xy"], a["z_vals"], isval=True)


def test_query_points_eval_fake_shapes_and_schema():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from nof import _torch_ops as T
    assert "query_points_eval" in T.op_names()
    assert str(torch.ops.pcnerf.query_points_eval.default._schema).startswith("pcnerf::query_points_eval(")
    with FakeTensorMode():
        packed = torch.empty(T._packed_floats(), device="meta")
        assert torch.ops.pcnerf.query_points_eval(torch.empty(35, 3, device="meta"), packed).shape == (35,)
        assert torch.ops.pcnerf.query_points_eval(torch.empty(5, 7, 3, device="meta"), packed).shape == (5, 7)
