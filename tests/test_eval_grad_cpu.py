"""Eval-mode geometry gradients, the parts that need no GPU: the three new operators' schemas and fake shapes, the two
ABI entries (present, and their host-side size checks run before any launch), and the oracle route of
tests/eval_grad_ref.py pinned to the reference's own autograd (tests/golden/eval_grads.npz)."""
import numpy as np
import pytest
import torch

from conftest import golden
from eval_grad_ref import points_grad
from gradcheck import check_grads_elem
from nof import _hip
from nof import _torch_ops as T

NEW_OPS = ("fold_eval", "points_grad_eval", "rays_grad_eval")
SEED = 1234


def test_new_operators_registered_with_schemas():
    for name in NEW_OPS:
        assert name in T.op_names()
        schema = str(getattr(torch.ops.pcnerf, name).default._schema)
        assert schema.startswith(f"pcnerf::{name}("), schema
    assert "Tensor[] params" in str(torch.ops.pcnerf.fold_eval.default._schema)


def test_new_operators_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    P = torch.ops.pcnerf
    with FakeTensorMode():
        params = [torch.empty(s, device="meta") for s in T._param_shapes()]
        fold = P.fold_eval(params)
        assert fold.shape == (64,) and fold.dtype == torch.float64
        g = P.points_grad_eval(torch.empty(35, 3, device="meta"), torch.empty(35, device="meta"), fold)
        assert g.shape == (35, 3) and g.dtype == torch.float32
        g = P.points_grad_eval(torch.empty(5, 7, 3, device="meta"), torch.empty(5, 7, device="meta"), fold)
        assert g.shape == (5, 7, 3)
        g = P.rays_grad_eval(torch.empty(5, 15, device="meta"), torch.empty(5, 48, device="meta"),
                             torch.empty(5, 48, device="meta"), fold)
        assert g.shape == (5, 6) and g.dtype == torch.float32


def test_abi_symbols_and_host_side_checks():
    """Both entries are exported with the bound signatures; empty inputs succeed without a launch and bad sizes are
    refused on the host (none of these calls reaches the device)."""
    assert {"pcnerf_nof_points_eval_backward", "pcnerf_nof_query_eval_backward"} <= set(_hip.exported_symbols())
    L = _hip.lib()
    assert L.pcnerf_nof_points_eval_backward(None, 0, None, None, None, None) == 0
    assert L.pcnerf_nof_query_eval_backward(None, 0, 8, None, 64, None, None, None, None) == 0
    assert L.pcnerf_nof_points_eval_backward(None, -1, None, None, None, None) != 0
    assert b"n < 0" in L.pcnerf_last_error()
    assert L.pcnerf_nof_points_eval_backward(None, 5, None, None, None, None) != 0
    assert b"null" in L.pcnerf_last_error()
    assert L.pcnerf_nof_query_eval_backward(None, 0, 5, None, 64, None, None, None, None) != 0
    assert b"ray_stride" in L.pcnerf_last_error()
    assert L.pcnerf_nof_query_eval_backward(None, 0, 8, None, 0, None, None, None, None) != 0
    assert b"n_samples" in L.pcnerf_last_error()
    assert L.pcnerf_nof_query_eval_backward(None, -2, 8, None, 64, None, None, None, None) != 0
    assert b"n_rays" in L.pcnerf_last_error()
    assert L.pcnerf_nof_query_eval_backward(None, 3, 8, None, 64, None, None, None, None) != 0
    assert b"null" in L.pcnerf_last_error()


@pytest.mark.parametrize("case", ["a", "b", "n"])
def test_oracle_route_matches_reference_autograd(case):
    """The oracle's float32 d/d samples_xy (ref_cpu embed / nof_forward / composite under torch autograd) in place of
    the HIP path, under the GPU tests' own check against the reference fixture: the route test_eval_grad_gpu uses
    for render_rays_val is the reference's arithmetic."""
    g = golden("eval_grads")
    k = case + "/"
    pts, z, cot = (torch.from_numpy(g[k + n]) for n in ("pts", "z", "cot"))
    noise = torch.from_numpy(g[k + "noise"]) * float(g[k + "noise_std"]) if k + "noise" in g else None
    assert (k + "noise" in g) == (case == "n")
    got = points_grad(SEED, pts, z, cot, torch.float32, noise)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(g[k + "samples_xy"].shape)
    check_grads_elem(lambda _: got.numpy(), ["samples_xy"], g, k, "eval_grad_oracle_" + case)
    # and in float64 it reproduces the reference's float64 run to float64 rounding
    got64 = points_grad(SEED, pts, z, cot, torch.float64, noise).numpy()
    ref64 = g["f64:" + k + "samples_xy"]
    assert np.abs(got64 - ref64).max() <= 1e-9 * np.abs(ref64).max()


def test_fixture_shapes_and_magnitudes():
    g = golden("eval_grads")
    assert tuple(g["a/pts"].shape) == (37, 50, 3) and tuple(g["b/pts"].shape) == (5, 384, 3)
    assert tuple(g["n/noise"].shape) == (37, 50) and float(g["n/noise_std"]) == 1.0
    for c in "abn":
        assert g[c + "/samples_xy"].dtype == np.float32 and g["f64:" + c + "/samples_xy"].dtype == np.float64
        assert 20.0 < np.abs(g[c + "/pts"]).max() < 80.0   # scan-range positions (inference_fns.npz: 25.5 m)
