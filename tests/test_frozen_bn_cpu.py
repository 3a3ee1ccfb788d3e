"""Frozen-BatchNorm training, the parts that need no GPU: the pseudo-sample identity behind the eval-mode parameter
backward (tests/frozen_bn_ref.py against per-sample torch float64 autograd of the oracle's eval network), and the new
surface -- the C entries declared, exported and bound, the four operators' schemas and fake shapes, the host-side
argument checks that run before any launch."""
import ctypes
import os
import re

import numpy as np
import torch

import frozen_bn_ref as FR
from conftest import REPO
from nof import _hip
from nof import _torch_ops as T
from oracle import ref_cpu as O

NEW_ENTRIES = ("pcnerf_nof_eval_pgrad_workspace_bytes", "pcnerf_nof_query_eval_param_backward",
               "pcnerf_nof_points_eval_param_backward", "pcnerf_nof_forward_eval_param_backward",
               "pcnerf_nof_eval_gmoments_rays", "pcnerf_nof_eval_gmoments_points",
               "pcnerf_nof_eval_gmoments_embedded", "pcnerf_nof_eval_param_grads")
NEW_OPS = ("eval_gmoments_rays", "eval_gmoments_points", "eval_gmoments_embedded", "eval_param_grads")


def test_pseudo_sample_identity_against_per_sample_autograd():
    """2,000 encoded random positions with |x| up to 25 m, a random g: each of the 34 tensors within 1e-12 max|ref|
    (float64 summation over 2,000 terms with margin; 5e-15 measured), and the Linear-bias and BatchNorm-shift
    gradients are NOT at noise level -- gradcheck.noise_level_grads is a train-mode fact only."""
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.uniform(-25.0, 25.0, size=(2000, 3)))
    E = O.embed(x).numpy()
    g = rng.standard_normal(2000)
    P = FR.params64(1234)
    ref = FR.autograd_param_grads(P, E, g)
    got = FR.param_grads(P, FR.moments(E, g))
    worst = 0.0
    for k in FR.GRAD_KEYS:
        assert got[k].shape == ref[k].shape, k
        scale = np.abs(ref[k]).max()
        err = np.abs(got[k] - ref[k]).max()
        worst = max(worst, err / scale)
        assert err <= 1e-12 * scale, (k, err, scale)
    print("worst err / max|ref| over the 34 tensors:", worst)
    for lin, bn in zip(O.LIN, O.BN):
        scale = np.abs(ref[bn + ".weight"]).max()
        assert np.abs(ref[lin + ".bias"]).max() > 1e-3 * scale, lin
        assert np.abs(ref[bn + ".bias"]).max() > 1e-3 * scale, bn


def test_header_declares_and_library_exports_the_entries():
    txt = open(os.path.join(REPO, "include", "pcnerf_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _hip.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _hip.exported_symbols() and hasattr(L, name), name
    assert L.pcnerf_nof_eval_pgrad_workspace_bytes.restype == ctypes.c_size_t


def test_workspace_size_is_a_function_of_the_sample_count():
    L = _hip.lib()
    ws = L.pcnerf_nof_eval_pgrad_workspace_bytes
    assert ws(0) == ws(1) == ws(256) == (64 + 64) * 8           # one workgroup's partials after the moments
    assert ws(257) == (64 + 2 * 64) * 8                         # four 64-sample tiles per workgroup
    assert ws(65536 * 384) == ws(1 << 40) == (64 + 1024 * 64) * 8   # capped at 1024 workgroups


def test_host_side_checks_run_before_any_launch():
    """Zero samples succeed without a launch; negative sizes, null pointers and a short workspace are refused with a
    message (none of these calls reaches the device)."""
    L = _hip.lib()
    one = ctypes.c_void_p(64)   # a non-null address that is never dereferenced: every call below fails earlier
    assert L.pcnerf_nof_eval_gmoments_rays(None, 0, 8, None, 64, None, None, 0, None, None) == 0
    assert L.pcnerf_nof_eval_gmoments_points(None, 0, None, None, 0, None, None) == 0
    assert L.pcnerf_nof_eval_gmoments_embedded(None, 0, None, None, None, 0, None, None) == 0
    assert L.pcnerf_nof_query_eval_param_backward(None, 0, 8, None, 64, None, 1e-5, None, None, 0, None, None) == 0
    assert L.pcnerf_nof_points_eval_param_backward(None, 0, None, 1e-5, None, None, 0, None, None) == 0
    assert L.pcnerf_nof_forward_eval_param_backward(None, 0, None, 1e-5, None, None, None, 0, None, None) == 0
    assert L.pcnerf_nof_eval_gmoments_rays(None, -1, 8, None, 64, None, None, 0, None, None) != 0
    assert b"n_rays" in L.pcnerf_last_error()
    assert L.pcnerf_nof_eval_gmoments_rays(None, 0, 5, None, 64, None, None, 0, None, None) != 0
    assert b"ray_stride" in L.pcnerf_last_error()
    assert L.pcnerf_nof_eval_gmoments_rays(None, 0, 8, None, 0, None, None, 0, None, None) != 0
    assert b"n_samples" in L.pcnerf_last_error()
    assert L.pcnerf_nof_eval_gmoments_rays(None, 3, 8, None, 64, None, None, 0, None, None) != 0
    assert b"null" in L.pcnerf_last_error()
    assert L.pcnerf_nof_eval_gmoments_rays(one, 3, 8, one, 64, one, one, 8, one, None) != 0
    assert b"workspace too small" in L.pcnerf_last_error()
    assert L.pcnerf_nof_eval_gmoments_points(None, -1, None, None, 0, None, None) != 0
    assert b"n < 0" in L.pcnerf_last_error()
    assert L.pcnerf_nof_eval_gmoments_points(one, 5, one, one, 8, one, None) != 0
    assert b"workspace too small" in L.pcnerf_last_error()
    assert L.pcnerf_nof_eval_gmoments_embedded(None, 5, None, None, None, 0, None, None) != 0
    assert b"null" in L.pcnerf_last_error()
    assert L.pcnerf_nof_eval_param_grads(None, 1e-5, None, None, None) != 0
    assert b"null" in L.pcnerf_last_error()
    assert L.pcnerf_nof_eval_param_grads(ctypes.byref(_hip.NofParams()), 1e-5, one, ctypes.byref(_hip.NofGrads()),
                                         None) != 0
    assert b"null parameter pointer" in L.pcnerf_last_error()
    assert L.pcnerf_nof_points_eval_param_backward(one, 5, ctypes.byref(_hip.NofParams()), 1e-5, one, one, 8,
                                                   ctypes.byref(_hip.NofGrads()), None) != 0
    assert b"workspace too small" in L.pcnerf_last_error()
    assert L.pcnerf_nof_forward_eval_param_backward(one, 5, ctypes.byref(_hip.NofParams()), 1e-5, None, one, one,
                                                    1 << 20, ctypes.byref(_hip.NofGrads()), None) != 0
    assert b"null" in L.pcnerf_last_error()


def test_operators_registered_with_schemas():
    for name in NEW_OPS:
        assert name in T.op_names()
        schema = str(getattr(torch.ops.pcnerf, name).default._schema)
        assert schema.startswith(f"pcnerf::{name}("), schema
    s = str(torch.ops.pcnerf.eval_param_grads.default._schema)
    assert "Tensor[] params" in s and s.endswith("-> Tensor[]"), s


def test_operators_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    P = torch.ops.pcnerf
    with FakeTensorMode():
        m = P.eval_gmoments_rays(torch.empty(5, 15, device="meta"), torch.empty(5, 48, device="meta"),
                                 torch.empty(5, 48, device="meta"))
        assert m.shape == (64,) and m.dtype == torch.float64
        m = P.eval_gmoments_points(torch.empty(5, 7, 3, device="meta"), torch.empty(5, 7, device="meta"))
        assert m.shape == (64,) and m.dtype == torch.float64
        m = P.eval_gmoments_embedded(torch.empty(35, 63, device="meta"), torch.empty(35, device="meta"))
        assert m.shape == (64,) and m.dtype == torch.float64
        params = [torch.empty(s, device="meta") for s in T._param_shapes()]
        grads = P.eval_param_grads(params, m, 1e-5)
        assert len(grads) == 34 and all(t.dtype == torch.float32 for t in grads)
        want = T._param_shapes()[:32] + T._param_shapes()[48:]
        assert [tuple(t.shape) for t in grads] == want


def test_grad_order_matches_the_module():
    """pcnerf::eval_param_grads returns the gradients in nof._ops.grad_params order, the reference's state_dict names
    of tests/frozen_bn_ref.GRAD_KEYS."""
    from nof import _ops
    from nof.networks import NOF_coarse
    m = NOF_coarse()
    named = dict(m.named_parameters())
    assert [tuple(named[k].shape) for k in FR.GRAD_KEYS] == [tuple(t.shape) for t in _ops.grad_params(m)]
    assert all(named[k] is t for k, t in zip(FR.GRAD_KEYS, _ops.grad_params(m)))
