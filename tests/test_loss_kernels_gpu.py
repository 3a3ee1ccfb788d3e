"""k_pointwise_loss / k_pointwise_loss_bwd and k_child_range_scatter / _reduce / _bwd against the float64 torch losses
and float64 autograd (tests/sampling_f64.py; the inputs' conditions are checked without a GPU in
tests/test_sampling_f64_cpu.py).  Scalars and per-element gradients follow parity_helpers.Tally -- e_hip <=
max(4 e32, 2.4e-7), e32 the float32 torch evaluation's error --; what the branch structure decides (SmoothL1 at
|d| = 1, d = 0, empty selections, rays of no child) is asserted exactly."""
import numpy as np
import pytest
import torch

from nof import _ops

import sampling_f64 as F
from parity_helpers import Tally

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("n", F.LOSS_N)
def test_pointwise_loss_vs_f64(n):
    """mean loss and d(0.7 loss)/dpred for mse / l1 / smoothl1 at n on both sides of the single block's 1,024
    threads, with no mask, a random half, all ones, a single one at index 0 and at index n - 1, and all zero (the
    forward is NaN as torch's is, the backward all zeros).  The planted pairs -- d = 0, +-1 exactly, +-1 one float32
    ulp inside and outside -- are taken one at a time through a single-one mask and asserted exactly: the value
    0.5 d^2 or |d| - 0.5 on the right side of the strict <, the gradient d or +-1, and 0 at d = 0.
    Measured on the MI355X: worst e_hip / max(4 e32, 2.4e-7) 0.28 (n 4097, mse, no mask, gradient: e_hip 1.2e-7,
    e32 1.1e-7); every error is below the 2.4e-7 floor (loss at most 8.9e-8)."""
    pred, target, where, which = F.loss_case(n)
    a, b = pred.to(DEV), target.to(DEV)
    g_out = torch.tensor(0.7, device=DEV)
    one = torch.tensor(1.0, device=DEV)
    t = Tally("pointwise_loss")
    for kind in F.LOSS_KINDS:
        for name in F.LOSS_MASKS:
            m = F.loss_mask(name, n)
            got = _ops.pointwise_loss(a, b, kind, _dev(m)).cpu()
            grad = _ops.pointwise_loss_backward(a, b, kind, _dev(m), g_out).cpu()
            l64, g64 = F.pointwise_ref(pred, target, kind, m, torch.float64, 0.7)
            l32, g32 = F.pointwise_ref(pred, target, kind, m, torch.float32, 0.7)
            tag = f"n{n}:{kind}:{name}"
            if m is not None and not bool(m.any()):      # (the random half of one element is empty too)
                assert bool(torch.isnan(got)) and bool(torch.isnan(l32)), tag
                assert not bool(grad.any()), tag
                continue
            assert got.shape == ()
            t.check(tag, "loss", got, l32, l64)
            t.check(tag, "grad", grad, g32, g64)
            if m is not None:
                assert not bool(grad[~m].any()), tag
        for i, p in zip(where, which):
            m = torch.zeros(n, dtype=torch.bool)
            m[i] = True
            value, slope = F.planted_exact(p, kind)
            got = _ops.pointwise_loss(a, b, kind, m.to(DEV)).cpu()
            grad = _ops.pointwise_loss_backward(a, b, kind, m.to(DEV), one).cpu()
            assert np.float32(got) == value, (n, kind, F.PLANTED[p], float(got), value)
            assert np.float32(grad[i]) == slope, (n, kind, F.PLANTED[p], float(grad[i]), slope)
            assert int((grad != 0).sum()) == (0 if slope == 0 else 1)
    t.done()


@pytest.mark.parametrize("N", F.RANGE_CHILDREN)
@pytest.mark.parametrize("n", F.RANGE_N)
def test_child_range_loss_vs_f64(n, N):
    """The per-child range loss (train_kitti.py:125-142) and d(0.7 loss)/dpred: n on both sides of the scatter's
    256-thread block, N up to more children than the reduce block has threads (15,333 > 1,024), pre 10, post 0.1
    and 0.05, the three kinds; ids 0 and N + 1 (no child), k + 0.4 / k + 0.5 / k + 0.6 (child k, none, child k + 1:
    sampling_f64.child_of), children owning no ray, and one child owning every ray.  Rays of no child get gradient
    exactly 0.  Each backward runs after another forward with another workspace, and reads its own.
    Measured on the MI355X: worst e_hip / max(4 e32, 2.4e-7) 0.25 (n 257, N 15333, smoothl1: loss e_hip 6.1e-8, e32
    3.3e-8); every error is below the 2.4e-7 floor (loss and gradient at most 1.0e-7; the float32 torch loss is off
    by up to 5.2e-6)."""
    t = Tally("child_range_loss")
    g_out = torch.tensor([0.7], device=DEV)
    o_pred, o_target, o_rays = (x.to(DEV) for x in F.range_case(max(n, 300), N, "mixed", seed=5))
    for pattern in F.RANGE_PATTERNS:
        pred, target, rays = F.range_case(n, N, pattern)
        a, b, r = pred.to(DEV), target.to(DEV), rays.to(DEV)
        ids = rays[:, 9]
        for kind in F.LOSS_KINDS:
            for post in F.RANGE_POSTS:
                got, ws = _ops.child_range_loss(a, b, r, N, kind, F.RANGE_PRE, post)
                other, ws_other = _ops.child_range_loss(o_pred, o_target, o_rays, N, kind, F.RANGE_PRE, post)
                assert ws.data_ptr() != ws_other.data_ptr()
                grad = _ops.child_range_loss_backward(a, b, r, N, kind, F.RANGE_PRE, post, ws, g_out).cpu()
                l64, g64, slot = F.range_ref(pred, target, ids, N, kind, F.RANGE_PRE, post, torch.float64, 0.7)
                l32, g32, _ = F.range_ref(pred, target, ids, N, kind, F.RANGE_PRE, post, torch.float32, 0.7)
                tag = f"n{n}N{N}:{pattern}:{kind}:{post}"
                assert got.shape == (1,)
                assert not bool(grad[slot < 0].any()), tag
                if not bool((slot >= 0).any()):
                    assert float(got) == 0.0, tag
                    continue
                t.check(tag, "loss", got.cpu().reshape(()), l32, l64)
                t.check(tag, "grad", grad[None], g32[None], g64[None])
    t.done()
