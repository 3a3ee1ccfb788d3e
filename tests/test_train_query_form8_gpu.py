"""Form 4 of the store-less train query in its 8-wave geometry (nof._ops.set_train_query_form(4); k_nof_eval_h3
<true, false, 8, 8> in csrc/nof_eval.hip): 8 sample blocks, 128 samples per workgroup, with the activations and the
encoding operands as the CU's whole LDS -- the BatchNorm coefficients come from L2 per layer, the sample positions and
per-sample scales sit in the activation area until layer 0, occ_out's partial sums in the encoding area.

None of that changes an operand of any fma or MFMA, so p must be BIT-equal to query geometry 0 (the 4-wave kernel, on
which the form does not act): at the sample totals where the bookkeeping changes (under a block, 127 / 128 / 129,
form 2's 112 / 113, several blocks with a short last one, and 3 rays x 128 samples where a block is one ray as in the
coarse launch), with BatchNorm chunks that are no multiple of 128 (a short last block per chunk, a block that is more
than half padding, a short last chunk) and chunks of exactly 10 blocks with different coefficients, from the point
source, and into the train backward, whose gradients must not change by a bit.  One case pins the form to the float64
oracle through the embedded entry (which also covers the `ein` source), with test_query_geometry_gpu's tolerance
(rtol 1e-4, atol 1e-6)."""
import numpy as np
import pytest
import torch

from nof import _ops
from nof import synthetic as syn
from nof.networks import NOF_coarse
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 1234
FORM = 4
# rays x samples giving totals 47, 127, 128, 129, 112, 113, 2 * 128 + 5 and 3 * 128 (one ray per block)
SHAPES = [(1, 47), (127, 1), (8, 16), (129, 1), (7, 16), (113, 1), (261, 1), (3, 128)]


def model(train=True):
    return syn.load_into(NOF_coarse(), syn.init_nof_params(SEED)).to(DEV).train(train)


def inputs(R, S, seed):
    rays = torch.from_numpy(syn.make_rays(R, seed=seed)).to(DEV)
    gen = torch.Generator().manual_seed(seed)
    z = (rays[:, 7:8].cpu() * torch.rand(R, S, generator=gen)).to(DEV).contiguous()
    return rays, z


def run_both(fn, geometry=1):
    """fn() under geometry 0 (4 waves: no form applies) and under the 8-wave geometry with form 4; selectors
    restored."""
    pg, pf = _ops.set_query_geometry(0), _ops.set_train_query_form(0)
    try:
        base = fn()
        _ops.set_query_geometry(geometry)
        _ops.set_train_query_form(FORM)
        got = fn()
    finally:
        _ops.set_query_geometry(pg)
        _ops.set_train_query_form(pf)
    return base, got


def assert_same_bits(base, got, what):
    assert torch.isfinite(base).all(), what
    assert got.shape == base.shape, what
    assert torch.equal(got.view(torch.int32), base.view(torch.int32)), \
        f"{what}: form {FORM} differs from geometry 0 in {(got != base).sum().item()} of {got.numel()} values"


@pytest.mark.parametrize("R,S", SHAPES)
def test_form8_bits_one_chunk(R, S):
    rays, z = inputs(R, S, 4)
    with torch.no_grad():
        base, got = run_both(lambda: _ops.query(model(), rays, z, R * S))
    assert_same_bits(base, got, f"train query {R}x{S}")


@pytest.mark.parametrize("chunk", [1000, 50])
def test_form8_bits_odd_chunks(chunk):
    """2,530 samples in chunks of 1,000 (8 blocks, the last 104 samples; the last chunk 530) and of 50 (one block,
    more than half of it padding; the last chunk 30)."""
    rays, z = inputs(110, 23, 5)
    with torch.no_grad():
        base, got = run_both(lambda: _ops.query(model(), rays, z, chunk))
    assert_same_bits(base, got, f"train query 2530 samples, chunk {chunk}")


def test_form8_bits_whole_blocks_two_chunks():
    """2,560 samples in chunks of 1,280: exactly 10 blocks per chunk, no padding, two sets of coefficients."""
    rays, z = inputs(160, 16, 10)
    with torch.no_grad():
        base, got = run_both(lambda: _ops.query(model(), rays, z, 1280))
    assert_same_bits(base, got, "train query 2560 samples, chunk 1280")


@pytest.mark.parametrize("n", [129, 261])
def test_form8_points_bits(n):
    rays, z = inputs(n, 1, 6)
    pts = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).contiguous().view(-1, 3)
    with torch.no_grad():
        base, got = run_both(lambda: _ops.query_points(model(), pts, n, 1, n))
    assert_same_bits(base, got, f"train point query, {n} points")


def test_form8_vs_float64_oracle():
    gen = torch.Generator().manual_seed(7)
    e = torch.rand(129, 63, generator=gen) * 2 - 1
    P = {k: v.double() if v.is_floating_point() else v.clone() for k, v in
         O.params_from_numpy(syn.init_nof_params(SEED)).items()}
    ref = O.nof_forward(P, e.double(), True).reshape(-1).numpy()
    pg, pf = _ops.set_query_geometry(1), _ops.set_train_query_form(FORM)
    try:
        with torch.no_grad():
            p = model()(e.to(DEV)).reshape(-1).cpu().numpy()
    finally:
        _ops.set_query_geometry(pg)
        _ops.set_train_query_form(pf)
    np.testing.assert_allclose(p.astype(np.float64), ref, rtol=1e-4, atol=1e-6)


def test_form8_train_backward_bits():
    """The default (rematerialising) backward after a forward under form 4: 2,530 samples in chunks of 1,000."""
    rays, z = inputs(110, 23, 8)
    chunk = 1000
    gen = torch.Generator().manual_seed(9)
    g_logit = (torch.rand(110, 23, generator=gen) * 2 - 1).to(DEV)

    def grads():
        m = model()
        state = _ops.fold_state(DEV, z.numel(), chunk)
        with torch.no_grad():
            p = _ops.query(m, rays, z, chunk, keep=state)
            return [p] + [t.clone() for t in _ops.nof_query_backward_remat(m, rays, z, chunk, g_logit, state)]

    base, got = run_both(grads, geometry=-1)   # (-1: the train query's default geometry, 8 waves)
    assert len(base) > 1 and len(got) == len(base)
    for i, (a, b) in enumerate(zip(got, base)):
        assert torch.isfinite(b).all(), i
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
            f"form {FORM}: tensor {i} (0 = p, then the gradients) differs in {(a != b).sum().item()} values"
