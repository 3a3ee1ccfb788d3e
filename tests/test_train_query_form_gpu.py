"""The forms of the store-less train query in its 8-wave geometry (nof._ops.set_train_query_form; k_nof_eval_h3 in
csrc/nof_eval.hip): 0 = 6 sample blocks (96 samples per workgroup), 2 = 7 sample blocks (112 samples, the default).
FORMS lists every built form (form 1, a half-skewed schedule of form 0, passed these tests, measured slower and is
not built: HISTORY.md); the reference is query geometry 0, the 4-wave kernel, which the form does not act on.

Every form runs the same products in the same order per accumulator, so p must be BIT-equal to query geometry 0
-- at the sample totals where the bookkeeping changes (half a block of 96, the blocks of 96 and 112, several
blocks with a short last one), with BatchNorm chunks that are no multiple of a block (a short last chunk, surplus
blocks per chunk, a block that is more than half padding), from the point source, and into the train backward,
whose gradients must not change by a bit (the forward state it consumes is the same).  One case per form pins it to
the float64 oracle through the embedded entry, with test_query_geometry_gpu's tolerance (rtol 1e-4, atol 1e-6)."""
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
FORMS = [0, 2]
# rays x samples giving totals 47, 48, 49, 95, 96, 97, 111, 112, 113, 2 * 96 + 17 and 2 * 112 + 5
SHAPES = [(1, 47), (3, 16), (7, 7), (5, 19), (2, 48), (97, 1), (3, 37), (7, 16), (113, 1), (11, 19), (229, 1)]


def model(train=True):
    return syn.load_into(NOF_coarse(), syn.init_nof_params(SEED)).to(DEV).train(train)


def inputs(R, S, seed):
    rays = torch.from_numpy(syn.make_rays(R, seed=seed)).to(DEV)
    gen = torch.Generator().manual_seed(seed)
    z = (rays[:, 7:8].cpu() * torch.rand(R, S, generator=gen)).to(DEV).contiguous()
    return rays, z


def run_all(fn):
    """fn() under geometry 0 (4 waves: no form applies), and under the 8-wave geometry with every form; selectors
    restored."""
    pg, pf = _ops.set_query_geometry(0), _ops.set_train_query_form(0)
    try:
        base = fn()
        _ops.set_query_geometry(1)
        others = {}
        for form in FORMS:
            _ops.set_train_query_form(form)
            others[form] = fn()
    finally:
        _ops.set_query_geometry(pg)
        _ops.set_train_query_form(pf)
    return base, others


def assert_same_bits(base, others, what):
    assert torch.isfinite(base).all(), what
    for form, p in others.items():
        assert p.shape == base.shape, (what, form)
        assert torch.equal(p.view(torch.int32), base.view(torch.int32)), \
            f"{what}: form {form} differs from geometry 0 in {(p != base).sum().item()} of {p.numel()} values"


@pytest.mark.parametrize("R,S", SHAPES)
def test_train_query_bits_one_chunk(R, S):
    rays, z = inputs(R, S, 4)
    with torch.no_grad():
        base, others = run_all(lambda: _ops.query(model(), rays, z, R * S))
    assert_same_bits(base, others, f"train query {R}x{S}")


@pytest.mark.parametrize("chunk", [1000, 50])
def test_train_query_bits_odd_chunks(chunk):
    """2,530 samples in chunks of 1,000 (11 blocks of 96 or 9 of 112, the last chunk 530) and of 50 (one block, more
    than half of it padding; the last chunk 30)."""
    rays, z = inputs(110, 23, 5)
    with torch.no_grad():
        base, others = run_all(lambda: _ops.query(model(), rays, z, chunk))
    assert_same_bits(base, others, f"train query 2530 samples, chunk {chunk}")


@pytest.mark.parametrize("n", [97, 113])
def test_train_points_bits(n):
    rays, z = inputs(n, 1, 6)
    pts = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).contiguous().view(-1, 3)
    with torch.no_grad():
        base, others = run_all(lambda: _ops.query_points(model(), pts, n, 1, n))
    assert_same_bits(base, others, f"train point query, {n} points")


def embedded(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(n, 63, generator=gen) * 2 - 1


@pytest.mark.parametrize("form", FORMS)
def test_form_vs_float64_oracle(form):
    e = embedded(97, 7)
    P = {k: v.double() if v.is_floating_point() else v.clone() for k, v in
         O.params_from_numpy(syn.init_nof_params(SEED)).items()}
    ref = O.nof_forward(P, e.double(), True).reshape(-1).numpy()
    pg, pf = _ops.set_query_geometry(1), _ops.set_train_query_form(form)
    try:
        with torch.no_grad():
            p = model()(e.to(DEV)).reshape(-1).cpu().numpy()
    finally:
        _ops.set_query_geometry(pg)
        _ops.set_train_query_form(pf)
    np.testing.assert_allclose(p.astype(np.float64), ref, rtol=1e-4, atol=1e-6)


def test_train_backward_bits():
    """The default (rematerialising) backward after a forward under each form: 2,530 samples in chunks of 1,000."""
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

    pg = _ops.set_query_geometry(0)
    pf = _ops.set_train_query_form(0)
    try:
        base = grads()
        _ops.set_query_geometry(-1)   # (the train query's default geometry, 8 waves)
        others = {}
        for form in FORMS:
            _ops.set_train_query_form(form)
            others[form] = grads()
    finally:
        _ops.set_query_geometry(pg)
        _ops.set_train_query_form(pf)
    assert len(base) > 1
    for form, got in others.items():
        assert len(got) == len(base)
        for i, (a, b) in enumerate(zip(got, base)):
            assert torch.isfinite(b).all(), i
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                f"form {form}: tensor {i} (0 = p, then the gradients) differs in {(a != b).sum().item()} values"
