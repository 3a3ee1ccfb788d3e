"""The workgroup geometries of the split-fp16 fused query (nof._ops.set_query_geometry; k_nof_eval_h3 in
csrc/nof_eval.hip): 0 = two 4-wave workgroups of 48 samples per CU with a 2-slot weight ring (the form every other
test pins), bit 0 = one 8-wave workgroup of 96 samples, bit 1 = a 4-slot ring.

Every geometry runs the same products in the same order per accumulator, so p must be BIT-equal to geometry 0 -- at
the sample totals where the block bookkeeping changes (around 48 and 96, several blocks with a short last one), with
BatchNorm chunks that are no multiple of either block (short last chunk, surplus blocks per chunk), and through the
embedded-input entry.  One case per mode pins the 8-wave form to the float64 oracle as well, with the tolerance of
test_parity_gpu's float64 query tests (rtol 1e-4, atol 1e-6)."""
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
GEOMETRIES = [1, 2, 3]
# rays x samples giving totals 1, 47, 48, 49, 95, 96, 97 and 96 * 5 + 17
SHAPES = [(1, 1), (1, 47), (3, 16), (7, 7), (5, 19), (2, 48), (97, 1), (7, 71)]


def model(train):
    return syn.load_into(NOF_coarse(), syn.init_nof_params(SEED)).to(DEV).train(train)


def inputs(R, S, seed):
    rays = torch.from_numpy(syn.make_rays(R, seed=seed)).to(DEV)
    gen = torch.Generator().manual_seed(seed)
    z = (rays[:, 7:8].cpu() * torch.rand(R, S, generator=gen)).to(DEV).contiguous()
    return rays, z


def run_all(fn):
    """fn() under geometry 0 and every other geometry; the selector restored."""
    prev = _ops.set_query_geometry(0)
    try:
        base = fn()
        others = {}
        for geo in GEOMETRIES:
            _ops.set_query_geometry(geo)
            others[geo] = fn()
    finally:
        _ops.set_query_geometry(prev)
    return base, others


def assert_same_bits(base, others, what):
    assert torch.isfinite(base).all(), what
    for geo, p in others.items():
        assert p.shape == base.shape, (what, geo)
        assert torch.equal(p.view(torch.int32), base.view(torch.int32)), \
            f"{what}: geometry {geo} differs from geometry 0 in {(p != base).sum().item()} of {p.numel()} values"


@pytest.mark.parametrize("R,S", SHAPES)
def test_eval_query_bits(R, S):
    m = model(False)
    rays, z = inputs(R, S, 3)
    with torch.no_grad():
        base, others = run_all(lambda: _ops.query(m, rays, z, R * S))
    assert_same_bits(base, others, f"eval query {R}x{S}")


@pytest.mark.parametrize("R,S", SHAPES[1:])   # (BatchNorm over a single sample is undefined: no total of 1)
def test_train_query_bits_one_chunk(R, S):
    rays, z = inputs(R, S, 4)
    with torch.no_grad():
        base, others = run_all(lambda: _ops.query(model(True), rays, z, R * S))
    assert_same_bits(base, others, f"train query {R}x{S}")


@pytest.mark.parametrize("chunk", [1000, 50])
def test_train_query_bits_odd_chunks(chunk):
    """2,530 samples in chunks of 1,000 (11 blocks of 96 or 21 of 48, last chunk 530) and of 50 (one block of 96 with
    46 surplus samples' lanes, or two of 48; last chunk 30)."""
    rays, z = inputs(110, 23, 5)
    with torch.no_grad():
        base, others = run_all(lambda: _ops.query(model(True), rays, z, chunk))
    assert_same_bits(base, others, f"train query 2530 samples, chunk {chunk}")


def embedded(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(n, 63, generator=gen) * 2 - 1


def test_embedded_eval_bits():
    m = model(False)
    e = embedded(97, 6).to(DEV)
    with torch.no_grad():
        base, others = run_all(lambda: m(e))
    assert_same_bits(base, others, "embedded eval forward, 97 rows")


@pytest.mark.parametrize("train", [False, True])
def test_wide_form_vs_float64_oracle(train):
    e = embedded(97, 7)
    P = {k: v.double() if v.is_floating_point() else v.clone() for k, v in
         O.params_from_numpy(syn.init_nof_params(SEED)).items()}
    ref = O.nof_forward(P, e.double(), train).reshape(-1).numpy()
    prev = _ops.set_query_geometry(1)
    try:
        with torch.no_grad():
            p = model(train)(e.to(DEV)).reshape(-1).cpu().numpy()
    finally:
        _ops.set_query_geometry(prev)
    np.testing.assert_allclose(p.astype(np.float64), ref, rtol=1e-4, atol=1e-6)
