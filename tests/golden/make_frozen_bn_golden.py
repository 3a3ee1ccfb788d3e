"""Generate tests/golden/frozen_bn_grads.npz by importing the reference (``/root/reference/nof``) on CPU.

Run in the build container only (the reference does not travel to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_frozen_bn_golden.py

What it pins: the PARAMETER gradients of the reference's own ``inference_train`` (render.py:38-163) under torch
autograd with the module in EVAL mode (frozen BatchNorm): ``NOF_coarse().eval()`` with
``nof.synthetic.init_nof_params(1234)``, every parameter requiring grad, the scalar loss
``sum(cot * depth) + c1 * child_free_loss + c2 * child_depth_loss`` with a fixed random ``cot``, ``c1``, ``c2``.  The
positions are those of ``make_inference_golden.py``: ``o + d*z`` of synthetic scan-range rays plus uniform +-0.05 m of
jitter.  Cases ``<name>/``:

    a  (37, 50)   child losses on, plain branch, noise_std 0
    b  (5, 384)   child losses off
    d  (37, 50)   child losses on, divide branch (sub_nerf_test_num 32), noise_std 1 with the randn draw recorded

Per case: the inputs (rays, pts, z, cot, c1, c2, noise), the float32 forward (depth, free, depth_loss) and three
gradient runs -- float32 at one torch thread, float32 at four (``alt``), float64 (``module.double()`` on the same
float32-rounded inputs).  Tensors of <= 512 entries are stored in full, weight matrices as 2,048 fixed entries
(``@idx``, shared by every case and run, stored once per tensor under ``idx/``) + ``@val`` + ``@norm``.  To keep the
file small the second and third runs are stored relative to the first: ``ulp:<key>`` = int32 bit-pattern difference
alt - ref (lossless), ``res:<key>`` = float32(f64 - ref) (the float64 run to ~2^-24 of its DISTANCE from the float32
one, i.e. ~1e-14 of its value); tests/test_frozen_bn_gpu.load_golden rebuilds gradcheck's ``alt:`` / ``f64:`` keys.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

# our synthetic-data module, loaded by path (our package is also called ``nof``)
_spec = importlib.util.spec_from_file_location("pcnerf_synthetic",
                                               os.path.join(REPO, "pc-nerf_amd", "nof", "synthetic.py"))
syn = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(syn)

sys.path.insert(0, REF)
import nof.render as R  # noqa: E402  (the reference)
from nof.networks import Embedding, NOF_coarse  # noqa: E402

SEED = 1234
JITTER = 0.05
NOISE_SEED = 77
SUB = 32
# name, rays, samples, ray seed, use_child_nerf_loss, use_child_nerf_divide, noise_std
CASES = (("a", 37, 50, 41, 1, 0, 0), ("b", 5, 384, 43, 0, 0, 0), ("d", 37, 50, 47, 1, 1, 1))


def lin_z(near, far, n):
    s = torch.linspace(0, 1, n).expand(near.shape[0], n)   # render.py:430-432
    return near * (1 - s) + far * s


def segmented_z(rays, S, ratio):
    sp = int(S * (1 - ratio))
    zp = lin_z(rays[:, 6:7], rays[:, 7:8], sp)
    zc = lin_z(rays[:, 10:11], rays[:, 11:12], S - sp)
    return torch.sort(torch.cat([zp, zc], -1), -1)[0]


def jittered(rows, z, rng):
    pts = rows[:, None, 0:3] + rows[:, None, 3:6] * z[..., None]   # render.py:458
    jit = rng.uniform(-JITTER, JITTER, size=tuple(pts.shape)).astype(np.float32)
    return (pts + torch.from_numpy(jit)).contiguous()


def grad_run(dtype, threads, pts, rays, z, cot, c1, c2, losses, divide, noise_std):
    torch.set_num_threads(threads)
    m = syn.load_into(NOF_coarse(), syn.init_nof_params(SEED)).eval().to(dtype)
    for t in m.parameters():
        t.requires_grad_(True)
    r = rays.to(dtype)
    torch.manual_seed(NOISE_SEED)   # the reference draws randn (float32) inside, whatever noise_std is
    fl, dl, d, w = R.inference_train(m, Embedding(3, 10), pts.to(dtype), r, z.to(dtype), r[:, 10:12], r[:, 12:14],
                                     r[:, -1:], r[:, 8:9], noise_std=noise_std, sub_nerf_test_num=SUB,
                                     use_child_nerf_divide=divide, use_child_nerf_loss=losses)
    total = (d * cot.to(dtype)).sum() + c1 * fl.sum() + c2 * dl.sum()
    total.backward()
    running = torch.stack([torch.stack([b.running_mean, b.running_var]) for b in m.modules()
                           if isinstance(b, torch.nn.BatchNorm1d)])
    assert torch.equal(running.float(), torch.stack(
        [torch.stack([b.running_mean, b.running_var]) for b in
         syn.load_into(NOF_coarse(), syn.init_nof_params(SEED)).modules() if isinstance(b, torch.nn.BatchNorm1d)]))
    torch.set_num_threads(1)
    return (d.detach(), fl.detach(), dl.detach()), {k: p.grad.detach().numpy() for k, p in m.named_parameters()}


def main():
    out = {"seed": SEED, "jitter": JITTER, "sub_nerf_test_num": SUB}
    rng = np.random.default_rng(2026)
    idx = {}
    for k, p in NOF_coarse().named_parameters():
        if p.numel() > 512:
            idx[k] = np.sort(rng.choice(p.numel(), size=2048, replace=False)).astype(np.int32)
            out["idx/" + k] = idx[k]
    for name, n_rays, S, seed, losses, divide, noise_std in CASES:
        rays = torch.from_numpy(syn.make_rays(n_rays, seed=seed))
        z = segmented_z(rays, S, 0.2)
        pts = jittered(rays, z, rng)
        cot = torch.from_numpy(rng.standard_normal(n_rays).astype(np.float32))
        c1, c2 = (float(np.float32(v)) for v in rng.uniform(5.0, 15.0, size=2))
        args = (pts, rays, z, cot, c1, c2, losses, divide, noise_std)
        (d32, fl32, dl32), g32 = grad_run(torch.float32, 1, *args)
        _, galt = grad_run(torch.float32, 4, *args)
        (d64, _, _), g64 = grad_run(torch.float64, 1, *args)
        np.testing.assert_allclose(d32.numpy(), d64.numpy(), rtol=1e-3)
        k = name + "/"
        out.update({k + "rays": rays.numpy(), k + "pts": pts.numpy(), k + "z": z.numpy(), k + "cot": cot.numpy(),
                    k + "c1": c1, k + "c2": c2, k + "losses": losses, k + "divide": divide, k + "noise_std": noise_std,
                    k + "depth": d32.numpy(), k + "free": fl32.numpy(), k + "depth_loss": dl32.numpy()})
        if noise_std:
            torch.manual_seed(NOISE_SEED)
            out[k + "noise"] = torch.randn(n_rays, S).numpy()   # the draw inference_train took (render.py:57)
        worst = 0.0
        for key, ref in g32.items():
            assert ref.dtype == np.float32 and g64[key].dtype == np.float64 and np.isfinite(g64[key]).all()
            assert np.abs(g64[key]).max() > 0, key
            worst = max(worst, float(np.abs(ref - g64[key]).max() / np.abs(g64[key]).max()))
            sel = (lambda a: a.reshape(-1)[idx[key]]) if key in idx else (lambda a: a)
            sfx = "@val" if key in idx else ""
            r = np.ascontiguousarray(sel(ref))
            out[k + key + sfx] = r
            out["ulp:" + k + key + sfx] = (np.ascontiguousarray(sel(galt[key])).view(np.int32).astype(np.int64)
                                           - r.view(np.int32).astype(np.int64)).astype(np.int32)
            out["res:" + k + key + sfx] = (sel(g64[key]) - r.astype(np.float64)).astype(np.float32)
            if key in idx:
                out[k + key + "@norm"] = np.linalg.norm(ref.astype(np.float64))
                out["alt:" + k + key + "@norm"] = np.linalg.norm(galt[key].astype(np.float64))
                out["f64:" + k + key + "@norm"] = np.linalg.norm(g64[key])
        print(name, "worst max|g32 - g64| / max|g64| over the 34 tensors:", worst)
    path = os.path.join(HERE, "frozen_bn_grads.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
