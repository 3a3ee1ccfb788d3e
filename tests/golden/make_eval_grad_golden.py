"""Generate tests/golden/eval_grads.npz by importing the reference (``/root/reference/nof``) on CPU.

Run in the build container only (the reference does not travel to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval_grad_golden.py

What it pins: ``d/d samples_xy`` of the reference's own ``inference_val`` (render.py:13-36) under torch autograd, the
eval-mode module ``nof.synthetic.init_nof_params(1234)``, a fixed random cotangent on ``depth_final``.  The positions
are those of ``make_inference_golden.py``: ``o + d*z`` of synthetic scan-range rays (nof.synthetic.make_rays, |x| up
to ~25 m) plus uniform +-0.05 m of jitter, so they lie on no ray.  Per case ``<name>/``:

    pts (R, S, 3), z (R, S), cot (R,)            the inputs (float32) and the cotangent of depth_final
    depth (R,)                                   the float32 forward
    samples_xy (R, S, 3) float32                 the reference's float32 gradient
    f64:<name>/samples_xy (R, S, 3) float64      the same call in float64 on the SAME float32-rounded positions, depths
                                                 and weights (module.double())
    noise (R, S)                                 (noise case) the randn draws the reference took, recovered by seeding
                                                 torch's generator before the call and drawing again

Cases: ``a`` (37, 50) and ``b`` (5, 384) with noise_std = 0; ``n`` (37, 50) with noise_std = 1.
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

torch.set_num_threads(1)
SEED = 1234
JITTER = 0.05
NOISE_SEED = 77
CASES = (("a", 37, 50, 41, 0), ("b", 5, 384, 43, 0), ("n", 37, 50, 47, 1))   # name, rays, samples, ray seed, noise_std


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


def grad_run(dtype, pts, rays, z, cot, noise_std):
    m = syn.load_into(NOF_coarse(), syn.init_nof_params(SEED)).eval().to(dtype)
    for t in m.parameters():
        t.requires_grad_(False)
    x = pts.to(dtype).clone().requires_grad_(True)
    r = rays.to(dtype)
    torch.manual_seed(NOISE_SEED)   # the reference draws randn (float32) inside, whatever noise_std is
    d, w = R.inference_val(m, Embedding(3, 10), x, r, z.to(dtype), r[:, 10:12], r[:, 12:14], r[:, -1:], r[:, 8:9],
                           noise_std=noise_std)
    (d * cot.to(dtype)).sum().backward()
    return d.detach(), x.grad.detach()


def main():
    out = {"seed": SEED, "jitter": JITTER}
    rng = np.random.default_rng(2025)
    for name, n_rays, S, seed, noise_std in CASES:
        rays = torch.from_numpy(syn.make_rays(n_rays, seed=seed))
        z = segmented_z(rays, S, 0.2)
        pts = jittered(rays, z, rng)
        cot = torch.from_numpy(rng.standard_normal(n_rays).astype(np.float32))
        d32, g32 = grad_run(torch.float32, pts, rays, z, cot, noise_std)
        d64, g64 = grad_run(torch.float64, pts, rays, z, cot, noise_std)
        assert g32.dtype == torch.float32 and g64.dtype == torch.float64
        assert bool(torch.isfinite(g64).all()) and float(g64.abs().max()) > 0
        np.testing.assert_allclose(d32.numpy(), d64.numpy(), rtol=1e-3)
        k = name + "/"
        out.update({k + "pts": pts.numpy(), k + "z": z.numpy(), k + "cot": cot.numpy(), k + "depth": d32.numpy(),
                    k + "noise_std": noise_std, k + "samples_xy": g32.numpy(), "f64:" + k + "samples_xy": g64.numpy()})
        if noise_std:
            torch.manual_seed(NOISE_SEED)
            out[k + "noise"] = torch.randn(n_rays, S).numpy()   # the draw inference_val took (render.py:30)
        print(name, "max |g|", float(g64.abs().max()), "max |g32 - g64|", float((g32.double() - g64).abs().max()))
    path = os.path.join(HERE, "eval_grads.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
