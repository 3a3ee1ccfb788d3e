"""Generate tests/golden/inference_fns.npz by importing the reference (``/root/reference/nof``) on CPU.

Run in the build container only (the reference does not travel to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_inference_golden.py

What it pins: the four module-level helpers of the reference's ``nof/render.py`` that take MATERIALISED sample
positions -- ``inference_val`` (:13), ``inference_train`` (:38), ``inference`` (:166) and ``inference_0525_2`` (:229)
-- on positions that lie on no ray: ``o + d*z`` plus uniform +-0.05 m of jitter, so an implementation that ignores
``samples_xy`` (or rebuilds it from rays and z) fails; sin(512 x) makes the two outputs unrelated.  Stored with the
outputs: each function's ``inspect.signature`` parameter names and defaults (JSON strings) and every input.

No shim is applied (no ``sample_pdf`` is involved); the reference's ``print``s are swallowed.  All cases use the
weights ``nof.synthetic.init_nof_params(1234)`` and ``noise_std=0``.
"""
import contextlib
import importlib.util
import inspect
import io
import json
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
FUNCTIONS = ("inference_val", "inference_train", "inference", "inference_0525_2")


def model(train):
    return syn.load_into(NOF_coarse(), syn.init_nof_params(SEED)).train(train)


def running_stats(m):
    out = [torch.stack([mod.running_mean, mod.running_var]) for mod in m.modules()
           if isinstance(mod, torch.nn.BatchNorm1d)]
    return torch.stack(out).numpy()


def batches_tracked(m):
    return np.array([int(mod.num_batches_tracked) for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm1d)])


def t(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def signature_json(fn):
    """[[name, has_default, default], ...] in declaration order."""
    out = []
    for name, p in inspect.signature(fn).parameters.items():
        has = p.default is not inspect.Parameter.empty
        out.append([name, has, p.default if has else None])
    return json.dumps(out)


def lin_z(near, far, n):
    s = torch.linspace(0, 1, n).expand(near.shape[0], n)   # render.py:430-432
    return near * (1 - s) + far * s


def segmented_z(rays, S, ratio):
    """render.py:429-442: int(S * (1 - ratio)) parent samples plus the rest on the child bounds, merged by sort."""
    sp = int(S * (1 - ratio))
    zp = lin_z(rays[:, 6:7], rays[:, 7:8], sp)
    zc = lin_z(rays[:, 10:11], rays[:, 11:12], S - sp)
    return torch.sort(torch.cat([zp, zc], -1), -1)[0]


def jittered(rows, z, rng):
    pts = rows[:, None, 0:3] + rows[:, None, 3:6] * z[..., None]   # render.py:458
    jit = rng.uniform(-JITTER, JITTER, size=tuple(pts.shape)).astype(np.float32)
    return (pts + torch.from_numpy(jit)).contiguous()


def main():
    out = {"seed": SEED, "jitter": JITTER}
    for name in FUNCTIONS:
        out["sig_" + name] = signature_json(getattr(R, name))
    emb = Embedding(3, 10)
    rng = np.random.default_rng(2024)

    # ---- inference_val / inference (eval mode) and inference_train (train mode): 40 rays x 37 samples
    rays_np = syn.make_rays(40, seed=41)
    rays = torch.from_numpy(rays_np)
    z = segmented_z(rays, 37, 0.2)
    pts = jittered(rays, z, rng)
    nfc, nfp = rays[:, 10:12].view(-1, 2), rays[:, 12:14].view(-1, 2)
    ranges, rclass = rays[:, -1].view(-1, 1), rays[:, 8].view(-1, 1)
    out.update(a_rays=rays_np, a_z=t(z), a_pts=t(pts))
    with torch.no_grad():
        d, w = R.inference_val(model(False), emb, pts, rays, z, nfc, nfp, ranges, rclass, noise_std=0)
        out.update(val_depth=t(d), val_weights=t(w))
        d, w, o = R.inference(model(False), emb, pts, z, noise_std=0)
        out.update(inf_depth=t(d), inf_weights=t(w), inf_opacity=t(o))
        out["train_chunk"] = 500          # 1480 samples: 3 BatchNorm chunks, the last 480
        out["train_sub_nerf_test_num"] = 32
        for div in (0, 1):
            m = model(True)
            fl, dl, d, w = R.inference_train(m, emb, pts, rays, z, nfc, nfp, ranges, rclass, chunk=500, noise_std=0,
                                             sub_nerf_test_num=32, use_child_nerf_divide=div, use_child_nerf_loss=1)
            out.update({f"train{div}_free": t(fl), f"train{div}_depth_loss": t(dl), f"train{div}_depth": t(d),
                        f"train{div}_weights": t(w), f"train{div}_running": running_stats(m),
                        f"train{div}_batches": batches_tracked(m)})

    # ---- inference_0525_2 (eval mode): 82 two-step rows in 24 groups, 96 samples on the parent bounds
    rows_np, other_np, _ = syn.make_view_rows(24, seed=5)
    rows, other = torch.from_numpy(rows_np), torch.from_numpy(other_np)
    zv = lin_z(rows[:, 9:10], rows[:, 10:11], 96)        # render.py:622-628
    pv = jittered(rows, zv, rng)
    nfcv = rows[:, 6:8].view(-1, 2)
    out.update(v_rows=rows_np, v_other=other_np, v_z=t(zv), v_pts=t(pv))
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        for method in (0, 2):
            for ei, eps in enumerate((0, 1e-10)):
                d, w, o, f = R.inference_0525_2(model(False), emb, pv, zv, other, nfcv, noise_std=0, epsilon=eps,
                                                depth_inference_method=method)
                assert bool(torch.isfinite(d).all()), (method, eps)
                k = f"view_m{method}_e{ei}_"
                out.update({k + "depth": t(d), k + "weights": t(w), k + "opacity": t(o), k + "flag": t(f)})
    out["view_eps"] = np.array([0.0, 1e-10])

    path = os.path.join(HERE, "inference_fns.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
