"""Times the eval-mode render pass with and without its geometry gradient, at BASELINE config 2's fine pass (65,536 rays
x 384 samples, frozen eval-mode NOF_fine, noise_std = 0):

  (a) forward -- the eval query + compositing under no_grad (what render_rays_val runs per pass);
  (b) rays    -- the same pass as nof._autograd.EvalPass with rays requiring grad, then depth.backward(): the
                 compositing backward + pcnerf_nof_query_eval_backward (gradient to origins and directions);
  (c) points  -- nof._autograd.EvalPassPoints on pts = o + d*z computed beforehand, then depth.backward(): the
                 compositing backward + pcnerf_nof_points_eval_backward (gradient to every sample position).

The three alternate inside every repeat and every timing ends in a device synchronise.  Reported per route: median ms
and spread (max - min) over ``--repeats`` repeats; and the same way, on their own, the pass's kernels (query,
compositing backward, the two gradient kernels, the fold).  (b) and (c) must reproduce (a)'s depth bits; the script
exits non-zero if they do not.  It needs a GPU and refuses to run without one.

    python pc-nerf_amd/time_eval_grad.py --out profiles/eval_grad.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from nof import _autograd, _ops  # noqa: E402
from nof import render as R  # noqa: E402
from nof import synthetic as syn  # noqa: E402
from nof import _torch_ops as T  # noqa: E402
from nof.networks import NOF_fine  # noqa: E402

P = torch.ops.pcnerf


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(median_ms=statistics.median(ms), spread_ms=max(ms) - min(ms), repeats_ms=ms)


def measure(rays, z, pts, chunk, repeats, warmup):
    model = syn.load_into(NOF_fine(), syn.init_nof_params(5678)).cuda().eval()
    for t in model.parameters():
        t.requires_grad_(False)
    flat = pts.view(-1, 3)
    cot = torch.randn(z.shape[0], generator=torch.Generator().manual_seed(1)).cuda()
    keep = {}

    def forward():
        with torch.no_grad():
            p = R._query(model, rays, z, chunk)
            keep["a"] = P.composite(p, z, None, 0.0, R.EPSILON, None, 10, 11, 14, False)[1]

    def to_rays():
        r = rays.detach().requires_grad_(True)
        _, depth = _autograd.EvalPass.apply(R._query, model, r, z, None, 0.0, R.EPSILON, chunk, False)
        depth.backward(cot)
        keep["b"], keep["g_rays"] = depth.detach(), r.grad

    def to_points():
        x = flat.detach().requires_grad_(True)
        _, depth = _autograd.EvalPassPoints.apply(R._query_points, model, x, z, None, 0.0, R.EPSILON, chunk)
        depth.backward(cot)
        keep["c"], keep["g_pts"] = depth.detach(), x.grad

    routes = {"forward": forward, "to_rays": to_rays, "to_points": to_points}
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(keep["a"], keep["b"]) and torch.equal(keep["a"], keep["c"]))
    # the ray form against the summed point form (float64 sums of the float32 per-sample gradients)
    gp = keep["g_pts"].view(*z.shape, 3).double()
    want = torch.cat([gp.sum(1), (z.double()[..., None] * gp).sum(1)], 1)
    ray_vs_points = float(((keep["g_rays"][:, :6].double() - want).abs().max() / want.abs().max()))
    del gp, want

    # the pass's kernels on their own
    with torch.no_grad():
        p = R._query(model, rays, z, chunk)
        fold = P.fold_eval(T.eval_params(model))
        g_logit = _ops.composite_backward(p, z, None, 0.0, R.EPSILON, None, 0, cot, None, None)
    kernels = {"query": lambda: R._query(model, rays, z, chunk),
               "composite": lambda: P.composite(p, z, None, 0.0, R.EPSILON, None, 10, 11, 14, False),
               "fold_eval": lambda: P.fold_eval(T.eval_params(model)),
               "composite_backward": lambda: _ops.composite_backward(p, z, None, 0.0, R.EPSILON, None, 0, cot, None,
                                                                     None),
               "rays_grad_eval": lambda: P.rays_grad_eval(rays, z, g_logit, fold),
               "points_grad_eval": lambda: P.points_grad_eval(flat, g_logit.view(-1), fold)}
    for _ in range(warmup):
        for fn in list(routes.values()) + list(kernels.values()):
            fn()
    ms = {k: [] for k in list(routes) + list(kernels)}
    for _ in range(repeats):   # the routes alternate inside every repeat
        for k, fn in routes.items():
            ms[k].append(timed(fn))
        with torch.no_grad():
            for k, fn in kernels.items():
                ms[k].append(timed(fn))
    out = {k: stats(v) for k, v in ms.items()}
    fwd = out["forward"]["median_ms"]
    out["depth_bits_equal"] = same
    out["rays_vs_summed_points_max_rel_diff"] = ray_vs_points
    for k in ("to_rays", "to_points"):
        out[k + "_backward_ms"] = out[k]["median_ms"] - fwd
        out[k + "_backward_over_forward"] = (out[k]["median_ms"] - fwd) / fwd
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=384)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("time_eval_grad.py needs a ROCm GPU; there is no CPU path and nothing is measured without one",
              file=sys.stderr)
        return 2
    rays = torch.from_numpy(syn.make_rays(a.rays, seed=0)).cuda()
    gen = torch.Generator().manual_seed(0)
    s = torch.sort(torch.rand(a.rays, a.samples, generator=gen), -1)[0].cuda()
    z = (rays[:, 6:7] * (1 - s) + rays[:, 7:8] * s).contiguous()
    pts = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).contiguous()   # two ops: the kernel's roundings
    del s
    res = dict(device=torch.cuda.get_device_name(0), rays=a.rays, samples=a.samples, chunk=a.chunk,
               total_samples=a.rays * a.samples, repeats=a.repeats, warmup=a.warmup,
               eval_math=_ops.get_eval_math(), eval_fold=_ops.eval_fold_enabled())
    res.update(measure(rays, z, pts, a.chunk, a.repeats, a.warmup))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    return 0 if res["depth_bits_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
