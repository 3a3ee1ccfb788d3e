"""Times the fused render-with-Jacobian pass of the registration against the composed route it replaces, at BASELINE
config 2's fine-pass shapes capped to the fused kernel's limit (65,536 rays x 384 samples, frozen eval-mode NOF_fine):

  (a) fused         -- pcnerf::render_jac_fold with the Jacobian (one launch: depth, sumw, jac6);
  (b) composed_fold -- the operators the package had before it, with the eval fold switched on (set only inside this
                       script): eval query -> composite -> composite_backward(grad_depth = 1) -> rays_grad_eval;
  (c) composed      -- the same with the default eval math;
  (d) iteration     -- one full register_scan iteration on 65,536 rays at 128 + 256 samples (scan rays, both passes,
                       the normal equations, the read-back and the host solve).

The routes alternate inside every repeat after the warm-up rounds and every timing ends in a device synchronise.
Reported per route: median ms and spread (max - min) over ``--repeats`` repeats.  (a) counts as faster than (b) only
if its median is below (b)'s by more than the sum of the two spreads ("fused_faster_than_composed_fold").  (a) and (b)
evaluate the same p (one logit expression) and composite it in float64 rounded once (a) or with the float32 roundings
of render.py:51-61 (b); their depths are held to the per-kernel tests' rule against a float64 compositing of that p
(torch, on the device): e_a <= max(4 e_b, 2.4e-7), e = max |depth - depth64| / |depth64|; the script exits non-zero
otherwise.  It needs a GPU and refuses to run without one.

    python pc-nerf_amd/time_registration.py --out profiles/registration.json
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

from nof import _ops  # noqa: E402
from nof import registration as G  # noqa: E402
from nof import render as R  # noqa: E402
from nof import synthetic as syn  # noqa: E402
from nof import _torch_ops as T  # noqa: E402
from nof.networks import NOF_coarse, NOF_fine  # noqa: E402

P = torch.ops.pcnerf
FLOOR = 2.4e-7   # two float32 ulps for the final rounding (tests/parity_helpers.py)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(median_ms=statistics.median(ms), spread_ms=max(ms) - min(ms), repeats_ms=ms)


def frozen(cls, seed):
    m = syn.load_into(cls(), syn.init_nof_params(seed)).cuda().eval()
    return m.requires_grad_(False)


def measure(rays, z, chunk, repeats, warmup):
    coarse, fine = frozen(NOF_coarse, 1234), frozen(NOF_fine, 5678)
    with torch.no_grad():
        fold = P.fold_eval(T.eval_params(fine))
    ones = torch.ones(z.shape[0], device=z.device)
    pts = (rays[:, 3:6] * rays[:, 14:15]).contiguous()   # the scan: the rays' returns seen from the origin
    eye = torch.eye(4, dtype=torch.float64)
    keep = {}

    def fused():
        keep["a"] = P.render_jac_fold(rays, z, fold, R.EPSILON, False, True)

    def composed(tag, use_fold):
        prev = _ops.set_eval_fold(use_fold)
        try:
            p = R._query(fine, rays, z, chunk)
        finally:
            _ops.set_eval_fold(prev)
        depth = P.composite(p, z, None, 0.0, R.EPSILON, None, 10, 11, 14, False)[1]
        g = _ops.composite_backward(p, z, None, 0.0, R.EPSILON, None, 0, ones, None, None)
        keep[tag] = (depth, P.rays_grad_eval(rays, z, g, fold), p)

    def iteration():
        keep["d"] = G.register_scan(coarse, fine, pts, eye, syn.PARENT_LO, syn.PARENT_HI, N_samples=128,
                                    N_importance=256, iters=1, min_sumw=0.0)

    routes = {"fused": fused, "composed_fold": lambda: composed("b", True), "composed": lambda: composed("c", False),
              "iteration": iteration}
    with torch.no_grad():
        for _ in range(warmup):
            for fn in routes.values():
                fn()
        ms = {k: [] for k in routes}
        for _ in range(repeats):   # the routes alternate inside every repeat
            for k, fn in routes.items():
                ms[k].append(timed(fn))
    out = {k: stats(v) for k, v in ms.items()}
    # float64 compositing (render.py:51-61) of (b)'s p: the reference both depths are held against
    p64, z64 = keep["b"][2].double(), z.double()
    trans = torch.cumprod(torch.cat([torch.ones_like(p64[:, :1]), 1 - p64], -1), -1)[:, :-1]
    w64 = trans * p64
    d64 = (w64 * z64).sum(-1) / (w64.sum(-1) + R.EPSILON)
    del p64, z64, trans, w64
    rel = lambda d: float(((d.double() - d64).abs() / d64.abs().clamp(min=1e-30)).max())   # noqa: E731
    out["depth_err_fused"], out["depth_err_composed_fold"] = rel(keep["a"][0]), rel(keep["b"][0])
    out["depth_err_composed"] = rel(keep["c"][0])   # (the full network's p, not the fold's)
    out["depth_within_rule"] = bool(out["depth_err_fused"] <= max(4 * out["depth_err_composed_fold"], FLOOR))
    out["depth_bits_equal_fused_vs_composed_fold"] = bool(torch.equal(keep["a"][0], keep["b"][0]))
    ja, jb = keep["a"][3].double(), keep["b"][1].double()
    out["jac6_max_diff_over_max_fused_vs_composed_fold"] = float((ja - jb).abs().max() / jb.abs().max())
    a, b = out["fused"], out["composed_fold"]
    out["fused_over_composed_fold"] = a["median_ms"] / b["median_ms"]
    out["fused_over_composed"] = a["median_ms"] / out["composed"]["median_ms"]
    out["fused_faster_than_composed_fold"] = bool(b["median_ms"] - a["median_ms"] > a["spread_ms"] + b["spread_ms"])
    out["iteration_n_valid"] = int(keep["d"].n_valid)
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
        print("time_registration.py needs a ROCm GPU; there is no CPU path and nothing is measured without one",
              file=sys.stderr)
        return 2
    rays = torch.from_numpy(syn.make_rays(a.rays, seed=0)).cuda()
    gen = torch.Generator().manual_seed(0)
    s = torch.sort(torch.rand(a.rays, a.samples, generator=gen), -1)[0].cuda()
    z = (rays[:, 6:7] * (1 - s) + rays[:, 7:8] * s).contiguous()
    del s
    res = dict(device=torch.cuda.get_device_name(0), rays=a.rays, samples=a.samples, chunk=a.chunk,
               total_samples=a.rays * a.samples, repeats=a.repeats, warmup=a.warmup,
               eval_math=_ops.get_eval_math(), eval_fold=_ops.eval_fold_enabled(), iteration_samples=[128, 256])
    res.update(measure(rays, z, a.chunk, a.repeats, a.warmup))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    return 0 if res["depth_within_rule"] else 1


if __name__ == "__main__":
    sys.exit(main())
