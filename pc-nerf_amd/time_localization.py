"""Times pose-hypothesis scoring: 1,024 hypotheses x 2,048 beams x 64 + 128 samples on seeded random frozen networks
(the first 1,024 poses of pose_grid(identity, 0.6, 0.1, 0.3, 0.1): 13 x 13 x 7 = 1,183 hypotheses, x slowest):

  (a) fused    -- nof.localization.score_poses_fold: one launch of the whole two-pass render plus the per-pose sums;
  (b) composed -- what the package offered before it, in chunks of ``--chunk`` poses: scan_rays per pose, the rows
                  concatenated, render_scan (sample_coarse, render_jac_fold, resample, render_jac_fold) without the
                  Jacobian, then a float64 torch reduction per pose with the same validity rule.

The routes alternate inside every repeat after the warm-up rounds and every timing ends in a device synchronise.
Reported per route: median ms and spread (max - min) over ``--repeats`` repeats, and the peak device memory above the
inputs (torch's allocator, one extra untimed run each).  A difference counts only when it exceeds the sum of the two
spreads ("fused_faster_than_composed").  The two routes' scores are compared as a sanity check (n_valid equal, costs
to 1e-6 of the cost: they render the same depths up to the order of the float64 sums); the script exits non-zero
otherwise.  It needs a GPU and refuses to run without one.

    python pc-nerf_amd/time_localization.py --out profiles/localization.json
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

from nof import localization as L  # noqa: E402
from nof import registration as G  # noqa: E402
from nof import synthetic as syn  # noqa: E402
from nof import _torch_ops as T  # noqa: E402
from nof.networks import NOF_coarse, NOF_fine  # noqa: E402

P = torch.ops.pcnerf
NEAR = 0.05


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(median_ms=statistics.median(ms), spread_ms=max(ms) - min(ms), repeats_ms=ms)


def frozen_fold(cls, seed):
    m = syn.load_into(cls(), syn.init_nof_params(seed)).cuda().eval().requires_grad_(False)
    with torch.no_grad():
        return P.fold_eval(T.eval_params(m))


def composed(fold_c, fold_f, pts, poses, chunk, S, I, delta, min_sumw):
    """(P, 4) float64 scores by the composed route."""
    R = pts.shape[0]
    out = []
    for c0 in range(0, poses.shape[0], chunk):
        rows, rngs = zip(*(G.scan_rays(pts, T_, syn.PARENT_LO, syn.PARENT_HI, NEAR) for T_ in poses[c0:c0 + chunk]))
        depth, sumw, _ = G.render_scan(fold_c, fold_f, torch.cat(rows), S, I, False)
        tgt = torch.cat(rngs)
        usable = torch.isfinite(tgt) & (tgt > 0)
        valid = usable & (sumw.double() >= min_sumw) & torch.isfinite(depth)
        r = torch.where(valid, depth.double() - tgt.double(), torch.zeros((), dtype=torch.float64, device=pts.device))
        ar = r.abs()
        rho = 0.5 * r * r
        if delta > 0:
            rho = torch.where(ar > delta, delta * (ar - 0.5 * delta), rho)
        hit = torch.where(usable, sumw.double(), torch.zeros((), dtype=torch.float64, device=pts.device))
        out.append(torch.stack([v.reshape(-1, R).sum(1) for v in (rho, valid.double(), ar, hit)], 1))
    return torch.cat(out)


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def measure(a):
    fold_c, fold_f = frozen_fold(NOF_coarse, 1234), frozen_fold(NOF_fine, 5678)
    rays = torch.from_numpy(syn.make_rays(a.beams, seed=0))
    pts = (rays[:, 3:6] * rays[:, 14:15]).contiguous().cuda()   # the scan: the rays' returns seen from the origin
    grid = L.pose_grid(torch.eye(4, dtype=torch.float64), 0.6, 0.1, 0.3, 0.1)
    poses = grid[:a.poses].contiguous()
    assert poses.shape[0] == a.poses, f"the grid has {grid.shape[0]} hypotheses"
    kw = dict(N_samples=a.samples, N_importance=a.importance, huber_delta=a.huber_delta, min_sumw=a.min_sumw,
              near=NEAR)
    keep = {}

    def fused():
        keep["a"] = L.score_poses_fold(fold_c, fold_f, pts, poses, syn.PARENT_LO, syn.PARENT_HI, **kw)

    def fused_depth():
        keep["ad"] = L.score_poses_fold(fold_c, fold_f, pts, poses, syn.PARENT_LO, syn.PARENT_HI, want_depth=True,
                                        **kw)

    def comp():
        keep["b"] = composed(fold_c, fold_f, pts, poses, a.chunk, a.samples, a.importance, a.huber_delta, a.min_sumw)

    routes = {"fused": fused, "fused_with_depth": fused_depth, "composed": comp}
    with torch.no_grad():
        for _ in range(a.warmup):
            for fn in routes.values():
                fn()
        ms = {k: [] for k in routes}
        for _ in range(a.repeats):   # the routes alternate inside every repeat
            for k, fn in routes.items():
                ms[k].append(timed(fn))
        out = {k: stats(v) for k, v in ms.items()}
        sa, sb = keep["a"], keep["b"].cpu()
        keep.clear()
        for k, fn in routes.items():
            out[k]["peak_bytes_above_inputs"] = peak_above_inputs(fn)
            keep.clear()
    fa, fb = out["fused"], out["composed"]
    out["fused_over_composed"] = fa["median_ms"] / fb["median_ms"]
    out["fused_faster_than_composed"] = bool(fb["median_ms"] - fa["median_ms"] > fa["spread_ms"] + fb["spread_ms"])
    out["samples_per_call"] = a.poses * a.beams * (a.samples + a.importance)
    out["n_valid_equal"] = bool(torch.equal(sa.n_valid.cpu(), sb[:, 1].round().long()))
    out["n_valid_min_max"] = [int(sa.n_valid.min()), int(sa.n_valid.max())]
    cost = sa.cost.cpu()
    out["cost_max_rel_diff"] = float(((cost - sb[:, 0]).abs() / sb[:, 0].abs().clamp(min=1e-300)).max())
    out["routes_agree"] = bool(out["n_valid_equal"] and out["cost_max_rel_diff"] <= 1e-6)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--poses", type=int, default=1024)
    ap.add_argument("--beams", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--importance", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=32, help="poses per chunk of the composed route")
    ap.add_argument("--huber-delta", type=float, default=0.0)
    ap.add_argument("--min-sumw", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("time_localization.py needs a ROCm GPU; there is no CPU path and nothing is measured without one",
              file=sys.stderr)
        return 2
    res = dict(device=torch.cuda.get_device_name(0), poses=a.poses, beams=a.beams, samples=[a.samples, a.importance],
               chunk=a.chunk, huber_delta=a.huber_delta, min_sumw=a.min_sumw, repeats=a.repeats, warmup=a.warmup)
    res.update(measure(a))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    return 0 if res["routes_agree"] else 1


if __name__ == "__main__":
    sys.exit(main())
