"""Times batched pose refinement: 2,048 beams x 64 + 128 samples x 20 evaluations on seeded random frozen networks,
starts from pose_grid(identity, 0.6, 0.1, 0.3, 0.1) (x slowest), ``min_sumw = 0`` and ``xi_tol = 0`` so that every
pose makes every evaluation on either route:

  (a) batched    -- nof.registration.refine_poses_fold for P in ``--batched-poses`` (1, 4, 64, 1024): per evaluation
                    one fused launch, a reduction and the per-pose solver kernel, no host synchronisation in between;
  (b) sequential -- nof.registration.register_scan_fold once per pose for P in ``--sequential-poses`` (1, 4, 16): what
                    the package offered before (scan_rays, four operator launches, gn_normal_eq, a 30-double read-back
                    and a host-side solve per evaluation) -- the baseline;
  (c) localize   -- nof.localization.localize_scan_fold over ``--hypotheses`` (1,024) hypotheses with ``top_k = 4``,
                    refine="sequential" against refine="batched".

All routes alternate inside every repeat after the warm-up rounds and every timing ends in a device synchronise.
Reported per route: median ms and spread (max - min) over ``--repeats`` repeats.  A route counts as faster only when
the gap exceeds the sum of the two spreads (the ``*_faster_than_*`` flags).  As a sanity check the batched and the
sequential refinement of the same starts are compared (evaluations made, final cost to 1e-6 of the first cost); the
script exits non-zero otherwise.  Not measured here: other beam and sample counts, scans with misses (a stopped pose
leaves the batch early), and anything under a profiler.  It needs a GPU and refuses to run without one.

    python pc-nerf_amd/time_refine.py --out profiles/refine.json
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


def faster(a, b):
    """a faster than b: the gap of the medians exceeds the sum of the two spreads."""
    return bool(b["median_ms"] - a["median_ms"] > a["spread_ms"] + b["spread_ms"])


def measure(a):
    fold_c, fold_f = frozen_fold(NOF_coarse, 1234), frozen_fold(NOF_fine, 5678)
    rays = torch.from_numpy(syn.make_rays(a.beams, seed=0))
    pts = (rays[:, 3:6] * rays[:, 14:15]).contiguous().cuda()   # the scan: the rays' returns seen from the origin
    grid = L.pose_grid(torch.eye(4, dtype=torch.float64), 0.6, 0.1, 0.3, 0.1)
    need = max(max(a.batched_poses), max(a.sequential_poses), a.hypotheses)
    assert grid.shape[0] >= need, f"the grid has {grid.shape[0]} hypotheses"
    # starts spread through the grid (not its first corner alone)
    order = torch.arange(grid.shape[0]).reshape(-1, 7).t().reshape(-1)
    starts = grid[order].contiguous()
    box = (syn.PARENT_LO, syn.PARENT_HI)
    kw = dict(N_samples=a.samples, N_importance=a.importance, huber_delta=a.huber_delta, min_sumw=0.0, near=NEAR)
    rkw = dict(iters=a.iters, damping=1e-6, xi_tol=0.0, **kw)
    keep = {}

    def batched(n):
        def run():
            keep["a", n] = G.refine_poses_fold(fold_c, fold_f, pts, starts[:n], *box, **rkw)
        return run

    def sequential(n):
        def run():
            keep["b", n] = [G.register_scan_fold(fold_c, fold_f, pts, starts[k], *box, **rkw) for k in range(n)]
        return run

    def localize(mode):
        def run():
            keep["c", mode] = L.localize_scan_fold(fold_c, fold_f, pts, grid[:a.hypotheses], *box, top_k=a.top_k,
                                                   refine_iters=a.iters, refine=mode, **kw)
        return run

    routes = {}
    for n in a.batched_poses:
        routes[f"batched_P{n}"] = batched(n)
    for n in a.sequential_poses:
        routes[f"sequential_P{n}"] = sequential(n)
    for mode in ("sequential", "batched"):
        routes[f"localize_{mode}"] = localize(mode)
    with torch.no_grad():
        for _ in range(a.warmup):
            for fn in routes.values():
                fn()
        ms = {k: [] for k in routes}
        for _ in range(a.repeats):   # the routes alternate inside every repeat
            for k, fn in routes.items():
                ms[k].append(timed(fn))
    out = {k: stats(v) for k, v in ms.items()}
    for n in a.batched_poses:
        out[f"batched_P{n}"]["ms_per_pose"] = out[f"batched_P{n}"]["median_ms"] / n
        r = keep["a", n]
        out[f"batched_P{n}"]["status_counts"] = [int((r.status == s).sum()) for s in range(4)]
        out[f"batched_P{n}"]["evaluations_min_max"] = [int(r.iterations.min()), int(r.iterations.max())]
    for n in a.sequential_poses:
        out[f"sequential_P{n}"]["ms_per_pose"] = out[f"sequential_P{n}"]["median_ms"] / n
        if n in a.batched_poses:
            out[f"batched_P{n}_faster_than_sequential_P{n}"] = faster(out[f"batched_P{n}"], out[f"sequential_P{n}"])
            out[f"batched_P{n}_over_sequential_P{n}"] = (out[f"batched_P{n}"]["median_ms"]
                                                         / out[f"sequential_P{n}"]["median_ms"])
    out["localize_batched_faster_than_sequential"] = faster(out["localize_batched"], out["localize_sequential"])
    out["localize_batched_over_sequential"] = (out["localize_batched"]["median_ms"]
                                               / out["localize_sequential"]["median_ms"])
    # the two refinements of the same starts
    n = min(max(a.sequential_poses), max(a.batched_poses))
    ra, rb = keep["a", max(a.batched_poses)], keep["b", max(a.sequential_poses)]
    cost = ra.cost.cpu()
    first = ra.eval_costs[:, 0].cpu()
    diff = max(abs(float(cost[k]) - rb[k].costs[-1]) / abs(float(first[k])) for k in range(n))
    same_evals = all(int(ra.iterations[k]) == rb[k].iterations for k in range(n))
    out["final_cost_max_diff_over_first_cost"] = diff
    out["evaluations_equal"] = bool(same_evals)
    ca, cb = keep["c", "batched"], keep["c", "sequential"]
    out["localize_index"] = [ca.index, cb.index]
    out["localize_pose_distance"] = list(L.pose_distance(ca.pose, cb.pose))
    out["routes_agree"] = bool(same_evals and diff <= 1e-6 and ca.index == cb.index)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--batched-poses", type=int, nargs="+", default=[1, 4, 64, 1024])
    ap.add_argument("--sequential-poses", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--top-k", type=int, default=4)
    ap.add_argument("--beams", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--importance", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--huber-delta", type=float, default=0.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("time_refine.py needs a ROCm GPU; there is no CPU path and nothing is measured without one",
              file=sys.stderr)
        return 2
    res = dict(device=torch.cuda.get_device_name(0), beams=a.beams, samples=[a.samples, a.importance], iters=a.iters,
               hypotheses=a.hypotheses, top_k=a.top_k, huber_delta=a.huber_delta, min_sumw=0.0, xi_tol=0.0,
               repeats=a.repeats, warmup=a.warmup)
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
