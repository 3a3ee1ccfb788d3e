"""Times localisation against a map of blocks and the device particle-filter step, on seeded random frozen networks
(no trained checkpoints are present): 4 blocks side by side along x, each the parent box of nof.synthetic with its own
pair of networks; the scan is 2,048 beams x 64 + 128 samples; the poses are pose_grid(identity, 0.6, 0.1, 0.3, 0.1)
shifted into the blocks, interleaved (pose p lies in block p mod 4).

  1. scoring   -- (a) map: nof.localization.score_poses_map with the block ids on the device: one launch plus the
                  reduction; (b) split: the parent commit's route, four nof.localization.score_poses_fold calls on the
                  host-split subsets and a scatter of the four results (the index lists are prepared outside the timing).
  2. step      -- one nof.mcl.ParticleFilter.step at each of ``--particles``; (b) composed: the same step from
                  apply_twists, a torch block assignment read back to split on the host, score_poses_fold per block, and
                  torch for the weights (float64 logsumexp), the effective sample size (read back for the decision),
                  cumsum, searchsorted and the gather.  Both start every repeat from the same fresh particle set.
  3. headline  -- with ``--parent-tree DIR`` (a checkout of the parent commit with its library built):
                  ``python bench.py --gpus 1 --steps 20 --warmup 5`` in DIR and in this tree, alternating, as fresh child
                  processes: ``--bench-rounds`` times parent, this, then the parent once more.

Protocol (time_localization.py's): the routes alternate inside every repeat after the warm-up rounds, every timing
ends in a device synchronise, results are median ms and spread (max - min) over ``--repeats`` repeats, and a route counts
as faster only when the difference of the medians exceeds the sum of the two spreads.  The routes' scores are compared
(equal bits) as a sanity check; the script exits non-zero otherwise.  It needs a GPU and refuses to run without one.

    python pc-nerf_amd/time_mcl.py --out profiles/mcl.json [--parent-tree DIR] [--only scoring,step,headline]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from nof import localization as L  # noqa: E402
from nof import mcl as M  # noqa: E402
from nof import registration as G  # noqa: E402
from nof import synthetic as syn  # noqa: E402
from nof import _torch_ops as T  # noqa: E402
from nof.networks import NOF_coarse, NOF_fine  # noqa: E402

P = torch.ops.pcnerf
NEAR = 0.05
BLOCKS = 4


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(median_ms=statistics.median(ms), spread_ms=max(ms) - min(ms), repeats_ms=ms)


def faster(a, b):
    """a is faster than b by the rule: the difference of the medians exceeds the sum of the spreads."""
    return bool(b["median_ms"] - a["median_ms"] > a["spread_ms"] + b["spread_ms"])


def frozen_fold(cls, seed):
    m = syn.load_into(cls(), syn.init_nof_params(seed)).cuda().eval().requires_grad_(False)
    with torch.no_grad():
        return P.fold_eval(T.eval_params(m))


def build_map():
    lo, hi = [float(v) for v in syn.PARENT_LO], [float(v) for v in syn.PARENT_HI]
    width = hi[0] - lo[0]
    boxes = [[lo[0] + b * width, lo[1], lo[2], hi[0] + b * width, hi[1], hi[2]] for b in range(BLOCKS)]
    fc = torch.stack([frozen_fold(NOF_coarse, 1234 + b) for b in range(BLOCKS)])
    ff = torch.stack([frozen_fold(NOF_fine, 5678 + b) for b in range(BLOCKS)])
    return L.BlockMap(fc, ff, torch.tensor(boxes, dtype=torch.float64).cuda()), boxes, width


def interleaved_poses(n, width):
    """(n, 4, 4) host poses: grid pose p // 4 shifted into block p mod 4."""
    grid = L.pose_grid(torch.eye(4, dtype=torch.float64), 0.6, 0.1, 0.3, 0.1)
    per = n // BLOCKS
    assert n % BLOCKS == 0 and per <= grid.shape[0], f"the grid has {grid.shape[0]} hypotheses"
    poses = grid[:per].repeat_interleave(BLOCKS, 0).clone()
    poses[:, 0, 3] += width * (torch.arange(n) % BLOCKS).double()
    return poses.contiguous()


def scan(beams):
    rays = torch.from_numpy(syn.make_rays(beams, seed=0))
    return (rays[:, 3:6] * rays[:, 14:15]).contiguous().cuda()


# ----------------------------------------------------------------------------------------------- 1. scoring
def measure_scoring(a, bm, boxes, width, pts, kw):
    poses = interleaved_poses(a.poses, width)
    ids_host = (torch.arange(a.poses) % BLOCKS).to(torch.int32)
    ids = ids_host.cuda()
    index = [torch.nonzero(ids_host == b).flatten() for b in range(BLOCKS)]   # prepared outside the timing
    index_dev = [i.cuda() for i in index]
    subsets = [poses[i].contiguous() for i in index]
    keep = {}

    def fused():
        keep["a"] = L.score_poses_map(bm, pts, poses, ids, **kw)

    def fused_assign():
        keep["aa"] = L.score_poses_map(bm, pts, poses, None, **kw)

    def split():
        cost = torch.empty(a.poses, dtype=torch.float64, device="cuda")
        n_valid = torch.empty(a.poses, dtype=torch.int64, device="cuda")
        for b in range(BLOCKS):
            s = L.score_poses_fold(bm.folds_c[b], bm.folds_f[b], pts, subsets[b], boxes[b][:3], boxes[b][3:], **kw)
            cost[index_dev[b]] = s.cost
            n_valid[index_dev[b]] = s.n_valid
        keep["b"] = (cost, n_valid)

    routes = {"map": fused, "map_with_assign_blocks": fused_assign, "split": split}
    with torch.no_grad():
        for _ in range(a.warmup):
            for fn in routes.values():
                fn()
        ms = {k: [] for k in routes}
        for _ in range(a.repeats):   # the routes alternate inside every repeat
            for k, fn in routes.items():
                ms[k].append(timed(fn))
    out = {k: stats(v) for k, v in ms.items()}
    out["map_over_split"] = out["map"]["median_ms"] / out["split"]["median_ms"]
    out["map_faster_than_split"] = faster(out["map"], out["split"])
    out["split_faster_than_map"] = faster(out["split"], out["map"])
    out["samples_per_call"] = a.poses * a.beams * (a.samples + a.importance)
    sa, (cost, n_valid) = keep["a"], keep["b"]
    out["n_valid_min_max"] = [int(sa.n_valid.min()), int(sa.n_valid.max())]
    out["routes_agree"] = bool(torch.equal(sa.cost, cost) and torch.equal(sa.n_valid, n_valid)
                               and torch.equal(keep["aa"].cost, cost))
    return out


# ----------------------------------------------------------------------------------------------- 2. the filter step
def composed_step(bm, boxes, pts, rows, logw, twist, sigma, gen, beta, miss, ess_frac, kw):
    """One particle-filter step from the parent commit's operators and torch -> (rows, logw)."""
    n, dev = rows.shape[0], rows.device
    xi = torch.randn((n, 6), dtype=torch.float64, device=dev, generator=gen) * sigma + twist
    rows = P.se3_apply(xi.contiguous(), rows)
    t = rows[:, 9:12]
    lo, hi = bm.boxes[:, :3], bm.boxes[:, 3:]
    inside = ((t[:, None, :] >= lo[None]) & (t[:, None, :] <= hi[None])).all(-1)
    clear = torch.minimum(t[:, None, :] - lo[None], hi[None] - t[:, None, :]).min(-1)[0]
    clear = torch.where(inside, clear, torch.full_like(clear, -1.0))
    ids = torch.where(inside.any(1), clear.argmax(1), torch.full((n,), -1, device=dev))
    ids_host = ids.cpu()                                     # the host has to split
    poses = G._rows_to_poses(rows)
    cost = torch.zeros(n, dtype=torch.float64, device=dev)
    n_valid = torch.zeros(n, dtype=torch.float64, device=dev)
    for b in range(BLOCKS):
        i = torch.nonzero(ids_host == b).flatten().to(dev)
        if i.numel() == 0:
            continue
        s = L.score_poses_fold(bm.folds_c[b], bm.folds_f[b], pts, poses[i], boxes[b][:3], boxes[b][3:], **kw)
        cost[i] = s.cost
        n_valid[i] = s.n_valid.double()
    rng = torch.linalg.norm(pts.double(), dim=-1).float()
    n_usable = (torch.isfinite(rng) & (rng > 0)).sum().double()
    mean = (cost + miss * (n_usable - n_valid)) / n_usable
    lw = logw - beta * mean
    lw = torch.where((ids < 0) | ~torch.isfinite(mean), torch.full_like(lw, -float("inf")), lw)
    lw = lw - torch.logsumexp(lw, 0)
    w = lw.exp()
    ess = 1.0 / float((w * w).sum())                         # read back for the decision
    if ess < ess_frac * n:
        u0 = torch.rand((1,), dtype=torch.float64, device=dev, generator=gen)
        c = torch.cumsum(w, 0)
        u = (torch.arange(n, dtype=torch.float64, device=dev) + u0) / n * c[-1]
        anc = torch.searchsorted(c, u, right=True).clamp(max=n - 1)
        rows, lw = rows[anc].contiguous(), torch.zeros_like(lw)
    return rows, lw


def measure_step(a, bm, boxes, width, pts, kw):
    out = {}
    twist, sigma = (0.02, 0.0, 0.0, 0.0, 0.0, 0.01), 0.01
    twist_dev = torch.tensor(twist, dtype=torch.float64).cuda()
    for n in a.particles:
        poses = interleaved_poses(n, width)
        rows0 = G._pose_rows(poses, "cuda")
        keep = {}

        def fresh():
            keep["pf"] = M.ParticleFilter(bm, poses, beta=a.beta, near=NEAR, N_samples=a.samples,
                                          N_importance=a.importance, huber_delta=a.huber_delta, min_sumw=a.min_sumw)
            keep["gen"] = torch.Generator(device="cuda").manual_seed(0)
            keep["rows"], keep["logw"] = rows0.clone(), torch.zeros(n, dtype=torch.float64, device="cuda")

        def device_step():
            keep["pf"].step(pts, twist, sigma, generator=keep["gen"])

        def composed():
            pf = keep["pf"]
            keep["rows"], keep["logw"] = composed_step(bm, boxes, pts, keep["rows"], keep["logw"], twist_dev, sigma,
                                                       keep["gen"], a.beta, pf.miss_cost, 0.5, kw)

        routes = {"device_step": device_step, "composed_step": composed}
        with torch.no_grad():
            for _ in range(a.warmup):
                for fn in routes.values():
                    fresh()
                    fn()
            ms = {k: [] for k in routes}
            for _ in range(a.repeats):   # the routes alternate inside every repeat, each from a fresh particle set
                for k, fn in routes.items():
                    fresh()
                    ms[k].append(timed(fn))
            fresh()
            device_step()
            resampled = bool((keep["pf"].logw == 0).all())
            ess = float(keep["pf"].ess)
        r = {k: stats(v) for k, v in ms.items()}
        r["device_over_composed"] = r["device_step"]["median_ms"] / r["composed_step"]["median_ms"]
        r["device_faster_than_composed"] = faster(r["device_step"], r["composed_step"])
        r["composed_faster_than_device"] = faster(r["composed_step"], r["device_step"])
        r["ess_of_the_timed_step"] = ess
        r["the_timed_step_resamples"] = resampled
        out[str(n)] = r
    return out


# ----------------------------------------------------------------------------------------------- 3. the headline
def bench_once(tree):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
    p = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, text=True, check=True)   # (a fresh child process)
    for line in reversed(p.stdout.strip().splitlines()):
        if line.startswith("{"):
            d = json.loads(line)
            return {"value": d["value"], "ms_per_step": d["ms_per_step"], "unit": d["unit"]}
    raise RuntimeError("bench.py printed no result line")


def measure_headline(a):
    runs = {"parent": [], "this": []}
    for _ in range(a.bench_rounds):   # the trees alternate: parent, this, ..., parent
        runs["parent"].append(bench_once(a.parent_tree))
        runs["this"].append(bench_once(REPO))
    runs["parent"].append(bench_once(a.parent_tree))   # (so that the parent has a spread of its own at one round)
    out = {"command": "python bench.py --gpus 1 --steps 20 --warmup 5", "rounds": a.bench_rounds,
           "order": "parent, this, ..., parent", "runs": runs}
    for k, v in runs.items():
        ms = [r["ms_per_step"] for r in v]
        out[k] = dict(median_ms_per_step=statistics.median(ms), spread_ms=max(ms) - min(ms),
                      median_value=statistics.median([r["value"] for r in v]), unit=v[0]["unit"])
    d = out["this"]["median_ms_per_step"] - out["parent"]["median_ms_per_step"]
    out["this_minus_parent_ms"] = d
    out["inside_the_parents_spread"] = bool(abs(d) <= out["parent"]["spread_ms"])
    out["differs_by_the_rule"] = bool(abs(d) > out["parent"]["spread_ms"] + out["this"]["spread_ms"])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here as well (sections of an existing file are kept)")
    ap.add_argument("--only", default="scoring,step,headline", help="comma-separated sections to run")
    ap.add_argument("--poses", type=int, default=1024)
    ap.add_argument("--particles", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--beams", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--importance", type=int, default=128)
    ap.add_argument("--huber-delta", type=float, default=0.0)
    ap.add_argument("--min-sumw", type=float, default=0.5)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=1)
    a = ap.parse_args(argv)
    only = set(a.only.split(","))
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    if "headline" in only:   # first: before this process opens the device
        if a.parent_tree:
            res["headline"] = measure_headline(a)
        else:
            res.setdefault("headline", {"measured": False, "why": "no --parent-tree given"})
    if not torch.cuda.is_available():
        print("time_mcl.py needs a ROCm GPU; there is no CPU path and nothing is measured without one",
              file=sys.stderr)
        return 2
    res.update(device=torch.cuda.get_device_name(0), blocks=BLOCKS, beams=a.beams, samples=[a.samples, a.importance],
               huber_delta=a.huber_delta, min_sumw=a.min_sumw, repeats=a.repeats, warmup=a.warmup,
               networks="seeded random frozen networks (no trained checkpoints are present)")
    kw = dict(N_samples=a.samples, N_importance=a.importance, huber_delta=a.huber_delta, min_sumw=a.min_sumw,
              near=NEAR)
    ok = True
    if only & {"scoring", "step"}:
        bm, boxes, width = build_map()
        pts = scan(a.beams)
        if "scoring" in only:
            res["scoring"] = dict(poses=a.poses, **measure_scoring(a, bm, boxes, width, pts, kw))
            ok = res["scoring"]["routes_agree"]
        if "step" in only:
            res["step"] = dict(beta=a.beta, **measure_step(a, bm, boxes, width, pts, kw))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
