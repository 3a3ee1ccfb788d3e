"""Times the map scoring with beams carried through the blocks they cross against the clipped scoring, on
time_mcl.py's scene: 4 blocks side by side along x, seeded random frozen networks (no trained checkpoints are present),
2,048 beams x 64 + 128 samples, 1,024 poses interleaved over the blocks.

Routes:
  map          nof.localization.score_poses_map (the clipped render)
  through_k1   score_poses_through, max_segments = 1 (the same render through the new kernel)
  through_k4   score_poses_through, max_segments = 4, min_transmittance = 1e-3
  through_k4_t0  the same with min_transmittance = 0

Protocol (time_localization.py's): the routes alternate inside every repeat after the warm-up rounds, every timing ends
in a device synchronise, results are median ms and spread (max - min).  Per route the segments rendered
(sum of n_segments; P x R for the clipped route) and the time per rendered segment are reported, and through_k1's
scores are compared with map's (equal bits); the script exits non-zero otherwise.  With ``--parent-tree DIR`` (a
checkout of the parent commit with its library built) the headline benchmark alternates between the two trees as
fresh child processes (time_mcl.py's measure_headline).  It needs a GPU and refuses to run without one.

    python pc-nerf_amd/time_through.py --out profiles/through.json [--parent-tree DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import time_mcl as TM  # noqa: E402
from nof import localization as L  # noqa: E402


def measure(a, bm, width, pts, kw):
    poses = TM.interleaved_poses(a.poses, width)
    ids = (torch.arange(a.poses) % TM.BLOCKS).to(torch.int32).cuda()
    keep = {}
    chains = {"through_k1": dict(max_segments=1), "through_k4": dict(max_segments=4, min_transmittance=1e-3),
              "through_k4_t0": dict(max_segments=4, min_transmittance=0.0)}

    def clipped():
        keep["map"] = L.score_poses_map(bm, pts, poses, ids, **kw)

    def through(name):
        def run():
            keep[name] = L.score_poses_through(bm, pts, poses, ids, seam_tol=a.seam_tol, **chains[name], **kw)
        return run

    routes = {"map": clipped, **{k: through(k) for k in chains}}
    with torch.no_grad():
        for _ in range(a.warmup):
            for fn in routes.values():
                fn()
        ms = {k: [] for k in routes}
        for _ in range(a.repeats):   # the routes alternate inside every repeat
            for k, fn in routes.items():
                ms[k].append(TM.timed(fn))
        out = {k: TM.stats(v) for k, v in ms.items()}
        out["map"]["segments"] = a.poses * a.beams
        for k, c in chains.items():   # the segment counts, outside the timing
            s = L.score_poses_through(bm, pts, poses, ids, seam_tol=a.seam_tol, want_depth=True, **c, **kw)
            out[k]["segments"] = int(s.n_segments.sum())
            out[k]["beams_by_segments"] = torch.bincount(s.n_segments.flatten(), minlength=5).tolist()
            out[k]["n_valid_min_max"] = [int(s.n_valid.min()), int(s.n_valid.max())]
    for k in routes:
        out[k]["ns_per_segment"] = out[k]["median_ms"] * 1e6 / max(out[k]["segments"], 1)
    out["through_k1_over_map"] = out["through_k1"]["median_ms"] / out["map"]["median_ms"]
    out["map_faster_than_through_k1"] = TM.faster(out["map"], out["through_k1"])
    out["n_valid_min_max_map"] = [int(keep["map"].n_valid.min()), int(keep["map"].n_valid.max())]
    out["routes_agree"] = bool(torch.equal(keep["map"].cost, keep["through_k1"].cost)
                               and torch.equal(keep["map"].n_valid, keep["through_k1"].n_valid)
                               and torch.equal(keep["map"].hit, keep["through_k1"].hit))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here as well (sections of an existing file are kept)")
    ap.add_argument("--only", default="scoring,headline", help="comma-separated sections to run")
    ap.add_argument("--poses", type=int, default=1024)
    ap.add_argument("--beams", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--importance", type=int, default=128)
    ap.add_argument("--huber-delta", type=float, default=0.0)
    ap.add_argument("--min-sumw", type=float, default=0.5)
    ap.add_argument("--seam-tol", type=float, default=1e-3)
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
            res["headline"] = TM.measure_headline(a)
        else:
            res.setdefault("headline", {"measured": False, "why": "no --parent-tree given"})
    if not torch.cuda.is_available():
        print("time_through.py needs a ROCm GPU; there is no CPU path and nothing is measured without one",
              file=sys.stderr)
        return 2
    ok = True
    if "scoring" in only:
        res.update(device=torch.cuda.get_device_name(0), blocks=TM.BLOCKS, beams=a.beams, poses=a.poses,
                   samples=[a.samples, a.importance], huber_delta=a.huber_delta, min_sumw=a.min_sumw,
                   seam_tol=a.seam_tol, repeats=a.repeats, warmup=a.warmup,
                   networks="seeded random frozen networks (no trained checkpoints are present)")
        kw = dict(N_samples=a.samples, N_importance=a.importance, huber_delta=a.huber_delta, min_sumw=a.min_sumw,
                  near=TM.NEAR)
        bm, _, width = TM.build_map()
        res["scoring"] = measure(a, bm, width, TM.scan(a.beams), kw)
        ok = res["scoring"]["routes_agree"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
