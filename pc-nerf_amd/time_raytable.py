"""Times the ray-table builders with the flat child scan and with the uniform-grid child index (nof.raytable).

Scenes: the KITTI-00 fixture scene of BASELINE config 3 (tests/golden/kitti_frames_full.npz: scans 1151..1200, every
16th point, ~3.4k children) and a seeded synthetic scene at the reference training shell's size (15,333 children over
+-62 m, 120,000 points per frame).  Per scene and per path: median ms per frame of the train rows and of the two-step
rows (method 2) over ``--repeats`` repeats, the spread (max - min) over those repeats, and the grid's build time.
Flat and grid alternate inside every repeat; every timing ends in a device synchronise.  Every flat/grid output pair
is compared first and the script exits non-zero if any differs.  It needs a GPU and refuses to run without one.

    python pc-nerf_amd/time_raytable.py --out profiles/raytable_grid.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from nof import dataset as D  # noqa: E402
from nof import io as nio  # noqa: E402
from nof.raytable import ChildGrid, build_train_rays, build_view_rows  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden")


def synthetic_scene(C, n, seed, origin, ext, frac_in=0.8):
    """Child boxes of half-extent 0.1..0.6 m scattered over +-ext, 80 % of the points inside a box, the rest around
    the scene (the generator of tests/test_raytable_grid.py)."""
    r = np.random.default_rng(seed)
    ctr = np.stack([r.uniform(-ext, ext, C), r.uniform(-ext, ext, C), r.uniform(-2.0, 0.5, C)], 1)
    half = r.uniform(0.1, 0.6, (C, 3))
    lo, hi = ctr - half, ctr + half
    b6 = np.concatenate([lo - 0.025, hi + 0.025], 1)
    k = r.integers(0, C, n)
    pts = lo[k] + r.uniform(0, 1, (n, 3)) * (hi[k] - lo[k])
    m = int(n * (1 - frac_in))
    pts[:m] = np.stack([r.uniform(-ext - 5, ext + 5, m), r.uniform(-ext - 5, ext + 5, m), r.uniform(-2.5, 1.0, m)], 1)
    return pts, np.asarray(origin, float), ctr, b6, np.array([-ext - 1, -ext - 1, -2.7, ext + 1, ext + 1, 1.2])


def shell_frames(dev, frames, points=120000, children=15333, ext=62.0):
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)   # noqa: E731
    pts, o, ctr, b6, p6 = synthetic_scene(children, points * frames, 5, (0.3, -0.2, -0.5), ext)
    per = [(t(pts[i * points:(i + 1) * points]), t(o)) for i in range(frames)]
    return dict(name=f"synthetic_{children}", children=children, centers=t(ctr), bounds6=t(b6), parent6=t(p6),
                train=per, view=per, view_bounds6=t(b6), view_parent6=t(p6))


def kitti_frames(dev, frames):
    """Config 3's scene as nof.dataset.kitti_dataload builds it (train rows of its first training frames), and the
    eval driver's scene over the same block (two-step rows of its first held-out frames)."""
    import eval_kitti_render as E
    g = dict(np.load(os.path.join(GOLDEN, "kitti_frames_full.npz"), allow_pickle=False))
    ds, de, rd = 1150, 1200, (3.0, 2.0, 1.25)
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "pcd")
        os.makedirs(root)
        for k, v in g.items():
            if k.startswith("f"):
                nio.write_pcd(os.path.join(root, f"{k[1:]}.pcd"), v)
        pose_path = os.path.join(tmp, "poses.txt")
        with open(pose_path, "w") as fh:
            for _ in range(int(g["pose_first"])):
                fh.write("1 0 0 0 0 1 0 0 0 0 1 0\n")
            for row in g["poses"]:
                fh.write(" ".join(repr(float(v)) for v in row) + "\n")
        poses = D.relative_poses(D.read_poses(pose_path), ds)
        positions = poses[ds + 1:de + 1, :3, 3]
        parent = D.fuse_frames(root, poses, ds, de, dev, rd, 0.168, -2.0, 20.0, 20.0)
        p64 = parent.to(torch.float64)
        parent6 = torch.cat([p64.min(0).values, p64.max(0).values])
        bounds6, centers = D.child_boxes(*D.split_children(parent))
        train = []
        for f in D.frame_ids(ds, de, "train", 50)[:frames]:
            p = D.filter_scan(torch.from_numpy(D.load_frame(root, f)).to(dev), rd, 0.168, -2.0)
            w = D.to_block(p, poses[f])
            w = w[D.interest_mask(w, positions, 20.0, 20.0)]
            train.append((w.to(torch.float64), poses[f][:3, 3].to(device=dev, dtype=torch.float64)))
        h = E.get_opts(f"""--dataset kitti --root_dir {root} --pose_path {pose_path} --data_start {ds} --data_end {de}
            --range_delete_x 3 --range_delete_y 2 --range_delete_z 1.25 --over_height 0.168 --over_low -2
            --interest_x 20 --interest_y 20""".split())
        sc = E.Scene(h, dev)
        view = [(sc.frame_points(f).to(torch.float64), sc.poses[f][:3, 3].to(device=dev, dtype=torch.float64))
                for f in E.test_frame_ids(ds, de)[:frames]]
    return dict(name="kitti_frames_full", children=int(bounds6.shape[0]), centers=centers, bounds6=bounds6,
                parent6=parent6, train=train, view=view, view_bounds6=sc.bounds6, view_parent6=sc.parent6)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(median_ms=statistics.median(ms), spread_ms=max(ms) - min(ms), repeats_ms=ms)


def measure(sc, repeats, warmup, cell):
    def train(index, grid=None):
        return [build_train_rays(p, o, sc["centers"], sc["bounds6"], sc["parent6"], 0.05, index=index, grid=grid)
                for p, o in sc["train"]]

    def view(index, grid=None):
        return [build_view_rows(p, o, sc["view_bounds6"], sc["view_parent6"], method=2, index=index, grid=grid)
                for p, o in sc["view"]]

    gt, gv = ChildGrid(centers=sc["centers"], cell=cell), ChildGrid(bounds6=sc["view_bounds6"], cell=cell)
    # outputs first: every flat/grid pair must be equal
    equal = all(torch.equal(a, b) for a, b in zip(train("flat"), train("grid", gt)))
    equal = equal and all(torch.equal(x, y) for a, b in zip(view("flat"), view("grid", gv)) for x, y in zip(a, b))
    for _ in range(warmup):
        train("flat"), train("grid", gt), view("flat"), view("grid", gv)
    nt, nv = len(sc["train"]), len(sc["view"])
    ms = {k: [] for k in ("train_flat", "train_grid", "view_flat", "view_grid", "build_train", "build_view")}
    for _ in range(repeats):   # flat and grid alternate inside every repeat
        ms["train_flat"].append(timed(lambda: train("flat")) / nt)
        ms["train_grid"].append(timed(lambda: train("grid", gt)) / nt)
        ms["view_flat"].append(timed(lambda: view("flat")) / nv)
        ms["view_grid"].append(timed(lambda: view("grid", gv)) / nv)
        ms["build_train"].append(timed(lambda: ChildGrid(centers=sc["centers"], cell=cell).n_cells))
        ms["build_view"].append(timed(lambda: ChildGrid(bounds6=sc["view_bounds6"], cell=cell).n_cells))
    out = dict(scene=sc["name"], children=sc["children"], outputs_equal=bool(equal), cell=gt.cell,
               grid_dims=list(gt.dims), grid_cells=gt.n_cells, frames=dict(train=nt, view=nv),
               points_per_frame=dict(train=int(np.mean([p.shape[0] for p, _ in sc["train"]])),
                                     view=int(np.mean([p.shape[0] for p, _ in sc["view"]]))))
    for kind, n in (("train", nt), ("view", nv)):
        flat, grid, build = stats(ms[f"{kind}_flat"]), stats(ms[f"{kind}_grid"]), stats(ms[f"build_{kind}"])
        # one grid per scene serves every frame; here its build is charged to the frames timed
        with_build = grid["median_ms"] + build["median_ms"] / n
        gap = flat["median_ms"] - with_build
        out[kind] = dict(flat=flat, grid=grid, grid_build=build, grid_with_build_median_ms=with_build,
                         gap_ms=gap, grid_faster_beyond_spread=bool(gap > max(flat["spread_ms"], grid["spread_ms"])))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=4, help="frames per scene and row kind")
    ap.add_argument("--cell", type=float, default=1.0)
    ap.add_argument("--shell-points", type=int, default=120000)
    ap.add_argument("--shell-children", type=int, default=15333)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("time_raytable.py needs a ROCm GPU; there is no CPU path and nothing is measured without one",
              file=sys.stderr)
        return 2
    dev = torch.device("cuda")
    scenes = [kitti_frames(dev, a.frames), shell_frames(dev, a.frames, a.shell_points, a.shell_children)]
    res = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, warmup=a.warmup,
               scenes=[measure(sc, a.repeats, a.warmup, a.cell) for sc in scenes])
    res["outputs_equal"] = all(s["outputs_equal"] for s in res["scenes"])
    res["grid_faster_everywhere"] = all(s[k]["grid_faster_beyond_spread"] for s in res["scenes"]
                                        for k in ("train", "view"))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    return 0 if res["outputs_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
