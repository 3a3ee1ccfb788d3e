"""Times the fused NOF query on its three routes to the same occupancies, at BASELINE config 2's fine pass (65,536 rays
x 384 samples, BatchNorm chunk 262,144):

  (a) ray   -- the ray-sourced fused query (nof._ops.query: positions o + d*z rebuilt in the kernel);
  (b) point -- the point-sourced fused query (nof._ops.query_points) on pts = o + d*z computed beforehand;
  (c) embed -- Embedding -> NOF.forward chunk by chunk (the reference's render.py:18-25 / 44-51 loop on this package's
               modules: a (chunk, 63) embedding written and re-read per chunk).

Eval and train mode (forward only, under no_grad); the three routes alternate inside every repeat and every timing ends
in a device synchronise.  Reported per route: median ms, spread (max - min) over ``--repeats`` repeats, and for (c) the
peak device memory above the inputs.  (a) and (b) must give the same bits; the script exits non-zero if they do not.
It needs a GPU and refuses to run without one.

    python pc-nerf_amd/time_point_query.py --out profiles/point_query.json
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
from nof import synthetic as syn  # noqa: E402
from nof.networks import Embedding, NOF_fine  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(median_ms=statistics.median(ms), spread_ms=max(ms) - min(ms), repeats_ms=ms)


def measure(train, rays, z, pts, chunk, repeats, warmup):
    R, S = z.shape
    model = syn.load_into(NOF_fine(), syn.init_nof_params(5678)).cuda().train(train)
    emb = Embedding(3, 10)
    flat = pts.view(-1, 3)

    def ray():
        return _ops.query(model, rays, z, chunk)

    def point():
        return _ops.query_points(model, flat, R, S, chunk)

    def embed():
        return torch.cat([model(emb(flat[i:i + chunk])) for i in range(0, flat.shape[0], chunk)], 0).view(R, S)

    with torch.no_grad():
        a, b = ray(), point()
        same_bits = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
        c = embed()
        embed_max_abs_diff = float((c - a).abs().max())
        del a, b, c
        for _ in range(warmup):
            ray(), point(), embed()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        embed()
        torch.cuda.synchronize()
        embed_peak = torch.cuda.max_memory_allocated() - base
        ms = {"ray": [], "point": [], "embed": []}
        for _ in range(repeats):   # the routes alternate inside every repeat
            ms["ray"].append(timed(ray))
            ms["point"].append(timed(point))
            ms["embed"].append(timed(embed))
    out = {k: stats(v) for k, v in ms.items()}
    out["point_equals_ray_bits"] = same_bits
    out["embed_max_abs_diff_vs_ray"] = embed_max_abs_diff
    out["embed_peak_extra_bytes"] = int(embed_peak)
    gap = out["point"]["median_ms"] - out["ray"]["median_ms"]
    out["point_minus_ray_ms"] = gap
    out["point_within_spread_of_ray"] = bool(abs(gap) <= max(out["point"]["spread_ms"], out["ray"]["spread_ms"]))
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
        print("time_point_query.py needs a ROCm GPU; there is no CPU path and nothing is measured without one",
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
               bytes_per_sample=dict(ray=4, point=12, embed=252),
               eval=measure(False, rays, z, pts, a.chunk, a.repeats, a.warmup),
               train=measure(True, rays, z, pts, a.chunk, a.repeats, a.warmup))
    res["point_equals_ray_bits"] = res["eval"]["point_equals_ray_bits"] and res["train"]["point_equals_ray_bits"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    return 0 if res["point_equals_ray_bits"] else 1


if __name__ == "__main__":
    sys.exit(main())
