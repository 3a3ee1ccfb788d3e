"""Times a frozen-BatchNorm training step next to its forward and to the default (train-mode) step, at BASELINE config
2's shapes (65,536 rays, 128 + 256 samples, BatchNorm chunks of 262,144, the training step's losses of
train_kitti.py:117-155):

  (a) forward -- render_rays_train + the losses under no_grad with eval-mode networks;
  (b) frozen  -- the same call with eval-mode networks whose parameters require grad, then loss.backward():
                 nof._autograd.FrozenPass (compositing backward + pcnerf::eval_gmoments_rays + pcnerf::eval_param_grads);
  (c) train   -- the same with train-mode networks: the existing default backward (rematerialised).

The three alternate inside every repeat and every timing ends in a device synchronise.  Reported per route: median ms
and spread (max - min) over ``--repeats`` repeats after ``--warmup`` warm-ups; (b) - (a) and (c) - (b); and the same
way, on their own, the frozen backward's stages on the fine pass -- eval_gmoments_rays, eval_param_grads -- next to
k_rays_grad_eval (pcnerf::rays_grad_eval), which does the same sincosf work per sample, and the compositing backward.
(b) must reproduce (a)'s output bits; the script exits non-zero if it does not.  It needs a GPU and refuses to run
without one.

    python pc-nerf_amd/time_frozen_bn.py --out profiles/frozen_bn.json
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
from nof import render as R  # noqa: E402
from nof import synthetic as syn  # noqa: E402
from nof import _torch_ops as T  # noqa: E402
from nof.criteria import nof_loss  # noqa: E402
from nof.networks import Embedding, NOF_coarse, NOF_fine  # noqa: E402

P = torch.ops.pcnerf


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(median_ms=statistics.median(ms), spread_ms=max(ms) - min(ms), repeats_ms=ms)


def networks(train, grad):
    out = []
    for cls, seed in ((NOF_coarse, 1234), (NOF_fine, 5678)):
        m = syn.load_into(cls(), syn.init_nof_params(seed)).cuda().train(train)
        for t in m.parameters():
            t.requires_grad_(grad)
        out.append(m)
    return out


def measure(rays, a):
    emb, loss_fn, gt = Embedding(3, 10), nof_loss["smoothl1"](), rays[:, 14].contiguous()
    kw = dict(sub_nerf_test_num=32, N_samples=a.samples, N_importance=a.importance, perturb=0, noise_std=0,
              chunk=a.chunk, issegmentated=1, childnerf_ratio=0.1, use_child_nerf_divide=0, use_child_nerf_loss=1)
    nets = {"forward": networks(False, False), "frozen": networks(False, True), "train": networks(True, True)}
    keep = {}

    def step(name, grad):
        mc, mf = nets[name]
        for m in (mc, mf):
            m.zero_grad(set_to_none=True)
        res = R.render_rays_train(mc, mf, emb, rays, **kw)
        loss = (1e-1 * loss_fn(1e1 * res["depth"], 1e1 * gt) + 1e-1 * loss_fn(1e1 * res["depth_fine"], 1e1 * gt)
                + 1e6 * res["child_free_loss_fine"] + 1e6 * res["child_free_loss"]
                + 1e5 * res["child_depth_loss_fine"] + 1e5 * res["child_depth_loss"])
        if grad:
            loss.backward()
        keep[name] = {k: v.detach() for k, v in res.items()}

    def forward():
        with torch.no_grad():
            step("forward", False)

    routes = {"forward": forward, "frozen": lambda: step("frozen", True), "train": lambda: step("train", True)}
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    same = all(torch.equal(keep["forward"][k], keep["frozen"][k]) for k in keep["forward"])

    # the frozen backward's stages on the fine pass, and k_rays_grad_eval on the same samples
    mf = nets["forward"][1]
    with torch.no_grad():
        z = R._coarse(rays, a.samples, 1, 0.1, 0, None)
        w = P.composite(R._query(nets["forward"][0], rays, z, a.chunk), z, None, 0.0, R.EPSILON, None, 10, 11, 14,
                        True)[0]
        zf = P.resample(z, w, a.importance, None)
        del z, w
        p = R._query(mf, rays, zf, a.chunk)
        cot = torch.randn(rays.shape[0], generator=torch.Generator().manual_seed(1)).cuda()
        one = torch.ones((), device="cuda")
        g_logit = _ops.composite_backward(p, zf, None, 0.0, R.EPSILON, rays, 0, cot, one, one)
        params = [t.detach() for t in T.eval_params(mf)]
        fold = P.fold_eval(params)
        mom = P.eval_gmoments_rays(rays, zf, g_logit)
    kernels = {"query_fine": lambda: R._query(mf, rays, zf, a.chunk),
               "composite_backward_fine": lambda: _ops.composite_backward(p, zf, None, 0.0, R.EPSILON, rays, 0, cot,
                                                                          one, one),
               "eval_gmoments_rays_fine": lambda: P.eval_gmoments_rays(rays, zf, g_logit),
               "eval_param_grads": lambda: P.eval_param_grads(params, mom, 1e-5),
               "rays_grad_eval_fine": lambda: P.rays_grad_eval(rays, zf, g_logit, fold)}
    for _ in range(a.warmup):
        for fn in list(routes.values()) + list(kernels.values()):
            fn()
    ms = {k: [] for k in list(routes) + list(kernels)}
    for _ in range(a.repeats):   # the routes alternate inside every repeat
        for k, fn in routes.items():
            ms[k].append(timed(fn))
        with torch.no_grad():
            for k, fn in kernels.items():
                ms[k].append(timed(fn))
    out = {k: stats(v) for k, v in ms.items()}
    out["forward_bits_equal"] = bool(same)
    out["frozen_minus_forward_ms"] = out["frozen"]["median_ms"] - out["forward"]["median_ms"]
    out["train_minus_frozen_ms"] = out["train"]["median_ms"] - out["frozen"]["median_ms"]
    out["frozen_backward_over_forward"] = out["frozen_minus_forward_ms"] / out["forward"]["median_ms"]
    out["gmoments_over_rays_grad_eval"] = (out["eval_gmoments_rays_fine"]["median_ms"]
                                           / out["rays_grad_eval_fine"]["median_ms"])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--importance", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("time_frozen_bn.py needs a ROCm GPU; there is no CPU path and nothing is measured without one",
              file=sys.stderr)
        return 2
    rays = torch.from_numpy(syn.make_rays(a.rays, seed=0)).cuda()
    res = dict(device=torch.cuda.get_device_name(0), rays=a.rays, samples=a.samples, importance=a.importance,
               chunk=a.chunk, fine_samples=a.rays * (a.samples + a.importance), repeats=a.repeats, warmup=a.warmup,
               eval_math=_ops.get_eval_math(), eval_fold=_ops.eval_fold_enabled(), train_math=_ops.get_train_math())
    res.update(measure(rays, a))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    return 0 if res["forward_bits_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
