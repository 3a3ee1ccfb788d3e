"""Restatement of the render carried through the blocks of a map (tests of pcnerf::score_poses_through and
nof.localization.score_poses_through / synthesize_scan) -- test infrastructure only, numpy and torch CPU.

Decisions (which block comes next, where a segment begins and ends, when the chain stops) use the kernel's float64
operations one for one, as map_ref.assign_blocks does, so they are compared for equality; the chain arithmetic is the
kernel's, operation by operation; a segment's render is registration_ref.render_two_pass on rows [o, d, near_k, far_k]
(float64 rows: the reference; the same rows cast to float32: the float32 restatement)."""
import functools

import numpy as np
import torch

import localization_ref as LR
import registration_ref as RR
from oracle import ref_cpu as O

EPS32 = float(np.float32(RR.EPS))   # the kernel takes eps as a float32
INF = float("inf")
SPLIT_X = 0.5
EMPTY_LOGIT = -30.0


# ----------------------------------------------------------------------------------------------- geometry
def pose_rows(poses) -> np.ndarray:
    """(P, 4, 4) -> (P, 12) float64 rows [R row-major, t] (nof.localization._poses12)."""
    T = np.asarray(torch.as_tensor(poses, dtype=torch.float64))
    return np.concatenate([T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], -1)


def ray_od(row12, pt32):
    """fr_pose_ray's float64 ray of the float32 sensor-frame point: (o (3,), d (3,), rng), operation by operation."""
    T = np.asarray(row12, np.float64)
    p = np.asarray(pt32, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rng = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
        ux, uy, uz = p[0] / rng, p[1] / rng, p[2] / rng
        d = np.array([(T[3 * m] * ux + T[3 * m + 1] * uy) + T[3 * m + 2] * uz for m in range(3)])
        dn = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        d = d / dn
    return T[9:12].copy(), d, float(rng)


def _fmax(a, b):
    """C's fmax: the other operand where one is NaN."""
    if a != a:
        return b
    if b != b:
        return a
    return max(a, b)


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return min(a, b)


def box_interval(o, d, box):
    """(tin, tout) of the ray in box = [lo, hi]: tout = min over the axes of max(t1, t2), a NaN t2 counting as +inf
    (fr_pose_ray's exit before the clamp to near); tin the mirror image, max over the axes of min(t1, t2), a NaN t1
    counting as -inf; any other NaN propagates."""
    box = np.asarray(box, np.float64)
    tin = tout = 0.0
    nan = float("nan")
    for m in range(3):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            inv = float(np.float64(1.0) / np.float64(d[m]))
            t1 = float((box[m] - o[m]) * np.float64(inv))
            t2 = float((box[3 + m] - o[m]) * np.float64(inv))
        tm = INF if t2 != t2 else (nan if t1 != t1 else _fmax(t1, t2))
        tn = -INF if t1 != t1 else (nan if t2 != t2 else _fmin(t1, t2))
        tout = tm if m == 0 else (nan if (tout != tout or tm != tm) else _fmin(tout, tm))
        tin = tn if m == 0 else (nan if (tin != tin or tn != tn) else _fmax(tin, tn))
    return tin, tout


def segment_exit(tout, near32):
    """far64 of a segment: never below its near (fr_pose_ray's clamp); NaN stays."""
    return tout if tout != tout else _fmax(tout, float(near32))


def is_candidate(tin, tout, te, seam_tol):
    if tin != tin or tout != tout:
        return False
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(tin <= te + seam_tol and tout > te and np.float32(tout) > np.float32(_fmax(te, tin)))


def next_block(o, d, boxes, cur, te, seam_tol):
    """-> (block, tin, tout) of the candidate with the largest tout, the lowest index on ties, or (-1, 0, 0)."""
    best = (-1, 0.0, 0.0)
    for j in range(len(boxes)):
        if j == cur:
            continue
        tin, tout = box_interval(o, d, boxes[j])
        if is_candidate(tin, tout, te, seam_tol) and (best[0] < 0 or tout > best[2]):
            best = (j, tin, tout)
    return best


# ----------------------------------------------------------------------------------------------- the chain
def chain_step(v, s, T, W, N, eps=EPS32):
    """One segment (depth v, hit probability s) joins the chain; every operation rounded separately."""
    v, s = np.float64(v), np.float64(s)
    with np.errstate(invalid="ignore", over="ignore"):
        c = T * s
        W = W + c
        N = N + T * (v * (s + np.float64(eps)))
        T = T * (np.float64(1.0) - s)
    if T < 0.0:
        T = np.float64(0.0)
    return T, W, N


def walk_many(boxes, row12, pts32, b0, K, seam_tol, t_min, segments, near=RR.NEAR, eps=EPS32, round32=True):
    """The chains of the beams to the float32 points pts32 (R, 3) under one pose.  ``segments(block, o, d, near_k,
    te)`` -> (depth (n,), sumw (n,)) renders the segments of n beams in block ``block``: o, d (n, 3) float64, near_k
    (n,) float32 values, te (n,) their float64 exits.  round32: the segment results are float32 values and so are the
    outputs (the kernel); otherwise everything stays float64 (the reference).
    -> one dict per beam: depth, sumw, n_segments, last_block, te (the exits), blocks, T (the transmittance in front
    of each segment)."""
    beams = []
    for p in np.asarray(pts32, np.float32).reshape(-1, 3):
        o, d, _ = ray_od(row12, p)
        _, tout = box_interval(o, d, boxes[b0])
        near_k = np.float32(near)
        beams.append({"o": o, "d": d, "near": near_k, "te_k": segment_exit(tout, near_k), "cur": int(b0),
                      "TWN": (np.float64(1.0), np.float64(0.0), np.float64(0.0)), "te": [], "blocks": [], "T": [],
                      "first": None, "live": True})
    for k in range(K):
        live = [w for w in beams if w["live"]]
        for blk in sorted({w["cur"] for w in live}):
            grp = [w for w in live if w["cur"] == blk]
            v, s = segments(blk, np.stack([w["o"] for w in grp]), np.stack([w["d"] for w in grp]),
                            np.array([w["near"] for w in grp], np.float32), np.array([w["te_k"] for w in grp]))
            for w, vi, si in zip(grp, np.asarray(v), np.asarray(s)):
                w["vs"] = (np.float32(vi), np.float32(si)) if round32 else (np.float64(vi), np.float64(si))
        for w in live:
            v, s = w["vs"]
            if w["first"] is None:
                w["first"] = (v, s)
            w["te"].append(w["te_k"])
            w["blocks"].append(w["cur"])
            w["T"].append(float(w["TWN"][0]))
            w["TWN"] = chain_step(v, s, *w["TWN"], eps)
            if k + 1 >= K or w["TWN"][0] <= t_min:
                w["live"] = False
                continue
            nb, tin, tout = next_block(w["o"], w["d"], boxes, w["cur"], w["te_k"], seam_tol)
            if nb < 0:
                w["live"] = False
                continue
            w["cur"] = nb
            w["near"] = np.float32(_fmax(w["te_k"], tin))
            w["te_k"] = segment_exit(tout, w["near"])
    out = []
    for w in beams:
        if len(w["blocks"]) == 1:
            depth, sumw = w["first"]
        else:
            _, W, N = w["TWN"]
            with np.errstate(invalid="ignore", divide="ignore"):
                depth, sumw = N / (W + np.float64(eps)), W
            if round32:
                depth, sumw = np.float32(depth), np.float32(sumw)
        out.append({"depth": depth, "sumw": sumw, "n_segments": len(w["blocks"]), "last_block": w["cur"],
                    "te": w["te"], "blocks": w["blocks"], "T": w["T"]})
    return out


def walk(boxes, row12, pt32, b0, K, seam_tol, t_min, segments, **kw):
    """walk_many's one beam."""
    return walk_many(boxes, row12, np.asarray(pt32, np.float32).reshape(1, 3), b0, K, seam_tol, t_min, segments,
                     **kw)[0]


def no_render(block, o, d, near_k, te):
    """Segments that see nothing: for tests of the rule alone."""
    return np.zeros(len(te)), np.zeros(len(te))


# ----------------------------------------------------------------------------------------------- segment renders
def rows_of(o, d, near_k, te, dtype=torch.float64):
    """(n, 8) rows [o, d, near_k, far_k] in ``dtype``."""
    r = np.concatenate([o, d, np.asarray(near_k, np.float64)[:, None], np.asarray(te, np.float64)[:, None]], 1)
    return torch.from_numpy(r).to(dtype)


def make_segments(folds_c, folds_f, S, I, dtype=torch.float64):
    """The restatement's segment render in ``dtype`` (float32: the same rows cast, as localization_ref.render_poses)."""
    def segments(block, o, d, near_k, te):
        dep, sw, _ = RR.render_two_pass(folds_c[block], folds_f[block], rows_of(o, d, near_k, te, dtype), S, I,
                                        want_jac=False)
        return dep.double().numpy(), sw.double().numpy()
    return segments


def segment_samples(fold_c, fold_f, rows, S, I):
    """registration_ref.render_two_pass's fine samples of float64 rows: (zf (R, S + I), p (R, S + I))."""
    z = O.lin_z(rows[:, 6:7], rows[:, 7:8], S).to(rows.dtype)
    _, w, _, _ = RR.render(fold_c, rows, z, rows.dtype, want_jac=False)
    zmid = .5 * (z[..., 1:] + z[..., :-1])
    u = torch.linspace(0., 1., steps=I, dtype=rows.dtype).expand(rows.shape[0], I)
    zs = O.sample_pdf(zmid, w[..., 1:-1], I, det=False, u=u)
    zf = torch.sort(torch.cat([z, zs], -1), -1)[0]
    x = rows[:, None, 0:3] + rows[:, None, 3:6] * zf[..., None]
    return zf, torch.sigmoid(RR.fold_logit(fold_f, x))


def through_render(scene, pose, pts32, b0, S, I, K, seam_tol, t_min, dtype=torch.float64):
    """Every beam of the scan under one pose -> dict of (R,) arrays depth, sumw (float64), n_segments, last_block.
    float64: the reference, nothing rounded on the way; float32: the rows cast and every segment's result a float32
    value, the chain still float64."""
    row = pose_rows(torch.as_tensor(pose)[None])[0]
    seg = make_segments(scene["folds_c"], scene["folds_f"], S, I, dtype)
    out = walk_many(scene["boxes"], row, np.asarray(pts32), b0, K, seam_tol, t_min, seg, round32=False)
    res = {k: np.array([w[k] for w in out]) for k in ("depth", "sumw", "n_segments", "last_block")}
    res["arriving_T"] = np.array([(w["T"] + [1.0])[1] for w in out])   # in front of segment 1 (1: there is none)
    return res


# ----------------------------------------------------------------------------------------------- scenes
def _scene(boxes, folds_c, folds_f=None):
    folds_f = folds_c if folds_f is None else folds_f
    return {"boxes": np.asarray(boxes, np.float64), "folds_c": torch.stack(list(folds_c)),
            "folds_f": torch.stack(list(folds_f))}


def empty_fold():
    a = torch.zeros(64, dtype=torch.float64)
    a[63] = EMPTY_LOGIT
    return a


def split_cavity():
    """The analytic cavity's box [-2.5, 2.5]^3 cut at x = 0.5 into two blocks that share the face; both hold the
    analytic field."""
    f = RR.analytic_fold()
    return _scene([[-2.5, -2.5, -2.5, SPLIT_X, 2.5, 2.5], [SPLIT_X, -2.5, -2.5, 2.5, 2.5, 2.5]], [f, f])


def one_box_cavity():
    return _scene([[-2.5, -2.5, -2.5, 2.5, 2.5, 2.5]], [RR.analytic_fold()])


WALL_X = 8.0


def row_of_three(gap=0.0, overlap=0.0):
    """Boxes [-2.5, 2.5], [2.5, 7.5], [7.5, 12.5] in x ([-2.5, 2.5] in y and z): two empty blocks (logit -30
    everywhere) and the plane field logit = 40 (x - 8) in the third.  gap: the second box begins that much later;
    overlap: that much earlier."""
    x1 = 2.5 + gap - overlap
    boxes = [[-2.5, -2.5, -2.5, 2.5, 2.5, 2.5], [x1, -2.5, -2.5, 7.5, 2.5, 2.5], [7.5, -2.5, -2.5, 12.5, 2.5, 2.5]]
    return _scene(boxes, [empty_fold(), empty_fold(), LR.plane_fold(40.0, WALL_X)])


def sixty_five_blocks():
    """The row of three among 62 decoys far from every beam: the start block at 0, the decoys at 1 .. 62, the wall
    block at 63 and the middle block at 64, so the search has to look past lane 63."""
    r = row_of_three()
    decoys = [[100.0 + 6 * k, 50.0, 50.0, 105.0 + 6 * k, 55.0, 55.0] for k in range(62)]
    boxes = [r["boxes"][0]] + decoys + [r["boxes"][2], r["boxes"][1]]
    order = [0] + [0] * 62 + [2, 1]
    return _scene(boxes, [r["folds_c"][i] for i in order])


ROW_TWIST = (0.3, -0.2, 0.1, 0.02, -0.05, 0.1)


def row_pose():
    from nof.registration import se3_exp
    return se3_exp(ROW_TWIST)


def cavity_pose():
    from nof.registration import se3_exp
    return se3_exp(RR.XI_STAR)


def row_directions(n, seed=0):
    """n unit directions: every third one anywhere on the sphere, the others in a cone around +x (within about 25
    degrees: they cross all three boxes or leave through a side of the second)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    fwd = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64) + 0.2 * v
    pick = (torch.arange(n) % 3 == 0)[:, None]
    v = torch.where(pick, v, fwd)
    return v / v.norm(dim=-1, keepdim=True)


def scan_points(dirs, ranges=None):
    """float32 sensor-frame points along the unit directions (ranges: 1.5 m where not given)."""
    r = torch.full((dirs.shape[0],), 1.5, dtype=torch.float64) if ranges is None else torch.as_tensor(ranges).double()
    r = torch.where(torch.isfinite(r) & (r > 0), r, torch.full_like(r, 1.5))
    return (dirs * r[:, None]).float()


@functools.lru_cache(maxsize=None)
def split_cavity_facts():
    """The split cavity seen from se3_exp(XI_STAR) along unit_directions(256, 0) at 64 + 128 samples, float64, computed
    once: clipped to the sensor's block and carried into the second (max_segments 2, min_transmittance 0)."""
    sc = split_cavity()
    pts = scan_points(RR.unit_directions(256, 0))
    pose = cavity_pose()
    clipped = through_render(sc, pose, pts, 0, 64, 128, 1, 1e-3, 0.0)
    through = through_render(sc, pose, pts, 0, 64, 128, 2, 1e-3, 0.0)
    return {"scene": sc, "points": pts, "pose": pose, "clipped": clipped, "through": through}
