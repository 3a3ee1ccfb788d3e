"""The render carried through the blocks of a map, the parts that need no GPU: the restatement on its own
(tests/through_ref.py: the chain against the compositing of the concatenated samples, the next-block rule, the facts of
the split cavity the GPU tests depend on), the operator's schema and fake shapes, the C entry's binding and argument
errors, and the public signatures."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import registration_ref as RR
import through_ref as TR
from oracle import ref_cpu as O
from nof import _hip
from nof import _torch_ops as T
from nof import localization as L
from nof import mcl as M

P = torch.ops.pcnerf
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)


# ----------------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("scene,pose,dirs,b0", [
    ("split", "cavity", "sphere", 0), ("row", "row", "row", 0), ("overlap", "row", "row", 0)])
def test_the_chain_of_float64_segments_is_the_compositing_of_the_concatenated_samples(scene, pose, dirs, b0):
    """1 - sum w = prod (1 - p): chaining the segments' (depth, sumw) in float64 gives the depth and the hit
    probability of one compositing over all the segments' samples in order, to 1e-12 relative."""
    sc = {"split": TR.split_cavity, "row": TR.row_of_three, "overlap": lambda: TR.row_of_three(overlap=1.0)}[scene]()
    T_pose = TR.cavity_pose() if pose == "cavity" else TR.row_pose()
    d = RR.unit_directions(48, 3) if dirs == "sphere" else TR.row_directions(48, 3)
    pts = TR.scan_points(d)
    row = TR.pose_rows(T_pose[None])[0]
    S, I = 16, 24
    kept = {}

    def segments(block, o, dd, near_k, te):
        rows = TR.rows_of(o, dd, near_k, te)
        zf, p = TR.segment_samples(sc["folds_c"][block], sc["folds_f"][block], rows, S, I)
        for i in range(rows.shape[0]):
            kept.setdefault(tuple(o[i]) + tuple(dd[i]), []).append((zf[i], p[i]))
        w, depth = O.composite(p, zf, TR.EPS32)
        return depth.numpy(), RR.unnormalised(p)[0].sum(-1).numpy()

    out = TR.walk_many(sc["boxes"], row, pts.numpy(), b0, 4, 1e-3, 0.0, segments, round32=False)
    assert max(w["n_segments"] for w in out) >= 2
    worst = 0.0
    for w, p32 in zip(out, pts.numpy()):
        o, dd, _ = TR.ray_od(row, p32)
        segs = kept[tuple(o) + tuple(dd)]
        assert len(segs) == w["n_segments"]
        z, p = torch.cat([s[0] for s in segs])[None], torch.cat([s[1] for s in segs])[None]
        # the segments follow one another along the beam (near_k is the exit rounded to float32: half an ulp of slack)
        assert bool((z[0, 1:] >= z[0, :-1] * (1 - 2.0 ** -24)).all())
        _, depth = O.composite(p, z, TR.EPS32)
        sumw = float(RR.unnormalised(p)[0].sum())
        worst = max(worst, abs(float(w["sumw"]) - sumw) / max(sumw, 1e-300),
                    abs(float(w["depth"]) - float(depth)) / abs(float(depth)))
    print("chain against the concatenated compositing: worst relative difference", worst)
    assert worst <= 1e-12


def test_chain_step_arithmetic():
    T, W, N = TR.chain_step(2.0, 0.25, np.float64(1.0), np.float64(0.0), np.float64(0.0), eps=0.0)
    assert (T, W, N) == (0.75, 0.25, 0.5)
    T, W, N = TR.chain_step(4.0, 0.5, T, W, N, eps=0.0)
    assert (T, W, N) == (0.375, 0.625, 0.5 + 0.75 * 2.0)
    assert TR.chain_step(1.0, 1.5, np.float64(1.0), np.float64(0.0), np.float64(0.0))[0] == 0.0   # never below 0
    assert np.isnan(TR.chain_step(1.0, float("nan"), np.float64(1.0), np.float64(0.0), np.float64(0.0))[0])


# ----------------------------------------------------------------------------------------------- the rule
def _rule(boxes, row, pt, b0=0, K=16, seam_tol=1e-3):
    return TR.walk(np.asarray(boxes, np.float64), row, pt, b0, K, seam_tol, 0.0, TR.no_render)


def test_axis_aligned_beam_through_the_row_gaps_and_overlap():
    """Identity rotation, the point (1, 0, 0): d = (1, 0, 0) exactly, 1 / d = inf on two axes."""
    pt = np.array([1, 0, 0], np.float32)
    o, d, rng = TR.ray_od(IDENTITY, pt)
    assert d.tolist() == [1.0, 0.0, 0.0] and rng == 1.0
    w = _rule(TR.row_of_three()["boxes"], IDENTITY, pt)
    assert w["blocks"] == [0, 1, 2] and w["te"] == [2.5, 7.5, 12.5] and w["n_segments"] == 3
    assert _rule(TR.row_of_three()["boxes"], IDENTITY, pt, K=2)["blocks"] == [0, 1]
    # a 0.5 mm gap is joined at seam_tol = 1e-3, a 5 mm gap ends the chain, and seam_tol = 0 joins a shared face only
    assert _rule(TR.row_of_three(gap=5e-4)["boxes"], IDENTITY, pt)["blocks"] == [0, 1, 2]
    assert _rule(TR.row_of_three(gap=5e-3)["boxes"], IDENTITY, pt)["blocks"] == [0]
    assert _rule(TR.row_of_three(gap=5e-4)["boxes"], IDENTITY, pt, seam_tol=0.0)["blocks"] == [0]
    assert _rule(TR.row_of_three()["boxes"], IDENTITY, pt, seam_tol=0.0)["blocks"] == [0, 1, 2]
    # overlap: the earlier block owns the beam up to its own exit
    w = _rule(TR.row_of_three(overlap=1.0)["boxes"], IDENTITY, pt)
    assert w["blocks"] == [0, 1, 2] and w["te"] == [2.5, 7.5, 12.5]
    # a beam along -x leaves the map at once; one outside the y slab of the next box does not enter it
    assert _rule(TR.row_of_three()["boxes"], IDENTITY, np.array([-1, 0, 0], np.float32))["blocks"] == [0]
    high = [[-2.5, -2.5, -2.5, 2.5, 2.5, 2.5], [2.5, 1.0, -2.5, 7.5, 2.5, 2.5]]
    assert _rule(high, IDENTITY, pt)["blocks"] == [0]
    # the 65-block map: the search goes past index 63
    w = _rule(TR.sixty_five_blocks()["boxes"], IDENTITY, pt)
    assert w["blocks"] == [0, 64, 63]


def test_ties_go_to_the_lower_index_and_the_longest_stay_wins():
    pt = np.array([1, 0, 0], np.float32)
    first = [-2.5, -2.5, -2.5, 2.5, 2.5, 2.5]
    nxt, longer = [2.5, -2.5, -2.5, 7.5, 2.5, 2.5], [2.5, -2.5, -2.5, 9.0, 2.5, 2.5]
    assert _rule([first, nxt, nxt], IDENTITY, pt)["blocks"] == [0, 1]
    assert _rule([nxt, first, nxt], IDENTITY, pt, b0=1)["blocks"] == [1, 0]
    assert _rule([nxt, nxt, first], IDENTITY, pt, b0=2)["blocks"] == [2, 0]
    assert _rule([first, nxt, longer], IDENTITY, pt)["blocks"] == [0, 2]      # the largest tout
    assert _rule([first, longer, nxt], IDENTITY, pt)["blocks"] == [0, 1]
    # a copy of the start block is no candidate: its tout is not past te
    assert _rule([first, first], IDENTITY, pt)["blocks"] == [0]


def test_a_nan_ray_stops_after_segment_zero():
    boxes = TR.row_of_three()["boxes"]
    for pt in ([0, 0, 0], [float("nan"), 0, 1], [float("inf"), 0, 0]):
        w = _rule(boxes, IDENTITY, np.array(pt, np.float32))
        assert w["n_segments"] == 1 and w["last_block"] == 0, pt
    row = IDENTITY.copy()
    row[9] = float("nan")
    assert _rule(boxes, row, np.array([1, 0, 0], np.float32))["n_segments"] == 1


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_boxes_exits_increase_and_no_block_comes_twice(seed):
    rng = np.random.default_rng(seed)
    B = 12
    lo = rng.uniform(-5, 1, size=(B, 3))
    boxes = np.concatenate([lo, lo + rng.uniform(2, 6, size=(B, 3))], 1)
    boxes[0] = [-1, -1, -1, 1, 1, 1]
    from nof.registration import se3_exp
    row = TR.pose_rows(se3_exp((0.1, -0.2, 0.05, 0.3, -0.2, 0.5))[None])[0]
    longest = 0
    for p in RR.unit_directions(64, seed).float().numpy():
        w = _rule(boxes, row, p, K=16, seam_tol=0.05)
        te = w["te"]
        assert all(b > a for a, b in zip(te, te[1:])), te
        assert len(set(w["blocks"])) == len(w["blocks"]) <= B
        longest = max(longest, w["n_segments"])
        # every step obeys the rule as stated: entry within seam_tol of the exit, exit past it
        o, d, _ = TR.ray_od(row, p)
        for a, b, t in zip(w["blocks"], w["blocks"][1:], te):
            tin, tout = TR.box_interval(o, d, boxes[b])
            assert a != b and tin <= t + 0.05 and tout > t
            for j in range(B):   # and no other candidate stays longer
                tj_in, tj_out = TR.box_interval(o, d, boxes[j])
                if j != a and TR.is_candidate(tj_in, tj_out, t, 0.05):
                    assert tj_out < tout or (tj_out == tout and j >= b)
    assert longest >= 3


# ----------------------------------------------------------------------------------------------- the split cavity
def test_split_cavity_facts():
    """Carried into the second block every one of the 256 beams is a hit; clipped to the sensor's block fewer are; no
    sumw of either lies within 0.01 of the threshold, so the GPU test can ask for the exact counts."""
    f = TR.split_cavity_facts()
    c, t = f["clipped"], f["through"]
    hits_c, hits_t = int((c["sumw"] >= 0.5).sum()), int((t["sumw"] >= 0.5).sum())
    gap_c, gap_t = float(np.abs(c["sumw"] - 0.5).min()), float(np.abs(t["sumw"] - 0.5).min())
    arriving = t["arriving_T"]
    part = int(((arriving > 1e-6) & (arriving < 1 - 1e-6)).sum())
    print("split cavity: hits clipped", hits_c, "through", hits_t, "gaps", gap_c, gap_t, "min through sumw",
          float(t["sumw"].min()), "two segments", int((t["n_segments"] == 2).sum()), "partly transmitted", part)
    assert hits_t == 256 and hits_c == 163 and hits_c < 256
    assert gap_c > 0.01 and gap_t > 0.01
    assert part == 103
    assert (c["n_segments"] == 1).all() and (t["last_block"][t["n_segments"] == 2] == 1).all()
    # a clipped beam and its first segment are the same render
    one = t["n_segments"] == 1
    assert (t["depth"][one] == c["depth"][one]).all() and (t["sumw"][one] == c["sumw"][one]).all()


# ----------------------------------------------------------------------------------------------- operator
def test_the_operator_is_registered_with_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert T.through_op_names() == ["score_poses_through"]
    for name in T.through_op_names():
        assert name not in T.op_names() and name not in T.map_op_names()
        assert str(getattr(P, name).default._schema).startswith(f"pcnerf::{name}(")
    assert "score_poses_map" in T.map_op_names() and len(T.map_op_names()) == 6
    with FakeTensorMode():
        f64 = lambda *s: torch.empty(s, dtype=torch.float64)   # noqa: E731
        i32 = lambda *s: torch.empty(s, dtype=torch.int32)     # noqa: E731
        pts = torch.empty((7, 3))
        for want in (True, False):
            s4, d, w, n, b = P.score_poses_through(pts, f64(5, 12), i32(5), f64(3, 6), f64(3, 64), f64(3, 64), 0.05,
                                                   64, 128, 1e-10, 0.0, 0.5, 4, 1e-3, 1e-3, want)
            shape = (5, 7) if want else (0,)
            assert tuple(s4.shape) == (5, 4) and s4.dtype == torch.float64
            assert tuple(d.shape) == tuple(w.shape) == tuple(n.shape) == tuple(b.shape) == shape
            assert d.dtype == w.dtype == torch.float32 and n.dtype == b.dtype == torch.int32


def _call(K=4, tol=1e-3, tmin=1e-3, S=64, I=128, pts=None, ids=None, boxes=None):
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)   # noqa: E731
    pts = torch.rand(4, 3) + 0.5 if pts is None else pts
    ids = torch.zeros(3, dtype=torch.int32) if ids is None else ids
    boxes = f64(2, 6) if boxes is None else boxes
    return P.score_poses_through(pts, f64(3, 12), ids, boxes, f64(2, 64), f64(2, 64), 0.05, S, I, 1e-10, 0.0, 0.5, K,
                                 tol, tmin, False)


def test_the_operator_checks_its_operands_on_the_host():
    with pytest.raises(RuntimeError, match="no CPU path"):   # right layouts, wrong place
        _call()
    with pytest.raises(RuntimeError, match="points must be a contiguous torch.float32"):
        _call(pts=torch.rand(4, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="block_of_pose"):
        _call(ids=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="block_of_pose has shape"):
        _call(ids=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="folds_coarse has shape"):
        _call(boxes=torch.zeros(3, 6, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="at most 1024"):
        _call(S=512, I=513)
    for K in (0, 17, -1):
        with pytest.raises(RuntimeError, match="max_segments"):
            _call(K=K)
    for tol in (-1e-9, float("nan")):
        with pytest.raises(RuntimeError, match="seam_tol"):
            _call(tol=tol)
    for tmin in (-0.1, 1.0, float("nan")):
        with pytest.raises(RuntimeError, match="min_transmittance"):
            _call(tmin=tmin)


# ----------------------------------------------------------------------------------------------- C ABI
def test_symbol_declared_bound_and_exported():
    header = (Path(__file__).resolve().parents[1] / "include" / "pcnerf_hip.h").read_text()
    lib = _hip.lib()
    name = "pcnerf_score_poses_through"
    assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert name in _hip.exported_symbols() and hasattr(lib, name)
    decl = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, header).group(1)
    mapd = re.search(r"int\s+pcnerf_score_poses_map\s*\(([^;]*)\);", header).group(1)
    assert len(decl.split(",")) == len(_hip._SIGS[name][1]) == len(mapd.split(",")) + 5 == 26
    assert lib.pcnerf_abi_version() == 1


def test_argument_errors_reach_no_device():
    lib = _hip.lib()
    f = lib.pcnerf_score_poses_through
    buf = (ctypes.c_double * 64)()
    here = ctypes.cast(buf, ctypes.c_void_p)   # host memory: never read, every error comes before the launch

    def call(R=8, Pn=4, S=64, I=128, K=4, tol=1e-3, tmin=1e-3, ptr=None, nbytes=0, B=1):
        return f(ptr, R, ptr, Pn, ptr, B, ptr, 0.05, S, I, ptr, ptr, 1e-10, 0.0, 0.5, K, tol, tmin, ptr, nbytes, ptr,
                 None, None, None, None, None)

    assert call(Pn=0) == 0   # no poses: a no-op
    for kw, word in ((dict(R=-1), b"negative"), (dict(Pn=-1), b"negative"), (dict(), b"null"), (dict(R=0), b"null"),
                     (dict(K=0), b"max_segments"), (dict(K=17), b"max_segments"), (dict(Pn=0, K=0), b"max_segments"),
                     (dict(tol=-1e-9), b"seam_tol"), (dict(tol=float("nan")), b"seam_tol"),
                     (dict(tmin=1.0), b"min_transmittance"), (dict(tmin=-0.5), b"min_transmittance"),
                     (dict(tmin=float("nan")), b"min_transmittance"),
                     (dict(S=2, I=8), b"n_samples < 3"), (dict(I=0), b"n_importance < 1"),
                     (dict(S=512, I=513), b"> 1024"),
                     (dict(ptr=here, nbytes=63), b"workspace smaller"), (dict(ptr=here, B=0), b"n_blocks < 1")):
        assert call(**kw) == -1, word
        assert word in lib.pcnerf_last_error(), (word, lib.pcnerf_last_error())


# ----------------------------------------------------------------------------------------------- signatures
def _kw_defaults(fn, skip=()):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items()
            if p.kind is inspect.Parameter.KEYWORD_ONLY and k not in skip}


CHAIN = {"max_segments": 4, "seam_tol": 1e-3, "min_transmittance": 1e-3}


def test_signatures_follow_score_poses_map():
    names = lambda fn: list(inspect.signature(fn).parameters)   # noqa: E731
    assert _kw_defaults(L.score_poses_through, skip=CHAIN) == _kw_defaults(L.score_poses_map)
    assert {k: _kw_defaults(L.score_poses_through)[k] for k in CHAIN} == CHAIN
    assert names(L.score_poses_through)[:7] == ["block_map", "points_sensor", "poses", "blocks", *CHAIN]
    assert inspect.signature(L.score_poses_through).parameters["blocks"].default is None
    assert L.ThroughScores._fields == L.PoseScores._fields + ("n_segments", "last_block")
    assert names(L.synthesize_scan)[:4] == ["block_map", "directions_sensor", "pose", "blocks"]
    syn_kw = _kw_defaults(L.synthesize_scan)
    assert {k: syn_kw[k] for k in CHAIN} == CHAIN
    ref = _kw_defaults(L.score_poses_map)
    assert all(syn_kw[k] == ref[k] for k in ("N_samples", "N_importance", "near"))
    assert L.SynthesizedScan._fields == ("points_sensor", "depth", "hit", "n_segments", "last_block")
    pf = _kw_defaults(M.ParticleFilter.__init__)
    assert pf["through"] is False and {k: pf[k] for k in CHAIN} == CHAIN


def test_public_functions_refuse_host_scans_and_bad_chain_parameters():
    pts = torch.rand(16, 3) + 0.5
    poses = torch.eye(4, dtype=torch.float64)[None]
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.score_poses_through(None, pts, poses)
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.synthesize_scan(None, pts, poses[0])
    with pytest.raises(RuntimeError, match="max_segments"):
        T.check_through_params("score_poses_through", 17, 1e-3, 1e-3)
