"""Uniform-grid child index of the ray tables (nof.raytable.ChildGrid, index="grid") vs the CPU oracle
(oracle/rays_cpu.py) and vs the flat kernels.  Every comparison is exact: the grid only chooses which children the
flat kernels' arithmetic is applied to, so rows, ranges, ``other`` and ``true_in`` must be equal bit for bit.

Scenes come from the seeded generator below (child boxes of half-extent 0.1..0.6 m scattered over +-ext, 80 % of the
points inside a box, the rest around the scene, also outside the grid) and from hand-built cases that a grid walk can
get wrong: a box behind the origin, centres on cell boundaries, the 0.65 m filter's rounding, distance ties,
child-index order with more than 64 hits, degenerate inputs."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import rays_cpu as RC

ORIGIN = (0.3, -0.2, -0.5)
SCENES = {"c10": (10, 300, 5, ORIGIN, 3), "c37": (37, 300, 5, ORIGIN, 6), "c1500": (1500, 600, 5, ORIGIN, 20),
          "c1500_outside": (1500, 600, 5, (-40, 5, 3), 20)}
CELLS = (0.37, 1.0, 5.0, 1000.0)   # 1000: a single cell; C = 10: the rings reach the whole grid
VIEW_MODES = ((2, "kitti"), (1, "kitti"), (2, "maicity"))


def scene(C, n, seed, origin, ext, frac_in=0.8):
    r = np.random.default_rng(seed)
    ctr = np.stack([r.uniform(-ext, ext, C), r.uniform(-ext, ext, C), r.uniform(-2.0, 0.5, C)], 1)
    half = r.uniform(0.1, 0.6, (C, 3)); lo, hi = ctr - half, ctr + half
    b6 = np.concatenate([lo - 0.025, hi + 0.025], 1)
    k = r.integers(0, C, n); pts = lo[k] + r.uniform(0, 1, (n, 3)) * (hi[k] - lo[k])
    m = int(n * (1 - frac_in))
    pts[:m] = np.stack([r.uniform(-ext-5, ext+5, m), r.uniform(-ext-5, ext+5, m), r.uniform(-2.5, 1.0, m)], 1)
    return pts, np.asarray(origin, float), ctr, b6, np.array([-ext-1, -ext-1, -2.7]), np.array([ext+1, ext+1, 1.2])


@functools.lru_cache(maxsize=None)
def named_scene(name):
    return scene(*SCENES[name])


@functools.lru_cache(maxsize=None)
def oracle_train(name):
    pts, o, ctr, b6, plo, phi = named_scene(name)
    return RC.build_train_rays(pts, o, ctr, b6, plo, phi, 0.05)


@functools.lru_cache(maxsize=None)
def oracle_view(name, method, rule):
    pts, o, ctr, b6, plo, phi = named_scene(name)
    return RC.build_view_rows(pts, o, b6, plo, phi, method, rule=rule)


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def train_rows(pts, o, ctr, b6, plo, phi, **kw):
    from nof.raytable import build_train_rays
    return build_train_rays(t(pts), t(o), t(ctr), t(b6), t(np.concatenate([plo, phi])), **kw).cpu().numpy()


def view_rows(pts, o, b6, plo, phi, **kw):
    from nof.raytable import build_view_rows
    return tuple(x.cpu().numpy() for x in build_view_rows(t(pts), t(o), t(b6), t(np.concatenate([plo, phi])), **kw))


def assert_view_equal(got, want):
    for g, w, what in zip(got, want, ("rows", "ranges", "other", "true_in")):
        assert g.shape == w.shape, (what, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=what)


def raw_train(pts, o, ctr, b6, plo, phi, rule, grid=None):
    """The C entry points themselves, for rule 0406's n_short (nof.raytable raises instead of returning it)."""
    from nof import _hip as H
    from nof._ops import _workspace
    L = H.lib()
    P, O, Cn, B, P6 = t(pts), t(o), t(ctr), t(b6), t(np.concatenate([plo, phi]))
    n, C = P.shape[0], B.shape[0]
    rows = torch.empty((n, 15), dtype=torch.float32, device="cuda")
    cnt = torch.empty((1,), dtype=torch.int64, device="cuda")
    short = torch.zeros((1,), dtype=torch.int32, device="cuda")
    head = (P.data_ptr(), n, O.data_ptr(), Cn.data_ptr(), B.data_ptr(), C, P6.data_ptr(), 0.05, rule)
    if grid is None:
        ws = _workspace(P.device, L.pcnerf_rays_workspace_bytes(n))
        fn = L.pcnerf_build_train_rays
    else:
        ws = _workspace(P.device, L.pcnerf_rays_grid_workspace_bytes(n))
        fn, head = L.pcnerf_build_train_rays_grid, head + (grid.ptr(C, P.device),)
    H.check(fn(*head, ws.data_ptr(), rows.data_ptr(), cnt.data_ptr(), short.data_ptr(), H.stream_of(P)))
    return rows[:int(cnt)].cpu().numpy(), int(short)


# ------------------------------------------------------------------------------------------ 1. vs the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", list(SCENES))
def test_train_rows_grid_match_oracle(name, cell):
    from nof.raytable import ChildGrid
    pts, o, ctr, b6, plo, phi = named_scene(name)
    grid = ChildGrid(centers=t(ctr), cell=cell)
    got = train_rows(pts, o, ctr, b6, plo, phi, index="grid", grid=grid)
    want = oracle_train(name)
    assert got.shape == want.shape and len(got) > 100
    np.testing.assert_array_equal(got, want)
    if cell == 1000.0:
        assert grid.n_cells == 1 and grid.dims == (1, 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", list(SCENES))
def test_view_rows_grid_match_oracle(name, cell):
    from nof.raytable import ChildGrid
    pts, o, ctr, b6, plo, phi = named_scene(name)
    grid = ChildGrid(bounds6=t(b6), cell=cell)
    for method, rule in VIEW_MODES:
        got = view_rows(pts, o, b6, plo, phi, method=method, rule=rule, index="grid", grid=grid)
        assert len(got[0]) > 100
        assert_view_equal(got, oracle_view(name, method, rule))


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", list(SCENES))
def test_train_rows_0406_grid_match_flat(name, cell):
    """Rule 0406 against the flat kernel (the oracle raises where the origin lies inside a child box): rows and
    the count of rays with fewer than two face hits."""
    from nof.raytable import ChildGrid
    sc = named_scene(name)
    rows_f, short_f = raw_train(*sc, 1)
    rows_g, short_g = raw_train(*sc, 1, grid=ChildGrid(centers=t(sc[2]), cell=cell))
    assert rows_g.shape == rows_f.shape and len(rows_f) > 100
    np.testing.assert_array_equal(rows_g, rows_f)
    assert short_g == short_f


# ------------------------------------------------------------------------------------------ 2. constructed cases
BIG = (np.array([-50.0, -50.0, -50.0]), np.array([50.0, 50.0, 50.0]))


@pytest.mark.gpu
def test_box_behind_the_origin_is_hit():
    """The 0.65 m filter measures from the whole line: this box's centre has a negative projection on the ray
    (0.492 m from the line) and the ray still enters the box at 0.2236 and leaves at 0.4472."""
    o = np.zeros(3)
    d = np.array([1.0, 0.5, 0.0]) / np.sqrt(1.25)
    pts = np.stack([3.0 * d, 0.3 * d])
    b6 = np.array([[-1.0, 0.1, -0.5, 0.4, 0.7, 0.5]])
    want = RC.build_view_rows(pts, o, b6, *BIG, 2)
    assert want[0].shape == (2, 13) and abs(want[0][0, 6] - 0.2236068) < 1e-6
    for cell in (0.37, 1.0):
        got = view_rows(pts, o, b6, *BIG, method=2, index="grid", grid=None if cell == 1.0 else _grid_b6(b6, cell))
        assert_view_equal(got, want)
    assert_view_equal(view_rows(pts, o, b6, *BIG, method=2), want)


def _grid_b6(b6, cell):
    from nof.raytable import ChildGrid
    return ChildGrid(bounds6=t(b6), cell=cell)


@functools.lru_cache(maxsize=None)
def lattice():
    """98 unit-spaced children whose centres sit exactly on the cell boundaries of a 1 m grid, and rays along the
    axes (direction components exactly zero), along diagonals and through centres."""
    g = np.arange(-3, 4, dtype=float)
    ctr = np.array([[x, y, z] for z in (-1.0, 0.0) for y in g for x in g])
    b6 = np.concatenate([ctr - (0.45 + 0.025), ctr + (0.45 + 0.025)], 1)
    o = np.array([0.5, 0.5, -0.5])
    pts = []
    for a in range(3):
        for s in (1.3, -1.3, 2.5, -2.5):
            e = np.zeros(3)
            e[a] = s
            pts.append(o + e)
    for v in ((1, 1, 0), (1, -1, 0), (1, 0, 1), (-1, 2, 0.5), (3, 1, -0.2)):
        for m in (0.7, 1.9):
            pts.append(o + m * np.array(v, float))
    pts = np.concatenate([np.array(pts), ctr[::7]])
    return pts, o, ctr, b6, np.array([-5.0, -5.0, -3.0]), np.array([5.0, 5.0, 2.0])


@pytest.mark.gpu
def test_lattice_centres_on_cell_boundaries():
    pts, o, ctr, b6, plo, phi = lattice()
    want_t = RC.build_train_rays(pts, o, ctr, b6, plo, phi, 0.05)
    want_v = RC.build_view_rows(pts, o, b6, plo, phi, 2)
    groups = np.flatnonzero(want_v[0][:, 12] >= 0)
    # what the oracle gives for this construction: 16 train rows, 24 groups of 90 rows, the largest group 6
    assert len(want_t) == 16 and (len(groups), len(want_v[0])) == (24, 90) and want_v[2].max() + 1 == 6
    got_t = train_rows(pts, o, ctr, b6, plo, phi, index="grid")
    np.testing.assert_array_equal(got_t, want_t)
    assert_view_equal(view_rows(pts, o, b6, plo, phi, method=2, index="grid"), want_v)
    assert_view_equal(view_rows(pts, o, b6, plo, phi, method=1, index="grid"),
                      RC.build_view_rows(pts, o, b6, plo, phi, 1))


@pytest.mark.gpu
def test_filter_boundary_follows_the_computed_distance():
    """Single children with centres (7, y, 0), y around 0.65, on a ray along +x: the oracle's computed distance
    decides membership (it rejects y = 0.65 and both neighbours, so it is not the true distance), and the walk's
    pad has to deliver every centre the computed distance accepts."""
    o, pts = np.zeros(3), np.array([[10.0, 0.0, 0.0]])
    ys = [np.nextafter(0.65, 0), 0.65, np.nextafter(0.65, 1), 0.65 - 1e-9, 0.65 - 3e-10, 0.65 - 1e-12,
          0.65 + 1e-12, 0.65 + 3e-10, 0.65 + 1e-9, 0.65 + 5e-7, 0.6, 0.7]
    member = []
    for y in ys:
        c = np.array([7.0, y, 0.0])
        half = np.array([0.3, 0.7, 0.3])   # the box spans the ray, so a child that passes the filter is hit
        b6 = np.concatenate([c - half, c + half])[None]
        want = RC.build_view_rows(pts, o, b6, *BIG, 2)
        member.append(len(want[0]))
        assert_view_equal(view_rows(pts, o, b6, *BIG, method=2, index="grid"), want)
        assert_view_equal(view_rows(pts, o, b6, *BIG, method=2, index="grid", grid=_grid_b6(b6, 0.37)), want)
    assert member[-2] == 1 and member[-1] == 0 and member[9] == 0


@pytest.mark.gpu
def test_distance_ties_keep_index_order():
    """30 centres are copies of lower-indexed ones, so exact distance ties exist; grid against flat only (the
    KD-tree's tie order is not defined)."""
    pts, o, ctr, b6, plo, phi = (a.copy() for a in named_scene("c1500"))
    r = np.random.default_rng(9)
    for _ in range(30):
        j, k = sorted(r.choice(len(ctr), 2, replace=False))
        ctr[k], b6[k] = ctr[j], b6[j]
    for cell in (0.37, 1.0):
        from nof.raytable import ChildGrid
        got = train_rows(pts, o, ctr, b6, plo, phi, index="grid", grid=ChildGrid(centers=t(ctr), cell=cell))
        np.testing.assert_array_equal(got, train_rows(pts, o, ctr, b6, plo, phi))
        for method in (2, 1):
            assert_view_equal(view_rows(pts, o, b6, plo, phi, method=method, index="grid", grid=_grid_b6(b6, cell)),
                              view_rows(pts, o, b6, plo, phi, method=method))


@pytest.mark.gpu
def test_hits_are_taken_in_child_index_order_and_overflow_keeps_the_lowest():
    """70 thin boxes stacked along one ray (from the origin (0, 0.15, 0) through (30, 0.15, 0)) in shuffled child
    order: the walk meets them in x order, the flat scan in index order.  Only 64 hits are kept: the 64 lowest
    indices; method 1 keeps the lowest index (the parent box ends at x = 1, so column 10 is that box's far face)."""
    x0 = 2.0 + 0.2 * np.arange(70)
    b6 = np.stack([x0, np.full(70, 0.05), np.full(70, -0.1), x0 + 0.1, np.full(70, 0.25), np.full(70, 0.1)], 1)
    b6 = b6[np.random.default_rng(3).permutation(70)]
    o, pts = np.array([0.0, 0.15, 0.0]), np.array([[30.0, 0.15, 0.0]])
    plo, phi = np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0])
    flat = view_rows(pts, o, b6, plo, phi, method=2)
    got = view_rows(pts, o, b6, plo, phi, method=2, index="grid")
    assert_view_equal(got, flat)
    assert got[0].shape == (64, 13)
    np.testing.assert_array_equal(got[0][:, 6], np.sort(b6[:64, 0]).astype(np.float32))
    flat1 = view_rows(pts, o, b6, plo, phi, method=1)
    got1 = view_rows(pts, o, b6, plo, phi, method=1, index="grid")
    assert_view_equal(got1, flat1)
    assert got1[0].shape == (1, 13) and got1[0][0, 10] == np.float32(b6[0, 3])


@pytest.mark.gpu
def test_degenerate_inputs():
    from nof.raytable import ChildGrid
    pts, o, ctr, b6, plo, phi = (a.copy() for a in named_scene("c37"))
    pts[5] = o                                    # a point on the origin: no direction
    sub = pts[:40]
    rows, _, _, _ = view_rows(sub, o, b6, plo, phi, method=2, index="grid")
    assert_view_equal(view_rows(sub, o, b6, plo, phi, method=2, index="grid"),
                      view_rows(sub, o, b6, plo, phi, method=2))
    assert_view_equal(view_rows(sub[5:6], o, b6, plo, phi, method=2, index="grid"),
                      view_rows(sub[5:6], o, b6, plo, phi, method=2))
    assert len(view_rows(sub[5:6], o, b6, plo, phi, method=2, index="grid")[0]) == 0 and len(rows) > 0
    np.testing.assert_array_equal(train_rows(sub, o, ctr, b6, plo, phi, index="grid"),
                                  train_rows(sub, o, ctr, b6, plo, phi))
    same = np.tile(ctr[:1], (12, 1))              # identical centres: a one-cell grid
    g = ChildGrid(centers=t(same), cell=0.5)
    assert g.dims == (1, 1, 1) and g.n_cells == 1 and g.cell == 0.5
    np.testing.assert_array_equal(train_rows(sub, o, same, b6[:12], plo, phi, index="grid", grid=g),
                                  train_rows(sub, o, same, b6[:12], plo, phi))
    with pytest.raises(RuntimeError, match="need points and >= 10 child boxes"):
        train_rows(sub, o, ctr[:9], b6[:9], plo, phi)
    with pytest.raises(RuntimeError, match="need points and >= 10 child boxes"):
        train_rows(sub, o, ctr[:9], b6[:9], plo, phi, index="grid")
    bad = ctr.copy()
    bad[3, 1] = np.inf
    with pytest.raises(RuntimeError, match="non-finite"):
        ChildGrid(centers=t(bad)).n_cells
    with pytest.raises(RuntimeError, match="cell edge"):
        ChildGrid(centers=t(ctr), cell=0.0).n_cells
    wide = ctr.copy()                             # 2e5 m across at a 0.5 m edge: the edge doubles under the cell cap
    wide[0, :2], wide[1, :2] = -1e5, 1e5
    g = ChildGrid(centers=t(wide), cell=0.5)
    assert g.n_cells <= 1 << 22 and g.cell > 0.5 and g.n_cells == g.dims[0] * g.dims[1] * g.dims[2]
    np.testing.assert_array_equal(train_rows(sub, o, wide, b6, plo, phi, index="grid", grid=g),
                                  train_rows(sub, o, wide, b6, plo, phi))


# ------------------------------------------------------------------------------------------ 3. the shell's size
@pytest.mark.gpu
def test_shell_child_count_grid_matches_flat_and_oracle_prefix():
    """15,333 children (the reference training shell's count): grid = flat on every output, and the rows of the
    first 512 points (rows come out in point order, so a prefix) equal the oracle's."""
    pts, o, ctr, b6, plo, phi = scene(15333, 4096, 5, ORIGIN, 62)
    got_t = train_rows(pts, o, ctr, b6, plo, phi, index="grid")
    np.testing.assert_array_equal(got_t, train_rows(pts, o, ctr, b6, plo, phi))
    got_v = view_rows(pts, o, b6, plo, phi, method=2, index="grid")
    assert_view_equal(got_v, view_rows(pts, o, b6, plo, phi, method=2))
    assert_view_equal(view_rows(pts, o, b6, plo, phi, method=1, index="grid"),
                      view_rows(pts, o, b6, plo, phi, method=1))
    want_t = RC.build_train_rays(pts[:512], o, ctr, b6, plo, phi, 0.05)
    want_v = RC.build_view_rows(pts[:512], o, b6, plo, phi, 2)
    assert 0 < len(want_t) < len(got_t) and 0 < len(want_v[0]) < len(got_v[0])
    np.testing.assert_array_equal(got_t[:len(want_t)], want_t)
    assert_view_equal(tuple(x[:len(want_v[0])] for x in got_v), want_v)


# ------------------------------------------------------------------------------------------ 4. callers
def write_scene(tmp, name="kitti_frames"):
    """The fixture as the reference's inputs (as tests/test_dataset.py writes it): <tmp>/pcd/<n>.pcd and a poses.txt
    whose rows pose_first.. are real."""
    from nof import io as nio
    g = golden(name)
    os.makedirs(os.path.join(tmp, "pcd"), exist_ok=True)
    for k, v in g.items():
        if k.startswith("f"):
            nio.write_pcd(os.path.join(tmp, "pcd", f"{k[1:]}.pcd"), v)
    ident = "1 0 0 0 0 1 0 0 0 0 1 0"
    first = int(g["pose_first"])
    with open(os.path.join(tmp, "poses.txt"), "w") as fh:
        for _ in range(first):
            fh.write(ident + "\n")
        for row in g["poses"]:
            fh.write(" ".join(repr(float(v)) for v in row) + "\n")
    return os.path.join(tmp, "pcd"), os.path.join(tmp, "poses.txt"), g


DS, DE, INTEREST = 1150, 1155, 20.0


@pytest.mark.gpu
def test_kitti_dataload_ray_index(tmp_path):
    from nof import dataset as D
    root, pose_path, _ = write_scene(str(tmp_path))
    kw = dict(data_start=DS, data_end=DE, cloud_size_val=64, range_delete_x=3, range_delete_y=2,
              range_delete_z=1.25, sub_nerf_test_num=0, surface_expand=0.05, over_height=0.168, over_low=-2.0,
              interest_x=INTEREST, interest_y=INTEREST, pose_path=pose_path, re_loaddata=1, device="cuda")
    for split in ("train", "val"):
        flat = D.kitti_dataload(root, split=split, ray_index="flat", **kw)
        grid = D.kitti_dataload(root, split=split, ray_index="grid", **kw)
        assert flat.rays.shape[0] > 100
        assert torch.equal(flat.rays, grid.rays) and torch.equal(flat.ranges, grid.ranges)


@pytest.mark.gpu
def test_eval_scene_ray_index(tmp_path):
    import eval_kitti_render as E
    root, pose_path, _ = write_scene(str(tmp_path))
    args = f"""--dataset kitti --root_dir {root} --pose_path {pose_path} --data_start {DS} --data_end {DE}
     --range_delete_x 3 --range_delete_y 2 --range_delete_z 1.25 --over_height 0.168 --over_low -2.0
     --interest_x {INTEREST} --interest_y {INTEREST}"""
    h = E.get_opts(args.split())
    f = E.test_frame_ids(DS, DE)[0]
    flat = E.Scene(h, "cuda", ray_index="flat").view_rows(f, 2)
    sc = E.Scene(h, "cuda", ray_index="grid")
    grid = sc.view_rows(f, 2)
    assert flat[0].shape[0] > 50 and sc._grid is not None
    for a, b in zip(flat, grid):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_child_grid_reused_across_frames():
    from nof.raytable import ChildGrid
    _, o, ctr, b6, plo, phi = named_scene("c1500")
    gt, gv = ChildGrid(centers=t(ctr)), ChildGrid(bounds6=t(b6))
    assert gt.cell == 1.0 and gt.n_cells == gt.dims[0] * gt.dims[1] * gt.dims[2] > 1000
    for seed in (6, 7, 8):
        pts = scene(1500, 400, seed, ORIGIN, 20)[0]    # another frame's points over the same children
        np.testing.assert_array_equal(train_rows(pts, o, ctr, b6, plo, phi, index="grid", grid=gt),
                                      train_rows(pts, o, ctr, b6, plo, phi, index="grid"))
        assert_view_equal(view_rows(pts, o, b6, plo, phi, index="grid", grid=gv),
                          view_rows(pts, o, b6, plo, phi, index="grid"))
    with pytest.raises(ValueError):
        train_rows(pts, o, ctr[:100], b6[:100], plo, phi, index="grid", grid=gt)


# ------------------------------------------------------------------------------------------ 5. without a GPU
GRID_SYMBOLS = ("pcnerf_child_grid_bytes", "pcnerf_build_child_grid", "pcnerf_rays_grid_workspace_bytes",
                "pcnerf_build_train_rays_grid", "pcnerf_count_view_rows_grid", "pcnerf_emit_view_rows_grid")


def test_library_exports_grid_symbols():
    from nof import _hip
    L = ctypes.CDLL(_hip.LIB_PATH)
    for name in GRID_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _hip.exported_symbols()


def test_grid_size_queries():
    from nof import _hip
    L = _hip.lib()

    def align(b):
        return (b + 255) // 256 * 256
    # header, cell_start at the 2^22-cell cap, cell_items and the sort's scratch
    assert L.pcnerf_child_grid_bytes(15333) == 256 + align(((1 << 22) + 1) * 4) + 2 * align(15333 * 4) == 16900608
    # the flat workspace, then 8 bytes (round) and 64 child indices per point
    assert L.pcnerf_rays_grid_workspace_bytes(120000) == L.pcnerf_rays_workspace_bytes(120000) + 120000 * (8 + 64 * 4)
    assert L.pcnerf_rays_grid_workspace_bytes(120000) == 33120256


def test_grid_argument_errors_are_reported_before_launch():
    from nof import _hip
    L = _hip.lib()
    assert L.pcnerf_build_child_grid(None, 10, 1.0, None, 0, None) != 0
    assert b"null" in L.pcnerf_last_error()
    assert L.pcnerf_build_train_rays_grid(None, 0, None, None, None, 0, None, 0.05, 0, None, None, None, None, None,
                                          None) != 0
    assert b"null" in L.pcnerf_last_error()
    assert L.pcnerf_count_view_rows_grid(None, 0, None, None, 0, None, 2, 0, None, None, None, None) != 0
    assert b"null" in L.pcnerf_last_error()
    assert L.pcnerf_emit_view_rows_grid(None, 0, None, None, 0, None, 2, 0, None, None, None, None, None, None,
                                        None) != 0
    assert b"null" in L.pcnerf_last_error()


def test_grid_refuses_cpu_tensors():
    from nof.raytable import ChildGrid, build_train_rays, build_view_rows
    pts, o, ctr, b6, plo, phi = (torch.as_tensor(a) for a in named_scene("c10"))
    p6 = torch.cat([plo, phi])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ChildGrid(centers=ctr)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ChildGrid(bounds6=b6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        build_train_rays(pts, o, ctr, b6, p6, index="grid")
    with pytest.raises(RuntimeError, match="no CPU path"):
        build_view_rows(pts, o, b6, p6, index="grid")
    with pytest.raises(ValueError):
        ChildGrid()
