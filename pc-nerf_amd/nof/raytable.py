"""Ray tables on the GPU -- the ray/AABB intersection that feeds the render path.

``build_train_rays`` produces the 15-column training rays of one LiDAR frame (nof/dataset/ipb2dmapping.py:736-768,
819-824) and ``build_view_rows`` the 13-column two-step rows grouped per ray plus ranges,
``other_interest_sub_nerf_number`` and the true-in flags (eval_kitti_render.py:675-803, 866-868).  Inputs are
float64 device tensors in the parent block's frame; child boxes are ``bounds6`` rows [xmin, ymin, zmin, xmax, ymax,
zmax] already grown by 0.025 m (ipb2dmapping.py:606-614).  The kernels are lib/libpcnerf_hip.so's
``pcnerf_build_train_rays`` / ``pcnerf_count_view_rows`` / ``pcnerf_emit_view_rows``.

``index="grid"`` runs the same row arithmetic on the children a uniform grid over the child centres
(``ChildGrid``, ``pcnerf_build_child_grid``) finds near the point or the ray instead of on every child
(``pcnerf_build_train_rays_grid`` / ``pcnerf_count_view_rows_grid`` / ``pcnerf_emit_view_rows_grid``); the rows
are the flat path's bit for bit.
"""
from __future__ import annotations

import struct

import torch

from . import _hip as H
from ._ops import _workspace


def _f64(t):
    H.require_device(t)
    return t.to(torch.float64).contiguous()


RAY_INDEXES = ("flat", "grid")


def _check_index(index):
    if index not in RAY_INDEXES:
        raise ValueError(f"index must be one of {RAY_INDEXES}, got {index!r}")


class ChildGrid:
    """Uniform grid over child centres, built on the device at first use and reusable for every frame of a scene.

    ``centers`` (C, 3) for train rows, or ``bounds6`` (C, 6) for two-step rows, which measure from the box
    midpoints (bounds6[:, :3] + bounds6[:, 3:]) / 2 -- pass exactly one.  ``cell`` is the requested edge; ``.cell``
    the edge in use (doubled until the grid has at most 2**22 cells), ``.dims`` the cells per axis, ``.n_cells``
    their product."""

    def __init__(self, centers=None, bounds6=None, cell=1.0):
        if (centers is None) == (bounds6 is None):
            raise ValueError("ChildGrid takes either centers or bounds6")
        if centers is not None:
            self.centers = _f64(centers).reshape(-1, 3)
        else:
            b = _f64(bounds6).reshape(-1, 6)
            self.centers = ((b[:, :3] + b[:, 3:]) / 2).contiguous()
        self.n_children = self.centers.shape[0]
        self.requested_cell = float(cell)
        self._buf = None

    def _build(self):
        if self._buf is None:
            L = H.lib()
            nbytes = L.pcnerf_child_grid_bytes(self.n_children)
            buf = torch.empty((nbytes,), dtype=torch.uint8, device=self.centers.device)
            H.check(L.pcnerf_build_child_grid(self.centers.data_ptr(), self.n_children, self.requested_cell,
                                              buf.data_ptr(), nbytes, H.stream_of(self.centers)))
            # header: magic u64, C i64, origin 3 f64, edge f64, dims 3 i32, n_cells i32
            hd = struct.unpack("<Qq4d4i", bytes(buf[:64].cpu().numpy()))
            self._cell, self._dims, self._n_cells = hd[5], tuple(hd[6:9]), hd[9]
            self._buf = buf
        return self._buf

    def ptr(self, n_children: int, device) -> int:
        if n_children != self.n_children or self.centers.device != device:
            raise ValueError(f"ChildGrid over {self.n_children} children on {self.centers.device} used with "
                             f"{n_children} children on {device}")
        return self._build().data_ptr()

    @property
    def cell(self) -> float:
        self._build()
        return self._cell

    @property
    def dims(self) -> tuple:
        self._build()
        return self._dims

    @property
    def n_cells(self) -> int:
        self._build()
        return self._n_cells


FACE_RULES = {"0606": 0, "0406": 1}   # compute_far_bound0606 (KITTI) / compute_far_bound0406 (MaiCity)


def build_train_rays(points, origin, centers, bounds6, parent6, surface_expand=0.05, face_rule="0606",
                     index="flat", grid=None) -> torch.Tensor:
    """15-column rows of one frame.  face_rule "0606" (kitti_dataload) drops rays that hit no face of their child
    box; "0406" (maicity_dataload) keeps every point in a child box and, like the reference's IndexError, raises
    when a ray hits fewer than two faces.  index "grid": the child lookup goes through ``grid`` (a ChildGrid over
    ``centers``; built for the call when None)."""
    _check_index(index)
    points, origin, centers, bounds6, parent6 = map(_f64, (points, origin, centers, bounds6, parent6))
    n, C = points.shape[0], bounds6.shape[0]
    L = H.lib()
    rows = torch.empty((n, 15), dtype=torch.float32, device=points.device)
    cnt = torch.empty((1,), dtype=torch.int64, device=points.device)
    short = torch.zeros((1,), dtype=torch.int32, device=points.device)
    if index == "grid":
        if grid is None:
            grid = ChildGrid(centers=centers)
        ws = _workspace(points.device, L.pcnerf_rays_grid_workspace_bytes(n))
        H.check(L.pcnerf_build_train_rays_grid(points.data_ptr(), n, origin.data_ptr(), centers.data_ptr(),
                                               bounds6.data_ptr(), C, parent6.data_ptr(), float(surface_expand),
                                               FACE_RULES[face_rule], grid.ptr(C, points.device), ws.data_ptr(),
                                               rows.data_ptr(), cnt.data_ptr(), short.data_ptr(),
                                               H.stream_of(points)))
    else:
        ws = _workspace(points.device, L.pcnerf_rays_workspace_bytes(n))
        H.check(L.pcnerf_build_train_rays(points.data_ptr(), n, origin.data_ptr(), centers.data_ptr(),
                                          bounds6.data_ptr(), C, parent6.data_ptr(), float(surface_expand),
                                          FACE_RULES[face_rule], ws.data_ptr(), rows.data_ptr(), cnt.data_ptr(),
                                          short.data_ptr(), H.stream_of(points)))
    if face_rule == "0406" and int(short):
        raise IndexError(f"compute_far_bound0406: {int(short)} ray(s) hit fewer than two faces of their child box "
                         "(the reference raises IndexError here)")
    return rows[:int(cnt)]


VIEW_RULES = {"kitti": 0, "maicity": 1}


def build_view_rows(points, origin, bounds6, parent6, method=2, rule="kitti", index="flat", grid=None):
    """-> (rows (M,13) float32, ranges (M,) float32, other (M,) int64, true_in (M,) bool).  rule "maicity":
    multi_frame_maicity's expansion step (0.005) and parent-far column.  index "grid": the candidate children come
    from ``grid`` (a ChildGrid over ``bounds6``; built for the call when None)."""
    _check_index(index)
    points, origin, bounds6, parent6 = map(_f64, (points, origin, bounds6, parent6))
    n, C = points.shape[0], bounds6.shape[0]
    L = H.lib()
    dev = points.device
    cnt = torch.empty((1,), dtype=torch.int64, device=dev)
    st = H.stream_of(points)
    args = (points.data_ptr(), n, origin.data_ptr(), bounds6.data_ptr(), C, parent6.data_ptr(), int(method),
            VIEW_RULES[rule])
    if index == "grid":
        if grid is None:
            grid = ChildGrid(bounds6=bounds6)
        args += (grid.ptr(C, dev),)
        count, emit = L.pcnerf_count_view_rows_grid, L.pcnerf_emit_view_rows_grid
        ws = _workspace(dev, L.pcnerf_rays_grid_workspace_bytes(n))
    else:
        count, emit = L.pcnerf_count_view_rows, L.pcnerf_emit_view_rows
        ws = _workspace(dev, L.pcnerf_rays_workspace_bytes(n))
    H.check(count(*args, ws.data_ptr(), cnt.data_ptr(), st))
    m = int(cnt)
    rows = torch.empty((m, 13), dtype=torch.float32, device=dev)
    ranges = torch.empty((m,), dtype=torch.float32, device=dev)
    other = torch.empty((m,), dtype=torch.int64, device=dev)
    tin = torch.empty((m,), dtype=torch.bool, device=dev)
    if m:
        H.check(emit(*args, ws.data_ptr(), rows.data_ptr(), ranges.data_ptr(), other.data_ptr(), tin.data_ptr(), st))
    return rows, ranges, other, tin
