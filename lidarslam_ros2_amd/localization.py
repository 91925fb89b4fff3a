"""Localising in a saved map, host side: the per-scan sequence of a localiser that registers every scan against a map.pcd the mapping
nodes wrote earlier, in the style of `frontend.FrontendReplay` — nothing here computes, every step is one call into the registration
object.

    map          set_map(records) / load_map(path, leaf): the whole map stays resident in HBM as pcl::PointXYZI records
    target       NOT the whole map: setInputTarget lays one int32 cell table over the bounding box of what it is given, and a map is
                 kilometres where a scan reaches a hundred metres.  The target is the WINDOW of the map around the pose
                 (Registration.setInputTargetWindow: the records whose voxel cell lies in a box of whole cells, cut out in input order on
                 the device).  The voxel lattice is anchored at the origin, so with leaf = the NDT resolution every cell of the window
                 holds the points the whole-map grid holds there: a registration that stays inside the window has the whole map's bits
    per scan     receive_cloud: setInputSourcePointCloud2 (range filter + VoxelGrid) -> align(previous pose, or the caller's guess) ->
                 the re-cut rule
    re-cut rule  two per-axis parameters in metres: `reach`, how far scan points lie from the pose, and `slack`.  A cut is
                 mapWindowAround(t, reach + slack, leaf) around the translation t of the pose.  The map is cut at set_initial_pose, and
                 again after an align whose translation has left the cut's centre by more than slack / 2 on any axis — before
                 receive_cloud returns, so the next scan finds its target.  A pose outside the current window altogether sets `lost`
                 (and the map is cut around it: it is never hidden)
    window=False the A/B arm, and fine for small maps: the whole map is set as target once (setInputTarget)
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .map_array import _as_float_records
from .registration import PC2_XYZI, MapWindow, _is_torch_cuda, mapWindowAround


@dataclass
class LocalizerParams:
    scan_min_range: float = 0.1            # the frontend's range filter and VoxelGrid of the incoming scan (scanmatcher_component.cpp:210-218, :324-328)
    scan_max_range: float = 100.0
    vg_size_for_input: float = 0.2
    reach: Tuple[float, float, float] = (100.0, 100.0, 30.0)   # [m] per axis: how far scan points lie from the pose
    slack: Tuple[float, float, float] = (20.0, 20.0, 10.0)     # [m] per axis: the margin of a cut; the map is cut again after slack / 2 of travel
    registration_method: str = "NDT"       # "NDT": the window's leaf is the object's resolution; "GICP": window_leaf
    window_leaf: float = 1.0


def needs_recut(translation, center, slack) -> bool:
    """The re-cut rule: has the pose left the centre of the current cut by more than slack / 2 on any axis?"""
    t, c, s = (np.asarray(v, np.float64)[:3] for v in (translation, center, slack))
    return bool(np.any(np.abs(t - c) > s / 2))


class Localizer:
    """`reg`: a registration object (NormalDistributionsTransform / GeneralizedIterativeClosestPoint) with its parameters set."""

    def __init__(self, reg, params: Optional[LocalizerParams] = None, window: bool = True):
        self.reg = reg
        self.p = params or LocalizerParams()
        if self.p.registration_method not in ("NDT", "GICP"):
            raise ValueError("registration_method must be \"NDT\" or \"GICP\"")
        self.use_window = bool(window)
        self.map = None                    # the resident map: (n, 32) uint8 pcl::PointXYZI records (a CUDA tensor when a device is there)
        self.window: Optional[MapWindow] = None
        self.center = np.zeros(3)          # translation the current window was cut around
        self.pose = np.eye(4, dtype=np.float32)
        self.lost = False                  # an align has ended outside the window it was registered against
        self.n_recuts = 0                  # cuts after the first
        self.n_target = 0
        self._whole_map_set = False
        self.last_search = None            # report of the last relocalize (Registration.searchPose)

    # -- the map -------------------------------------------------------------------------------------------------------------------
    def set_map(self, records):
        """The map as pcl::PointXYZI records (PC2_XYZI): a host array, uploaded once, or a CUDA tensor, kept as it is."""
        if not _is_torch_cuda(records):
            import torch

            host = np.ascontiguousarray(records).reshape(-1).view(np.uint8).reshape(-1, PC2_XYZI[0])
            records = torch.from_numpy(host).to(torch.device("cuda", getattr(self.reg, "_device", 0)))
        self.map = records
        self.window = None
        self._whole_map_set = False

    def load_map(self, path, leaf: Optional[float] = None):
        """map.pcd read on the device (loadPCDFile(device=True)); `leaf`: thinned there with that leaf size (voxelGridFilterMap)."""
        records = self.reg.loadPCDFile(path, PC2_XYZI, device=True)
        if leaf is not None:
            records = self.reg.voxelGridFilterMap(records, float(leaf))
        self.set_map(records)

    # -- the target ----------------------------------------------------------------------------------------------------------------
    def _leaf(self) -> float:
        return float(self.reg.getResolution()) if self.p.registration_method == "NDT" else float(self.p.window_leaf)

    def _cut(self, translation):
        half = np.asarray(self.p.reach, np.float64) + np.asarray(self.p.slack, np.float64)
        self.window = mapWindowAround(translation, half, self._leaf())
        self.center = np.asarray(translation, np.float64)[:3].copy()
        self.n_target = self.reg.setInputTargetWindow(self.map, self.window, PC2_XYZI)

    def set_initial_pose(self, T):
        if self.map is None:
            raise RuntimeError("set_map or load_map first")
        self.pose = np.asarray(T, np.float32).reshape(4, 4).copy()
        self.lost = False
        if not self.use_window:
            if not self._whole_map_set:
                records = _as_float_records(self.map, PC2_XYZI[0])
                self.reg.setInputTarget(records)
                self.n_target = int(records.shape[0])
                self._whole_map_set = True
            return
        self._cut(self.pose[:3, 3])

    # -- per scan ------------------------------------------------------------------------------------------------------------------
    def receive_cloud(self, payload, n_points: int, guess=None) -> np.ndarray:
        """One scan (raw PointCloud2 payload of pcl::PointXYZI records, host or CUDA) -> its registered pose (4x4 fp32)."""
        if self.use_window and self.window is None or not self.use_window and not self._whole_map_set:
            raise RuntimeError("set_initial_pose first")
        p = self.p
        self.reg.setInputSourcePointCloud2(payload, n_points, PC2_XYZI[0], PC2_XYZI[1], p.scan_min_range, p.scan_max_range, p.vg_size_for_input)
        self.reg.align(self.pose if guess is None else np.asarray(guess, np.float32))
        self.pose = self.reg.getFinalTransformation()
        if self.use_window:
            t = self.pose[:3, 3]
            outside = not self.window.contains(t)
            if outside:
                self.lost = True
            if outside or needs_recut(t, self.center, p.slack):
                self._cut(t)
                self.n_recuts += 1
        return self.pose

    # -- without a guess -----------------------------------------------------------------------------------------------------------
    def relocalize(self, payload, n_points: int, center=None, half_extent=(10.0, 10.0, 0.0), step=(1.0, 1.0, 1.0),
                   yaw_half_range: float = math.pi, yaw_step: float = math.radians(5.0), top_k: int = 16,
                   min_sep=(0.9, math.radians(7.5))) -> np.ndarray:
        """Find the pose of one scan with no guess inside NDT's basin of convergence (Registration.searchPose): the scan's NDT score
        over the lattice center +- half_extent (metres per axis, `step` apart) x yaw +- yaw_half_range (yaw_step apart), the distinct
        best top_k refined, the winner adopted.  `center` (4x4): defaults to the current pose.  The window is cut around the centre with
        reach + slack + half_extent, so every candidate finds its target.  Clears `lost`, applies the re-cut rule, keeps the report in
        `last_search`.  Nothing kept (no candidate puts a point into a voxel): raises, and pose, window and `lost` stay as they were."""
        if self.map is None:
            raise RuntimeError("set_map or load_map first")
        if self.p.registration_method != "NDT":
            raise RuntimeError("relocalize needs an NDT registration object")
        p = self.p
        C0 = np.asarray(self.pose if center is None else center, np.float32).reshape(4, 4)
        half_extent = np.asarray(half_extent, np.float64)
        n = [2 * int(round(half_extent[k] / step[k])) + 1 if step[k] > 0 else 1 for k in range(3)]
        n_yaw = max(1, 2 * int(round(yaw_half_range / yaw_step)) + (0 if yaw_half_range >= math.pi else 1)) if yaw_step > 0 else 1
        if self.use_window:
            half = np.asarray(p.reach, np.float64) + np.asarray(p.slack, np.float64) + half_extent
            window = mapWindowAround(C0[:3, 3], half, self._leaf())
            n_target = self.reg.setInputTargetWindow(self.map, window, PC2_XYZI)   # keeps nothing: raises, the previous target stays
        elif not self._whole_map_set:
            records = _as_float_records(self.map, PC2_XYZI[0])
            self.reg.setInputTarget(records)
            self.n_target, self._whole_map_set = int(records.shape[0]), True
        self.reg.setInputSourcePointCloud2(payload, n_points, PC2_XYZI[0], PC2_XYZI[1], p.scan_min_range, p.scan_max_range, p.vg_size_for_input)
        pose, _, report = self.reg.searchPose(C0, n, step, n_yaw, yaw_step, top_k, min_sep[0], min_sep[1])
        if pose is None:
            if self.use_window and self.window is not None:   # the target the tracker had: the next receive_cloud finds it again
                self.reg.setInputTargetWindow(self.map, self.window, PC2_XYZI)
            raise RuntimeError("relocalize: no candidate pose puts a scan point into a map voxel")
        self.last_search = report
        self.pose = pose
        self.lost = False
        if self.use_window:
            self.window, self.center, self.n_target = window, np.asarray(C0[:3, 3], np.float64).copy(), n_target
            t = self.pose[:3, 3]
            if not self.window.contains(t) or needs_recut(t, self.center, p.slack):
                self._cut(t)
                self.n_recuts += 1
        return self.pose
