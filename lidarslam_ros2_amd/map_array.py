"""lidarslam_msgs/MapArray, host side: the list of SubMaps both nodes pass around, and what they do with it when they publish the map
 — ScanMatcherComponent::publishMap (scanmatcher_component.cpp:529-552) and the map half of
GraphBasedSlamComponent::doPoseAdjustment (graph_based_slam_component.cpp:321-368) — behind `Registration.assembleMap`.

The submaps are `loop_closure.SubMap`s, so `search_loop(reg, ma.submaps, ...)` takes them unchanged.  A pose is stored the way the
message stores it: the position as given and the quaternion Eigen's Quaterniond(Matrix3d) makes of the rotation block
(scanmatcher_component.cpp:394-398).  The map is moved by the pose that round trip yields (tf2::fromMsg, :538-542), not by the
registration's float matrix: that is what the reference publishes.

Nothing here computes on the points: every map is one call into the registration object.
"""
from __future__ import annotations

from typing import List

import numpy as np

from . import _capi
from .loop_closure import SubMap
from .posemath import matrix_from_pose, quaternion_from_matrix
from .registration import PC2_XYZI, ScanContextParams, VisibilityParams, _is_torch_cuda


def _as_float_records(records, point_step: int):
    """A record buffer as the (n, point_step / 4) float32 view search_loop and setInputTargetFrames take (no copy)."""
    if _is_torch_cuda(records):
        import torch

        t = records if records.is_contiguous() else records.contiguous()
        if t.dtype == torch.float32 and t.dim() == 2:
            return t
        return t.view(-1).view(torch.uint8).view(-1, point_step).view(torch.float32)
    a = np.ascontiguousarray(records)
    if a.dtype == np.float32 and a.ndim == 2:
        return a
    return a.reshape(-1).view(np.uint8).reshape(-1, point_step).view(np.float32)


class MapArray:
    """`layout`: (point_step, (x, y, z, intensity or None)) of the submaps' records AND of the published map (pcl::PointXYZI's by default)."""

    def __init__(self, layout=PC2_XYZI):
        self.layout = layout
        self.submaps: List[SubMap] = []
        self._published = None        # resident buffer of extend_published: uint8, capacity * point_step bytes
        self._published_submaps = 0   # submaps it holds
        self._published_records = 0   # records it holds
        self._first_record = [0]
        self._sc_table = None         # resident descriptor table of scan_contexts: (capacity, R, S) float32
        self._sc_count = 0            # submaps it holds
        self._sc_params = None
        self._di_table = None         # resident eroded depth images of depth_images: (capacity, H, 4 W) float32
        self._di_count = 0            # submaps it holds
        self._di_params = None
        self.last_static = None       # (records kept, records removed) of the last map assembled with remove_moving

    def __len__(self) -> int:
        return len(self.submaps)

    def append(self, records, pose4x4, distance: float) -> SubMap:
        """One SubMap message: `records` (pose-local, this object's layout; numpy array or CUDA tensor), the registered pose, the
        accumulated travel distance (updateMap, scanmatcher_component.cpp:471-480)."""
        P = np.asarray(pose4x4, np.float64)
        sm = SubMap(cloud=_as_float_records(records, int(self.layout[0])), position=tuple(float(v) for v in P[:3, 3]),
                    orientation=tuple(float(v) for v in quaternion_from_matrix(P[:3, :3])), distance=float(distance))
        self.submaps.append(sm)
        return sm

    def publish_map(self, reg, out=None, leaf=None, remove_moving=None):
        """publishMap (:529-552): every submap moved by its stored pose, concatenated.  -> (records, first_record).  `leaf`: a leaf
        size thins the map on the device before it leaves the call (Registration.voxelGridFilterMap) -> (records, None).
        `remove_moving`: VisibilityParams — the records a neighbouring keyframe saw through are left out first
        (Registration.assembleMapStatic over depth_images; first_record then indexes the kept records)."""
        return self._map(reg, None, out, leaf, remove_moving)

    def modified_map(self, reg, poses, out=None, leaf=None, remove_moving=None):
        """The map half of doPoseAdjustment (:321-368): every submap moved by the optimiser's estimate for it (4x4 fp64 each).
        records[first_record[i]:first_record[i + 1]] is modified_map_array.submaps[i].cloud (:343-351).  -> (records, first_record).
        `leaf`, `remove_moving`: as for publish_map (the votes are taken under the same `poses`)."""
        return self._map(reg, poses, out, leaf, remove_moving)

    def _map(self, reg, poses, out, leaf, remove_moving):
        if remove_moving is None:
            if leaf is None:
                return reg.assembleMap(self.submaps, poses, self.layout, self.layout, out)
            return reg.assembleMap(self.submaps, poses, self.layout, self.layout, out, leaf)
        if leaf is None:
            records, first, removed = reg.assembleMapStatic(self.submaps, self.depth_images(reg, remove_moving), remove_moving, poses,
                                                            self.layout, self.layout, out)
            self.last_static = (int(records.shape[0]), removed)
            return records, first
        static = self._static_on_device(reg, poses, remove_moving)
        return reg.voxelGridFilterMap(static, float(leaf), self.layout, self.layout, out), None

    def _static_on_device(self, reg, poses, remove_moving):
        """The static map as records that stay on the device, whatever the residency of the submaps."""
        records, _, removed = reg.assembleMapStatic(self.submaps, self.depth_images(reg, remove_moving), remove_moving, poses, self.layout,
                                                    self.layout, None, device_out=True)
        self.last_static = (int(records.shape[0]), removed)
        return records

    def save_map(self, reg, path, poses=None, data="ascii", leaf=None, remove_moving=None) -> int:
        """`pcl::io::savePCDFileASCII("map.pcd", *map_ptr)` at the end of doPoseAdjustment (:369): the map by the stored poses, or by
        the optimiser's `poses` when given (4x4 fp64 each), written to `path` as ASCII PCD with fields x y z intensity — one call into
        the registration object, the map never visits the host as records.  `data`: "ascii" (the default: those bytes), "binary" or
        "binary_compressed" (the LZF stream compressed on the device).  `leaf`: a leaf size thins the map on the device before it is
        written (Registration.voxelGridFilterMap's records; their number: reg.getSavedMapPoints()).  `remove_moving`:
        VisibilityParams — the static map (publish_map) is assembled on the device, thinned there when `leaf` is given, and written
        from that buffer (Registration.savePCDFile); self.last_static = (kept, removed).  -> the file's size in bytes."""
        if remove_moving is not None:
            static = self._static_on_device(reg, poses, remove_moving)
            if leaf is not None:
                static = reg.voxelGridFilterMap(static, float(leaf), self.layout, self.layout)
            return reg.savePCDFile(path, static, self.layout, data)
        if leaf is not None:   # the map thinned with this leaf size on the device before it is written
            return reg.saveMapPCDFile(path, self.submaps, poses, self.layout, data, leaf)
        if data == "ascii":
            return reg.saveMapPCDFileASCII(path, self.submaps, poses, self.layout)
        return reg.saveMapPCDFile(path, self.submaps, poses, self.layout, data)

    def stored_poses(self) -> np.ndarray:
        """(n, 4, 4) fp64: the pose every stored SubMap message stands for (Eigen::fromMsg, graph_based_slam_component.cpp:279-281)."""
        return np.stack([matrix_from_pose(s.position, s.orientation) for s in self.submaps])

    def pose_adjustment(self, reg, loop_edges, num_adjacent: int = 5, max_iterations: int = 10, result=None):
        """The optimiser half of doPoseAdjustment (:267-319): the stored poses as vertices (vertex 0 fixed), the odometry edges of
        :289-303, one edge per accepted `LoopEdge` of `loop_edges` (what the reference keeps in loop_edges_; rejected ones are skipped),
        optimize(max_iterations) on the device.  -> (n, 4, 4) fp64 poses for `modified_map`.  `result`: a list that receives the
        pose_graph.PoseGraphResult.  The solve's band is min(num_adjacent, LSR_POSE_GRAPH_MAX_BAND = 8): with num_adjacent > 8 the
        odometry edges longer than 8 count as edges outside the band, like every loop edge.  Up to LSR_POSE_GRAPH_LONG_MAX_OFFBAND_EDGES
        = 1024 of those are served (lsr_optimize_pose_graph_long: every loop edge a node has accepted over a few laps; past 64 the dense
        part of the solve is a blocked Cholesky); beyond that the call raises (invalid argument) and changes nothing."""
        from . import pose_graph

        poses = self.stored_poses()
        edges = pose_graph.adjacent_edges(poses, num_adjacent)
        edges += [(int(e.pair_id[0]), int(e.pair_id[1]), np.asarray(e.relative_pose, np.float64)) for e in loop_edges
                  if getattr(e, "accepted", True)]
        out, res = reg.optimizePoseGraph(poses, edges, max_iterations, min(int(num_adjacent), _capi.POSE_GRAPH_MAX_BAND))
        if result is not None:
            result.append(res)
        return out

    def extend_published(self, reg):
        """publishMap for a frontend whose stored poses never change: only the submaps added since the last call are moved, appended to
        a resident buffer that grows geometrically (on the device when the submaps are).  -> (records, first_record) of the whole map,
        a view of that buffer, valid until the next call."""
        step = int(self.layout[0])
        new = self.submaps[self._published_submaps:]
        if new:
            add = int(sum(int(s.cloud.shape[0]) for s in new))
            need = self._published_records + add
            cap = 0 if self._published is None else self._published.shape[0] // step
            if need > cap:
                grown = self._empty(max(need, 2 * cap, 1) * step, any(_is_torch_cuda(s.cloud) for s in self.submaps), reg)
                if self._published_records:
                    grown[: self._published_records * step] = self._published[: self._published_records * step]
                self._published = grown
            _, first = reg.assembleMap(new, None, self.layout, self.layout, self._published[self._published_records * step:])
            self._first_record += [self._published_records + int(v) for v in first[1:]]
            self._published_submaps = len(self.submaps)
            self._published_records = need
        if self._published is None:
            self._published = self._empty(step, False, reg)
        n = self._published_records
        return self._published[: n * step].reshape(n, step), np.array(self._first_record, np.int64)

    def scan_contexts(self, reg, params: ScanContextParams = ScanContextParams()):
        """The Scan Context descriptor of every submap, for loop_closure.search_loop_appearance: a resident table (on the device when
        the submaps are) that grows geometrically and is extended by the submaps added since the last call only — a descriptor depends
        on its own cloud alone.  Other `params` than last time start the table again.  -> (n, R, S) float32, a view of that table,
        valid until the next call."""
        params = ScanContextParams(*params)
        R, S = int(params.num_rings), int(params.num_sectors)
        if self._sc_params != params:
            self._sc_table, self._sc_count, self._sc_params = None, 0, params
        n = len(self.submaps)
        if n > self._sc_count:
            cap = 0 if self._sc_table is None else int(self._sc_table.shape[0])
            if n > cap:
                on_device = any(_is_torch_cuda(s.cloud) for s in self.submaps)
                grown = self._empty(max(n, 2 * cap, 1) * R * S * 4, on_device, reg)
                if on_device:
                    import torch

                    grown = grown.view(torch.float32).reshape(-1, R, S)
                else:
                    grown = grown.view(np.float32).reshape(-1, R, S)
                if self._sc_count:
                    grown[: self._sc_count] = self._sc_table[: self._sc_count]
                self._sc_table = grown
            reg.scanContext(self.submaps[self._sc_count:], params, self.layout, self._sc_table[self._sc_count:])
            self._sc_count = n
        if self._sc_table is None:
            return np.zeros((0, R, S), np.float32)
        return self._sc_table[:n]

    def depth_images(self, reg, params: VisibilityParams = VisibilityParams()):
        """The eroded depth image of every submap, for Registration.assembleMapStatic: a resident table (on the device when the
        submaps are) that grows geometrically and is extended by the submaps added since the last call only — an image depends on
        its own cloud alone, not on any pose.  Other image parameters than last time start the table again.  -> (n, height,
        4 face_width) float32, a view of that table, valid until the next call."""
        params = VisibilityParams(*params)
        key = (int(params.face_width), int(params.height), float(params.max_tan_elevation), float(params.min_range), float(params.max_range),
               tuple(float(v) for v in params.sensor_origin))   # what an image depends on
        H, W4 = params.shape
        if self._di_params != key:
            self._di_table, self._di_count, self._di_params = None, 0, key
        n = len(self.submaps)
        if n > self._di_count:
            cap = 0 if self._di_table is None else int(self._di_table.shape[0])
            if n > cap:
                on_device = any(_is_torch_cuda(s.cloud) for s in self.submaps)
                grown = self._empty(max(n, 2 * cap, 1) * H * W4 * 4, on_device, reg)
                if on_device:
                    import torch

                    grown = grown.view(torch.float32).reshape(-1, H, W4)
                else:
                    grown = grown.view(np.float32).reshape(-1, H, W4)
                if self._di_count:
                    grown[: self._di_count] = self._di_table[: self._di_count]
                self._di_table = grown
            reg.depthImages(self.submaps[self._di_count:], params, self.layout, self._di_table[self._di_count:])
            self._di_count = n
        if self._di_table is None:
            return np.zeros((0, H, W4), np.float32)
        return self._di_table[:n]

    @staticmethod
    def _empty(nbytes: int, on_device: bool, reg):
        if on_device:
            import torch

            return torch.empty(nbytes, dtype=torch.uint8, device=torch.device("cuda", getattr(reg, "_device", 0)))
        return np.zeros(nbytes, np.uint8)
