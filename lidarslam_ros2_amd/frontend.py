"""The frontend's per-scan sequence, host side: what ScanMatcherComponent::receiveCloud and ::updateMap do around the
registration object (scanmatcher/src/scanmatcher_component.cpp:296-356 and :436-481), written against the method names of
`lidarslam_ros2_amd.registration` so that the same loop drives the gfx950 core (bench.py `frontend_stream`,
tests/test_frontend_stream_gpu.py) and — through an adapter with the same methods — the CPU oracle the tests compare with.

    per scan (receiveCloud)      raw PointCloud2 payload -> range filter (:210-218) -> VoxelGrid(vg_size_for_input) (:324-328) ->
                                 setInputSource (:329) -> align(previous pose) (:353) -> getFinalTransformation (:356)
    every trans_for_mapupdate m  (updateMap) VoxelGrid(vg_size_for_map) of the scan (:442-446), kept with the registered pose as the newest
                                 submap (:466-478); target = that scan + the num_targeted_cloud - 1 submaps before it, each moved by its
                                 pose and concatenated (:448-464); setInputTarget at the start of the next callback (:304-307)
    use_imu                      (:204-208) the raw payload is de-skewed once, on the device, before anything else reads it
                                 (deskewPointCloud2); the de-skewed records feed the scan path AND the map side, as `tmp_ptr` does;
                                 IMU messages arrive through receive_imu (:501-527)
    sensor mount                 (:188-199) a payload in the sensor frame is moved into the robot frame first: inside the ingest launch of
                                 the scan side and of the `mapper` (setInputSourcePointCloud2(sensor_transform=...)), by
                                 transformPointCloud2 in front of the de-skew (use_imu) and on the host map path's copy
    use_odom                     (:333-348) the guess of align is odomGuess(previous pose, previous odometry, odometry of this scan)
    registration_method "GICP"   the same loop; the assembled window is put through VoxelGrid(vg_size_for_input) before setInputTarget
                                 (:308-316): setInputTargetFramesFiltered + prepareTarget (the target's covariances) on the map side
    map_array                    (optional) the lidarslam_msgs/MapArray updateMap keeps (:466-481): every keyframe with the pose the message
                                 stores and `latest_distance_ += trans_`; with map_publish_every = k every k-th update ends with
                                 publishMap (:485-490, :529-552) — the new keyframes appended to a map that stays resident

Nothing here computes: every step is one call into the registration object.

The reference runs updateMap on a worker thread (:427-434) and takes the new target over at the start of a later callback
(:298-320: `mapping_future_.wait_for(0s)` — whenever the thread happens to be done).  Two things model that here:
  * `async_update=True` + a `builder` object: the map side — filter of the new keyframe (`mapper`), assembly of the window AND the
    voxel-grid build (`builder.setInputTargetFrames`, on the builder's own stream) — runs on a worker thread while the callback thread
    registers the next scans; the hand-over is `reg.shareTargetOf(builder)` (lsr_share_target: a pointer swap, the old target goes back
    to the builder for recycling).  The reference builds the voxel grid INSIDE the callback (`registration_->setInputTarget`, :307);
    here the callback never builds a grid.
  * `swap_lag`: the reference's hand-over is racy (it depends on how long the thread took); a replay must be deterministic, so the
    lag is a parameter — the target of an update triggered by scan k is in place for scan k + 1 + swap_lag (0 = before the very next
    scan, which is what a 10 Hz sensor sees with a map side of a fraction of a millisecond; 1 = one scan later, i.e. the next scan is
    registered WHILE the map side runs).  The callback that is due waits for the worker (`swap_wait_seconds`).  While an update is
    pending no new one is triggered (`!mapping_flag_`, :427).  The serial replay with the same lag gives the same poses bit for bit.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

PC2_XYZI = (32, (0, 4, 8, 16))   # pcl::PointXYZI as pcl::toROSMsg lays it out: point_step 32, x@0 y@4 z@8 intensity@16


def as_pc2_payload(xyz: np.ndarray, intensity: Optional[np.ndarray] = None) -> np.ndarray:
    """(n,3) fp32 -> (n,32) uint8 PointCloud2 payload in pcl::PointXYZI's layout."""
    n = int(xyz.shape[0])
    rec = np.zeros((n, 8), np.float32)
    rec[:, :3] = xyz
    if intensity is not None:
        rec[:, 4] = intensity
    return rec.view(np.uint8).reshape(n, 32)


def _records(payload: np.ndarray) -> np.ndarray:
    """(m,32) uint8 PointXYZI payload -> the same bytes as (m,8) fp32 records (what setInputTargetFrames takes)."""
    return np.ascontiguousarray(payload).view(np.float32).reshape(-1, 8)


@dataclass
class FrontendParams:   # scanmatcher_component.cpp:36-60 (declare_parameter defaults; vg sizes as BASELINE cfg 1/2 uses them)
    vg_size_for_input: float = 0.2
    vg_size_for_map: float = 0.1
    trans_for_mapupdate: float = 1.5
    scan_min_range: float = 0.1
    scan_max_range: float = 100.0
    num_targeted_cloud: int = 10
    registration_method: str = "NDT"   # :98-125 — "NDT" or "GICP"
    gicp_solver: str = "gauss_newton"  # GICP mode: the inner optimiser of `reg` — "gauss_newton", or "bfgs" (the reference's own schedule)
    use_imu: bool = False              # :78 — de-skew the raw scan with the IMU queue before the range filter (:204-208)
    scan_period: float = 0.1           # :80 — lidar_undistortion_.setScanPeriod
    # :193-195 — lookupTransform(robot_frame_id_, msg->header.frame_id): where the sensor sits on the robot (mapping_car.launch.py:28
    # mounts it at 1.2 0 2.0).  The identity (the default) means the payloads are in the robot frame already: no transform is made
    sensor_translation: tuple = (0.0, 0.0, 0.0)
    sensor_rotation_xyzw: tuple = (0.0, 0.0, 0.0, 1.0)
    use_odom: bool = False             # :333-348 — the alignment guess follows the odometry between two scans (receive_cloud's `odom`)


@dataclass
class FrontendResult:
    poses: List[np.ndarray] = field(default_factory=list)          # registered pose of every scan (4x4)
    iterations: List[int] = field(default_factory=list)
    points_kept: List[int] = field(default_factory=list)
    scan_seconds: List[float] = field(default_factory=list)         # scan in -> pose out (hand-over of a due target + preprocess + setInputSource + align)
    update_seconds: List[float] = field(default_factory=list)       # map updates: VoxelGrid(map) + assembly + setInputTarget (on the worker thread when asynchronous)
    update_at: List[int] = field(default_factory=list)              # index of the scan after which each update was triggered
    swap_wait_seconds: List[float] = field(default_factory=list)    # asynchronous replay: what the due callback waited for the worker + the pointer swap
    swap_at: List[int] = field(default_factory=list)                # index of the scan whose callback took each new target over
    publish_seconds: List[float] = field(default_factory=list)      # publishMap at the end of a map update (map_publish_every): extend_published


class FrontendReplay:
    """`reg`: a registration object (lidarslam_ros2_amd.NormalDistributionsTransform or an adapter with the same methods).
    `to_device` (optional): maps a kept submap — (m,8) fp32 pcl::PointXYZI records on the host — to what `reg.setInputTargetFrames`
    should be given (e.g. a CUDA tensor, so that the keyframes stay resident in HBM); identity when None."""

    def __init__(self, reg, params: FrontendParams | None = None, to_device=None, mapper=None, builder=None, async_update: bool = False,
                 swap_lag: int = 0, map_array=None, map_publish_every: int = 0):
        self.reg = reg
        self.p = params or FrontendParams()
        if self.p.registration_method not in ("NDT", "GICP"):
            raise ValueError("registration_method must be \"NDT\" or \"GICP\" (scanmatcher_component.cpp:121-124)")
        if self.p.gicp_solver not in ("gauss_newton", "bfgs"):
            raise ValueError("gicp_solver must be \"gauss_newton\" or \"bfgs\"")
        if self.p.registration_method == "GICP":   # the object that aligns follows the parameter (a builder never aligns)
            if hasattr(reg, "setOptimizer"):
                reg.setOptimizer(self.p.gicp_solver)
            elif self.p.gicp_solver != "gauss_newton":
                raise ValueError("gicp_solver = \"bfgs\" needs a registration object with setOptimizer")
        self.to_device = to_device or (lambda a: a)
        # `mapper` (optional): a second registration object whose input-source slot serves as the map side's filter — with it and a
        # device-resident payload the new keyframe (range filter + VoxelGrid(vg_size_for_map)) is produced and kept in HBM
        self.mapper = mapper
        # `builder` (optional): the object that builds the targets (same method and resolution as `reg`, its own stream); `reg` takes
        # them over with shareTargetOf.  Without it `reg` builds its own targets.
        self.builder = builder
        self.async_update = bool(async_update)
        if self.async_update and builder is None:
            raise ValueError("an asynchronous map update needs a builder object (the callback's object must not build targets)")
        self.swap_lag = int(swap_lag)
        # `map_array` (optional): a lidarslam_ros2_amd.map_array.MapArray that receives every keyframe as a SubMap message would carry it
        # (the window logic below keeps its own `self.submaps`); `map_publish_every` = k > 0: every k-th map update ends with publishMap.
        # The reference's trigger is wall-clock (map_publish_period, :485-490); a replay must be deterministic, so updates are counted.
        self.map_array = map_array
        self.map_publish_every = int(map_publish_every)
        if self.map_publish_every > 0 and map_array is None:
            raise ValueError("map_publish_every needs a map_array")
        self.published = None            # (records, first_record) of the last publishMap
        self._latest_distance = 0.0      # latest_distance_ (:474)
        self._n_updates = 0
        self._publish_seconds: list = []
        self._pool = None
        self._pending = None             # (due scan index, future or job, trigger time)
        self._n_scans = 0
        self.submaps: list = []          # [(payload as given to setInputTargetFrames, pose 4x4 f64)]
        self.pose = np.eye(4)
        self.key_position = np.zeros(3)
        t, q = tuple(float(v) for v in self.p.sensor_translation), tuple(float(v) for v in self.p.sensor_rotation_xyzw)
        if len(t) != 3 or len(q) != 4:
            raise ValueError("sensor_translation is x y z, sensor_rotation_xyzw a quaternion x y z w")
        self._mount = None if (t, q) == ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)) else (t, q)
        self._previous_odom = np.eye(4, dtype=np.float32)   # previous_odom_mat_
        if self.p.use_imu:
            self.reg.imuReset(self.p.scan_period)

    def receive_imu(self, orientation_xyzw, angular_velocity, linear_acceleration, stamp: float) -> bool:
        """One sensor_msgs/Imu message (receiveImu, :501-527); ignored unless use_imu (:503)."""
        if not self.p.use_imu:
            return False
        return self.reg.receiveImu(orientation_xyzw, angular_velocity, linear_acceleration, stamp)

    def initialise(self, frames_xyz, frame_poses, pose0):
        """The map the drive starts from: the keyframes so far (sensor frame, already VoxelGrid(vg_size_for_map)-filtered) and their poses."""
        self.close()
        self.submaps = [(self.to_device(_records(as_pc2_payload(f))), np.asarray(P, np.float64)) for f, P in zip(frames_xyz, frame_poses)]
        if self.map_array is not None:   # the MapArray holds the whole map, not the window: distance = path length over the keyframes
            self._latest_distance, self._n_updates = 0.0, 0
            for k, (rec, P) in enumerate(self.submaps):
                if k:
                    self._latest_distance += float(np.linalg.norm(P[:3, 3] - self.submaps[k - 1][1][:3, 3]))
                self.map_array.append(rec, P, self._latest_distance)
        self.submaps = self.submaps[-self.p.num_targeted_cloud:]
        self._set_target()
        self._hand_over()
        self.pose = np.asarray(pose0, np.float64)
        self.key_position = np.asarray(frame_poses[-1], np.float64)[:3, 3].copy()
        self._n_scans = 0
        self._previous_odom = np.eye(4, dtype=np.float32)

    def close(self):
        """Drains a pending update and stops the worker thread."""
        if self._pending is not None and hasattr(self._pending[1], "result"):
            self._pending[1].result()
        self._pending = None
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def _set_target(self):
        # newest first, as updateMap concatenates (:448-464); the voxel grid does not depend on the order
        window = self.submaps[-self.p.num_targeted_cloud:][::-1]
        obj = self.builder or self.reg
        if self.p.registration_method == "GICP":
            # the GICP branch (:308-316): the assembled window goes through VoxelGrid(vg_size_for_input) before setInputTarget (here
            # the order does matter: it is the order of the filter's float sums), and what the reference's first align against the new
            # target would compute lazily — the target's k-NN covariances — is built here, on the object and the thread that built the
            # target, so that the hand-over stays a pointer swap and the scan that takes the target over registers like any other
            obj.setInputTargetFramesFiltered([w[0] for w in window], [w[1] for w in window], self.p.vg_size_for_input)
            obj.prepareTarget()
            return
        obj.setInputTargetFrames([w[0] for w in window], [w[1] for w in window])

    def _hand_over(self):
        if self.builder is not None:
            self.reg.shareTargetOf(self.builder)

    def _update_job(self, payload, n_points, payload_host, T, trans: float = 0.0, mount=None):
        """updateMap (:436-481) up to and including the target of the next scans; -> seconds.  `mount`: the payload is still in the
        sensor frame (a mounted sensor without IMU: the scan side moved it inside its ingest) and is moved here the same way."""
        step, offs = PC2_XYZI
        t2 = time.perf_counter()
        if self.mapper is not None and hasattr(payload, "is_cuda") and payload.is_cuda:
            # the whole map side on the device: (sensor -> robot frame +) range filter + VoxelGrid(vg_size_for_map) into the mapper's
            # source slot, from there into a keyframe buffer in HBM (lsr_set_input_source_pc2 / _tf + lsr_get_source_pc2_device)
            kw = {} if mount is None else {"sensor_transform": mount}
            self.mapper.setInputSourcePointCloud2(payload, n_points, step, offs, self.p.scan_min_range, self.p.scan_max_range,
                                                  self.p.vg_size_for_map, **kw)
            keyframe = self.mapper.getInputSourceDeviceRecords()
        else:
            src = payload if payload_host is None else payload_host
            if hasattr(src, "is_cuda") and src.is_cuda:
                src = src.cpu().numpy()      # (a de-skewed device payload and no mapper object: the host-side filter needs a copy)
            host = np.asarray(src).reshape(n_points, step)
            if mount is not None:            # doTransform (:195) of the host copy, ahead of the range mask as in the callback
                host = (self.builder or self.reg).transformPointCloud2(host, n_points, step, offs, mount[0], mount[1]).reshape(n_points, step)
            # updateMap filters the cloud the callback received, i.e. AFTER the subscription's range filter (:210-218: horizontal range,
            # open interval, in double) — a host-side mask here, as in the reference
            xy = host[:, :8].copy().view(np.float32).astype(np.float64)
            r = np.sqrt(xy[:, 0] ** 2 + xy[:, 1] ** 2)
            ranged = np.ascontiguousarray(host[(self.p.scan_min_range < r) & (r < self.p.scan_max_range)])
            filtered = (self.builder or self.reg).voxelGridFilterPointCloud2(ranged, int(ranged.shape[0]), step, offs, self.p.vg_size_for_map)
            keyframe = self.to_device(_records(filtered))
        self.submaps.append((keyframe, T.copy()))
        self.submaps = self.submaps[-self.p.num_targeted_cloud:]
        self._set_target()
        dt = time.perf_counter() - t2
        if self.map_array is not None:
            # :471-480 — latest_distance_ += trans_, the pose as the message stores it; :485-490 — publishMap, on its own clock
            self._latest_distance += trans
            self.map_array.append(keyframe, T, self._latest_distance)
            self._n_updates += 1
            if self.map_publish_every > 0 and self._n_updates % self.map_publish_every == 0:
                t3 = time.perf_counter()
                self.published = self.map_array.extend_published(self.builder or self.reg)
                self._publish_seconds.append(time.perf_counter() - t3)
        return dt

    def _settle(self, out: FrontendResult, force: bool = False):
        """Start of a callback (:298-320): a target that is due is taken over (the callback waits for the worker if it must)."""
        if self._pending is None:
            return
        due, job, _ = self._pending
        if not force and self._n_scans < due:
            return
        t0 = time.perf_counter()
        if hasattr(job, "result"):
            out.update_seconds.append(job.result())      # the worker's own clock
        else:
            out.update_seconds.append(job())             # serial replay: the update runs here, between two scans
            t0 = time.perf_counter()
        if self._publish_seconds:
            out.publish_seconds.extend(self._publish_seconds)
            self._publish_seconds = []
        self._hand_over()
        out.swap_wait_seconds.append(time.perf_counter() - t0)
        out.swap_at.append(self._n_scans)
        self._pending = None

    def receive_cloud(self, payload, n_points: int, out: FrontendResult, payload_host=None, scan_time: Optional[float] = None, odom=None):
        """One LiDAR message.  `payload`: the raw PointCloud2 data (host array or CUDA tensor), in the sensor frame when the parameters
        name a mount; `payload_host`: a host copy for the map update (the reference's callback holds the cloud on the host anyway);
        defaults to `payload`.  `scan_time`: the message's header stamp [s]; needed with use_imu, where the payload is (moved into
        the robot frame and) de-skewed first and the de-skewed records replace it for everything that follows (the host copy
        included: the map side reads them back when it needs one).  `odom`: the 4x4 odom_frame -> robot_frame of the scan's stamp
        (:336-343); needed with use_odom — the reference logs a failed lookup and goes on with a default-constructed transform, which
        is not reproduced: ValueError."""
        step, offs = PC2_XYZI
        if self.p.use_imu and scan_time is None:
            raise ValueError("use_imu needs the scan's header stamp (scan_time)")
        if self.p.use_odom and odom is None:
            raise ValueError("use_odom needs the odometry of the scan's stamp (odom)")
        t0 = time.perf_counter()
        mount = self._mount
        if self.p.use_imu:
            if mount is not None:        # :188-208 — doTransform, then adjustDistortion on the transformed cloud (in place: the buffer is ours)
                payload = self.reg.transformPointCloud2(payload, n_points, step, offs, mount[0], mount[1])
                payload, _ = self.reg.deskewPointCloud2(payload, n_points, step, offs, scan_time, out=payload)
                mount = None
            else:
                payload, _ = self.reg.deskewPointCloud2(payload, n_points, step, offs, scan_time)
            payload_host = None
        if self.async_update:
            self._settle(out)            # inside the scan's clock: what the callback really waits
        # without IMU a mounted sensor's payload is moved inside the ingest launch (lsr_set_input_source_pc2_tf): no pass of its own
        kw = {} if mount is None else {"sensor_transform": mount}
        kept = self.reg.setInputSourcePointCloud2(payload, n_points, step, offs, self.p.scan_min_range, self.p.scan_max_range,
                                                  self.p.vg_size_for_input, **kw)
        guess = self.pose.astype(np.float32)
        if self.p.use_odom:              # :333-348
            from .registration import odomGuess
            odom = np.asarray(odom, np.float64).astype(np.float32)    # odom_affine.matrix().cast<float>()
            guess = odomGuess(guess, self._previous_odom, odom)
            self._previous_odom = odom
        self.reg.align(guess)
        T = np.asarray(self.reg.getFinalTransformation(), np.float64)
        t1 = time.perf_counter()
        self.pose = T
        out.poses.append(T); out.points_kept.append(int(kept)); out.scan_seconds.append(t1 - t0)
        out.iterations.append(int(self.reg.getFinalNumIteration()))
        self._n_scans += 1
        # displacement since the last map update (:412-427): trans_ >= trans_for_mapupdate_ && !mapping_flag_
        trans = float(np.linalg.norm(T[:3, 3] - self.key_position))
        if self._pending is None and trans >= self.p.trans_for_mapupdate:
            self.key_position = T[:3, 3].copy()
            out.update_at.append(len(out.poses) - 1)
            job = (lambda p=payload, n=n_points, h=payload_host, TT=T.copy(), d=trans, m=mount: self._update_job(p, n, h, TT, d, m))
            if self.async_update:
                if self._pool is None:
                    from concurrent.futures import ThreadPoolExecutor
                    self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="lsr-map")
                job = self._pool.submit(job)
            self._pending = (self._n_scans + self.swap_lag, job, t1)
        if not self.async_update:
            self._settle(out)            # the serial replay does the due update between two scans, on its own clock (update_seconds)

    def finish(self, out: FrontendResult):
        """End of a drive: an update still pending is completed (its time is reported, nothing registers against it)."""
        self._settle(out, force=True)
        self.close()
