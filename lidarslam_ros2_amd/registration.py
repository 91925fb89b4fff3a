"""Host-side mirror of the `pcl::Registration` surface the reference's two nodes call
(SURVEY.md §8b), on top of the C ABI in include/lidarslam_reg.h.

Method names, argument meaning and defaults follow pclomp / PCL so call sites read like the
reference's: scanmatcher/src/scanmatcher_component.cpp:105-120,275,307,329,353-376 and
graph_based_slam/src/graph_based_slam_component.cpp:64-82,181,227-231.

Clouds may be numpy arrays (host) or torch CUDA tensors (already resident in HBM): shape (n, c)
float32 with c >= 3 and xyz in the first three columns (c = 8 is pcl::PointXYZI's 32-byte record).
4x4 transforms are numpy (4,4) float32, row/col indexed normally (converted to Eigen's
column-major order at the boundary).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _capi as capi

DIRECT7, DIRECT1, DIRECT26, KDTREE = capi.DIRECT7, capi.DIRECT1, capi.DIRECT26, capi.KDTREE
PC2_XYZI = (32, (0, 4, 8, 16))   # pcl::PointXYZI as pcl::toROSMsg lays it out: (point_step, (x, y, z, intensity or None))


class MapWindow(NamedTuple):
    """lsr_map_window: a leaf size and, per axis, the inclusive range lo .. hi of absolute voxel cells (cell = floor(p / leaf))."""
    leaf: float
    lo: Tuple[int, int, int]
    hi: Tuple[int, int, int]

    def contains(self, p) -> bool:
        """Whether the point p (fp32 arithmetic, the cut's own predicate) lies in the window."""
        f = np.floor(np.asarray(p, np.float32)[:3] * (np.float32(1.0) / np.float32(self.leaf)))
        return bool(np.all((np.asarray(self.lo, np.float32) <= f) & (f <= np.asarray(self.hi, np.float32))))


def mapWindowAround(center, half_extent, leaf: float) -> MapWindow:
    """The window of whole cells of size `leaf` that covers center +- half_extent (metres, per axis) through lsr_map_window_around;
    needs no device.  A cell of 2^24 or beyond raises (LSR_ERR_INDEX_OVERFLOW)."""
    c = (C.c_double * 3)(*[float(v) for v in center])
    e = (C.c_double * 3)(*[float(v) for v in half_extent])
    w = capi.MapWindow()
    capi.check(capi.load().lsr_map_window_around(c, e, C.c_float(leaf), C.byref(w)), "mapWindowAround")
    return MapWindow(float(w.leaf), tuple(int(v) for v in w.lo), tuple(int(v) for v in w.hi))


def _poses_to_col16(poses) -> np.ndarray:
    """(count, 4, 4) row/col indexed -> (count, 16) in Eigen's column-major order."""
    P = np.asarray(poses, np.float32)
    if P.ndim == 2:
        P = P[None]
    if P.ndim != 3 or P.shape[1:] != (4, 4):
        raise ValueError("poses must be (count, 4, 4)")
    return np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(-1, 16)


def poseLattice(center, n=(1, 1, 1), step=(1.0, 1.0, 1.0), n_yaw: int = 1, yaw_step: float = 0.0) -> np.ndarray:
    """The pose lattice of lsr_pose_lattice_poses around `center` (4x4): n[0] x n[1] x n[2] translations `step` apart times n_yaw
    headings yaw_step apart, all centred -> (count, 4, 4) fp32, candidate ((m n[2] + k) n[1] + j) n[0] + i.  Needs no device."""
    c = _mat_to_col16(center)
    L = capi.PoseLattice((C.c_int32 * 3)(*[int(v) for v in n]), (C.c_double * 3)(*[float(v) for v in step]), int(n_yaw), float(yaw_step))
    lib = capi.load()
    count = C.c_size_t(0)
    cp = c.ctypes.data_as(C.POINTER(C.c_float))
    capi.check(lib.lsr_pose_lattice_poses(cp, C.byref(L), None, 0, C.byref(count)), "poseLattice")
    out = np.zeros((count.value, 16), np.float32)
    capi.check(lib.lsr_pose_lattice_poses(cp, C.byref(L), out.ctypes.data_as(C.POINTER(C.c_float)), count.value, C.byref(count)), "poseLattice")
    return np.ascontiguousarray(out.reshape(-1, 4, 4).transpose(0, 2, 1))


def selectPoses(score, poses, top_k: int = 16, min_sep_m: float = 0.9, min_sep_rad: float = 0.1308996938995747) -> np.ndarray:
    """The distinct best of a scored pose list (lsr_select_poses): indices, best first.  Needs no device."""
    s = np.ascontiguousarray(score, np.float64).reshape(-1)
    p = _poses_to_col16(poses)
    if p.shape[0] != s.shape[0]:
        raise ValueError("one score per pose")
    kept = np.zeros(capi.POSE_SEARCH_MAX_KEPT, np.int32)
    n = C.c_int(0)
    capi.check(capi.load().lsr_select_poses(s.ctypes.data_as(C.POINTER(C.c_double)), p.ctypes.data_as(C.POINTER(C.c_float)), s.shape[0],
                                            int(top_k), float(min_sep_m), float(min_sep_rad), kept.ctypes.data_as(C.POINTER(C.c_int32)),
                                            C.byref(n)), "selectPoses")
    return kept[:n.value].copy()


class ScanContextParams(NamedTuple):
    """lsr_scan_context_params: num_rings x num_sectors cells out to max_radius [m]; z_offset = the sensor's height above ground."""
    num_rings: int = 20
    num_sectors: int = 60
    max_radius: float = 80.0
    z_offset: float = 2.0

    def struct(self) -> "capi.ScanContextParams":
        return capi.ScanContextParams(int(self.num_rings), int(self.num_sectors), float(self.max_radius), float(self.z_offset))


def scanContextTables(params: ScanContextParams = ScanContextParams()):
    """The two tables of the descriptor through lsr_scan_context_tables; needs no device.  -> (edge2 (R,) float32: the squared ring
    edges k = 1 .. R-1, then L2; boundaries (S/2 - 1, 2) float32: cos, sin of 2 pi k / S for k = 1 .. S/2-1)."""
    R, S = int(params.num_rings), int(params.num_sectors)
    edge2 = np.zeros(max(R, 1), np.float32)
    b = np.zeros(max(S, 2), np.float32)
    cp = params.struct()
    fp = C.POINTER(C.c_float)
    capi.check(capi.load().lsr_scan_context_tables(C.byref(cp), edge2.ctypes.data_as(fp), b.ctypes.data_as(fp)), "scanContextTables")
    return edge2[:R].copy(), b[: S - 2].reshape(-1, 2).copy()


def _pose_submap(sm) -> "capi.SubMap":
    s = capi.SubMap()
    s.position[:] = [float(v) for v in sm.position]
    s.orientation[:] = [float(v) for v in sm.orientation]
    s.distance = float(getattr(sm, "distance", 0.0))
    return s


def scanContextGuess(candidate, latest, shift: int, num_sectors: int = 60) -> np.ndarray:
    """lsr_align's guess from appearance through lsr_scan_context_guess: M_cand Rz(shift 2 pi / S) M_latest^-1 in fp64 from the two
    stored poses (objects with `position` and `orientation`), cast to float.  Needs no device.  -> (4, 4) fp32."""
    a, b = _pose_submap(candidate), _pose_submap(latest)
    g = np.zeros(16, np.float32)
    capi.check(capi.load().lsr_scan_context_guess(C.byref(a), C.byref(b), int(shift), int(num_sectors), g.ctypes.data_as(C.POINTER(C.c_float))),
               "scanContextGuess")
    return _col16_to_mat(g)


class VisibilityParams(NamedTuple):
    """lsr_visibility_params: the depth image of a keyframe is `height` rows x 4 `face_width` columns (four cube faces side by side)
    out to +-max_tan_elevation and from min_range to max_range [m]; a record is voted against by a neighbouring keyframe (within
    keyframe_range [m], the max_neighbours nearest) whose eroded image is more than `margin` [m] deeper where the record would be;
    min_votes such votes take it out of the static map.  sensor_origin: the lidar in the keyframe's frame."""
    face_width: int = 128
    height: int = 32
    max_tan_elevation: float = 0.5773502691896257   # tan 30 degrees
    min_range: float = 0.5
    max_range: float = 80.0
    margin: float = 0.5
    keyframe_range: float = 30.0
    max_neighbours: int = 32
    min_votes: int = 2
    sensor_origin: Tuple[float, float, float] = (0.0, 0.0, 0.0)

    def struct(self) -> "capi.VisibilityParams":
        return capi.VisibilityParams(int(self.face_width), int(self.height), float(self.max_tan_elevation), float(self.min_range),
                                     float(self.max_range), float(self.margin), float(self.keyframe_range), int(self.max_neighbours),
                                     int(self.min_votes), (C.c_double * 3)(*[float(v) for v in self.sensor_origin]))

    @property
    def shape(self) -> Tuple[int, int]:
        """(rows, columns) of one image"""
        return int(self.height), 4 * int(self.face_width)


def _pose_table(submaps, poses):
    """The lsr_submap array (poses only, no clouds) and the column-major fp64 poses (or None) of a host-only entry."""
    n = len(submaps)
    arr = (capi.SubMap * n)()
    for i, sm in enumerate(submaps):
        arr[i].position[:] = [float(v) for v in sm.position]
        arr[i].orientation[:] = [float(v) for v in sm.orientation]
        arr[i].distance = float(getattr(sm, "distance", 0.0))
    P = None
    if poses is not None:
        if len(poses) != n:
            raise ValueError("one pose per submap")
        P = np.ascontiguousarray(np.stack([np.asarray(p, np.float64).reshape(4, 4).T.reshape(16) for p in poses]), np.float64)
    return arr, P


def visibilityPairs(submaps, poses=None, params: VisibilityParams = VisibilityParams()):
    """Which keyframes look at which (lsr_visibility_pairs; needs no device): `submaps` = objects with `position` and `orientation`,
    `poses` = None (the stored poses) or one 4x4 fp64 per submap.  -> (first_pair (n + 1,) int32, other (m,) int32, rel12 (m, 3, 4)
    float32): the pairs of keyframe i are first_pair[i] .. first_pair[i + 1], other[p] = k, rel12[p] = the first three rows of
    M_k^-1 M_i."""
    n = len(submaps)
    if n == 0:
        raise ValueError("visibilityPairs needs at least one submap")
    arr, P = _pose_table(submaps, poses)
    cap = n * max(min(int(params.max_neighbours), n - 1), 1)
    first = np.zeros(n + 1, np.int32)
    other = np.zeros(cap, np.int32)
    rel = np.zeros((cap, 12), np.float32)
    m = C.c_size_t()
    cp = VisibilityParams(*params).struct()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    capi.check(capi.load().lsr_visibility_pairs(arr, n, P.ctypes.data_as(C.POINTER(C.c_double)) if P is not None else None, C.byref(cp),
                                                first.ctypes.data_as(ip), other.ctypes.data_as(ip), rel.ctypes.data_as(fp), cap,
                                                C.byref(m)), "visibilityPairs")
    return first, other[: m.value].copy(), rel[: m.value].reshape(-1, 3, 4).copy()


def _window_struct(window) -> capi.MapWindow:
    leaf, lo, hi = window
    return capi.MapWindow(float(leaf), (C.c_int32 * 3)(*[int(v) for v in lo]), (C.c_int32 * 3)(*[int(v) for v in hi]))


def _is_torch_cuda(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def _cloud_args(cloud, reg=None):
    """-> (pointer, stride_bytes, n, on_device, keepalive).  reg: the registration object that is going to read the cloud —
    for a CUDA tensor its stream is ordered after torch's current stream AFTER any .contiguous() copy has been enqueued there
    (the copy is the buffer the core reads; an event recorded before it would not cover it)."""
    if _is_torch_cuda(cloud):
        import torch

        t = cloud
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < 3:
            raise ValueError("device cloud must be float32 of shape (n, c>=3)")
        if not t.is_contiguous():
            t = t.contiguous()
        if reg is not None:
            _order_after_torch(reg, t)
        return C.c_void_p(t.data_ptr()), t.shape[1] * 4, t.shape[0], True, t
    a = np.asarray(cloud)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("cloud must have shape (n, c>=3)")
    a = np.ascontiguousarray(a, np.float32)
    return C.c_void_p(a.ctypes.data), a.shape[1] * 4, a.shape[0], False, a


def _record_args(buf, point_step: int):
    """A PointCloud2 payload as raw records -> (pointer, n_records, on_device, keepalive).  `buf`: numpy array or CUDA tensor of any
    4-byte or 1-byte dtype, 1-D or (n, c), contiguous, whose bytes are whole records of `point_step`."""
    if _is_torch_cuda(buf):
        t = buf if buf.is_contiguous() else buf.contiguous()
        nbytes, ptr, dev = t.numel() * t.element_size(), t.data_ptr(), True
    else:
        t = np.ascontiguousarray(buf)
        nbytes, ptr, dev = t.nbytes, t.ctypes.data, False
    if nbytes % point_step:
        raise ValueError(f"buffer of {nbytes} bytes does not hold whole records of {point_step}")
    return ptr, nbytes // point_step, dev, t


def _mat_to_col16(M) -> np.ndarray:
    M = np.asarray(M, np.float32)
    if M.shape != (4, 4):
        raise ValueError("transform must be 4x4")
    return np.ascontiguousarray(M.T).reshape(16)


def _col16_to_mat(v) -> np.ndarray:
    return np.asarray(v, np.float32).reshape(4, 4).T.copy()


def _sensor_transform(translation, rotation_xyzw) -> "capi.SensorTransform":
    t, q = np.asarray(translation, np.float64).reshape(-1), np.asarray(rotation_xyzw, np.float64).reshape(-1)
    if t.shape != (3,) or q.shape != (4,):
        raise ValueError("a sensor transform is a translation (3,) and a quaternion x y z w (4,)")
    return capi.SensorTransform((C.c_double * 3)(*t), (C.c_double * 4)(*q))


def sensorTransformMatrix(translation, rotation_xyzw) -> np.ndarray:
    """The (3, 4) fp32 matrix the kernels move a sensor-frame point with (lsr_sensor_transform_matrix): the double 4x4 of
    lookupTransform(robot_frame, msg.frame_id) (scanmatcher_component.cpp:193-194), quaternion not normalised, cast element by element."""
    tf = _sensor_transform(translation, rotation_xyzw)
    out = np.zeros(12, np.float32)
    capi.check(capi.load().lsr_sensor_transform_matrix(C.byref(tf), out.ctypes.data_as(C.POINTER(C.c_float))), "sensorTransformMatrix")
    return out.reshape(3, 4)


def odomGuess(sim_trans, previous_odom, odom) -> np.ndarray:
    """receiveCloud's use_odom guess (scanmatcher_component.cpp:333-348) through lsr_odom_guess: sim_trans when previous_odom is
    exactly the identity, else sim_trans * previous_odom^-1 * odom (double arithmetic on the fp32 inputs, rounded once).  4x4 in,
    4x4 fp32 out."""
    fp = C.POINTER(C.c_float)
    s, p, o = (_mat_to_col16(M) for M in (sim_trans, previous_odom, odom))
    g = np.zeros(16, np.float32)
    capi.check(capi.load().lsr_odom_guess(s.ctypes.data_as(fp), p.ctypes.data_as(fp), o.ctypes.data_as(fp), g.ctypes.data_as(fp)), "odomGuess")
    return _col16_to_mat(g)


def _order_after_torch(reg, cloud):
    """A CUDA tensor may be the result of kernels still running on torch's current stream: make the handle's stream wait
    for that stream (lsr_wait_stream: event record + stream wait, no host wait) before the core reads the tensor."""
    if _is_torch_cuda(cloud):
        import torch

        capi.check(reg._lib.lsr_wait_stream(reg._h, C.c_void_p(torch.cuda.current_stream(cloud.device).cuda_stream)), "lsr_wait_stream")


def _payload_args(reg, data, point_step: int = 1):
    """A record buffer `reg` is about to read — a raw PointCloud2 `data` buffer or records of `point_step` bytes; bytes / bytearray,
    numpy array or CUDA tensor — -> (pointer, n_records, on_device, keepalive) through _record_args.  The keepalive is the buffer the
    core reads: the uint8 view of the host array, or the tensor, behind which `reg`'s stream is ordered after torch's current one."""
    host = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data
    ptr, n, dev, keep = _record_args(host, point_step)
    if dev:
        _order_after_torch(reg, keep)
    return C.c_void_p(ptr), n, dev, keep if dev else keep.view(np.uint8)


def _payload_pair(reg, data, out):
    """(data, out) of a records -> records method -> (source pointer, destination pointer, on_device, out).  out: None = a new buffer
    of data's kind (uint8 numpy array / CUDA tensor), else the buffer to write (`data` itself: in place)."""
    src, _, dev, keep = _payload_args(reg, data)
    if out is None:
        out = keep.new_empty(keep.shape) if dev else np.empty_like(keep)
    return src, C.c_void_p(out.data_ptr() if dev else out.ctypes.data), dev, out


class Registration:
    """pcl::Registration<PointXYZI, PointXYZI>-shaped base."""

    _method = capi.METHOD_NDT

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._lib = capi.load()
        h = C.c_void_p()
        capi.check(self._lib.lsr_create(self._method, device, C.c_void_p(stream) if stream else None, C.byref(h)),
                   "lsr_create")
        self._h = h
        self._device = device
        self._keep = {}
        self._last = capi.Result()

    # -- lifetime --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.lsr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- setters exercised by the reference ---------------------------------------------------
    def _setf(self, key, v, where):
        capi.check(self._lib.lsr_set_f64(self._h, key, float(v)), where)

    def _seti(self, key, v, where):
        capi.check(self._lib.lsr_set_i32(self._h, key, int(v)), where)

    def _getf(self, key):
        v = C.c_double()
        capi.check(self._lib.lsr_get_f64(self._h, key, C.byref(v)), "lsr_get_f64")
        return v.value

    def _geti(self, key):
        v = C.c_int32()
        capi.check(self._lib.lsr_get_i32(self._h, key, C.byref(v)), "lsr_get_i32")
        return v.value

    def setTransformationEpsilon(self, eps: float):  # scanmatcher_component.cpp:108,119
        self._setf(capi.TRANSFORMATION_EPSILON, eps, "setTransformationEpsilon")

    def getTransformationEpsilon(self) -> float:
        return self._getf(capi.TRANSFORMATION_EPSILON)

    def setMaximumIterations(self, n: int):  # graph_based_slam_component.cpp:66,77
        self._seti(capi.MAX_ITERATIONS, n, "setMaximumIterations")

    def getMaximumIterations(self) -> int:
        return self._geti(capi.MAX_ITERATIONS)

    def setMaxCorrespondenceDistance(self, d: float):  # scanmatcher_component.cpp:118
        self._setf(capi.MAX_CORRESPONDENCE_DISTANCE, d, "setMaxCorrespondenceDistance")

    def setEuclideanFitnessEpsilon(self, eps: float):  # graph_based_slam_component.cpp:80
        self._setf(capi.EUCLIDEAN_FITNESS_EPSILON, eps, "setEuclideanFitnessEpsilon")

    def setRANSACIterations(self, n: int):  # graph_based_slam_component.cpp:81
        self._seti(capi.RANSAC_ITERATIONS, n, "setRANSACIterations")

    # -- clouds ------------------------------------------------------------------------------
    def setInputTarget(self, cloud):  # scanmatcher_component.cpp:275,307,315; graph_based_slam_component.cpp:227
        p, stride, n, dev, keep = _cloud_args(cloud, self)
        fn = self._lib.lsr_set_input_target_device if dev else self._lib.lsr_set_input_target
        capi.check(fn(self._h, p, stride, n), "setInputTarget")
        self._keep["target"] = None  # the core keeps its own SoA copy in HBM

    def _frame_args(self, frames, poses):
        """-> (n_frames, pointers, counts, stride, poses as (n,16) fp32 column-major, on_device, keepalive)."""
        args = [_cloud_args(f) for f in frames]
        dev_frames = [a[4] for a in args if _is_torch_cuda(a[4])]
        if dev_frames:
            _order_after_torch(self, dev_frames[-1])   # one ordering, after every .contiguous() copy has been enqueued
        dev = args[0][3]
        if any(a[3] != dev for a in args) or any(a[1] != args[0][1] for a in args):
            raise ValueError("frames must all be host or all device, with one record stride")
        nf = len(args)
        ptrs = (C.c_void_p * nf)(*[a[0] for a in args])
        counts = (C.c_size_t * nf)(*[a[2] for a in args])
        P = np.ascontiguousarray(np.stack([_mat_to_col16(p) for p in poses]), np.float32)
        return nf, ptrs, counts, args[0][1], P, dev, args

    def setInputTargetFrames(self, frames, poses):
        """Submap assembly on the device: frame f transformed by poses[f] (4x4), concatenated, then
        setInputTarget (scanmatcher_component.cpp:449-464,307).  Frames: host arrays or CUDA tensors, same layout."""
        nf, ptrs, counts, stride, P, dev, args = self._frame_args(frames, poses)
        capi.check(self._lib.lsr_set_input_target_frames(self._h, nf, ptrs, counts, stride,
                                                         P.ctypes.data_as(C.POINTER(C.c_float)), 1 if dev else 0),
                   "setInputTargetFrames")
        self._n_target = int(sum(a[2] for a in args))

    def setInputTargetFramesFiltered(self, frames, poses, leaf: float) -> int:
        """The same followed by pcl::VoxelGrid(leaf) of the assembled cloud; the FILTERED cloud becomes the target — the GICP branch of
        a map update (scanmatcher_component.cpp:308-316,448-464), all in HBM.  The frames' order (newest first in the frontend) decides
        the float sums' order, hence the bits.  Returns the number of target points."""
        nf, ptrs, counts, stride, P, dev, args = self._frame_args(frames, poses)
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_set_input_target_frames_filtered(self._h, nf, ptrs, counts, stride,
                                                                  P.ctypes.data_as(C.POINTER(C.c_float)), 1 if dev else 0,
                                                                  C.c_float(leaf), C.byref(n_out)), "setInputTargetFramesFiltered")
        self._n_target = int(n_out.value)
        return self._n_target

    def prepareTarget(self):
        """Builds now, on this object's stream, what the first align against the current target would still have to build (GICP: the
        target's k-NN covariances; NDT: as a rule nothing) and returns when it is done.  Needs no input source."""
        capi.check(self._lib.lsr_prepare_target(self._h), "prepareTarget")

    def targetPrepared(self) -> bool:
        """True when an align with this object's parameters has nothing left to build on the current target (LSR_TARGET_PREPARED)."""
        return bool(self._geti(capi.TARGET_PREPARED))

    def setInputSource(self, cloud):  # scanmatcher_component.cpp:329; graph_based_slam_component.cpp:181
        p, stride, n, dev, keep = _cloud_args(cloud, self)
        fn = self._lib.lsr_set_input_source_device if dev else self._lib.lsr_set_input_source
        capi.check(fn(self._h, p, stride, n), "setInputSource")
        self._n_source = n
        self._keep["source"] = keep if dev else None  # device upload is asynchronous on the handle's stream

    def setInputSourceFiltered(self, cloud, leaf: float) -> int:
        """pcl::VoxelGrid(leaf).filter + setInputSource on the device (scanmatcher_component.cpp:324-329);
        returns the number of points kept."""
        p, stride, n, dev, keep = _cloud_args(cloud, self)
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_set_input_source_filtered(self._h, p, stride, n, C.c_float(leaf), 1 if dev else 0,
                                                           C.byref(n_out)), "setInputSourceFiltered")
        self._n_source = int(n_out.value)
        return self._n_source

    def setInputSourceFrontend(self, cloud, scan_min_range: float, scan_max_range: float, vg_size_for_input: float) -> int:
        """Range filter (scanmatcher_component.cpp:210-218) + VoxelGrid (:324-328) + setInputSource (:329) on the
        device; returns the number of points kept."""
        p, stride, n, dev, keep = _cloud_args(cloud, self)
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_set_input_source_frontend(self._h, p, stride, n, float(scan_min_range), float(scan_max_range),
                                                           C.c_float(vg_size_for_input), 1 if dev else 0, C.byref(n_out)),
                   "setInputSourceFrontend")
        self._n_source = int(n_out.value)
        return self._n_source

    # -- sensor_msgs/PointCloud2 codec ----------------------------------------------
    @staticmethod
    def _layout(point_step, offsets):
        ox, oy, oz, oi = offsets
        return capi.Pc2Layout(int(point_step), int(ox), int(oy), int(oz), int(-1 if oi is None else oi))

    def setInputSourcePointCloud2(self, data, n_points: int, point_step: int, offsets, scan_min_range: float, scan_max_range: float,
                                  vg_size_for_input: float, sensor_transform=None) -> int:
        """pcl::fromROSMsg + range filter + VoxelGrid + setInputSource from a raw PointCloud2 `data` buffer (bytes / uint8 numpy
        array / CUDA uint8 tensor); offsets = (x, y, z, intensity or None) in bytes.  Returns the number of points kept.
        sensor_transform: (translation xyz, rotation xyzw) of lookupTransform(robot_frame, msg.frame_id) — the payload is in the sensor
        frame and is moved into the robot frame as it is read (tf2::doTransform, scanmatcher_component.cpp:195), before the range
        filter; None: the payload is in the robot frame already."""
        lay = self._layout(point_step, offsets)
        n_out = C.c_size_t()
        ptr, _, dev, keep = _payload_args(self, data)
        if sensor_transform is None:
            st = self._lib.lsr_set_input_source_pc2(self._h, ptr, int(n_points), C.byref(lay), float(scan_min_range), float(scan_max_range),
                                                    C.c_float(vg_size_for_input), dev, C.byref(n_out))
        else:
            tf = _sensor_transform(*sensor_transform)
            st = self._lib.lsr_set_input_source_pc2_tf(self._h, ptr, int(n_points), C.byref(lay), C.byref(tf), float(scan_min_range),
                                                       float(scan_max_range), C.c_float(vg_size_for_input), dev, C.byref(n_out))
        capi.check(st, "setInputSourcePointCloud2")
        self._n_source = int(n_out.value)
        return self._n_source

    def transformPointCloud2(self, data, n_points: int, point_step: int, offsets, translation, rotation_xyzw, out=None):
        """tf2::doTransform(*msg, transformed_msg, transform) on a raw PointCloud2 `data` buffer (scanmatcher_component.cpp:195), on the
        device: x / y / z of every record moved by the transform (translation xyz, quaternion x y z w, not normalised), every other
        byte copied.  `data`: uint8 numpy array / bytes (-> numpy array out) or CUDA uint8 tensor (-> CUDA tensor out, nothing leaves
        HBM).  `out`: None = a new buffer, or the buffer to write (`data` itself: in place).  Returns the records."""
        lay = self._layout(point_step, offsets)
        tf = _sensor_transform(translation, rotation_xyzw)
        src, dst, dev, out = _payload_pair(self, data, out)
        capi.check(self._lib.lsr_transform_pc2(self._h, src, int(n_points), C.byref(lay), C.byref(tf), dev, dst), "transformPointCloud2")
        return out

    # -- IMU de-skew of the raw scan (use_imu: scanmatcher_component.cpp:204-208, 501-527) ---------------------------
    def imuReset(self, scan_period: float = 0.1):
        """A fresh LidarUndistortion with setScanPeriod(scan_period): empties the IMU ring of this object."""
        capi.check(self._lib.lsr_imu_reset(self._h, float(scan_period)), "imuReset")

    def receiveImu(self, orientation_xyzw, angular_velocity, linear_acceleration, stamp: float) -> bool:
        """ScanMatcherComponent::receiveImu (scanmatcher_component.cpp:501-527) through lsr_imu_receive: the library removes gravity
        from the linear acceleration with the roll / pitch of the orientation (:505-511) and pushes the sample into the ring.
        orientation: geometry_msgs/Quaternion order x y z w.  False: the sample was refused (stamp out of order)."""
        q, w, a = (np.ascontiguousarray(v, np.float64) for v in (orientation_xyzw, angular_velocity, linear_acceleration))
        if q.shape != (4,) or w.shape != (3,) or a.shape != (3,):
            raise ValueError("receiveImu takes orientation (4,), angular velocity (3,) and linear acceleration (3,)")
        dp = C.POINTER(C.c_double)
        st = self._lib.lsr_imu_receive(self._h, q.ctypes.data_as(dp), w.ctypes.data_as(dp), a.ctypes.data_as(dp), float(stamp))
        return st == capi.OK

    def imuInfo(self) -> dict:
        info = np.zeros(4, np.int32)
        capi.check(self._lib.lsr_imu_info(self._h, info.ctypes.data_as(C.POINTER(C.c_int32))), "imuInfo")
        return dict(count=int(info[0]), last=int(info[1]), last_iter=int(info[2]))

    def deskewPointCloud2(self, data, n_points: int, point_step: int, offsets, scan_time: float, out=None):
        """lidar_undistortion_.adjustDistortion(cloud, scan_time) on a raw PointCloud2 `data` buffer (scanmatcher_component.cpp:207),
        on the device: every point moves into the sensor frame of the scan's first point, every other byte of a record is copied.
        `data`: uint8 numpy array / bytes (-> numpy array out) or CUDA uint8 tensor (-> CUDA tensor out, nothing leaves HBM).
        `out`: None = a new buffer, or the buffer to write (`data` itself: in place).  Returns (records, info) with info =
        dict(n_skipped, start_missing, half_index, cursor)."""
        lay = self._layout(point_step, offsets)
        info = capi.DeskewInfo()
        n_points = int(n_points)
        src, dst, dev, out = _payload_pair(self, data, out)
        capi.check(self._lib.lsr_deskew_pc2(self._h, src, n_points, C.byref(lay), float(scan_time), dev, dst, C.byref(info)),
                   "deskewPointCloud2")
        self._n_deskew = n_points
        return out, dict(n_skipped=int(info.n_skipped), start_missing=int(info.start_missing), half_index=int(info.half_index),
                         cursor=int(info.cursor))

    def deskewTrace(self) -> dict:
        """Inspection (lsr_deskew_trace): what the last deskewPointCloud2 decided per point — rel_time (n,) fp32, the ring slot the IMU
        pointer stood on (n,) int32 (-1 everywhere when that call moved nothing because the ring was too short), skipped (n,) uint8."""
        n = int(getattr(self, "_n_deskew", 0))
        rel, slot, sk = np.zeros(n, np.float32), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
        capi.check(self._lib.lsr_deskew_trace(self._h, rel.ctypes.data_as(C.POINTER(C.c_float)), slot.ctypes.data_as(C.POINTER(C.c_int32)),
                                              sk.ctypes.data_as(C.POINTER(C.c_uint8))), "deskewTrace")
        return dict(rel_time=rel, slot=slot, skipped=sk)

    def voxelFilterForm(self) -> int:
        """Which form the last VoxelGrid filter on this object took (LSR_VOXEL_FILTER_FORM): 1 = grid dimensions on the host, 2 = on the
        device (one host wait per scan), 3 = the device form came back flagged and the host form ran; 0 = none yet."""
        return self._geti(capi.VOXEL_FILTER_FORM)

    def getInputSourcePointCloud2(self, point_step: int = 32, offsets=(0, 4, 8, 16)) -> np.ndarray:
        """pcl::toROSMsg of the current input source: (n, point_step) uint8 records (default: pcl::PointXYZI's layout)."""
        lay = self._layout(point_step, offsets)
        out = np.zeros((max(self._n_source, 1), point_step), np.uint8)
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_get_source_pc2(self._h, C.c_void_p(out.ctypes.data), out.shape[0], C.byref(lay), C.byref(n_out)),
                   "getInputSourcePointCloud2")
        return out[: n_out.value].copy()

    def getInputSourceDeviceRecords(self):
        """The current input source as pcl::PointXYZI records in HBM: an (n, 8) fp32 CUDA tensor (x y z _ intensity _ _ _), e.g. a
        keyframe for setInputTargetFrames that never leaves the device (lsr_get_source_pc2_device)."""
        import torch

        lay = self._layout(32, (0, 4, 8, 16))
        # on the OBJECT's device (not torch's current one), and the object's stream ordered behind whatever torch's stream may
        # still be doing with the block the caching allocator hands out
        dev = torch.device("cuda", self._device)
        out = torch.empty((max(self._n_source, 1), 8), dtype=torch.float32, device=dev)
        capi.check(self._lib.lsr_wait_stream(self._h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "lsr_wait_stream")
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_get_source_pc2_device(self._h, C.c_void_p(out.data_ptr()), out.shape[0], C.byref(lay), C.byref(n_out)),
                   "getInputSourceDeviceRecords")
        return out[: n_out.value]

    def voxelGridFilterPointCloud2(self, data, n_points: int, point_step: int, offsets, leaf: float, out_point_step: int = 32,
                                   out_offsets=(0, 4, 8, 16)) -> np.ndarray:
        """pcl::VoxelGrid(leaf).filter on a PointCloud2 payload (host), all four fields averaged per leaf; -> (m, out_point_step) uint8."""
        li, lo = self._layout(point_step, offsets), self._layout(out_point_step, out_offsets)
        src, _, dev, keep = _payload_args(self, data)
        if dev:
            raise ValueError("voxelGridFilterPointCloud2 takes a host payload")
        out = np.zeros((max(int(n_points), 1), out_point_step), np.uint8)
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_voxel_grid_filter_pc2(self._h, src, int(n_points), C.byref(li), C.c_float(leaf),
                                                       C.c_void_p(out.ctypes.data), out.shape[0], C.byref(lo), C.byref(n_out)),
                   "voxelGridFilterPointCloud2")
        return out[: n_out.value].copy()

    def voxelGridFilter(self, cloud, leaf: float) -> np.ndarray:
        """Stand-alone pcl::VoxelGrid(leaf).filter on the device; host (n,c>=3) in, (m,3) fp32 out."""
        p, stride, n, dev, keep = _cloud_args(cloud)
        if dev:
            raise ValueError("voxelGridFilter takes a host array")
        out = np.zeros((max(n, 1), 3), np.float32)
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_voxel_grid_filter(self._h, p, stride, n, C.c_float(leaf), C.c_void_p(out.ctypes.data), 12,
                                                   out.shape[0], C.byref(n_out)), "voxelGridFilter")
        return out[: n_out.value].copy()

    # -- the whole map from its submaps ---------------------------------------------
    def assembleMap(self, submaps, poses=None, in_layout=PC2_XYZI, out_layout=PC2_XYZI, out=None, leaf=None):
        """ScanMatcherComponent::publishMap (scanmatcher_component.cpp:529-552) and the map half of doPoseAdjustment
        (graph_based_slam_component.cpp:321-368) through lsr_assemble_map: every submap moved by its pose, the records concatenated.
        `submaps`: objects with `cloud`, `position`, `orientation` (x y z w) — loop_closure.SubMap; the clouds are record buffers
        of `in_layout`, all numpy arrays or all CUDA tensors.  `poses`: None = each submap's own pose, or one 4x4 (fp64) per submap:
        the optimiser's estimates.  Layouts: (point_step, (x, y, z, intensity or None)).  `out`: None = a new buffer, or the uint8
        buffer to write (numpy array or CUDA tensor; a view of a resident map advanced by first_record[k] records appends).
        Returns (records, first_record): (total, out point_step) uint8 — a CUDA tensor when the submaps are CUDA tensors or `out` is
        one, else a numpy array — and the (n + 1,) int64 index of every submap's first record, the last entry the total.
        `leaf`: None = the raw map as above; a leaf size = that map thinned by voxelGridFilterMap before it leaves the call
        (lsr_assemble_map_filtered: the raw map stays in HBM) -> (records, None): a leaf mixes submaps, there is no first_record."""
        n = len(submaps)
        if n == 0:
            raise ValueError("assembleMap needs at least one submap")
        if leaf is not None:
            return self._assemble_map_filtered(submaps, poses, in_layout, out_layout, out, float(leaf)), None
        li, lo = self._layout(*in_layout), self._layout(*out_layout)
        out_step = int(out_layout[0])
        arr, keep, residency, total, P = self._submap_table(submaps, poses, int(in_layout[0]))
        if out is None:
            if residency:
                import torch

                out = torch.empty((max(total, 1), out_step), dtype=torch.uint8, device=torch.device("cuda", self._device))
            else:
                out = np.zeros((max(total, 1), out_step), np.uint8)
        out_dev = _is_torch_cuda(out)
        if out_dev:
            if not out.is_contiguous() or out.element_size() != 1:
                raise ValueError("out must be a contiguous uint8 buffer")
            flat, optr, cap = out.view(-1), out.data_ptr(), out.numel() // out_step
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable):
                raise ValueError("out must be a writeable contiguous uint8 buffer")
            flat, optr, cap = out.reshape(-1), out.ctypes.data, out.nbytes // out_step
        # ONE ordering of the handle's stream after torch's current stream, after every .contiguous() copy above has been enqueued there
        dev_holders = [h for h in keep if _is_torch_cuda(h)]
        if dev_holders:
            _order_after_torch(self, dev_holders[-1])
        if out_dev:
            _order_after_torch(self, out)
        first = (C.c_size_t * (n + 1))()
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_assemble_map(self._h, arr, n, C.byref(li), 1 if residency else 0,
                                              P.ctypes.data_as(C.POINTER(C.c_double)) if P is not None else None, C.c_void_p(optr), cap,
                                              C.byref(lo), 1 if out_dev else 0, first, C.byref(n_out)), "assembleMap")
        return flat[: n_out.value * out_step].reshape(n_out.value, out_step), np.array(first[:], np.int64)

    def _out_records(self, out, out_step: int, rows: int, on_device: bool):
        """The output buffer of a records -> records method -> (buffer, flat uint8 view, pointer, capacity in records, on_device).
        out: None = a new uninitialised buffer of `rows` records (a CUDA tensor when on_device), else the uint8 buffer to write."""
        if out is None:
            if on_device:
                import torch

                out = torch.empty((max(rows, 1), out_step), dtype=torch.uint8, device=torch.device("cuda", self._device))
            else:
                out = np.empty((max(rows, 1), out_step), np.uint8)
        if _is_torch_cuda(out):
            if not out.is_contiguous() or out.element_size() != 1:
                raise ValueError("out must be a contiguous uint8 buffer")
            _order_after_torch(self, out)
            return out, out.view(-1), out.data_ptr(), out.numel() // out_step, True
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("out must be a writeable contiguous uint8 buffer")
        return out, out.reshape(-1), out.ctypes.data, out.nbytes // out_step, False

    @staticmethod
    def _trimmed(flat, count: int, out_step: int, capacity: int, own: bool):
        """The first `count` records of a result buffer; one this object allocated for many more is not kept alive by the view."""
        view = flat[: count * out_step].reshape(count, out_step)
        if own and 2 * count < capacity:
            return view.clone() if _is_torch_cuda(view) else view.copy()
        return view

    def _assemble_map_filtered(self, submaps, poses, in_layout, out_layout, out, leaf: float):
        n = len(submaps)
        li, lo = self._layout(*in_layout), self._layout(*out_layout)
        out_step = int(out_layout[0])
        arr, keep, residency, total, P = self._submap_table(submaps, poses, int(in_layout[0]))
        dev_holders = [h for h in keep if _is_torch_cuda(h)]
        if dev_holders:
            _order_after_torch(self, dev_holders[-1])
        own = out is None
        _, flat, optr, cap, out_dev = self._out_records(out, out_step, total, bool(residency))
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_assemble_map_filtered(self._h, arr, n, C.byref(li), 1 if residency else 0,
                                                       P.ctypes.data_as(C.POINTER(C.c_double)) if P is not None else None, C.c_float(leaf),
                                                       C.c_void_p(optr), cap, C.byref(lo), 1 if out_dev else 0, C.byref(n_out)),
                   "assembleMap")
        return self._trimmed(flat, int(n_out.value), out_step, cap, own)

    def voxelGridFilterMap(self, records, leaf: float, layout=PC2_XYZI, out_layout=PC2_XYZI, out=None):
        """pcl::VoxelGrid(leaf).filter for a map-sized cloud through lsr_voxel_grid_filter_map: records in, records out, on the device,
        the leaf index carried in 64 bits (a map of kilometres at a 0.1 m leaf, which pcl::VoxelGrid and voxelGridFilterPointCloud2
        refuse).  One record per occupied leaf in ascending leaf index, all four fields averaged in float in input order; wherever
        voxelGridFilterPointCloud2 accepts the cloud, the same bytes.  `records`: a record buffer of `layout` — numpy array (->
        uint8 numpy array) or CUDA tensor (-> uint8 CUDA tensor, nothing leaves HBM).  `out`: None = a new buffer, or the uint8 buffer
        to write (numpy array or CUDA tensor).  -> (m, out point_step) uint8."""
        li, lo = self._layout(*layout), self._layout(*out_layout)
        out_step = int(out_layout[0])
        ptr, n, dev, keep = _payload_args(self, records, int(layout[0]))
        own = out is None
        _, flat, optr, cap, out_dev = self._out_records(out, out_step, n, dev)
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_voxel_grid_filter_map(self._h, ptr, n, C.byref(li), 1 if dev else 0, C.c_float(leaf), C.c_void_p(optr), cap,
                                                       C.byref(lo), 1 if out_dev else 0, C.byref(n_out)), "voxelGridFilterMap")
        return self._trimmed(flat, int(n_out.value), out_step, cap, own)

    def cropMap(self, records, window, layout=PC2_XYZI, out_layout=PC2_XYZI, out=None):
        """The records of a map whose absolute voxel cell lies in `window` (MapWindow, or (leaf, lo, hi)), in input order, through
        lsr_crop_map: x, y, z and intensity moved from `layout` to `out_layout`, every other byte zero.  `records`: numpy array (->
        uint8 numpy array) or CUDA tensor (-> uint8 CUDA tensor, nothing leaves HBM).  `out`: None = the records are counted first and a
        buffer of that size is allocated; else the uint8 buffer to write.  -> (m, out point_step) uint8."""
        li, lo, w = self._layout(*layout), self._layout(*out_layout), _window_struct(window)
        out_step = int(out_layout[0])
        ptr, n, dev, keep = _payload_args(self, records, int(layout[0]))
        n_out = C.c_size_t()
        own = out is None
        if own:
            capi.check(self._lib.lsr_crop_map(self._h, ptr, n, C.byref(li), 1 if dev else 0, C.byref(w), None, 0, C.byref(lo), 0,
                                              C.byref(n_out)), "cropMap")
        _, flat, optr, cap, out_dev = self._out_records(out, out_step, int(n_out.value), dev)
        capi.check(self._lib.lsr_crop_map(self._h, ptr, n, C.byref(li), 1 if dev else 0, C.byref(w), C.c_void_p(optr), cap, C.byref(lo),
                                          1 if out_dev else 0, C.byref(n_out)), "cropMap")
        return self._trimmed(flat, int(n_out.value), out_step, cap, own)

    def countMapWindow(self, records, window, layout=PC2_XYZI) -> int:
        """How many records cropMap would keep (lsr_crop_map without an output buffer)."""
        li, lo, w = self._layout(*layout), self._layout(*PC2_XYZI), _window_struct(window)
        ptr, n, dev, keep = _payload_args(self, records, int(layout[0]))
        n_out = C.c_size_t()
        capi.check(self._lib.lsr_crop_map(self._h, ptr, n, C.byref(li), 1 if dev else 0, C.byref(w), None, 0, C.byref(lo), 0,
                                          C.byref(n_out)), "countMapWindow")
        return int(n_out.value)

    def setInputTargetWindow(self, records, window, layout=PC2_XYZI) -> int:
        """setInputTarget from the window of a resident map (lsr_set_input_target_window): cropMap into a buffer kept on the object,
        then setInputTarget over it, the same target bit for bit.  Returns the number of target points; a window that keeps none
        raises and the previous target stays."""
        li, w = self._layout(*layout), _window_struct(window)
        ptr, n, dev, keep = _payload_args(self, records, int(layout[0]))
        n_kept = C.c_size_t()
        capi.check(self._lib.lsr_set_input_target_window(self._h, ptr, n, C.byref(li), 1 if dev else 0, C.byref(w), C.byref(n_kept)),
                   "setInputTargetWindow")
        self._n_target = int(n_kept.value)
        self._keep["target"] = None
        return self._n_target

    def mapWindowMs(self) -> float:
        """hipEvent time [ms] of the three launches of the last cropMap / setInputTargetWindow on this object (LSR_MAP_WINDOW_MS; needs
        LSR_PROFILE = 1, else 0)."""
        return self._getf(capi.MAP_WINDOW_MS)

    def mapFilterKeyBits(self) -> int:
        """The bits of the largest leaf index of the last map filter on this object (LSR_MAP_FILTER_KEY_BITS); above 32 the index was
        sorted as two words; 0 = none yet."""
        return self._geti(capi.MAP_FILTER_KEY_BITS)

    # -- Scan Context -----------------------------------------------------------------
    def scanContext(self, submaps, params: "ScanContextParams" = None, layout=PC2_XYZI, out=None):
        """The Scan Context descriptor of every submap through lsr_scan_context_build, one launch over all of them.  `submaps`:
        objects with `cloud` (record buffers of `layout`, pose-local; all numpy arrays or all CUDA tensors), as assembleMap takes
        them.  `out`: None = a new buffer (a CUDA tensor when the clouds are), or the float32 buffer to write — a view of a resident
        table advanced by k descriptors appends.  -> (n, num_rings, num_sectors) float32."""
        params = params or ScanContextParams()
        n = len(submaps)
        if n == 0:
            raise ValueError("scanContext needs at least one submap")
        li = self._layout(*layout)
        arr, keep, residency, _, _ = self._submap_table(submaps, None, int(layout[0]))
        R, S = int(params.num_rings), int(params.num_sectors)
        if out is None:
            if residency:
                import torch

                out = torch.empty((n, R, S), dtype=torch.float32, device=torch.device("cuda", self._device))
            else:
                out = np.zeros((n, R, S), np.float32)
        out_dev = _is_torch_cuda(out)
        if out_dev:
            import torch

            if not out.is_contiguous() or out.dtype != torch.float32 or out.numel() < n * R * S:
                raise ValueError("out must be a contiguous float32 buffer of n x num_rings x num_sectors")
            optr, flat = out.data_ptr(), out.view(-1)
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable
                    and out.size >= n * R * S):
                raise ValueError("out must be a writeable contiguous float32 buffer of n x num_rings x num_sectors")
            optr, flat = out.ctypes.data, out.reshape(-1)
        dev_holders = [h for h in keep if _is_torch_cuda(h)]
        if dev_holders:
            _order_after_torch(self, dev_holders[-1])
        if out_dev:
            _order_after_torch(self, out)
        cp = params.struct()
        capi.check(self._lib.lsr_scan_context_build(self._h, arr, n, C.byref(li), 1 if residency else 0, C.byref(cp), C.c_void_p(optr),
                                                    1 if out_dev else 0), "scanContext")
        return flat[: n * R * S].reshape(n, R, S)

    def matchScanContext(self, q, c, params: "ScanContextParams" = None):
        """Every query descriptor against every candidate descriptor at every yaw shift through lsr_scan_context_match, one launch.
        q: (nq, R, S) or (R, S); c: (nc, R, S) or (R, S); both numpy arrays or both CUDA tensors, float32.
        -> (dist (nq, nc) float32, shift (nq, nc) int32): the smallest distance over the shifts and the lowest shift that has it."""
        params = params or ScanContextParams()
        cells = int(params.num_rings) * int(params.num_sectors)
        dev = _is_torch_cuda(q)
        if dev != _is_torch_cuda(c):
            raise ValueError("q and c must share residency (host/device)")
        holders = []
        ptrs, counts = [], []
        for d in (q, c):
            if dev:
                import torch

                t = d if d.is_contiguous() else d.contiguous()
                if t.dtype != torch.float32 or t.numel() == 0 or t.numel() % cells:
                    raise ValueError("descriptors must be float32 of shape (n, num_rings, num_sectors)")
                ptrs.append(t.data_ptr()); counts.append(t.numel() // cells)
            else:
                t = np.ascontiguousarray(d, np.float32)
                if t.size == 0 or t.size % cells:
                    raise ValueError("descriptors must be float32 of shape (n, num_rings, num_sectors)")
                ptrs.append(t.ctypes.data); counts.append(t.size // cells)
            holders.append(t)
        if dev:
            _order_after_torch(self, holders[-1])
        nq, nc = counts
        dist, shift = np.zeros((nq, nc), np.float32), np.zeros((nq, nc), np.int32)
        cp = params.struct()
        capi.check(self._lib.lsr_scan_context_match(self._h, C.c_void_p(ptrs[0]), nq, C.c_void_p(ptrs[1]), nc, 1 if dev else 0, C.byref(cp),
                                                    dist.ctypes.data_as(C.POINTER(C.c_float)), shift.ctypes.data_as(C.POINTER(C.c_int32))),
                   "matchScanContext")
        return dist, shift

    def scanContextMs(self):
        """hipEvent time [ms] of the launches of the last scanContext and of the last matchScanContext / search_loop_appearance
        comparison on this object (setProfiling(True)), else 0.  -> (build, match)"""
        return self._getf(capi.SCAN_CONTEXT_BUILD_MS), self._getf(capi.SCAN_CONTEXT_MATCH_MS)

    # -- moving objects out of the map: visibility votes ---------------------------------
    def _float_out(self, out, shape, on_device: bool, what: str):
        """A float32 result buffer of `shape` -> (buffer, pointer, on_device); out: None = a new one."""
        count = int(np.prod(shape))
        if out is None:
            if on_device:
                import torch

                out = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", self._device))
            else:
                out = np.zeros(shape, np.float32)
        if _is_torch_cuda(out):
            import torch

            if not out.is_contiguous() or out.dtype != torch.float32 or out.numel() < count:
                raise ValueError(f"{what} must be a contiguous float32 buffer of {shape}")
            _order_after_torch(self, out)
            return out, out.data_ptr(), True
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable and out.size >= count):
            raise ValueError(f"{what} must be a writeable contiguous float32 buffer of {shape}")
        return out, out.ctypes.data, False

    def depthImages(self, submaps, params: "VisibilityParams" = None, layout=PC2_XYZI, out=None, eroded: bool = True):
        """The depth image of every submap through lsr_depth_images_build: one launch over all of them, and with `eroded` (the
        default: what the votes compare against) the 3 x 3 minimum in one more.  `submaps` as for scanContext.  `out`: None = a new
        buffer (a CUDA tensor when the clouds are), or the float32 buffer to write — a view of a resident table advanced by k images
        appends.  -> (n, height, 4 face_width) float32; an empty pixel is +inf."""
        params = VisibilityParams(*(params or VisibilityParams()))
        n = len(submaps)
        if n == 0:
            raise ValueError("depthImages needs at least one submap")
        li = self._layout(*layout)
        arr, keep, residency, _, _ = self._submap_table(submaps, None, int(layout[0]))
        H, W4 = params.shape
        out, optr, out_dev = self._float_out(out, (n, H, W4), bool(residency), "out")
        dev_holders = [h for h in keep if _is_torch_cuda(h)]
        if dev_holders:
            _order_after_torch(self, dev_holders[-1])
        cp = params.struct()
        capi.check(self._lib.lsr_depth_images_build(self._h, arr, n, C.byref(li), 1 if residency else 0, C.byref(cp), 1 if eroded else 0,
                                                    C.c_void_p(optr), 1 if out_dev else 0), "depthImages")
        flat = out.view(-1) if out_dev else out.reshape(-1)
        return flat[: n * H * W4].reshape(n, H, W4)

    def _images_arg(self, images, n: int, params):
        H, W4 = params.shape
        if _is_torch_cuda(images):
            import torch

            t = images if images.is_contiguous() else images.contiguous()
            if t.dtype != torch.float32 or t.numel() < n * H * W4:
                raise ValueError("images must be float32 of shape (n, height, 4 face_width)")
            _order_after_torch(self, t)
            return t.data_ptr(), 1, t
        t = np.ascontiguousarray(images, np.float32)
        if t.size < n * H * W4:
            raise ValueError("images must be float32 of shape (n, height, 4 face_width)")
        return t.ctypes.data, 0, t

    def visibilityVotes(self, submaps, images, params: "VisibilityParams" = None, poses=None, layout=PC2_XYZI, device_out: bool = False):
        """The visibility votes against every record through lsr_visibility_votes: `images` = the ERODED depth images of the same
        submaps (depthImages; numpy array or CUDA tensor), `poses` as for assembleMap.  -> (votes (total,) int32 in assembly order — a
        CUDA tensor with device_out —, first_record (n + 1,) int64)."""
        params = VisibilityParams(*(params or VisibilityParams()))
        n = len(submaps)
        if n == 0:
            raise ValueError("visibilityVotes needs at least one submap")
        li = self._layout(*layout)
        arr, keep, residency, total, P = self._submap_table(submaps, poses, int(layout[0]))
        iptr, idev, ikeep = self._images_arg(images, n, params)   # ikeep: the buffer the call reads, kept alive until it returns
        if device_out:
            import torch

            votes = torch.empty(max(total, 1), dtype=torch.int32, device=torch.device("cuda", self._device))
            _order_after_torch(self, votes)
            vptr = votes.data_ptr()
        else:
            votes = np.zeros(max(total, 1), np.int32)
            vptr = votes.ctypes.data
        dev_holders = [h for h in keep if _is_torch_cuda(h)]
        if dev_holders:
            _order_after_torch(self, dev_holders[-1])
        first = (C.c_size_t * (n + 1))()
        n_rec = C.c_size_t()
        cp = params.struct()
        capi.check(self._lib.lsr_visibility_votes(self._h, arr, n, C.byref(li), 1 if residency else 0,
                                                  P.ctypes.data_as(C.POINTER(C.c_double)) if P is not None else None, C.c_void_p(iptr), idev,
                                                  C.byref(cp), C.c_void_p(vptr), 1 if device_out else 0, first, C.byref(n_rec)),
                   "visibilityVotes")
        return votes[: n_rec.value], np.array(first[:], np.int64)

    def assembleMapStatic(self, submaps, images, params: "VisibilityParams" = None, poses=None, in_layout=PC2_XYZI, out_layout=PC2_XYZI,
                          out=None, device_out=None, count_only: bool = False):
        """assembleMap without what moved (lsr_assemble_map_static): the records of assembleMap(submaps, poses, ...) with fewer than
        params.min_votes visibility votes against them, in input order.  `images`: the eroded depth images of the same submaps
        (depthImages / MapArray.depth_images).  `out` as for assembleMap; `device_out`: where a new buffer lives (None: where the
        clouds are).  -> (records (kept, out point_step) uint8, first_record (n + 1,) int64 indexing the kept records, n_removed);
        count_only: records is None and nothing is written."""
        params = VisibilityParams(*(params or VisibilityParams()))
        n = len(submaps)
        if n == 0:
            raise ValueError("assembleMapStatic needs at least one submap")
        li, lo = self._layout(*in_layout), self._layout(*out_layout)
        out_step = int(out_layout[0])
        arr, keep, residency, total, P = self._submap_table(submaps, poses, int(in_layout[0]))
        iptr, idev, ikeep = self._images_arg(images, n, params)   # ikeep: the buffer the call reads, kept alive until it returns
        dev_holders = [h for h in keep if _is_torch_cuda(h)]
        if dev_holders:
            _order_after_torch(self, dev_holders[-1])
        own = out is None
        flat, optr, cap, out_dev = None, None, 0, False
        if not count_only:
            _, flat, optr, cap, out_dev = self._out_records(out, out_step, total, bool(residency) if device_out is None else bool(device_out))
        first = (C.c_size_t * (n + 1))()
        n_out, n_removed = C.c_size_t(), C.c_size_t()
        cp = params.struct()
        capi.check(self._lib.lsr_assemble_map_static(self._h, arr, n, C.byref(li), 1 if residency else 0,
                                                     P.ctypes.data_as(C.POINTER(C.c_double)) if P is not None else None, C.c_void_p(iptr), idev,
                                                     C.byref(cp), C.c_void_p(optr) if optr is not None else None, cap, C.byref(lo),
                                                     1 if out_dev else 0, first, C.byref(n_out), C.byref(n_removed)), "assembleMapStatic")
        records = None if count_only else self._trimmed(flat, int(n_out.value), out_step, cap, own)
        return records, np.array(first[:], np.int64), int(n_removed.value)

    def visibilityPieceBytes(self, nbytes: Optional[int] = None) -> int:
        """Bytes per staging piece of host clouds in depthImages / visibilityVotes / assembleMapStatic (LSR_VISIBILITY_PIECE_BYTES,
        256 .. 1 << 30): sets it when given, returns the current value.  The images and the votes do not depend on it."""
        if nbytes is not None:
            capi.check(self._lib.lsr_set_i32(self._h, capi.VISIBILITY_PIECE_BYTES, int(nbytes)), "visibilityPieceBytes")
        return self._geti(capi.VISIBILITY_PIECE_BYTES)

    def visibilityMs(self):
        """hipEvent time [ms] of the launches of the last depthImages and of the last visibilityVotes / assembleMapStatic on this object
        (setProfiling(True)), else 0.  -> (images, votes)"""
        return self._getf(capi.DEPTH_IMAGES_MS), self._getf(capi.VISIBILITY_MS)

    def _submap_table(self, submaps, poses, in_step: int):
        """The lsr_submap array of assembleMap / saveMapPCDFileASCII -> (array, keepalives, on_device, total records, column-major
        poses or None)."""
        n = len(submaps)
        arr = (capi.SubMap * n)()
        keep, residency = [], None
        for i, sm in enumerate(submaps):
            ptr, cnt, dev, holder = _record_args(sm.cloud, in_step)
            keep.append(holder)
            if cnt:
                if residency is None:
                    residency = dev
                elif dev != residency:
                    raise ValueError("all submap clouds must share residency (host/device)")
            arr[i].position[:] = [float(v) for v in sm.position]
            arr[i].orientation[:] = [float(v) for v in sm.orientation]
            arr[i].distance = float(getattr(sm, "distance", 0.0))
            arr[i].cloud = ptr if cnt else None
            arr[i].n_points = cnt
        if residency is None:
            residency = any(_is_torch_cuda(h) for h in keep)
        total = int(sum(a.n_points for a in arr))
        P = None
        if poses is not None:
            if len(poses) != n:
                raise ValueError("one pose per submap")
            P = np.ascontiguousarray(np.stack([np.asarray(p, np.float64).reshape(4, 4).T.reshape(16) for p in poses]), np.float64)
        return arr, keep, residency, total, P

    # -- map.pcd ---------------------------------------------------------------------
    def formatPCDASCII(self, records, layout=PC2_XYZI, out=None):
        """The bytes pcl::io::savePCDFileASCII writes for a cloud of these records (header and body), formatted on the
        device through lsr_format_pcd_ascii.  `records`: a record buffer of `layout` — numpy array (-> uint8 numpy array) or CUDA
        tensor (-> uint8 CUDA tensor, nothing leaves HBM).  `out`: None = a new buffer, or a contiguous uint8 buffer to write; the
        result is the view of it that holds the text."""
        lay = self._layout(*layout)
        ptr, n, dev, keep = _payload_args(self, records, int(layout[0]))
        size = C.c_size_t()
        if out is None:
            capi.check(self._lib.lsr_format_pcd_ascii(self._h, ptr, n, C.byref(lay), 1 if dev else 0, None, 0, 0, C.byref(size)),
                       "formatPCDASCII")
            if dev:
                import torch

                out = torch.empty(size.value, dtype=torch.uint8, device=torch.device("cuda", self._device))
            else:
                out = np.zeros(size.value, np.uint8)
        out_dev = _is_torch_cuda(out)
        if out_dev:
            if not out.is_contiguous() or out.element_size() != 1:
                raise ValueError("out must be a contiguous uint8 buffer")
            flat, optr, cap = out.view(-1), out.data_ptr(), out.numel()
            _order_after_torch(self, out)
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable):
                raise ValueError("out must be a writeable contiguous uint8 buffer")
            flat, optr, cap = out.reshape(-1), out.ctypes.data, out.nbytes
        capi.check(self._lib.lsr_format_pcd_ascii(self._h, ptr, n, C.byref(lay), 1 if dev else 0, C.c_void_p(optr), cap,
                                                  1 if out_dev else 0, C.byref(size)), "formatPCDASCII")
        return flat[: size.value]

    def savePCDFileASCII(self, path, records, layout=PC2_XYZI) -> int:
        """pcl::io::savePCDFileASCII(path, cloud) through lsr_save_pcd_ascii: the same bytes, formatted on the device piece by piece
        while this thread writes the file.  `records` as for formatPCDASCII.  Returns the file's size in bytes."""
        lay = self._layout(*layout)
        ptr, n, dev, keep = _payload_args(self, records, int(layout[0]))
        size = C.c_size_t()
        capi.check(self._lib.lsr_save_pcd_ascii(self._h, os.fsencode(path), ptr, n, C.byref(lay), 1 if dev else 0, C.byref(size)),
                   "savePCDFileASCII")
        return int(size.value)

    def saveMapPCDFileASCII(self, path, submaps, poses=None, in_layout=PC2_XYZI, leaf=None) -> int:
        """`if (do_save_map) pcl::io::savePCDFileASCII("map.pcd", *map_ptr)` (graph_based_slam_component.cpp:369) in one call
        (lsr_save_map_pcd_ascii): the submaps moved by their poses (`poses`: None = their own, or the optimiser's, as for assembleMap)
        into a map that stays on the device, and that map written as text.  Returns the file's size in bytes.  `leaf`: as for
        saveMapPCDFile."""
        if leaf is not None:
            return self.saveMapPCDFile(path, submaps, poses, in_layout, "ascii", leaf)
        n = len(submaps)
        if n == 0:
            raise ValueError("saveMapPCDFileASCII needs at least one submap")
        li = self._layout(*in_layout)
        arr, keep, residency, _, P = self._submap_table(submaps, poses, int(in_layout[0]))
        dev_holders = [h for h in keep if _is_torch_cuda(h)]
        if dev_holders:
            _order_after_torch(self, dev_holders[-1])
        size = C.c_size_t()
        capi.check(self._lib.lsr_save_map_pcd_ascii(self._h, os.fsencode(path), arr, n, C.byref(li), 1 if residency else 0,
                                                    P.ctypes.data_as(C.POINTER(C.c_double)) if P is not None else None, C.byref(size)),
                   "saveMapPCDFileASCII")
        return int(size.value)

    # -- map.pcd as DATA binary / DATA binary_compressed ----------------------------------------------
    @staticmethod
    def _pcd_kind(data) -> int:
        """"ascii" / "binary" / "binary_compressed" -> lsr_pcd_data; an integer is passed on as it is (the library judges it)."""
        if isinstance(data, str):
            if data not in capi.PCD_DATA_KINDS:
                raise ValueError(f"data must be one of {sorted(capi.PCD_DATA_KINDS)}")
            return capi.PCD_DATA_KINDS[data]
        return int(data)

    def formatPCD(self, records, layout=PC2_XYZI, data="binary", out=None):
        """The whole image of a .pcd file of these records through lsr_format_pcd: `data` = "binary" (packed records, the fields bit for
        bit), "binary_compressed" (the field-major image as one LZF stream, compressed on the device; the stream depends on the
        image alone) or "ascii" (formatPCDASCII's bytes).  `records`, `out` and the result as for formatPCDASCII."""
        kind = self._pcd_kind(data)
        lay = self._layout(*layout)
        ptr, n, dev, keep = _payload_args(self, records, int(layout[0]))
        size = C.c_size_t()
        if out is None:
            capi.check(self._lib.lsr_format_pcd(self._h, ptr, n, C.byref(lay), 1 if dev else 0, kind, None, 0, 0, C.byref(size)), "formatPCD")
            if dev:
                import torch

                out = torch.empty(size.value, dtype=torch.uint8, device=torch.device("cuda", self._device))
            else:
                out = np.zeros(size.value, np.uint8)
        out_dev = _is_torch_cuda(out)
        if out_dev:
            if not out.is_contiguous() or out.element_size() != 1:
                raise ValueError("out must be a contiguous uint8 buffer")
            flat, optr, cap = out.view(-1), out.data_ptr(), out.numel()
            _order_after_torch(self, out)
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable):
                raise ValueError("out must be a writeable contiguous uint8 buffer")
            flat, optr, cap = out.reshape(-1), out.ctypes.data, out.nbytes
        capi.check(self._lib.lsr_format_pcd(self._h, ptr, n, C.byref(lay), 1 if dev else 0, kind, C.c_void_p(optr), cap,
                                            1 if out_dev else 0, C.byref(size)), "formatPCD")
        return flat[: size.value]

    def savePCDFile(self, path, records, layout=PC2_XYZI, data="ascii") -> int:
        """The same image written to `path` through lsr_save_pcd: a binary body packed and copied piece by piece while this thread writes
        the file; a compressed body compressed whole in HBM, then copied and written in pieces.  Returns the file's size in bytes."""
        kind = self._pcd_kind(data)
        lay = self._layout(*layout)
        ptr, n, dev, keep = _payload_args(self, records, int(layout[0]))
        size = C.c_size_t()
        capi.check(self._lib.lsr_save_pcd(self._h, os.fsencode(path), ptr, n, C.byref(lay), 1 if dev else 0, kind, C.byref(size)), "savePCDFile")
        return int(size.value)

    def saveMapPCDFile(self, path, submaps, poses=None, in_layout=PC2_XYZI, data="ascii", leaf=None) -> int:
        """saveMapPCDFileASCII with a body kind (lsr_save_map_pcd): the submaps moved by their poses into a map that stays on the device,
        and that map written as `data`.  Returns the file's size in bytes.  `leaf`: None = the raw map; a leaf size = the map
        thinned by voxelGridFilterMap on the device before it is written (lsr_save_map_pcd_filtered; the number of records in the
        file is then getSavedMapPoints())."""
        kind = self._pcd_kind(data)
        n = len(submaps)
        if n == 0:
            raise ValueError("saveMapPCDFile needs at least one submap")
        li = self._layout(*in_layout)
        arr, keep, residency, _, P = self._submap_table(submaps, poses, int(in_layout[0]))
        dev_holders = [h for h in keep if _is_torch_cuda(h)]
        if dev_holders:
            _order_after_torch(self, dev_holders[-1])
        size = C.c_size_t()
        if leaf is not None:
            n_pts = C.c_size_t()
            capi.check(self._lib.lsr_save_map_pcd_filtered(self._h, os.fsencode(path), arr, n, C.byref(li), 1 if residency else 0,
                                                           P.ctypes.data_as(C.POINTER(C.c_double)) if P is not None else None,
                                                           C.c_float(float(leaf)), kind, C.byref(n_pts), C.byref(size)), "saveMapPCDFile")
            self._saved_map_points = int(n_pts.value)
            return int(size.value)
        capi.check(self._lib.lsr_save_map_pcd(self._h, os.fsencode(path), arr, n, C.byref(li), 1 if residency else 0,
                                              P.ctypes.data_as(C.POINTER(C.c_double)) if P is not None else None, kind, C.byref(size)),
                   "saveMapPCDFile")
        return int(size.value)

    def getSavedMapPoints(self) -> int:
        """The number of records the last saveMapPCDFile(..., leaf=...) on this object wrote (0 = none yet)."""
        return int(getattr(self, "_saved_map_points", 0))

    def lzfDeflate(self, image):
        """The compressor alone (lsr_lzf_deflate): the LZF stream of `image` — bytes / uint8 numpy array (-> uint8 numpy array) or CUDA
        uint8 tensor (-> CUDA tensor) — under the chunked rule of include/lidarslam_reg.h; a function of the bytes alone."""
        if _is_torch_cuda(image):
            if not image.is_contiguous() or image.element_size() != 1:
                raise ValueError("image must be a contiguous uint8 buffer")
            _order_after_torch(self, image)
            ptr, size, dev, keep = image.data_ptr(), image.numel(), 1, image
        else:
            keep = np.frombuffer(image, np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else np.ascontiguousarray(image).reshape(-1).view(np.uint8)
            ptr, size, dev = keep.ctypes.data, keep.size, 0
        n = C.c_size_t()
        capi.check(self._lib.lsr_lzf_deflate(self._h, C.c_void_p(ptr), size, dev, None, 0, 0, C.byref(n)), "lzfDeflate")
        if dev:
            import torch

            out = torch.empty(n.value, dtype=torch.uint8, device=torch.device("cuda", self._device))
            _order_after_torch(self, out)
            optr = out.data_ptr()
        else:
            out = np.zeros(n.value, np.uint8)
            optr = out.ctypes.data
        capi.check(self._lib.lsr_lzf_deflate(self._h, C.c_void_p(ptr), size, dev, C.c_void_p(optr), n.value, dev, C.byref(n)), "lzfDeflate")
        return out

    def pcdDeflateMs(self) -> float:
        """With LSR_PROFILE = 1, the hipEvent time [ms] of the deflate launches of the last compressed formatPCD / savePCDFile /
        saveMapPCDFile on this object (LSR_PCD_DEFLATE_MS); 0 after another kind."""
        return self._getf(capi.PCD_DEFLATE_MS)

    def pcdPieceRecords(self, records: Optional[int] = None) -> int:
        """Records per piece of savePCDFileASCII / saveMapPCDFileASCII (LSR_PCD_PIECE_RECORDS, 64 .. 1 << 22): sets it when given,
        returns the current value.  The file's bytes do not depend on it."""
        if records is not None:
            capi.check(self._lib.lsr_set_i32(self._h, capi.PCD_PIECE_RECORDS, int(records)), "pcdPieceRecords")
        return self._geti(capi.PCD_PIECE_RECORDS)

    # -- reading .pcd files ----------------------------------------------------------------------------
    def decodePCD(self, image, layout=PC2_XYZI):
        """The records of a whole .pcd file image (PCD v0.7, DATA ascii or binary, binary_compressed after pcdReadCompressed(True); the
        inverse of formatPCDASCII), decoded on the device
        through lsr_decode_pcd.  `image`: bytes / uint8 numpy array (-> (n, point_step) uint8 numpy array) or CUDA uint8 tensor (-> CUDA
        tensor, nothing leaves HBM).  `layout`: (point_step, (x, y, z, intensity or None)) of the records wanted."""
        lay = self._layout(*layout)
        step = int(layout[0])
        if _is_torch_cuda(image):
            if not image.is_contiguous() or image.element_size() != 1:
                raise ValueError("image must be a contiguous uint8 buffer")
            _order_after_torch(self, image)
            ptr, size, dev, keep = image.data_ptr(), image.numel(), 1, image
        else:
            keep = np.frombuffer(image, np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else np.ascontiguousarray(image).reshape(-1).view(np.uint8)
            ptr, size, dev = keep.ctypes.data, keep.size, 0
        n = C.c_size_t()
        capi.check(self._lib.lsr_decode_pcd(self._h, C.c_void_p(ptr), size, dev, None, 0, None, 0, C.byref(n)), "decodePCD")
        if dev:
            import torch

            out = torch.empty((n.value, step), dtype=torch.uint8, device=torch.device("cuda", self._device))
            _order_after_torch(self, out)
            optr = out.data_ptr()
        else:
            out = np.zeros((n.value, step), np.uint8)
            optr = out.ctypes.data
        capi.check(self._lib.lsr_decode_pcd(self._h, C.c_void_p(ptr), size, dev, C.c_void_p(optr), n.value, C.byref(lay), dev, C.byref(n)),
                   "decodePCD")
        return out

    def loadPCDFile(self, path, layout=PC2_XYZI, device=False):
        """The records of the .pcd file `path` through lsr_load_pcd: read piece by piece by this thread while the device parses the
        piece before.  -> (n, point_step) uint8: a numpy array, or with device=True a CUDA tensor."""
        lay = self._layout(*layout)
        step = int(layout[0])
        n = C.c_size_t()
        capi.check(self._lib.lsr_load_pcd(self._h, os.fsencode(path), None, 0, None, 0, C.byref(n)), "loadPCDFile")
        if device:
            import torch

            out = torch.empty((n.value, step), dtype=torch.uint8, device=torch.device("cuda", self._device))
            _order_after_torch(self, out)
            optr = out.data_ptr()
        else:
            out = np.zeros((n.value, step), np.uint8)
            optr = out.ctypes.data
        capi.check(self._lib.lsr_load_pcd(self._h, os.fsencode(path), C.c_void_p(optr), n.value, C.byref(lay), 1 if device else 0, C.byref(n)),
                   "loadPCDFile")
        return out

    def setInputTargetPCD(self, path) -> int:
        """setInputTarget from a .pcd file (lsr_set_input_target_pcd): the file's records stay on the device.  Returns the point count."""
        n = C.c_size_t()
        capi.check(self._lib.lsr_set_input_target_pcd(self._h, os.fsencode(path), C.byref(n)), "setInputTargetPCD")
        self._n_target = int(n.value)
        self._keep["target"] = None
        return self._n_target

    def pcdReadPieceBytes(self, nbytes: Optional[int] = None) -> int:
        """Bytes per piece of loadPCDFile / setInputTargetPCD (LSR_PCD_READ_PIECE_BYTES, 2048 .. 1 << 28): sets it when given, returns
        the current value.  The records do not depend on it."""
        if nbytes is not None:
            capi.check(self._lib.lsr_set_i32(self._h, capi.PCD_READ_PIECE_BYTES, int(nbytes)), "pcdReadPieceBytes")
        return self._geti(capi.PCD_READ_PIECE_BYTES)

    def pcdReadCompressed(self, on: Optional[bool] = None) -> bool:
        """Whether decodePCD / loadPCDFile / setInputTargetPCD of this object read DATA binary_compressed files, the LZF stream inflated
        on the device (LSR_PCD_READ_COMPRESSED, off by default: such a file is then refused as not implemented): sets it when given,
        returns the current value."""
        if on is not None:
            capi.check(self._lib.lsr_set_i32(self._h, capi.PCD_READ_COMPRESSED, 1 if on else 0), "pcdReadCompressed")
        return bool(self._geti(capi.PCD_READ_COMPRESSED))

    def pcdUnresolvedTokens(self) -> int:
        """Values of the last decodePCD / loadPCDFile / setInputTargetPCD the device left to the C library (LSR_PCD_UNRESOLVED_TOKENS)."""
        return self._geti(capi.PCD_UNRESOLVED_TOKENS)

    def optimizePoseGraph(self, poses, edges, max_iterations: int = 10, band: int = 5):
        """The optimiser half of doPoseAdjustment (graph_based_slam_component.cpp:267-319) through lsr_optimize_pose_graph_long: g2o's
        VertexSE3 / EdgeSE3 graph (identity information, vertex 0 fixed) under its Levenberg-Marquardt controller, on this object's
        device.  `poses`: (n, 4, 4) fp64; `edges`: (from, to, 4x4 measurement from^-1 * to) — pose_graph.adjacent_edges(poses) followed by
        the loop edges, up to 1024 of them outside the band.  Returns ((n, 4, 4) fp64 poses — what assembleMap takes as `poses` —,
        pose_graph.PoseGraphResult)."""
        from . import pose_graph

        return pose_graph.optimize(self, poses, edges, max_iterations, band)

    def mapAssemblyForm(self) -> int:
        """Which kernel form the last assembleMap on this object took (LSR_MAP_ASSEMBLY_FORM): 1 = wide, 2 = general; 0 = none yet."""
        return self._geti(capi.MAP_ASSEMBLY_FORM)

    def shareTargetOf(self, other: "Registration"):
        """Register against the target already resident in `other` (N keyframes vs one submap)."""
        capi.check(self._lib.lsr_share_target(self._h, other._h), "shareTargetOf")

    # -- align + accessors -------------------------------------------------------------------
    def align(self, guess=None, output: bool = False):
        """registration_->align(output, guess) (scanmatcher_component.cpp:353).  Returns the
        transformed source as (n,3) fp32 when output=True, else None (both reference callers
        discard it)."""
        g = _mat_to_col16(guess) if guess is not None else None
        gp = g.ctypes.data_as(C.POINTER(C.c_float)) if g is not None else None
        fin = np.zeros(16, np.float32)
        out = None
        outp, stride = None, 0
        if output:
            out = np.zeros((self._n_source, 3), np.float32)
            outp, stride = C.c_void_p(out.ctypes.data), 12
        capi.check(self._lib.lsr_align(self._h, gp, fin.ctypes.data_as(C.POINTER(C.c_float)), C.byref(self._last), outp,
                                       stride), "align")
        return out

    def getFinalTransformation(self) -> np.ndarray:  # scanmatcher_component.cpp:356
        fin = np.zeros(16, np.float32)
        capi.check(self._lib.lsr_get_final_transformation(self._h, fin.ctypes.data_as(C.POINTER(C.c_float))),
                   "getFinalTransformation")
        return _col16_to_mat(fin)

    def hasConverged(self) -> bool:  # scanmatcher_component.cpp:375
        v = C.c_int32()
        capi.check(self._lib.lsr_has_converged(self._h, C.byref(v)), "hasConverged")
        return bool(v.value)

    def getFitnessScore(self, max_range: float = 1.7976931348623157e308) -> float:  # graph_based_slam_component.cpp:231
        v = C.c_double()
        capi.check(self._lib.lsr_get_fitness_score(self._h, float(max_range), C.byref(v)), "getFitnessScore")
        return v.value

    # -- extras (not part of the PCL surface) -------------------------------------------------
    @property
    def last_result(self) -> dict:
        r = self._last
        return dict(converged=bool(r.converged), iterations=int(r.iterations), score=float(r.score),
                    n_evaluations=int(r.n_evaluations), n_correspondences=int(r.n_correspondences),
                    gpu_ms=float(r.gpu_ms))

    def getFinalNumIteration(self) -> int:
        return int(self._last.iterations)

    def nearestNeighbors(self, T=None):
        idx = np.zeros(self._n_source, np.int32)
        d2 = np.zeros(self._n_source, np.float32)
        t = _mat_to_col16(T) if T is not None else None
        capi.check(self._lib.lsr_nearest_neighbors(self._h, t.ctypes.data_as(C.POINTER(C.c_float)) if t is not None else None,
                                                   idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   d2.ctypes.data_as(C.POINTER(C.c_float))), "nearestNeighbors")
        return idx, d2

    def setTuning(self, workgroup: Optional[int] = None, table_mode: Optional[int] = None, grid_builder: Optional[int] = None,
                  wait_mode: Optional[int] = None, quad: Optional[int] = None, split: Optional[int] = None):
        """Tuning keys of the core (no effect on results: every derivative kernel returns the same bits): NDT workgroup (0 auto;
        quad kernel: 64 / 128 points, lane kernel: 512 / 1024 threads), kernel (quad: -1 auto, 0 lane kernel, 1 quad kernel),
        where the derivative pass reads the voxel table (-1 auto, 0 dense global, 1 compact global, 2 LDS), the
        grid builder (0 auto, 1 radix sort), how the calling thread waits (0 spin, 1 yield, 2 sleep), two waves per chunk in the
        512-thread lane kernel of a single registration (split: -1 auto, 0, 1)."""
        if workgroup is not None:
            self._seti(capi.NDT_WORKGROUP, workgroup, "setTuning(workgroup)")
        if table_mode is not None:
            self._seti(capi.NDT_TABLE_MODE, table_mode, "setTuning(table_mode)")
        if grid_builder is not None:
            self._seti(capi.GRID_BUILDER, grid_builder, "setTuning(grid_builder)")
        if wait_mode is not None:
            self._seti(capi.WAIT_MODE, wait_mode, "setTuning(wait_mode)")
        if quad is not None:
            self._seti(capi.NDT_QUAD, quad, "setTuning(quad)")
        if split is not None:
            self._seti(capi.NDT_SPLIT, split, "setTuning(split)")

    def setProfiling(self, on: bool):
        self._seti(capi.PROFILE, 1 if on else 0, "setProfiling")

    def getProfile(self, reset: bool = False) -> dict:
        p = capi.Profile()
        capi.check(self._lib.lsr_get_profile(self._h, C.byref(p), 1 if reset else 0), "getProfile")
        return dict(deriv_ms_total=p.deriv_ms_total, deriv_launches=p.deriv_launches, deriv_points=p.deriv_points,
                    deriv_pairs=p.deriv_pairs)


class NormalDistributionsTransform(Registration):
    """pclomp::NormalDistributionsTransform<PointXYZI,PointXYZI> (scanmatcher_component.cpp:105-113)."""

    _method = capi.METHOD_NDT

    def setResolution(self, res: float):  # scanmatcher_component.cpp:107
        self._setf(capi.RESOLUTION, res, "setResolution")

    def getResolution(self) -> float:
        return self._getf(capi.RESOLUTION)

    def setStepSize(self, s: float):
        self._setf(capi.STEP_SIZE, s, "setStepSize")

    def getStepSize(self) -> float:
        return self._getf(capi.STEP_SIZE)

    def setOulierRatio(self, r: float):  # (sic) PCL spells it this way
        self._setf(capi.OUTLIER_RATIO, r, "setOulierRatio")

    setOutlierRatio = setOulierRatio

    def setNeighborhoodSearchMethod(self, method: int):  # scanmatcher_component.cpp:110
        self._seti(capi.NEIGHBORHOOD, method, "setNeighborhoodSearchMethod")

    def setNumThreads(self, n: int):  # scanmatcher_component.cpp:111 — CPU hint, accepted and ignored
        self._seti(capi.NUM_THREADS, n, "setNumThreads")

    def setHessianD1Sign(self, sign: int):
        self._seti(capi.HESSIAN_D1_SIGN, sign, "setHessianD1Sign")

    def getTransformationProbability(self) -> float:
        return float(self._last.score)

    # inspection ----------------------------------------------------------------------------
    def gridInfo(self) -> dict:
        info = np.zeros(8, np.int32)
        capi.check(self._lib.lsr_ndt_grid_info(self._h, info.ctypes.data_as(C.POINTER(C.c_int32))), "gridInfo")
        return dict(min_b=info[0:3].copy(), max_b=info[3:6].copy(), n_leaves=int(info[6]), n_valid=int(info[7]))

    def gridDump(self) -> dict:
        n = self.gridInfo()["n_leaves"]
        idx, npts = np.zeros(n, np.int32), np.zeros(n, np.int32)
        mean, icov = np.zeros((n, 3)), np.zeros((n, 3, 3))
        capi.check(self._lib.lsr_ndt_grid_dump(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                               npts.ctypes.data_as(C.POINTER(C.c_int32)),
                                               mean.ctypes.data_as(C.POINTER(C.c_double)),
                                               icov.ctypes.data_as(C.POINTER(C.c_double))), "gridDump")
        return dict(idx=idx, n=npts, mean=mean, icov=icov)

    def gridCentroids(self) -> np.ndarray:
        """(n_leaves, 3) fp32, in gridDump's order: the leaves' FLOAT centroids (the points of the voxel-centroid kd-tree that the
        KDTREE neighbourhood searches); NaN for leaves outside the kd-tree (fewer than 6 points)."""
        c = np.zeros((self.gridInfo()["n_leaves"], 3), np.float32)
        capi.check(self._lib.lsr_ndt_grid_centroids(self._h, c.ctypes.data_as(C.POINTER(C.c_float))), "gridCentroids")
        return c

    def derivatives(self, p, T=None, compute_hessian=True, with_pairs: bool = False):
        """One derivative pass.  compute_hessian: False / True, or 2 for the fused form of a line search's tenth trial (score and
        gradient reduced as a gradient-only pass, the Hessian as a pass with Hessian).  with_pairs: also return the pair count."""
        p = np.ascontiguousarray(p, np.float64)
        t = _mat_to_col16(T) if T is not None else None
        score, pairs = C.c_double(), C.c_double()
        g, H = np.zeros(6), np.zeros((6, 6))
        form = 2 if (compute_hessian is not True and compute_hessian == 2) else (1 if compute_hessian else 0)
        capi.check(self._lib.lsr_ndt_derivatives_pairs(self._h, p.ctypes.data_as(C.POINTER(C.c_double)),
                                                       t.ctypes.data_as(C.POINTER(C.c_float)) if t is not None else None,
                                                       form, C.byref(score),
                                                       g.ctypes.data_as(C.POINTER(C.c_double)),
                                                       H.ctypes.data_as(C.POINTER(C.c_double)), C.byref(pairs)), "derivatives")
        if with_pairs:
            return score.value, g, H, pairs.value
        return score.value, g, H

    # pose search ---------------------------------------------------------------------------
    poseLattice = staticmethod(poseLattice)
    selectPoses = staticmethod(selectPoses)

    def scorePoses(self, poses):
        """The NDT score and pair count of the source at every pose of `poses` ((count, 4, 4)) in one launch (lsr_ndt_score_poses):
        the bits derivatives(p, T=pose, compute_hessian=False, with_pairs=True) returns per pose.  -> (score, pairs), fp64."""
        p = _poses_to_col16(poses)
        score, pairs = np.zeros(p.shape[0]), np.zeros(p.shape[0])
        capi.check(self._lib.lsr_ndt_score_poses(self._h, p.ctypes.data_as(C.POINTER(C.c_float)), p.shape[0],
                                                 score.ctypes.data_as(C.POINTER(C.c_double)),
                                                 pairs.ctypes.data_as(C.POINTER(C.c_double))), "scorePoses")
        return score, pairs

    def poseSearchMs(self) -> float:
        """hipEvent time [ms] of the last scorePoses / searchPose's scoring launch on this object (setProfiling(True)), else 0."""
        return self._getf(capi.POSE_SEARCH_MS)

    def searchPose(self, center, n=(1, 1, 1), step=(1.0, 1.0, 1.0), n_yaw: int = 1, yaw_step: float = 0.0, top_k: int = 16,
                   min_sep_m: float = 0.9, min_sep_rad: float = 0.1308996938995747):
        """lsr_ndt_search_pose: the lattice around `center` scored, the distinct best top_k refined as one candidate set, the winner
        by trans_probability.  -> (pose, result, report): pose (4, 4) fp32 or None when nothing was kept; result as last_result;
        report: n_candidates, kept, coarse_score, refined (n_kept, 4, 4), results (one dict per kept candidate), winner."""
        c = _mat_to_col16(center)
        prm = capi.PoseSearchParams(capi.PoseLattice((C.c_int32 * 3)(*[int(v) for v in n]), (C.c_double * 3)(*[float(v) for v in step]),
                                                     int(n_yaw), float(yaw_step)), int(top_k), float(min_sep_m), float(min_sep_rad))
        best = np.zeros(16, np.float32)
        rep = capi.PoseSearchReport()
        capi.check(self._lib.lsr_ndt_search_pose(self._h, c.ctypes.data_as(C.POINTER(C.c_float)), C.byref(prm),
                                                 best.ctypes.data_as(C.POINTER(C.c_float)), C.byref(self._last), C.byref(rep)), "searchPose")
        k = int(rep.n_kept)

        def as_dict(r):
            return dict(converged=bool(r.converged), iterations=int(r.iterations), score=float(r.score),
                        n_evaluations=int(r.n_evaluations), n_correspondences=int(r.n_correspondences), gpu_ms=float(r.gpu_ms))

        refined = np.ctypeslib.as_array(rep.refined16).reshape(16, 4, 4)[:k].transpose(0, 2, 1).copy()
        report = dict(n_candidates=int(rep.n_candidates), n_kept=k, winner=int(rep.winner),
                      kept=np.array(rep.kept[:k], np.int32), coarse_score=np.array(rep.coarse_score[:k], np.float64),
                      refined=refined, results=[as_dict(rep.refined[e]) for e in range(k)])
        return (_col16_to_mat(best) if k > 0 else None), self.last_result, report


class GeneralizedIterativeClosestPoint(Registration):
    """pclomp::GeneralizedIterativeClosestPoint<PointXYZI,PointXYZI> (scanmatcher_component.cpp:115-120)."""

    _method = capi.METHOD_GICP

    def setRotationEpsilon(self, eps: float):
        self._setf(capi.ROTATION_EPSILON, eps, "setRotationEpsilon")

    def setCorrespondenceRandomness(self, k: int):
        self._seti(capi.K_CORRESPONDENCES, k, "setCorrespondenceRandomness")

    def setMaximumOptimizerIterations(self, n: int):
        self._seti(capi.MAX_INNER_ITERATIONS, n, "setMaximumOptimizerIterations")

    def covariances(self, which: str, raw: bool = False) -> np.ndarray:
        """Per-point covariances; raw=True: the k-neighbour sample covariance before the eigen-regularisation."""
        w = (0 if which == "source" else 1) + (2 if raw else 0)
        n = self._n_source if w in (0, 2) else self._n_target
        cov = np.zeros((n, 3, 3))
        capi.check(self._lib.lsr_gicp_covariances(self._h, w, cov.ctypes.data_as(C.POINTER(C.c_double))), "covariances")
        return cov

    def setInputTarget(self, cloud):
        super().setInputTarget(cloud)
        self._n_target = int(np.shape(cloud)[0]) if not _is_torch_cuda(cloud) else int(cloud.shape[0])

    def linearize(self, guess=None, trans=None, use_seeds: bool = False) -> dict:
        """Inspection (lsr_gicp_linearize): the first correspondence pass and the first Gauss-Newton accumulation of the outer
        iteration of align(guess) whose transformation_ is `trans` (4x4, None = identity), run by align's own launches.
        use_seeds: offer the neighbours of the previous align / linearize as search seeds (an outer iteration after the first).
        Returns out (n,3) = guess * source, nn_idx (n,), valid (n,), M6 (n,6) = 00 01 02 11 12 22 of the Mahalanobis matrices,
        q (n,3) paired target points, x6, T12 (3,4) fp32, dR (3,3,3) of the state, m, sums28 (before the division by m)."""
        n = self._n_source
        fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
        g = _mat_to_col16(guess) if guess is not None else None
        t = _mat_to_col16(trans) if trans is not None else None
        r = dict(out=np.zeros((n, 3), np.float32), nn_idx=np.zeros(n, np.int32), valid=np.zeros(n, np.int32),
                 M6=np.zeros((n, 6)), q=np.zeros((n, 3), np.float32), x6=np.zeros(6), T12=np.zeros((3, 4), np.float32),
                 dR=np.zeros((3, 3, 3)), sums28=np.zeros(28))
        m = C.c_int32()
        capi.check(self._lib.lsr_gicp_linearize(
            self._h, g.ctypes.data_as(fp) if g is not None else None, t.ctypes.data_as(fp) if t is not None else None,
            1 if use_seeds else 0, r["out"].ctypes.data_as(fp), r["nn_idx"].ctypes.data_as(ip), r["valid"].ctypes.data_as(ip),
            r["M6"].ctypes.data_as(dp), r["q"].ctypes.data_as(fp), r["x6"].ctypes.data_as(dp), r["T12"].ctypes.data_as(fp),
            r["dR"].ctypes.data_as(dp), C.byref(m), r["sums28"].ctypes.data_as(dp)), "linearize")
        r["m"] = int(m.value)
        return r

    _OPTIMIZERS = {"gauss_newton": capi.GICP_GAUSS_NEWTON, "bfgs": capi.GICP_BFGS}

    def setOptimizer(self, name: str):
        """The inner optimiser of align(): "gauss_newton" (default) or "bfgs", the reference's own schedule (LSR_GICP_SOLVER)."""
        if name not in self._OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {sorted(self._OPTIMIZERS)}, not {name!r}")
        self._seti(capi.GICP_SOLVER, self._OPTIMIZERS[name], "setOptimizer")

    def getOptimizer(self) -> str:
        v = self._geti(capi.GICP_SOLVER)
        return next(k for k, c in self._OPTIMIZERS.items() if c == v)

    BFGS_REASONS = {0: "running", 1: "no_progress", 2: "gradient_tolerance", 3: "max_inner", 4: "non_finite"}

    def bfgs_trace(self, guess=None, trans=None, capacity: int = 4096) -> dict:
        """Inspection (lsr_gicp_bfgs_trace): ONE outer iteration of align(guess) under the BFGS optimiser — the correspondence pass at
        transformation_ = `trans` (4x4, None = identity) and the whole inner loop — run by align's own launches.
        Returns x (e,6), f (e,), g (e,6), inner (e,) per evaluation (the first `capacity`), n_evals, n_inner, reason (code) and
        reason_name, x_final (6,), m."""
        fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
        g = _mat_to_col16(guess) if guess is not None else None
        t = _mat_to_col16(trans) if trans is not None else None
        cap = max(int(capacity), 0)
        x, f, gr = np.zeros((max(cap, 1), 6)), np.zeros(max(cap, 1)), np.zeros((max(cap, 1), 6))
        inner = np.zeros(max(cap, 1), np.int32)
        xf = np.zeros(6)
        ne, ni, why, m = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        capi.check(self._lib.lsr_gicp_bfgs_trace(
            self._h, g.ctypes.data_as(fp) if g is not None else None, t.ctypes.data_as(fp) if t is not None else None, cap,
            x.ctypes.data_as(dp), f.ctypes.data_as(dp), gr.ctypes.data_as(dp), inner.ctypes.data_as(ip), C.byref(ne), C.byref(ni),
            C.byref(why), xf.ctypes.data_as(dp), C.byref(m)), "bfgs_trace")
        e = min(int(ne.value), cap)
        return dict(x=x[:e], f=f[:e], g=gr[:e], inner=inner[:e], n_evals=int(ne.value), n_inner=int(ni.value),
                    reason=int(why.value), reason_name=self.BFGS_REASONS.get(int(why.value), "?"), x_final=xf, m=int(m.value))


def set_input_target_batch(regs: Sequence[Registration], clouds):
    """setInputTarget of every candidate of a set with the builds overlapped on the device (lsr_set_input_target_batch;
    graph_based_slam_component.cpp:181-227 per candidate).  regs[b] receives clouds[b]; all host arrays or all CUDA tensors."""
    lib = capi.load()
    B = len(regs)
    if len(clouds) != B:
        raise ValueError("one cloud per registration object")
    args = [_cloud_args(c, r) for r, c in zip(regs, clouds)]
    if B and (any(a[3] != args[0][3] for a in args) or any(a[1] != args[0][1] for a in args)):
        raise ValueError("clouds must all be host or all device, with one record stride")
    hs = (C.c_void_p * B)(*[r._h for r in regs])
    ptrs = (C.c_void_p * B)(*[a[0] for a in args])
    counts = (C.c_size_t * B)(*[a[2] for a in args])
    capi.check(lib.lsr_set_input_target_batch(hs, B, ptrs, counts, args[0][1] if B else 12, 1 if (B and args[0][3]) else 0),
               "set_input_target_batch")
    for r, a in zip(regs, args):
        r._keep["target"] = None
        if hasattr(r, "_n_target"):
            r._n_target = a[2]


def set_input_source_batch(regs: Sequence[Registration], clouds):
    """setInputSource of every candidate of a set in shared launches (lsr_set_input_source_batch)."""
    lib = capi.load()
    B = len(regs)
    if len(clouds) != B:
        raise ValueError("one cloud per registration object")
    args = [_cloud_args(c, r) for r, c in zip(regs, clouds)]
    if B and (any(a[3] != args[0][3] for a in args) or any(a[1] != args[0][1] for a in args)):
        raise ValueError("clouds must all be host or all device, with one record stride")
    hs = (C.c_void_p * B)(*[r._h for r in regs])
    ptrs = (C.c_void_p * B)(*[a[0] for a in args])
    counts = (C.c_size_t * B)(*[a[2] for a in args])
    capi.check(lib.lsr_set_input_source_batch(hs, B, ptrs, counts, args[0][1] if B else 12, 1 if (B and args[0][3]) else 0),
               "set_input_source_batch")
    for r, a in zip(regs, args):
        r._n_source = a[2]
        r._keep["source"] = a[4] if a[3] else None


def fitness_score_batch(regs: Sequence[Registration], max_range: float = 1.7976931348623157e308):
    """getFitnessScore of every candidate of a set, all searches enqueued before the first wait (lsr_get_fitness_score_batch)."""
    lib = capi.load()
    B = len(regs)
    hs = (C.c_void_p * B)(*[r._h for r in regs])
    out = (C.c_double * max(B, 1))()
    capi.check(lib.lsr_get_fitness_score_batch(hs, B, float(max_range), out), "fitness_score_batch")
    return [float(out[b]) for b in range(B)]


def align_batch(regs: Sequence[Registration], guesses=None):
    """Advance B registrations together in shared launches (BASELINE.json cfg 4).  Returns
    (finals (B,4,4) fp32, list of result dicts)."""
    lib = capi.load()
    B = len(regs)
    hs = (C.c_void_p * B)(*[r._h for r in regs])
    g = None
    if guesses is not None:
        g = np.ascontiguousarray(np.stack([_mat_to_col16(x) for x in guesses]), np.float32)
    fin = np.zeros((B, 16), np.float32)
    res = (capi.Result * B)()
    capi.check(lib.lsr_align_batch(hs, B, g.ctypes.data_as(C.POINTER(C.c_float)) if g is not None else None,
                                   fin.ctypes.data_as(C.POINTER(C.c_float)), res), "align_batch")
    finals = np.stack([_col16_to_mat(fin[b]) for b in range(B)])
    out = []
    for b, r in enumerate(regs):
        r._last = capi.Result.from_buffer_copy(res[b])
        out.append(r.last_result)
    return finals, out


def align_fitness_batch(regs: Sequence[Registration], guesses=None, max_range: float = 1.7976931348623157e308):
    """align() followed by getFitnessScore() for every candidate of a set in one call (graph_based_slam_component.cpp:230-231):
    returns (finals (B,4,4) fp32, list of result dicts, fitness scores (B,) fp64) — what align_batch + fitness_score_batch return,
    with the searches of the candidates that finish early running under the launch chain of the others."""
    lib = capi.load()
    B = len(regs)
    hs = (C.c_void_p * B)(*[r._h for r in regs])
    g = None
    if guesses is not None:
        g = np.ascontiguousarray(np.stack([_mat_to_col16(x) for x in guesses]), np.float32)
    fin = np.zeros((B, 16), np.float32)
    res = (capi.Result * B)()
    fit = np.zeros(B, np.float64)
    capi.check(lib.lsr_align_fitness_batch(hs, B, g.ctypes.data_as(C.POINTER(C.c_float)) if g is not None else None,
                                           fin.ctypes.data_as(C.POINTER(C.c_float)), res, C.c_double(max_range),
                                           fit.ctypes.data_as(C.POINTER(C.c_double))), "align_fitness_batch")
    finals = np.stack([_col16_to_mat(fin[b]) for b in range(B)])
    out = []
    for b, r in enumerate(regs):
        r._last = capi.Result.from_buffer_copy(res[b])
        out.append(r.last_result)
    return finals, out, fit
