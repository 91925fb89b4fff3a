"""Loop-closure gate: the compute half of GraphBasedSlamComponent::searchLoop()
(graph_based_slam_component.cpp:164-252) behind `lsr_search_loop`.

`SubMap` mirrors lidarslam_msgs/msg/SubMap (distance, pose, cloud); `LoopClosureParams` the node parameters
searchLoop() reads (graph_based_slam_component.cpp:23-38, same names and defaults).  `search_loop` returns the
`LoopEdge`s the reference would push into `loop_edges_` (accepted ones) plus the rejected evaluations.  The pose
graph optimisation that follows (doPoseAdjustment, graph_based_slam_component.cpp:267-319) is
`map_array.MapArray.pose_adjustment` (`Registration.optimizePoseGraph`, pose_graph.py; no g2o), and what the caller
does with the optimiser's poses right afterwards — every submap moved by its new pose, the whole map put together
(:321-368) — is `map_array.MapArray.modified_map` (`Registration.assembleMap`).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Sequence

import numpy as np

from . import _capi
from .registration import Registration, ScanContextParams, _cloud_args, _is_torch_cuda, _order_after_torch


@dataclass
class SubMap:
    """lidarslam_msgs/msg/SubMap.msg: `distance`, `pose` (position + quaternion x,y,z,w), `cloud` (pose-local xyz)."""
    cloud: object  # (n, >=3) float32 numpy array or CUDA tensor
    position: Sequence[float]
    orientation: Sequence[float] = (0.0, 0.0, 0.0, 1.0)
    distance: float = 0.0


@dataclass
class LoopClosureParams:
    threshold_loop_closure_score: float = 1.0       # graph_based_slam_component.cpp:31
    distance_loop_closure: float = 20.0             # :33
    range_of_searching_loop_closure: float = 20.0   # :35
    search_submap_num: int = 3                      # :37
    voxel_leaf_size: float = 0.2                    # :23
    top_k: int = 1                                  # 1 = the reference (nearest candidate only)
    gicp_solver: str = "gauss_newton"               # a GICP `registration`: its inner optimiser — "gauss_newton" or "bfgs" (the reference's)


@dataclass
class LoopEdge:
    pair_id: tuple                # (candidate index, num_submaps - 1)   :240
    relative_pose: np.ndarray     # 4x4 fp64: from^-1 * (final * init)   :241-245
    fitness_score: float          # :231
    accepted: bool                # fitness_score < threshold            :233
    final_transformation: np.ndarray = field(repr=False, default=None)
    converged: bool = False
    iterations: int = 0
    n_target_points: int = 0
    candidate_distance: float = 0.0


def search_loop(registration: Registration, submaps: Sequence[SubMap], params: LoopClosureParams = LoopClosureParams()) -> List[LoopEdge]:
    """All candidate evaluations, nearest candidate first (empty list = no candidate passed the distance gates)."""
    lib = _capi.load()
    if params.gicp_solver not in ("gauss_newton", "bfgs"):
        raise ValueError("gicp_solver must be \"gauss_newton\" or \"bfgs\"")
    if hasattr(registration, "setOptimizer"):   # a GICP object: every candidate's align follows it (the key travels with the object)
        registration.setOptimizer(params.gicp_solver)
    n = len(submaps)
    if n == 0:
        return []
    arr = (_capi.SubMap * n)()
    keep = []
    on_device, stride = None, None
    for i, sm in enumerate(submaps):
        ptr, st, cnt, dev, holder = _cloud_args(sm.cloud)
        keep.append(holder)
        if on_device is None:
            on_device, stride = dev, st
        elif cnt and (dev != on_device or st != stride):
            raise ValueError("all submap clouds must share residency (host/device) and point stride")
        arr[i].position[:] = [float(v) for v in sm.position]
        arr[i].orientation[:] = [float(v) for v in sm.orientation]
        arr[i].distance = float(sm.distance)
        arr[i].cloud = ptr.value
        arr[i].n_points = cnt
    # ONE ordering of the handle's stream after torch's current stream, after every .contiguous() copy above has been enqueued
    # there (an event per submap was 21 x (event record + stream wait) = 0.1 ms of a 0.55 ms call)
    dev_holders = [h for h in keep if _is_torch_cuda(h)]
    if dev_holders:
        _order_after_torch(registration, dev_holders[-1])
    cp = _capi.LoopParams(params.threshold_loop_closure_score, params.distance_loop_closure,
                          params.range_of_searching_loop_closure, params.search_submap_num, params.voxel_leaf_size,
                          params.top_k, 0)
    cap = max(1, params.top_k)
    edges = (_capi.LoopEdge * cap)()
    n_eval = C.c_int32(0)
    _capi.check(lib.lsr_search_loop(registration._h, arr, n, stride, int(bool(on_device)), C.byref(cp), edges, cap,
                                    C.byref(n_eval)), "searchLoop")
    if n_eval.value and hasattr(registration, "_n_target"):
        registration._n_target = int(edges[0].n_target_points)   # the object now holds the nearest candidate's window as its target
    out = []
    for e in edges[:n_eval.value]:
        out.append(LoopEdge(pair_id=(e.id_from, e.id_to),
                            relative_pose=np.array(e.relative_pose[:], np.float64).reshape(4, 4, order="F"),
                            fitness_score=e.fitness_score, accepted=bool(e.accepted),
                            final_transformation=np.array(e.final_transformation[:], np.float32).reshape(4, 4, order="F"),
                            converged=bool(e.converged), iterations=e.iterations, n_target_points=e.n_target_points,
                            candidate_distance=e.candidate_distance))
    return out


@dataclass
class AppearanceLoopParams:
    """lsr_appearance_loop_params: the node parameters of searchLoop() (`loop`; its range gate is not applied), the Scan Context
    parameters, the largest Scan Context distance a candidate may have, and the pose lattice searched around the appearance guess."""
    loop: LoopClosureParams = field(default_factory=LoopClosureParams)
    scan_context: ScanContextParams = ScanContextParams()
    sc_distance_threshold: float = 0.4
    lattice_n: Sequence[int] = (7, 7, 1)
    lattice_step: Sequence[float] = (1.0, 1.0, 1.0)
    n_yaw: int = 1
    yaw_step: float = 0.0
    search_top_k: int = 16
    min_sep_m: float = 0.9
    min_sep_rad: float = 0.1308996938995747


@dataclass
class AppearanceLoopEdge(LoopEdge):
    shift: int = 0                # the yaw shift of the best Scan Context distance: the candidate sees the latest scene turned by shift 2 pi / S
    sc_distance: float = 0.0      # that distance


def search_loop_appearance(registration: Registration, submaps: Sequence[SubMap], descriptors,
                           params: AppearanceLoopParams = None) -> List[AppearanceLoopEdge]:
    """The loop gate with candidate and heading from appearance (`lsr_search_loop_appearance`): the latest descriptor compared with all
    of `descriptors` ((n, R, S) float32 of Registration.scanContext / MapArray.scan_contexts; numpy array or CUDA tensor), the
    travel-gated submaps below the distance threshold ranked by it, and for each of the first `loop.top_k` the window target of
    search_loop, a pose search around the appearance guess (NDT) or one align from it (GICP), the fitness and the relative pose.
    All evaluations, most alike first (empty list = no candidate)."""
    params = params or AppearanceLoopParams()
    lib = _capi.load()
    lp = params.loop
    if lp.gicp_solver not in ("gauss_newton", "bfgs"):
        raise ValueError("gicp_solver must be \"gauss_newton\" or \"bfgs\"")
    if hasattr(registration, "setOptimizer"):
        registration.setOptimizer(lp.gicp_solver)
    n = len(submaps)
    if n == 0:
        return []
    arr = (_capi.SubMap * n)()
    keep = []
    on_device, stride = None, None
    for i, sm in enumerate(submaps):
        ptr, st, cnt, dev, holder = _cloud_args(sm.cloud)
        keep.append(holder)
        if on_device is None:
            on_device, stride = dev, st
        elif cnt and (dev != on_device or st != stride):
            raise ValueError("all submap clouds must share residency (host/device) and point stride")
        arr[i].position[:] = [float(v) for v in sm.position]
        arr[i].orientation[:] = [float(v) for v in sm.orientation]
        arr[i].distance = float(sm.distance)
        arr[i].cloud = ptr.value
        arr[i].n_points = cnt
    sc = params.scan_context
    cells = int(sc.num_rings) * int(sc.num_sectors)
    desc_dev = _is_torch_cuda(descriptors)
    if desc_dev:
        import torch

        d = descriptors if descriptors.is_contiguous() else descriptors.contiguous()
        if d.dtype != torch.float32 or d.numel() % cells:
            raise ValueError("descriptors must be float32 of shape (n, num_rings, num_sectors)")
        dptr, nd = d.data_ptr(), d.numel() // cells
    else:
        d = np.ascontiguousarray(descriptors, np.float32)
        if d.size % cells:
            raise ValueError("descriptors must be float32 of shape (n, num_rings, num_sectors)")
        dptr, nd = d.ctypes.data, d.size // cells
    dev_holders = [h for h in keep if _is_torch_cuda(h)]
    if dev_holders:
        _order_after_torch(registration, dev_holders[-1])
    if desc_dev:
        _order_after_torch(registration, d)
    cp = _capi.AppearanceLoopParams(
        _capi.LoopParams(lp.threshold_loop_closure_score, lp.distance_loop_closure, lp.range_of_searching_loop_closure,
                         lp.search_submap_num, lp.voxel_leaf_size, lp.top_k, 0),
        sc.struct(), float(params.sc_distance_threshold),
        _capi.PoseSearchParams(_capi.PoseLattice((C.c_int32 * 3)(*[int(v) for v in params.lattice_n]),
                                                 (C.c_double * 3)(*[float(v) for v in params.lattice_step]), int(params.n_yaw),
                                                 float(params.yaw_step)),
                               int(params.search_top_k), float(params.min_sep_m), float(params.min_sep_rad)))
    cap = max(1, lp.top_k)
    edges = (_capi.LoopEdge * cap)()
    shifts = (C.c_int32 * cap)()
    sc_dist = (C.c_float * cap)()
    n_eval = C.c_int32(0)
    _capi.check(lib.lsr_search_loop_appearance(registration._h, arr, n, stride, int(bool(on_device)), C.c_void_p(dptr), nd, int(desc_dev),
                                               C.byref(cp), edges, shifts, sc_dist, cap, C.byref(n_eval)), "searchLoopAppearance")
    if n_eval.value and hasattr(registration, "_n_target"):
        registration._n_target = int(edges[0].n_target_points)   # the object now holds the first candidate's window as its target
    out = []
    for k, e in enumerate(edges[:n_eval.value]):
        out.append(AppearanceLoopEdge(pair_id=(e.id_from, e.id_to),
                                      relative_pose=np.array(e.relative_pose[:], np.float64).reshape(4, 4, order="F"),
                                      fitness_score=e.fitness_score, accepted=bool(e.accepted),
                                      final_transformation=np.array(e.final_transformation[:], np.float32).reshape(4, 4, order="F"),
                                      converged=bool(e.converged), iterations=e.iterations, n_target_points=e.n_target_points,
                                      candidate_distance=e.candidate_distance, shift=int(shifts[k]), sc_distance=float(sc_dist[k])))
    return out
