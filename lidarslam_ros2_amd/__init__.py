"""MI355X-native scan-matching registration core for lidarslam_ros2's hot path.

Only the `pcl::Registration` path (NDT / GICP setInputTarget, setInputSource, align,
getFitnessScore) is implemented here — hand-written HIP kernels for gfx950 behind the C ABI in
include/lidarslam_reg.h.  See DESIGN.md.
"""
from .registration import (DIRECT1, DIRECT7, DIRECT26, KDTREE, GeneralizedIterativeClosestPoint, MapWindow,
                           NormalDistributionsTransform, Registration, ScanContextParams, align_batch, mapWindowAround, odomGuess, poseLattice,
                           scanContextGuess, scanContextTables, selectPoses, sensorTransformMatrix, VisibilityParams, visibilityPairs)
from .loop_closure import (AppearanceLoopEdge, AppearanceLoopParams, LoopClosureParams, LoopEdge, SubMap, search_loop,
                           search_loop_appearance)
from .map_array import MapArray
from .localization import Localizer, LocalizerParams
from . import pose_graph

__all__ = ["Registration", "NormalDistributionsTransform", "GeneralizedIterativeClosestPoint", "align_batch",
           "odomGuess", "sensorTransformMatrix", "SubMap", "LoopClosureParams", "LoopEdge", "search_loop", "MapArray", "pose_graph",
           "MapWindow", "mapWindowAround", "Localizer", "LocalizerParams", "poseLattice", "selectPoses",
           "ScanContextParams", "scanContextTables", "scanContextGuess", "AppearanceLoopParams", "AppearanceLoopEdge",
           "search_loop_appearance", "VisibilityParams", "visibilityPairs", "DIRECT1", "DIRECT7", "DIRECT26", "KDTREE"]
