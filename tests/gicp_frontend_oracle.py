"""TEST INFRASTRUCTURE: the CPU oracle behind the method names lidarslam_ros2_amd.frontend.FrontendReplay calls in GICP mode
(scanmatcher_component.cpp:115-120 sets the object up, :308-316 filters the assembled window before setInputTarget, :329,353
register against the filtered cloud), so that the same loop runs once on the gfx950 core and once on the oracle.  The two
PointCloud2 methods (the scan's range filter + VoxelGrid, the keyframe's VoxelGrid) are frontend_oracle's, unchanged."""
import numpy as np

from frontend_oracle import OracleFrontendRegistration
from oracle import oracle as O


class OracleGicpFrontendRegistration(OracleFrontendRegistration):
    """solver: 1 = Gauss-Newton (the optimiser the gfx950 core runs), 0 = BFGS (the reference's schedule)."""

    def __init__(self, solver=1, max_corr_dist=5.0, trans_eps=1e-8, num_threads=0):
        super().__init__()
        self.solver, self.corr, self.eps, self.nt = int(solver), float(max_corr_dist), float(trans_eps), int(num_threads)
        self.target = None
        self.nn_target = None
        self.cov_target = None
        self.target_sizes = []          # points of every target this object was given, in order
        self.n_correspondences = 0

    def _threads(self):
        return self.nt or min(32, O.max_threads())

    def setInputTargetFrames(self, frames, poses):
        raise AssertionError("the GICP frontend filters the assembled window: setInputTargetFramesFiltered")

    def setInputTargetFramesFiltered(self, frames, poses, leaf):
        chunks = []
        for fr, P in zip(frames, poses):
            rec = np.asarray(fr, np.float32).reshape(-1, 8)     # (m,8) fp32 pcl::PointXYZI records
            chunks.append(O.transform_point_cloud(rec[:, :3], np.asarray(P, np.float32)))   # pcl::transformPointCloud, fp32
        self.target = O.voxel_grid_filter(np.concatenate(chunks), leaf)                     # :309-314
        self.nn_target = O.NearestNeighbour(self.target, 1.0)
        self.cov_target = O.gicp_covariances(self.nn_target, self.target, num_threads=self._threads())
        self.target_sizes.append(int(self.target.shape[0]))
        return int(self.target.shape[0])

    def prepareTarget(self):
        pass   # the covariances above are what it stands for

    def align(self, guess):
        cov_source = O.gicp_covariances(O.NearestNeighbour(self.source, 1.0), self.source, num_threads=self._threads())
        r = O.gicp_align(self.nn_target, self.target, self.cov_target, self.source, cov_source, np.asarray(guess, np.float32),
                         max_corr_dist=self.corr, trans_eps=self.eps, solver=self.solver, num_threads=self._threads())
        self.final = np.asarray(r["final"], np.float64)
        self.iterations = int(r["iterations"])
        self.n_correspondences = int(r["n_correspondences"])
