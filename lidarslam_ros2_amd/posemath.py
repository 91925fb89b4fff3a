"""Small SE(3) helpers shared by tests, smoke and bench (host side, numpy)."""
import numpy as np


def pose_delta(A, B):
    """(translation distance [m], rotation angle [rad]) between two 4x4 poses.

    The angle comes from the skew part of dR (sin theta), not arccos(trace): arccos near 1 turns the
    6e-8 rounding of fp32 matrix entries into ~3e-4 rad of fake rotation."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    dt = float(np.linalg.norm(A[:3, 3] - B[:3, 3]))
    dR = A[:3, :3] @ B[:3, :3].T
    v = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    s = float(np.linalg.norm(v))
    c = (np.trace(dR) - 1.0) / 2.0
    return dt, float(np.arctan2(s, c))


def quaternion_from_matrix(R) -> np.ndarray:
    """Eigen's Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<.., 3, 3>), operation for operation in
    float64: the trace branch when the trace is positive, otherwise the branch of the largest diagonal element.  -> (x, y, z, w), the
    order of geometry_msgs/Quaternion.  This is how the frontend turns a registered pose into the pose of a SubMap message
    (scanmatcher_component.cpp:394-398); no normalisation, as there."""
    m = np.asarray(R, np.float64)[:3, :3]
    q = np.zeros(4, np.float64)   # x y z w
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def matrix_from_pose(position, orientation) -> np.ndarray:
    """tf2::fromMsg(geometry_msgs/Pose) -> Eigen::Affine3d = Translation * Quaterniond (Eigen's toRotationMatrix, no normalisation):
    the 4x4 float64 matrix a stored SubMap pose stands for, in the expression order of the library's submap_pose_matrix."""
    x, y, z, w = (float(v) for v in orientation)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    M = np.eye(4)
    M[0, :3] = [1 - (tyy + tzz), txy - twz, txz + twy]
    M[1, :3] = [txy + twz, 1 - (txx + tzz), tyz - twx]
    M[2, :3] = [txz - twy, tyz + twx, 1 - (txx + tyy)]
    M[:3, 3] = [float(v) for v in position]
    return M
