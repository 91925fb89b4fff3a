"""TEST INFRASTRUCTURE: numpy restatement of lsr_assemble_map (publishMap, scanmatcher_component.cpp:529-552; the map half of
doPoseAdjustment, graph_based_slam_component.cpp:321-368).  The pose matrix is built in float64 in the expression order of the
library's submap_pose_matrix and cast to float32 element by element; the points are moved with float32 array operations in the order
((m00*x + m01*y) + m02*z) + m03 — numpy rounds every operation and never fuses; the records are written with zero fill.  Every
comparison against it is np.array_equal on the raw bytes."""
import numpy as np

XYZI = (32, (0, 4, 8, 16))


def pose_matrix(position, orientation) -> np.ndarray:
    """tf2::fromMsg(Pose) -> Affine3d.matrix(): float64 4x4, Eigen's toRotationMatrix order, no normalisation."""
    x, y, z, w = (np.float64(v) for v in orientation)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    M = np.zeros((4, 4), np.float64)
    M[0, 0] = 1 - (tyy + tzz); M[0, 1] = txy - twz; M[0, 2] = txz + twy
    M[1, 0] = txy + twz; M[1, 1] = 1 - (txx + tzz); M[1, 2] = tyz - twx
    M[2, 0] = txz - twy; M[2, 1] = tyz + twx; M[2, 2] = 1 - (txx + tyy)
    M[:3, 3] = [np.float64(v) for v in position]
    M[3, 3] = 1.0
    return M


def _field(buf: np.ndarray, step: int, off: int, n: int, dtype):
    """Field at byte offset `off` of n records of `step` bytes starting at buf[0] (buf: 1-D uint8, any alignment)."""
    idx = (np.arange(n, dtype=np.int64) * step + off)[:, None] + np.arange(4)[None, :]
    return buf[idx].copy().view(dtype).reshape(n)


def move_records(raw, n: int, M, in_layout=XYZI, out_layout=XYZI) -> np.ndarray:
    """n records of in_layout in `raw` (any array; its bytes) moved by the 4x4 `M` (cast to float32) -> (n, out_step) uint8."""
    in_step, (ix, iy, iz, ii) = in_layout
    out_step, (ox, oy, oz, oi) = out_layout
    buf = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    m = np.asarray(M, np.float64).astype(np.float32)
    x, y, z = (_field(buf, in_step, o, n, np.float32) for o in (ix, iy, iz))
    inten = _field(buf, in_step, ii, n, np.uint32) if ii is not None and ii >= 0 else np.zeros(n, np.uint32)
    out = np.zeros((n, out_step), np.uint8)
    with np.errstate(all="ignore"):
        for r, o in enumerate((ox, oy, oz)):
            q = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
            assert q.dtype == np.float32
            out[:, o:o + 4] = q.view(np.uint8).reshape(n, 4)
    if oi is not None and oi >= 0:
        out[:, oi:oi + 4] = inten.view(np.uint8).reshape(n, 4)
    return out


def count_records(cloud, step: int) -> int:
    return int(np.asarray(cloud).nbytes // step)


def assemble_map(submaps, poses=None, in_layout=XYZI, out_layout=XYZI):
    """-> (records (total, out_step) uint8, first_record (n + 1,) int64).  submaps: objects with cloud / position / orientation."""
    parts, first = [], [0]
    for i, sm in enumerate(submaps):
        n = count_records(sm.cloud, in_layout[0])
        M = pose_matrix(sm.position, sm.orientation) if poses is None else np.asarray(poses[i], np.float64)
        parts.append(move_records(sm.cloud, n, M, in_layout, out_layout))
        first.append(first[-1] + n)
    return np.concatenate(parts) if parts else np.zeros((0, out_layout[0]), np.uint8), np.array(first, np.int64)


class FakeRegistration:
    """A registration object for the host-side bookkeeping tests: assembleMap is this module; every call is recorded."""

    def __init__(self):
        self.calls = []

    def assembleMap(self, submaps, poses=None, in_layout=XYZI, out_layout=XYZI, out=None):
        self.calls.append(("assembleMap", len(submaps)))
        rec, first = assemble_map(submaps, poses, in_layout, out_layout)
        if out is not None:
            flat = out.reshape(-1)
            flat[: rec.size] = rec.reshape(-1)
            rec = flat[: rec.size].reshape(rec.shape)
        return rec, first
