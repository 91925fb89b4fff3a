"""The host side of the NDT pose search restated in Python (lsr_pose_lattice_poses, lsr_select_poses; include/lidarslam_reg.h states the
definitions), the search procedure on the CPU oracle, and the inputs the search tests share.  Independent of csrc/pose_search.hip.

cos and sin are math.cos / math.sin per angle — the C library's, what the C entry calls — and not np.cos / np.sin: numpy's vectorised
routines may differ from libm in the last bit."""
import math

import numpy as np

MAX_POSES = 1 << 20
MAX_KEPT = 16


# ---- the lattice ---------------------------------------------------------------------------------------------------------------------
def lattice(center, n, step, n_yaw, yaw_step):
    """(count, 4, 4) fp32: candidate ((m n[2] + k) n[1] + j) n[0] + i = Rz(psi_m) R_center | t_center + offsets, in double from the
    float centre, every entry rounded to float once."""
    C = np.asarray(center, np.float32).reshape(4, 4).astype(np.float64)
    count = int(n[0]) * int(n[1]) * int(n[2]) * int(n_yaw)
    out = np.zeros((count, 4, 4), np.float32)
    c = 0
    for m in range(n_yaw):
        psi = (m - (n_yaw - 1) / 2.0) * float(yaw_step)
        cs, sn = math.cos(psi), math.sin(psi)
        R = np.zeros((3, 3))
        for col in range(3):
            R[0, col] = cs * C[0, col] - sn * C[1, col]
            R[1, col] = sn * C[0, col] + cs * C[1, col]
            R[2, col] = C[2, col]
        for k in range(n[2]):
            tz = C[2, 3] + (k - (n[2] - 1) / 2.0) * float(step[2])
            for j in range(n[1]):
                ty = C[1, 3] + (j - (n[1] - 1) / 2.0) * float(step[1])
                for i in range(n[0]):
                    tx = C[0, 3] + (i - (n[0] - 1) / 2.0) * float(step[0])
                    out[c, :3, :3] = R.astype(np.float32)
                    out[c, :3, 3] = np.array([tx, ty, tz]).astype(np.float32)
                    out[c, 3, 3] = 1.0
                    c += 1
    return out


# ---- the selection -------------------------------------------------------------------------------------------------------------------
def _close(A, B, min_sep_m, cos_sep):
    dx, dy, dz = (float(A[r, 3]) - float(B[r, 3]) for r in range(3))
    dist = math.sqrt(dx * dx + dy * dy + dz * dz)
    tr = 0.0
    for col in range(3):          # the nine products in storage (column-major) order
        for r in range(3):
            tr += float(A[r, col]) * float(B[r, col])
    return dist < min_sep_m and (tr - 1.0) / 2.0 > cos_sep


def select(score, poses, top_k, min_sep_m, min_sep_rad):
    """Indices of the distinct best, best first: descending score (ties: ascending index; NaN or not > 0 never kept), greedy, a
    candidate close to a kept one is skipped."""
    score = np.asarray(score, np.float64)
    poses = np.asarray(poses, np.float32)
    order = [c for c in range(score.shape[0]) if score[c] > 0]
    order.sort(key=lambda c: -score[c])         # stable: ties keep ascending index
    cos_sep = math.cos(min_sep_rad)
    kept = []
    for c in order:
        if any(_close(poses[c], poses[e], min_sep_m, cos_sep) for e in kept):
            continue
        kept.append(c)
        if len(kept) == top_k:
            break
    return np.array(kept, np.int32)


# ---- pair counts of a pass from the oracle's grid ------------------------------------------------------------------------------------
_OFF7 = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def pair_counts(grid, src, poses):
    """Valid (point, voxel) pairs of a DIRECT7 pass per pose, from the CPU oracle's grid (oracle.VoxelGridCovariance): the point moved in
    the reference's fp32 order ((m00 x + m01 y) + m02 z) + m03, its cell floor(x' / leaf), the seven cells, a pair for every usable
    leaf (six points or more, covariance not invalidated).  Exact wherever gauss_d2 < 1 — every pair then passes the reference's
    0 <= d2 exp(..) <= 1 test (resolution 2.0, outlier ratio 0.55: d2 = 0.248)."""
    d = grid.dump()
    div = (grid.max_b - grid.min_b + 1).astype(np.int64)
    usable = np.zeros(int(div[0] * div[1] * div[2]), bool)
    usable[d["idx"][d["n"] >= 6]] = True
    s = np.asarray(src, np.float32)[:, :3]
    leaf = np.float32(grid.leaf)
    out = np.zeros(len(poses), np.float64)
    for c, T in enumerate(np.asarray(poses, np.float32)):
        t = [((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)]
        cell = [np.floor(v / leaf).astype(np.int64) for v in t]
        total = 0
        for off in _OFF7:
            a = [cell[k] + off[k] - int(grid.min_b[k]) for k in range(3)]
            inside = np.ones(s.shape[0], bool)
            for k in range(3):
                inside &= (a[k] >= 0) & (a[k] < div[k])
            lin = np.where(inside, a[0] + a[1] * div[0] + a[2] * div[0] * div[1], 0)
            total += int(np.count_nonzero(inside & usable[lin]))
        out[c] = total
    return out


# ---- the inputs of the search tests --------------------------------------------------------------------------------------------------
RES, EPS = 2.0, 0.01
SEEDS = (0, 2)
DISPLACEMENTS = ((2.3, -1.6, 17.0), (-3.2, 2.7, -22.0), (0.4, 3.6, 8.0))      # (dx [m], dy [m], dyaw [deg]) of the centre off the truth
LATTICE = dict(n=(9, 9, 1), step=(1.0, 1.0, 1.0), n_yaw=13, yaw_step=math.radians(5.0))
TOP_K, SEP_M, SEP_RAD = 16, 0.9, math.radians(7.5)
INPUTS = [(seed, d) for seed in SEEDS for d in range(len(DISPLACEMENTS))]

_cases = {}


def case(seed):
    from lidarslam_ros2_amd import synth

    if seed not in _cases:
        _cases[seed] = synth.small_case(n_source=2000, n_keyframes=3, seed=seed)
    return _cases[seed]


def yaw_of(T):
    return math.atan2(float(T[1, 0]), float(T[0, 0]))


def displaced_center(truth, d):
    """The truth displaced by DISPLACEMENTS[d] in x, y and yaw; z, roll and pitch zero."""
    from lidarslam_ros2_amd import synth

    dx, dy, dyaw = DISPLACEMENTS[d]
    T = np.asarray(truth, np.float64)
    return synth.pose_matrix(T[0, 3] + dx, T[1, 3] + dy, 0.0, yaw_of(T) + math.radians(dyaw)).astype(np.float32)


def oracle_search(O, grid, src, center, score=None):
    """The procedure on the CPU oracle: scores over LATTICE (or the given ones), the restated selection, O.ndt_align from each kept
    candidate, the winner by trans_probability (ties: lower rank).  -> dict(poses, score, kept, refined, winner)."""
    poses = lattice(center, **LATTICE)
    if score is None:
        p0 = np.zeros(6)
        score = np.array([O.ndt_derivatives(grid, src, p0, T=T, compute_hessian=False, resolution=RES)[0] for T in poses])
    kept = select(score, poses, TOP_K, SEP_M, SEP_RAD)
    refined = [O.ndt_align(grid, src, poses[c], resolution=RES, trans_eps=EPS) for c in kept]
    winner = -1
    for e, r in enumerate(refined):
        if winner < 0 or r["trans_probability"] > refined[winner]["trans_probability"]:
            winner = e
    return dict(poses=poses, score=np.asarray(score), kept=kept, refined=refined, winner=winner)
