"""Scan Context restated in numpy float32 (include/lidarslam_reg.h states the definitions): the tables, the descriptor, the distance over
all yaw shifts, the appearance guess — and the whole appearance loop gate on the CPU oracle's primitives.  Independent of
csrc/scan_context.hip and csrc/loop_search.hip.

Every float32 array operation below is one rounded operation per element, the definition's; sums that the definition orders are Python
loops over the ordered index with the other indices vectorised.  cos and sin are math.cos / math.sin (the C library's, what the C entry
calls), not np.cos / np.sin, whose vectorised routines may differ in the last bit."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_search_numpy as PS  # noqa: E402

F = np.float32
DEFAULT = dict(num_rings=20, num_sectors=60, max_radius=80.0, z_offset=2.0)
SHAPES = ((20, 60), (1, 2), (7, 10), (40, 120))


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def tables(num_rings, num_sectors, max_radius, z_offset=2.0):
    """-> (edge2 (R,) f32: the squared edges k = 1 .. R-1, then L2; b (S/2 - 1, 2) f32: cos, sin of 2 pi k / S)."""
    R, S, L = int(num_rings), int(num_sectors), float(max_radius)
    edge2 = np.zeros(R, F)
    for k in range(1, R):
        e = float(k) * L / float(R)
        edge2[k - 1] = F(e * e)
    edge2[R - 1] = F(L * L)
    b = np.zeros((S // 2 - 1, 2), F)
    for k in range(1, S // 2):
        a = 2.0 * 3.141592653589793 * float(k) / float(S)
        b[k - 1] = (F(math.cos(a)), F(math.sin(a)))
    return edge2, b


# ---- the descriptor ------------------------------------------------------------------------------------------------------------------
def cells_of(pts, num_rings, num_sectors, max_radius, z_offset=2.0):
    """Per point: (kept, ring, sector, value)."""
    R, S = int(num_rings), int(num_sectors)
    edge2, b = tables(R, S, max_radius)
    p = np.asarray(pts, F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        xx, yy = x * x, y * y
        r2 = xx + yy
        kept = finite & ~(r2 >= edge2[R - 1])
        ring = np.zeros(p.shape[0], np.int64)
        for k in range(R - 1):
            ring += (r2 >= edge2[k])
        upper = (y > 0) | ((y == 0) & (x >= 0))
        xp, yp = np.where(upper, x, -x), np.where(upper, y, -y)
        sector = np.where(upper, 0, S // 2).astype(np.int64)
        for k in range(S // 2 - 1):
            a, c = b[k, 0] * yp, b[k, 1] * xp
            sector += ((a - c) >= 0)
        t = z + F(z_offset)
        v = np.where(t > 0, t, F(0)).astype(F)
    return kept, ring, sector, v


def descriptor(pts, num_rings=20, num_sectors=60, max_radius=80.0, z_offset=2.0):
    """(R, S) f32 of one cloud ((n, >= 3) float32, pose-local)."""
    R, S = int(num_rings), int(num_sectors)
    out = np.zeros(R * S, F)
    a = np.asarray(pts, F)
    if a.shape[0] == 0:
        return out.reshape(R, S)
    kept, ring, sector, v = cells_of(a, R, S, max_radius, z_offset)
    np.maximum.at(out, (ring * S + sector)[kept], v[kept])
    return out.reshape(R, S)


# ---- the distance --------------------------------------------------------------------------------------------------------------------
def match(Q, C, num_rings=20, num_sectors=60):
    """Q (nq, R, S), C (nc, R, S) f32 -> (dist (nq, nc) f32, shift (nq, nc) i32)."""
    R, S = int(num_rings), int(num_sectors)
    Q = np.asarray(Q, F).reshape(-1, R, S)
    C = np.asarray(C, F).reshape(-1, R, S)
    nq, nc = Q.shape[0], C.shape[0]
    idx = (np.arange(S)[None, :] + np.arange(S)[:, None]) % S          # [n, j] = (j + n) mod S
    dist, shift = np.zeros((nq, nc), F), np.zeros((nq, nc), np.int32)
    with np.errstate(all="ignore"):
        nC = np.zeros((nc, S), F)
        for r in range(R):
            nC = nC + C[:, r, :] * C[:, r, :]
        nC = np.sqrt(nC)
        for iq in range(nq):
            q = Q[iq]
            nQ = np.zeros(S, F)
            for r in range(R):
                nQ = nQ + q[r] * q[r]
            nQ = np.sqrt(nQ)
            dot = np.zeros((nc, S, S), F)                               # [c, n, j]
            for r in range(R):
                dot = dot + q[r][None, None, :] * C[:, r, :][:, idx]
            ncs = nC[:, idx]                                            # [c, n, j] = nc_(j + n)
            counts = (nQ[None, None, :] > 0) & (ncs > 0)
            term = F(1.0) - dot / (nQ[None, None, :] * ncs)
            acc = np.zeros((nc, S), F)
            for j in range(S):
                acc = np.where(counts[:, :, j], acc + term[:, :, j], acc)
            cnt = counts.sum(axis=2)
            d = np.where(cnt > 0, acc / np.maximum(cnt, 1).astype(F), F(1.0)).astype(F)
            shift[iq] = np.argmin(d, axis=1)                            # the first minimum: ties to the lowest shift
            dist[iq] = d[np.arange(nc), shift[iq]]
    return dist, shift


def rank(dist_row, travel_ok, threshold):
    """Candidate indices, most alike first (ties: lower index)."""
    order = [i for i in range(len(dist_row)) if travel_ok[i] and float(dist_row[i]) < threshold]
    order.sort(key=lambda i: dist_row[i])
    return order


# ---- the guess -----------------------------------------------------------------------------------------------------------------------
def guess64(candidate, latest, shift, num_sectors):
    """M_cand Rz(shift 2 pi / S) M_latest^-1 in float64; candidate / latest: dicts with position and orientation (x y z w)."""
    from oracle import oracle

    Mc = oracle.pose_msg_to_matrix(candidate["position"], candidate["orientation"])
    Ml = oracle.pose_msg_to_matrix(latest["position"], latest["orientation"])
    a = float(shift) * (2.0 * 3.141592653589793) / float(num_sectors)
    Rz = np.eye(4)
    Rz[0, 0], Rz[0, 1], Rz[1, 0], Rz[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    Mi = np.eye(4)
    Mi[:3, :3] = Ml[:3, :3].T
    Mi[:3, 3] = -Ml[:3, :3].T @ Ml[:3, 3]
    return Mc @ Rz @ Mi


# ---- the drifted route ---------------------------------------------------------------------------------------------------------------
DRIFT_END = (25.0, -15.0, 0.3, 0.5)   # (dx, dy, dz, dyaw) at the last submap; zero up to the turn, linear in the travelled distance after it

_route = {}


def drifted_route():
    """synth.make_loop_route(drift=(0, 0, 0, 0)) — 21 submaps — re-posed: the stored poses are the truth up to the turn (submap 9) and
    then drift linearly with the travelled distance to DRIFT_END at the last submap.  The clouds are pose-local and stay as they are."""
    from lidarslam_ros2_amd import synth

    if "r" not in _route:
        base = synth.make_loop_route(drift=(0.0, 0.0, 0.0, 0.0))
        turn = len(base) // 2 - 1
        d0, d1 = base[turn]["distance"], base[-1]["distance"]
        out = []
        for sm in base:
            f = min(max((sm["distance"] - d0) / (d1 - d0), 0.0), 1.0)
            T = sm["truth"]
            yaw = math.atan2(T[1, 0], T[0, 0]) + DRIFT_END[3] * f
            out.append(dict(cloud=sm["cloud"], truth=T, distance=sm["distance"],
                            position=(float(T[0, 3]) + DRIFT_END[0] * f, float(T[1, 3]) + DRIFT_END[1] * f, DRIFT_END[2] * f),
                            orientation=(0.0, 0.0, math.sin(0.5 * yaw), math.cos(0.5 * yaw))))
        _route["r"] = out
        _route["d"] = np.stack([descriptor(sm["cloud"], **DEFAULT) for sm in out])
    return _route["r"]


def route_descriptors():
    drifted_route()
    return _route["d"]


# ---- the gate on the oracle ----------------------------------------------------------------------------------------------------------
def window_target(route, id_min, search_submap_num, voxel_leaf_size):
    from oracle import oracle

    parts = []
    for j in range(2 * search_submap_num + 1):
        idx = id_min + j - search_submap_num
        if idx < 0 or idx >= len(route):
            continue
        sm = route[idx]
        if len(sm["cloud"]):
            parts.append(oracle.transform_point_cloud(sm["cloud"], oracle.pose_msg_to_matrix(sm["position"], sm["orientation"]).astype(F)))
    window = np.concatenate(parts) if parts else np.zeros((0, 3), F)
    return oracle.voxel_grid_filter(window, voxel_leaf_size)


def appearance_gate(route, descriptors, *, threshold_loop_closure_score=1.0, distance_loop_closure=20.0, search_submap_num=3,
                    voxel_leaf_size=0.2, top_k=1, sc=DEFAULT, sc_distance_threshold=0.4, lattice_n=(7, 7, 1), lattice_step=(1.0, 1.0, 1.0),
                    n_yaw=1, yaw_step=0.0, search_top_k=16, min_sep_m=0.9, min_sep_rad=0.1308996938995747, ndt_resolution=5.0,
                    trans_eps=0.01, max_iterations=100, num_threads=0, starts=None):
    """lsr_search_loop_appearance restated on the oracle's primitives.  starts: {candidate rank: (4, 4) pose} replaces the lattice and
    its selection by that one start (a test hands the device's coarse winner in).  -> one dict per evaluated candidate."""
    from oracle import oracle

    n = len(route)
    latest = route[-1]
    init = oracle.pose_msg_to_matrix(latest["position"], latest["orientation"])
    source = oracle.transform_point_cloud(latest["cloud"], init.astype(F))
    dist, shift = match(descriptors[n - 1], descriptors, sc["num_rings"], sc["num_sectors"])
    dist, shift = dist[0], shift[0]
    travel_ok = [latest["distance"] - sm["distance"] > distance_loop_closure for sm in route]
    out = []
    for e, i in enumerate(rank(dist, travel_ok, sc_distance_threshold)[:max(1, top_k)]):
        G = guess64(route[i], latest, int(shift[i]), sc["num_sectors"]).astype(F)
        target = window_target(route, i, search_submap_num, voxel_leaf_size)
        grid = oracle.VoxelGridCovariance(target, ndt_resolution)
        if starts is not None and e in starts:
            kept_poses = [np.asarray(starts[e], F)]
        else:
            poses = PS.lattice(G, lattice_n, lattice_step, n_yaw, yaw_step)
            p0 = np.zeros(6)
            score = np.array([oracle.ndt_derivatives(grid, source, p0, T=T, compute_hessian=False, resolution=ndt_resolution,
                                                     num_threads=num_threads)[0] for T in poses])
            kept_poses = [poses[c] for c in PS.select(score, poses, search_top_k, min_sep_m, min_sep_rad)]
        refined = [oracle.ndt_align(grid, source, P, resolution=ndt_resolution, trans_eps=trans_eps, max_iterations=max_iterations,
                                    num_threads=num_threads) for P in kept_poses]
        w = -1
        for k, r in enumerate(refined):
            if w < 0 or r["trans_probability"] > refined[w]["trans_probability"]:
                w = k
        r = refined[w] if w >= 0 else dict(final=G, iterations=0, converged=False)
        fitness = oracle.NearestNeighbour(target).fitness_score(source, r["final"], num_threads=num_threads)
        frm = oracle.pose_msg_to_matrix(route[i]["position"], route[i]["orientation"])
        inv = np.eye(4)
        inv[:3, :3] = frm[:3, :3].T
        inv[:3, 3] = -frm[:3, :3].T @ frm[:3, 3]
        pos = np.asarray(latest["position"], np.float64) - np.asarray(route[i]["position"], np.float64)
        out.append(dict(pair_id=(i, n - 1), shift=int(shift[i]), sc_distance=float(dist[i]), guess=G, fitness_score=float(fitness),
                        accepted=bool(fitness < threshold_loop_closure_score), relative_pose=inv @ (r["final"].astype(np.float64) @ init),
                        final=r["final"], iterations=r["iterations"], converged=r["converged"], n_target_points=int(target.shape[0]),
                        candidate_distance=float(np.linalg.norm(pos)), start=kept_poses[w] if w >= 0 else None))
    return out
