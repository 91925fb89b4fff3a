"""The visibility votes restated in numpy float32 (include/lidarslam_reg.h states the definition): the pixel of a point, the depth image
of a keyframe, its erosion, the votes against every record and the static map's mask — steps 1 - 3, 5 and 6.  Independent of
csrc/map_visibility.hip.  Step 4 (neighbours and relative transforms, fp64 on the host) is taken from lsr_visibility_pairs, so equality
with the device does not hang on the bits of an fp64 inverse; pairs64 below is the fp64 evaluation that entry is held against.

Every float32 array operation below is one rounded operation per element, the definition's.  Also here: the scene of the behaviour test
(a car driving ahead of the vehicle through the synthetic world), built once and shared by the CPU and the GPU tests."""
import functools
import math

import numpy as np

F = np.float32
INF_BITS = 0x7F800000


def _xyz(cloud):
    """(n, >= 3) float records -> their x y z (the restatement takes the default field order)."""
    a = np.asarray(cloud, F)
    return a.reshape(a.shape[0], -1)[:, :3] if a.size else np.zeros((0, 3), F)


def params(**kw):
    from lidarslam_ros2_amd import VisibilityParams

    return VisibilityParams(**kw)


def consts(p):
    """The constants of step 0: made in double, each rounded to float once."""
    W, H, T = int(p.face_width), int(p.height), float(p.max_tan_elevation)
    return dict(W=W, H=H, hw=F(W // 2), Tf=F(T), rs=F(float(H) / (2.0 * T)), min_range=F(p.min_range), max_range=F(p.max_range),
                margin=F(p.margin), origin=np.array([F(v) for v in p.sensor_origin], F))


# ---- step 1 ----------------------------------------------------------------------------------------------------------------------------
def pixel(pts, p):
    """Sensor-centred points (n, 3) -> (has (n,) bool, row (n,) int, col (n,) int, r (n,) f32); row / col are 0 where there is no pixel."""
    c = consts(p)
    q = np.asarray(pts, F).reshape(-1, 3)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        ax, ay = np.abs(x), np.abs(y)
        d = np.where(ax > ay, ax, ay)
        ok &= ~(d == 0)
        xdom = ax >= ay
        u = np.where(xdom, y / x, (-x) / y).astype(F)
        face = np.where(xdom, np.where(x > 0, 0, 2), np.where(y > 0, 1, 3))
        xx, yy, zz = x * x, y * y, z * z
        s = xx + yy
        r = np.sqrt(s + zz).astype(F)
        ok &= ~((r < c["min_range"]) | (r >= c["max_range"]))
        v = z / d
        a = v + c["Tf"]
        rowf = np.floor(a * c["rs"])
        ok &= (rowf >= 0) & (rowf < F(c["H"]))
        e = (u + F(1.0)) * c["hw"]
        colf = np.floor(e)
    assert r.dtype == F and rowf.dtype == F and colf.dtype == F
    row = np.where(ok, rowf, 0).astype(np.int64)
    col = face * c["W"] + np.minimum(c["W"] - 1, np.where(ok, colf, 0).astype(np.int64))
    return ok, row, np.where(ok, col, 0), r


# ---- steps 2 and 3 ---------------------------------------------------------------------------------------------------------------------
def depth_image(pts, p):
    """The keyframe's own records (n, >= 3; pose-local) -> D (H, 4 W) f32, +inf where no record has a pixel."""
    c = consts(p)
    q = _xyz(pts)
    with np.errstate(all="ignore"):
        q = (q - c["origin"][None, :]).astype(F)
    ok, row, col, r = pixel(q, p)
    D = np.full(c["H"] * 4 * c["W"], np.inf, F)
    np.minimum.at(D, (row * 4 * c["W"] + col)[ok], r[ok])
    return D.reshape(c["H"], 4 * c["W"])


def erode(D):
    """E[row][col] = min of D over rows row-1 .. row+1 clamped and columns col-1 .. col+1 modulo the width."""
    rows = np.minimum(np.minimum(np.concatenate([D[:1], D[:-1]]), D), np.concatenate([D[1:], D[-1:]]))
    return np.minimum(np.minimum(np.roll(rows, 1, axis=1), rows), np.roll(rows, -1, axis=1))


def images(clouds, p, eroded=True):
    out = [depth_image(cl, p) for cl in clouds]
    return np.stack([erode(D) for D in out] if eroded else out)


# ---- step 5 ----------------------------------------------------------------------------------------------------------------------------
def votes(clouds, first_pair, other, rel12, E, p):
    """The votes against every record, in assembly order.  clouds[i]: (n_i, >= 3) f32 pose-local; first_pair / other / rel12: the table
    of lsr_visibility_pairs; E: (n, H, 4 W) eroded images."""
    c = consts(p)
    out = []
    for i, cl in enumerate(clouds):
        q = _xyz(cl)
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        v = np.zeros(q.shape[0], np.int32)
        for pr in range(int(first_pair[i]), int(first_pair[i + 1])):
            m = np.asarray(rel12[pr], F).reshape(3, 4)
            with np.errstate(all="ignore"):
                t = np.stack([((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)], axis=1)
                t = (t - c["origin"][None, :]).astype(F)
            assert t.dtype == F
            ok, row, col, r = pixel(t, p)
            e = E[int(other[pr])][row, col]
            with np.errstate(all="ignore"):
                v += (ok & np.isfinite(e) & ((r + c["margin"]) < e)).astype(np.int32)
        out.append(v)
    return np.concatenate(out) if out else np.zeros(0, np.int32)


def static_votes(clouds, submaps, p, poses=None):
    """Steps 1 - 5 on the restatement with the pair table of the host entry -> (votes, E)."""
    from lidarslam_ros2_amd import visibilityPairs

    first, other, rel = visibilityPairs(submaps, poses, p)
    E = images(clouds, p)
    return votes(clouds, first, other, rel, E, p), E


# ---- step 4 in fp64: what lsr_visibility_pairs is held against -------------------------------------------------------------------------
def pairs64(M, p):
    """M: (n, 4, 4) fp64 poses -> (first_pair, other, rel (m, 3, 4) fp64)."""
    n = len(M)
    first, other, rel = [0], [], []
    for i in range(n):
        near = []
        for k in range(n):
            if k == i:
                continue
            dx, dy, dz = (M[k][:3, 3] - M[i][:3, 3])
            dist = math.sqrt((dx * dx + dy * dy) + dz * dz)
            if dist <= float(p.keyframe_range):
                near.append((dist, k))
        near.sort()
        for _, k in sorted(near[: int(p.max_neighbours)], key=lambda e: e[1]):
            Rk, tk = M[k][:3, :3], M[k][:3, 3]
            inv = np.eye(4)
            inv[:3, :3] = Rk.T
            inv[:3, 3] = -(Rk.T @ tk)
            other.append(k)
            rel.append((inv @ M[i])[:3])
        first.append(len(other))
    return np.array(first, np.int32), np.array(other, np.int32), np.array(rel, np.float64).reshape(-1, 3, 4)


# ---- the scene of the behaviour test ---------------------------------------------------------------------------------------------------
CAR = (4.0, 1.8, 1.5)   # length, width, height [m]


@functools.lru_cache(maxsize=None)
def car_scene(with_car=True):
    """synth.make_world(), vlp32(), default_rng(1), 8 keyframes at trajectory_pose(3 i); scan i is raycast in the world plus one box of
    4 x 1.8 x 1.5 m on the ground centred at (12 + 5 i, 1.0) — a car driving ahead —, then voxel_downsample(0.2).
    -> dict(ma: MapArray (host records), clouds: the (n_i, 8) f32 records, is_car: (total,) bool in assembly order — the records
    whose map position lies within 0.2 m of that scan's box and above ground + 0.15 m)."""
    from lidarslam_ros2_amd import MapArray, synth

    world, sensor, rng = synth.make_world(), synth.vlp32(), np.random.default_rng(1)
    ma, clouds, is_car = MapArray(), [], []
    gz = world.ground_z
    for i in range(8):
        T = synth.trajectory_pose(3.0 * i)
        cx, cy = 12.0 + 5.0 * i, 1.0
        box = np.array([cx - CAR[0] / 2, cy - CAR[1] / 2, gz, cx + CAR[0] / 2, cy + CAR[1] / 2, gz + CAR[2]])
        w = synth.World(np.concatenate([world.boxes, box[None, :]]), world.cyls, gz) if with_car else world
        pts = synth.voxel_downsample(synth.raycast(w, sensor, T, rng), 0.2)
        rec = synth.as_pointxyzi(pts)
        rec[:, 4] = np.arange(len(rec), dtype=F) % F(97.0)   # an intensity that tells records apart
        m = pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        is_car.append(np.all((m >= box[:3] - 0.2) & (m <= box[3:] + 0.2), axis=1) & (m[:, 2] > gz + 0.15))
        clouds.append(rec)
        ma.append(rec, T, 3.0 * i)
    return dict(ma=ma, clouds=clouds, is_car=np.concatenate(is_car))


def behaviour(votes_with, votes_without, min_votes=2):
    """The three figures of the behaviour test from the votes of the two scenes -> dict."""
    car = car_scene(True)["is_car"]
    removed = votes_with >= min_votes
    removed0 = votes_without >= min_votes
    return dict(n_static=int((~car).sum()), static_removed=int((removed & ~car).sum()), n_car=int(car.sum()),
                car_removed=int((removed & car).sum()), n_empty_scene=int(removed0.size), empty_scene_removed=int(removed0.sum()))


def assert_behaviour(b):
    print("behaviour", b)
    assert b["n_car"] > 100 and b["n_static"] > 100000
    assert b["static_removed"] <= 0.001 * b["n_static"], b            # at most 0.1 % of what stands still
    assert b["car_removed"] >= 0.6 * b["n_car"], b                    # at least 60 % of the car
    assert b["empty_scene_removed"] <= 0.001 * b["n_empty_scene"], b  # no car anywhere: at most 0.1 %
