"""Plain numpy references and inputs for the nearest-neighbour tests: brute force with the device's fp32 arithmetic, the two-level
grid of nn.hip built with numpy, the adversarial clouds, and the query sets that take the search forms of nn_search_device /
nn_fitness_begin_group by SHAPE (tests/test_nn_numpy_cpu.py asserts, with brute force, every property the GPU tests rely on)."""
import functools

import numpy as np

F = np.float32
DBL_MAX = 1.7976931348623157e308
NN_MAX_FINE_RINGS = 4                 # nn_device.hpp
NN_BUCKET_MAX_KEYS = 16 << 20         # nn_device.hpp: larger (coarse, fine) key spaces are built by sorting
NN_WAVE_MAX_QUERIES = 262144          # nn_search_device: larger query sets take the capped per-thread walk + the work list
FIT_BALL_CELLS = 5                    # nn.hip


# ---- brute force ---------------------------------------------------------------------------------------------------------------
def brute_nn1(pts, q):
    """(distance, index) minimum with the device's fp32 arithmetic: ((dx*dx + dy*dy) + dz*dz), no contraction."""
    d = (pts - q[None, :]).astype(np.float32)
    d2 = ((d[:, 0] * d[:, 0]).astype(np.float32) + (d[:, 1] * d[:, 1]).astype(np.float32)).astype(np.float32)
    d2 = (d2 + (d[:, 2] * d[:, 2]).astype(np.float32)).astype(np.float32)
    j = int(np.lexsort((np.arange(len(pts)), d2))[0])
    return j, d2[j]


def transform_rn(q, T):
    """fp32 point transform in the reference's order: ((m0*x + m1*y) + m2*z) + m3, every operation rounded on its own."""
    q = np.ascontiguousarray(q, F).reshape(-1, 3)
    if T is None:
        return q
    M = np.asarray(T, F)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    out = np.empty_like(q)
    with np.errstate(all="ignore"):
        for k in range(3):
            out[:, k] = ((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z) + M[k, 3]
    return out


def brute_nn(target, queries, T=None, chunk=4096):
    """Exact 1-NN of every (transformed) query among the finite target points: (index int32, d2 fp32), minimum by (d2, index).
    d2 = (dx*dx + dy*dy) + dz*dz in fp32.  A query that is non-finite after the transform has no neighbour: (-1, inf); so has one
    whose every d2 overflows to inf — inf is the 'no neighbour' distance, a candidate has to be strictly closer to be taken."""
    target = np.asarray(target, F).reshape(-1, 3)
    q = transform_rn(queries, T)
    n = len(q)
    idx = np.full(n, -1, np.int32)
    d2 = np.full(n, np.inf, F)
    keep = np.nonzero(np.isfinite(target).all(1))[0].astype(np.int32)
    if n == 0 or len(keep) == 0:
        return idx, d2
    tx, ty, tz = [np.ascontiguousarray(target[keep, k]) for k in range(3)]
    ok = np.isfinite(q).all(1)
    with np.errstate(all="ignore"):
        for s in range(0, n, chunk):
            rows = np.nonzero(ok[s:s + chunk])[0] + s
            if len(rows) == 0:
                continue
            c = q[rows]
            dx = tx[None, :] - c[:, 0:1]
            acc = dx * dx
            dx = ty[None, :] - c[:, 1:2]
            acc = acc + dx * dx
            dx = tz[None, :] - c[:, 2:3]
            acc = acc + dx * dx                       # fp32 throughout
            j = np.argmin(acc, axis=1)                # the lowest position on ties; `keep` is ascending, so the lowest index
            dj = acc[np.arange(len(rows)), j]
            found = dj < np.inf
            idx[rows[found]] = keep[j[found]]
            d2[rows[found]] = dj[found]
    return idx, d2


def brute_fitness(target, source, T, max_range=np.inf, nn=None):
    """pcl::Registration::getFitnessScore: fp64 mean of the fp32 d2 with d2 <= max_range; DBL_MAX without such a pair.
    nn: brute_nn(target, source, T) when the caller has it already."""
    idx, d2 = nn if nn is not None else brute_nn(target, source, T)
    d = d2.astype(np.float64)
    sel = (idx >= 0) & (d <= max_range)
    cnt = int(sel.sum())
    return float(d[sel].sum() / cnt) if cnt else DBL_MAX


def fitness_rel_tol(n):
    """Bound for an fp64 sum of n non-negative terms taken in another order (relative)."""
    return 2.0 * max(n, 1) * 2.0 ** -53


# ---- the two-level grid of nn.hip, built with numpy -------------------------------------------------------------------------------
def grid_dims(pts, cell):
    """(org, cdim) of nn_build_hash: fine-cell origin aligned down to a multiple of 8, coarse cells per axis."""
    pts = np.asarray(pts, F)
    pts = pts[np.isfinite(pts).all(1)]
    inv = np.float32(1.0) / np.float32(cell)
    f0 = np.floor(pts.min(0) * inv).astype(np.int64)
    f1 = np.floor(pts.max(0) * inv).astype(np.int64)
    org = np.where(f0 >= 0, f0 & ~7, -(((-f0) + 7) & ~7))
    cdim = ((f1 - org) >> 3) + 1
    return org, cdim


def build_grid(pts, cell):
    """The two-level grid of nn.hip, built with numpy (points ordered by (coarse cell, fine cell), stable)."""
    inv = np.float32(1.0) / np.float32(cell)
    f = np.floor(pts * inv).astype(np.int64)
    org, cdim = grid_dims(pts, cell)
    rel = f - org
    cc = rel >> 3
    clin = cc[:, 0] + cdim[0] * (cc[:, 1] + cdim[1] * cc[:, 2])
    fine = (rel[:, 0] & 7) | ((rel[:, 1] & 7) << 3) | ((rel[:, 2] & 7) << 6)
    order = np.argsort(clin * 512 + fine, kind="stable").astype(np.int32)
    ublk = np.unique(clin)
    coarse_block = -np.ones(int(np.prod(cdim)), np.int32)
    coarse_block[ublk] = np.arange(len(ublk), dtype=np.int32)
    blk_of = coarse_block[clin[order]]
    fkey = blk_of.astype(np.int64) * 513 + fine[order]
    fine_start = np.searchsorted(fkey, np.arange(len(ublk) * 513), side="left").astype(np.int32)
    block_off = np.searchsorted(blk_of, np.arange(len(ublk) + 1), side="left").astype(np.int32)
    s = pts[order]
    return dict(cell=np.float32(cell), org=org.astype(np.int32), cdim=cdim.astype(np.int32), coarse_block=coarse_block, block_off=block_off,
                fine_start=fine_start, sx=np.ascontiguousarray(s[:, 0]), sy=np.ascontiguousarray(s[:, 1]), sz=np.ascontiguousarray(s[:, 2]),
                order=order, rel=rel, pts=pts)


def fine_cell(q, cell, org):
    """Fine-cell coordinates of (already transformed) queries relative to the grid origin, as the device computes them."""
    inv = np.float32(1.0) / np.float32(cell)
    with np.errstate(all="ignore"):
        return np.floor(np.asarray(q, F) * inv).astype(np.int64) - np.asarray(org, np.int64)[None, :]


def cells_outside(q, cell, org, cdim):
    """Per query: by how many fine cells it lies outside the grid box on its worst axis (0 = inside)."""
    fq = fine_cell(q, cell, org)
    fdim = np.asarray(cdim, np.int64) * 8
    return np.maximum(np.maximum(-fq, fq - (fdim - 1)[None, :]), 0).max(1)


# ---- clouds ----------------------------------------------------------------------------------------------------------------------
def _frozen(a):
    a = np.ascontiguousarray(a, F)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _clouds():
    from lidarslam_ros2_amd import synth

    rng = np.random.default_rng(3)
    case = synth.small_case(n_source=1500, n_keyframes=2)
    dup = rng.uniform(-4, 4, (300, 3)).astype(np.float32)
    dup = np.vstack([dup, dup[:150]])            # exact duplicates: ties broken by the lowest index
    lattice = (np.stack(np.meshgrid(*[np.arange(-6, 6)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.5).astype(np.float32)   # points ON cell faces
    out = [("uniform", rng.uniform(-12, 12, (4000, 3)).astype(np.float32)), ("scan", case.target[:6000].astype(np.float32)), ("duplicates", dup),
           ("lattice", lattice)]
    rng = np.random.default_rng(31)
    one = np.float32([[1.3, -2.1, 0.4]])
    cube = (np.float32([1.0, 1.0, 1.0]) + rng.uniform(0.0, 0.05, (200, 3))).astype(np.float32)   # inside ONE fine cell at every cell size used
    pile = np.vstack([cube, cube[:100], rng.uniform(-4, 4, (200, 3)).astype(np.float32)])          # several waves' worth of candidates in it
    out += [("single", one), ("pair", np.vstack([one, one])), ("pile", pile)]
    return tuple((name, _frozen(p)) for name, p in out)


def clouds():
    """uniform, scan, exact duplicates, a lattice with points ON cell faces, one point, two identical points, and a pile: 300 points
    (100 of them exact duplicates) in one 0.05 m cube among 200 uniform ones.  Read-only arrays, the same objects on every call."""
    return list(_clouds())


def cloud(name):
    return dict(_clouds())[name]


def yaw_pose(deg=30.0, t=(0.3, -0.2, 0.1)):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    T[:3, 3] = t
    return T.astype(F)


def preimage(T, q):
    """Points p with T p ~= q (fp64 inverse, rounded to fp32): a source that the pose T puts where the test wants its queries."""
    if T is None:
        return np.ascontiguousarray(q, F)
    M = np.asarray(T, np.float64)
    R, t = M[:3, :3], M[:3, 3]
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(((np.asarray(q, np.float64) - t[None, :]) @ R).astype(F))   # R^T (q - t), rows


NONFINITE3 = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1e30, 1e30, 1e30]], F)


def face_points(pts, cell, cells=(1, 6)):
    """Per face of the bounding box of `pts`, a point exactly `c` fine cells outside it (the box's centre on the other axes)."""
    pts = np.asarray(pts, F)
    lo, hi = pts.min(0), pts.max(0)
    mid = ((lo + hi) * F(0.5)).astype(F)
    out = []
    for c in cells:
        for a in range(3):
            for side in (0, 1):
                p = mid.copy()
                p[a] = lo[a] - F(c) * F(cell) if side == 0 else hi[a] + F(c) * F(cell)
                out.append(p)
    return np.array(out, F)


def grid_face_points(pts, cell, cells=(1, 6)):
    """The same relative to the GRID box (aligned to 8 fine cells, so up to 7 cells wider than the bounding box): centres of the
    fine cells fq = -c and fq = cdim * 8 + c - 1 on one axis."""
    org, cdim = grid_dims(pts, cell)
    lo, hi = org.astype(np.float64), (org + 8 * cdim).astype(np.float64)
    pts = np.asarray(pts, F)
    mid = ((pts.min(0) + pts.max(0)) * F(0.5)).astype(np.float64)
    out = []
    for c in cells:
        for a in range(3):
            for side in (0, 1):
                p = mid.copy()
                p[a] = (lo[a] - c + 0.5) * cell if side == 0 else (hi[a] + c - 0.5) * cell
                out.append(p)
    return np.array(out, F)


def query_mix(pts, cell, seed=17, nonfinite=True):
    """Queries for one target cloud: 150 perturbed target points, 50 uniform in a box 1.25 x the target's (at least 4 cells wide per
    side for a cloud without extent), 30 exact hits, one point per face exactly one cell outside the bounding box and one six cells
    outside, the same twelve relative to the grid box (fq = -1, fq = cdim * 8, six cells beyond), and (nonfinite) [nan,0,0], [0,inf,0],
    [1e30,1e30,1e30]."""
    pts = np.asarray(pts, F)
    rng = np.random.default_rng(seed)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2 * 1.25, 4.0 * cell)
    near = pts[rng.integers(0, len(pts), 150)] + rng.normal(0, 0.2, (150, 3)).astype(F)
    box = rng.uniform(mid - half, mid + half, (50, 3)).astype(F)
    hits = pts[np.arange(30) % len(pts)]
    parts = [near, box, hits, face_points(pts, cell), grid_face_points(pts, cell)]
    if nonfinite:
        parts.append(NONFINITE3)
    return np.ascontiguousarray(np.vstack(parts), F)


# ---- more than 262 144 queries (nn1_kernel capped at two shells + nn1_coop_kernel over the work list) --------------------------------
LARGE_CELL = 0.5                      # NDT resolution 4.0 / 8
ISOLATED = np.float32([20.0, -20.0, 6.0])    # dyadic coordinates; nothing else of the target within 3 m
N_EXACT_GATE = 102                    # queries at exactly 0.5 m from ISOLATED along one axis: d2 == 0.25


@functools.lru_cache(maxsize=None)
def large_target():
    """<= 2 048 points: a slice of the scan inside a 60 m x 60 m x 12 m box (a coarse grid of about 16 x 16 x 4 cells of 4 m), the pile,
    and ISOLATED."""
    pile = cloud("pile")
    from lidarslam_ros2_amd import synth

    full = synth.small_case(n_source=1500, n_keyframes=2).target.astype(F)
    box = (np.abs(full[:, 0]) < 29.5) & (np.abs(full[:, 1]) < 29.5) & (full[:, 2] < 11.5)
    away = np.linalg.norm(full.astype(np.float64) - ISOLATED[None, :], axis=1) > 3.0
    s = full[box & away][: 2048 - len(pile) - 1]
    return _frozen(np.vstack([s, pile, ISOLATED[None, :]]))


@functools.lru_cache(maxsize=None)
def large_queries(n=NN_WAVE_MAX_QUERIES + 1):
    """n >= 262 145 queries in the TARGET frame, fixed seed, shuffled: 64 non-finite, N_EXACT_GATE at exactly 0.5 m from ISOLATED,
    1 200 exact hits, 40 000 uniform in the grid box (metres from the sparse target: deferred by the capped walk), 8 000 six to
    sixty cells outside the box, a tenth at a few cells' distance, the rest (> 55 %) within centimetres of a target point."""
    tgt = large_target()
    rng = np.random.default_rng(262145)
    org, cdim = grid_dims(tgt, LARGE_CELL)
    lo = org.astype(np.float64) * LARGE_CELL
    hi = (org + 8 * cdim).astype(np.float64) * LARGE_CELL
    bad = np.zeros((64, 3), F)
    bad[np.arange(64), np.arange(64) % 3] = np.array([np.nan, np.inf, -np.inf, np.nan], F)[np.arange(64) % 4]
    step = np.zeros((6, 3), F)
    step[np.arange(6), np.arange(6) % 3] = np.float32([0.5, 0.5, 0.5, -0.5, -0.5, -0.5])
    gate = ISOLATED[None, :] + step[np.arange(N_EXACT_GATE) % 6]
    hits = tgt[rng.integers(0, len(tgt), 1200)]
    inside = rng.uniform(lo, hi, (40000, 3)).astype(F)
    out = rng.uniform(lo, hi, (8000, 3))
    ax, side = rng.integers(0, 3, 8000), rng.integers(0, 2, 8000)
    far = rng.uniform(6, 60, 8000) * LARGE_CELL
    out[np.arange(8000), ax] = np.where(side == 0, lo[ax] - far, hi[ax] + far)
    n_mid = n // 10
    mid = tgt[rng.integers(0, len(tgt), n_mid)] + rng.normal(0, 0.7, (n_mid, 3)).astype(F)
    n_near = n - (64 + N_EXACT_GATE + 1200 + 40000 + 8000 + n_mid)
    near = tgt[rng.integers(0, len(tgt), n_near)] + rng.normal(0, 0.08, (n_near, 3)).astype(F)
    q = np.vstack([bad, gate, hits, inside, out.astype(F), mid, near]).astype(F)
    return _frozen(q[rng.permutation(n)])


@functools.lru_cache(maxsize=None)
def large_source(n=NN_WAVE_MAX_QUERIES + 1, posed=False):
    """The source cloud whose image under the pose (identity, or yaw_pose() when `posed`) is large_queries(n)."""
    return _frozen(preimage(yaw_pose() if posed else None, large_queries(n)))


@functools.lru_cache(maxsize=None)
def large_brute(n=NN_WAVE_MAX_QUERIES + 1, posed=False, shift=0.0):
    """brute_nn for large_source (computed once per process: about two seconds); shift: metres added to every source x."""
    src = large_source(n, posed)
    if shift:
        src = src + np.float32([shift, 0, 0])
    idx, d2 = brute_nn(large_target(), src, yaw_pose() if posed else None)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


# ---- members of a fitness group (nn1_ball_group_kernel + nn1_list_group_kernel) ----------------------------------------------------
GROUP_CELL = 0.5                      # NDT resolution 4.0 / 8
POSE_A = yaw_pose()
POSE_B = yaw_pose(-50.0, (-0.4, 0.25, -0.05))
POSE_FAR = np.eye(4, dtype=F)
POSE_FAR[:3, 3] = 1e30


@functools.lru_cache(maxsize=None)
def group_target():
    from lidarslam_ros2_amd import synth

    return _frozen(synth.small_case(n_source=4500, n_keyframes=4).target[::9][:3000])    # every ninth point: ground, walls and poles


@functools.lru_cache(maxsize=None)
def group_members():
    """[(name, pose, source)] for members 1..13 of the group fitness test.  Every source is the pre-image under its pose of the
    queries the member is about (built in the target frame), <= 4 400 points."""
    tgt = group_target()
    rng = np.random.default_rng(13)
    c = F(GROUP_CELL)
    lo, hi = tgt.min(0), tgt.max(0)
    on = lambda: (tgt + rng.normal(0, 0.02, tgt.shape)).astype(F)
    m1 = on()
    m2 = (tgt + F(1.3) * c).astype(F)                                   # 1.3 fine cells on every axis: the own cell is often empty
    m3 = on()
    m3[::2] += np.float32([hi[0] - lo[0] + 30.0, 0, 0])                 # every other point 30 m beyond the target
    m4 = (tgt + np.float32([500.0, 0, 0])).astype(F)
    m5 = np.tile(np.vstack([face_points(tgt, GROUP_CELL), grid_face_points(tgt, GROUP_CELL)]), (100, 1))   # fq = -1, fq = cdim * 8 and beyond, 2 400 points
    # 2 to 3 m from the nearest target point, inside the grid box: a ball of more than FIT_BALL_CELLS cells
    d = rng.normal(0, 1, (12000, 3))
    cand = (tgt[rng.integers(0, len(tgt), 12000)] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.2, 2.8, (12000, 1))).astype(F)
    org, cdim = grid_dims(tgt, GROUP_CELL)
    dist = np.sqrt(brute_nn(tgt, cand)[1].astype(np.float64))
    m6 = cand[(dist >= 2.0) & (dist <= 3.0) & (cells_outside(cand, GROUP_CELL, org, cdim) == 0)][:3000]
    m7 = on()[:2000]
    m7[rng.choice(2000, 64, replace=False)] = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3], F)[np.arange(64) % 4]
    m8 = np.zeros((0, 3), F)
    m9 = tgt[:1000]
    A = [("on", m1), ("shifted", m2), ("half_out", m3), ("far", m4), ("faces", m5), ("ball", m6), ("nonfinite", m7), ("empty", m8)]
    out = [(name, POSE_A, _frozen(preimage(POSE_A, q))) for name, q in A]
    out.append(("pose_1e30", POSE_FAR, _frozen(m9)))
    out += [(name + "_b", POSE_B, _frozen(preimage(POSE_B, q))) for name, q in A[:4]]
    return tuple(out)


def must_defer(target, source, T, cell):
    """Queries the sixteen-lane ball form has to put on the work list: the nearest target point lies outside the 3 x 3 x 3 fine cells
    around the query (nothing nearer can be in them: no seed), or farther than FIT_BALL_CELLS cells away (the ball is too wide)."""
    idx, d2 = brute_nn(target, source, T)
    q = transform_rn(source, T)
    org, _ = grid_dims(target, cell)
    ok = idx >= 0
    fq = fine_cell(q[ok], cell, org)
    ft = fine_cell(np.asarray(target, F)[idx[ok]], cell, org)
    out = np.zeros(len(q), bool)
    out[ok] = (np.abs(fq - ft).max(1) > 1) | (np.sqrt(d2[ok].astype(np.float64)) > FIT_BALL_CELLS * cell)
    return out


# ---- a target hundreds of metres wide (GICP object: the sort builder chosen by the key count) -----------------------------------------
WIDE_CELL = 0.5                       # nn_pick_cell


@functools.lru_cache(maxsize=None)
def wide_scene():
    from lidarslam_ros2_amd import synth

    return _frozen(synth.small_case(n_source=1500, n_keyframes=2).target[::7][:2000])    # every seventh point: the scene's full height


def wide_target(gap):
    """Two copies of the 2 000-point scene, `gap` metres apart in x and in y."""
    s = wide_scene()
    return np.ascontiguousarray(np.vstack([s, s + np.float32([gap, gap, 0])]), F)


def wide_queries(gap):
    """2 000 near each copy and 200 at up to 40 m from a copy; none in the empty middle (coop_knn walks coarse shells one by one)."""
    s = wide_scene()
    rng = np.random.default_rng(600)
    off = np.float32([gap, gap, 0])
    a = s + rng.normal(0, 0.15, s.shape).astype(F)
    b = s + off + rng.normal(0, 0.15, s.shape).astype(F)
    d = rng.normal(0, 1, (200, 3))
    d[:, 2] *= 0.2
    ring = s[rng.integers(0, len(s), 200)] + (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2, 40, (200, 1))).astype(F)
    ring[100:] += off
    return np.ascontiguousarray(np.vstack([a, b, ring]), F)
