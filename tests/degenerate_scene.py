"""A target whose degenerate NDT leaves are decided by geometry, not by rounding.  Test infrastructure only.

Resolution 2.0; every coordinate is a multiple of 1/16 m with |x| < 64, and every leaf whose covariance an assertion looks at
holds a power-of-two number of points.  Then every fp64 sum, mean, (n - 1) / n factor and single-pass covariance is exact, and so
are the fp32 running sums of Leaf::centroid: any summation order, with or without FMA, gives the same bits.  The degenerate
patterns are axis-aligned lattices, so their covariances are diagonal and every eigensolver returns that diagonal exactly.

Leaf kinds (cell -> kind in `Scene.kinds`):
  ordinary   32 random lattice points in the cell                     valid, carries the registration
  plane      4 x 4 lattice in an axis-aligned plane                   lambda0 = 0 -> valid, lambda0 clamped to 0.01 lambda2
  line       16 points on an axis-parallel line                       lambda0 = lambda1 = 0 -> valid, both clamped
  point      8 or 16 copies of one point                              cov = 0 -> invalid (nr_points = -1), but in the kd-tree
  five       5 random points                                          below min_points_per_voxel: in nothing
  six        6 random points                                          valid (not power-of-two: its mean is rounded, identically
                                                                      everywhere, but its covariance is not exact)
plus a few non-finite target points.  The source is made of points near every kind, moved by the inverse of `truth`, so that a
registration from the identity has `truth` to find.
"""
from dataclasses import dataclass

import numpy as np

RES = 2.0
# offsets from `truth` of the poses the tests (and the reference recipe's dump) evaluate the derivatives at
POSES = [np.zeros(6), np.array([0.05, -0.03, 0.02, 0.004, -0.002, 0.006]), np.array([-0.04, 0.06, -0.01, -0.003, 0.005, -0.002])]
Q = 1.0 / 16.0                      # coordinate quantum
CELLS_X, CELLS_Y, CELLS_Z = range(-6, 6), range(-3, 3), range(-1, 1)

# cell -> kind; every degenerate cell sits inside the slab, so all 26 of its neighbours exist (ordinary, or one more special cell)
SPECIAL = {
    (-4, -1, -1): ("plane", 2), (0, 1, 0): ("plane", 0), (3, -2, -1): ("plane", 1),
    (-2, 1, -1): ("line", 0), (2, 0, 0): ("line", 1), (4, 1, -1): ("line", 2),
    (-5, -2, 0): ("point", 8), (-3, 0, 0): ("point", 16), (-1, -2, -1): ("point", 8), (1, -1, 0): ("point", 16),
    (1, 1, -1): ("point", 8), (3, 0, 0): ("point", 16), (4, -2, 0): ("point", 8), (-1, 1, 0): ("point", 16),
    (-4, 1, 0): ("five", 5), (2, -2, 0): ("six", 6),
}


@dataclass
class Scene:
    target: np.ndarray          # (N, 3) float32, non-finite rows included
    source: np.ndarray          # (M, 3) float32
    truth: np.ndarray           # 6-vector pose (x, y, z, roll, pitch, yaw) that registers the source onto the target
    kinds: dict                 # linear leaf index -> kind name (every occupied leaf)
    exact: set                  # linear leaf indices with a power-of-two count (exactly computed covariance)


def _lattice(rng, origin, n):
    """n random distinct-ish lattice points inside the cell at `origin` (a 2 m cube)."""
    k = rng.integers(0, int(RES / Q), (n, 3))
    return origin + k * Q


def _pattern(kind, arg, origin, rng):
    o = np.asarray(origin, np.float64)
    if kind == "ordinary":
        return _lattice(rng, o, 32)
    if kind == "plane":        # normal along axis `arg`
        a, b = [k for k in range(3) if k != arg]
        u, v = np.meshgrid(np.arange(4) * 0.375 + 0.25, np.arange(4) * 0.25 + 0.5, indexing="ij")
        p = np.zeros((16, 3))
        p[:, a], p[:, b], p[:, arg] = u.ravel(), v.ravel(), 1.0625
        return o + p
    if kind == "line":         # along axis `arg`
        p = np.full((16, 3), 0.75)
        p[:, (arg + 1) % 3] = 1.3125
        p[:, arg] = np.arange(16) * 0.0625 + 0.4375
        return o + p
    if kind == "point":
        return np.repeat((o + np.array([0.8125, 1.1875, 0.9375]))[None], arg, axis=0)
    if kind in ("five", "six"):
        return _lattice(rng, o, arg)
    raise ValueError(kind)


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def leaf_index(cell):
    """Linear leaf index of a cell of the slab (the grid's min_b is the slab's lowest cell: the slab's corners are ordinary)."""
    nx, ny = len(CELLS_X), len(CELLS_Y)
    return (cell[0] - CELLS_X[0]) + (cell[1] - CELLS_Y[0]) * nx + (cell[2] - CELLS_Z[0]) * nx * ny


def make(seed=0, truth=(0.12, -0.08, 0.04, 0.006, -0.004, 0.009)):
    rng = np.random.default_rng(seed)
    tgt, src, kinds, exact = [], [], {}, set()
    for cz in CELLS_Z:
        for cy in CELLS_Y:
            for cx in CELLS_X:
                kind, arg = SPECIAL.get((cx, cy, cz), ("ordinary", 0))
                o = np.array([cx, cy, cz], np.float64) * RES
                pts = _pattern(kind, arg, o, rng)
                tgt.append(pts)
                li = leaf_index((cx, cy, cz))
                kinds[li] = kind
                if len(pts) & (len(pts) - 1) == 0:
                    exact.add(li)
                # source near this leaf: a few of its own points, jittered; around "point" leaves a ball of radius 1.5 m,
                # so that after the pose error many still lie within `resolution` of the leaf's centroid
                if kind == "point":
                    d = rng.normal(0, 1, (20, 3))
                    d *= (rng.uniform(0.2, 1.5, 20) / np.linalg.norm(d, axis=1))[:, None]
                    src.append(pts[0] + d)
                else:
                    pick = pts[rng.integers(0, len(pts), min(len(pts), 10))]
                    src.append(pick + rng.normal(0, 0.03, pick.shape))
    # shuffle the target so that the leaves' points interleave in cloud order, then add the non-finite points
    target = np.concatenate(tgt)
    target = target[rng.permutation(len(target))]
    bad = np.array([[np.nan, 0.5, 0.5], [1.0, np.inf, 0.0], [-np.inf, -np.inf, 2.0], [0.25, 0.25, np.nan]])
    target = np.insert(target, [7, 100, 1000, len(target) - 3], bad, axis=0).astype(np.float32)
    fin = target[np.isfinite(target).all(1)]
    assert np.abs(fin).max() < 64 and (np.round(fin / Q) * Q == fin).all()
    source = np.concatenate(src)
    source = source[rng.permutation(len(source))]
    p = np.asarray(truth, np.float64)
    R = _rot(*p[3:])
    # truth maps source -> target: target = R s + t  =>  s = R^T (x - t)
    source = ((source - p[:3]) @ R).astype(np.float32)
    return Scene(target=target, source=source, truth=p, kinds=kinds, exact=exact)
