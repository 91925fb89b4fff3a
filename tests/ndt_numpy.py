"""fp64 numpy restatement of the NDT score and gradient (Magnusson 2009 eqs 6.9, 6.12, 6.18-6.19) on a
voxel table — dumped from the oracle, or built from the raw points by `NumpyGrid` — the "maths truth" the C++ oracle's analytic
derivatives are checked against by finite differences (SURVEY.md §8c KAT 3).  Test infrastructure only."""
import numpy as np


class NumpyGrid:
    """pclomp::VoxelGridCovariance::applyFilter restated in fp64 numpy from the raw points, independent of the oracle: PCL's fp32
    bounding box and leaf index, fp64 running sums in cloud order, the single-pass covariance with its (n - 1) / n factor, the
    eigenvalue check and clamp (np.linalg.eigh), the inverse; the FLOAT Leaf::centroid running sum.  Per leaf (sorted by linear
    index, like the oracle's dump): `n` as the lookups see it (-1 = invalidated), the raw count, and three flags —
      in_tree: count >= min_points: the leaf's centroid is in the kd-tree (pushed BEFORE the eigen check, so invalidated leaves stay);
      valid:   in_tree and the eigen check passed (the DIRECT getters test nr_points >= min_points);
      clamped: the number of eigenvalues raised to eig_mult * lambda2.
    An invalidated leaf keeps Leaf's constructor icov_ = 0."""

    def __init__(self, pts, leaf, min_points=6, eig_mult=0.01):
        pts = np.asarray(pts, np.float32)[:, :3]
        pts = pts[np.isfinite(pts).all(1)]
        self.leaf = float(leaf)
        inv = np.float32(1.0) / np.float32(leaf)
        mn, mx = pts.min(0), pts.max(0)
        self.min_b = np.floor(mn * inv).astype(np.int64)
        self.max_b = np.floor(mx * inv).astype(np.int64)
        div = self.max_b - self.min_b + 1
        ijk = (np.floor(pts * inv) - self.min_b.astype(np.float32)).astype(np.int64)
        key = ijk @ np.array([1, div[0], div[0] * div[1]], np.int64)
        idx = np.unique(key)
        L = len(idx)
        self.idx, self.count = idx.astype(np.int32), np.zeros(L, np.int32)
        self.n = np.zeros(L, np.int32)
        self.mean, self.cov, self.icov = np.zeros((L, 3)), np.zeros((L, 3, 3)), np.zeros((L, 3, 3))
        self.centroid = np.zeros((L, 3), np.float32)
        self.in_tree, self.valid, self.clamped = np.zeros(L, bool), np.zeros(L, bool), np.zeros(L, np.int32)
        self.sum, self.sq = np.zeros((L, 3)), np.zeros((L, 3, 3))
        for li, k in enumerate(idx):
            p = pts[key == k]                        # cloud order
            n = len(p)
            s, sq, cs = np.zeros(3), np.zeros((3, 3)), np.zeros(3, np.float32)
            for q in p:                              # running sums, one point after the other
                q64 = q.astype(np.float64)
                s = s + q64
                sq = sq + np.outer(q64, q64)
                cs = (cs + q).astype(np.float32)
            self.count[li], self.n[li], self.sum[li], self.sq[li] = n, n, s, sq
            mean = s / n
            self.mean[li] = mean
            self.centroid[li] = cs / np.float32(n)
            if n < min_points:
                continue
            self.in_tree[li] = True
            cov = (sq - 2.0 * np.outer(s, mean)) / n + np.outer(mean, mean)
            cov = cov * ((n - 1.0) / n)
            w, V = np.linalg.eigh(cov)
            if w[0] < 0 or w[1] < 0 or w[2] <= 0:
                self.n[li] = -1
                continue
            lmin = eig_mult * w[2]
            if w[0] < lmin:
                w = w.copy()
                w[0] = lmin
                self.clamped[li] = 1
                if w[1] < lmin:
                    w[1] = lmin
                    self.clamped[li] = 2
                cov = V @ np.diag(w) @ np.linalg.inv(V)
            self.cov[li] = cov
            ic = np.linalg.inv(cov)
            if not np.isfinite(ic).all():
                self.n[li] = -1
                continue
            self.icov[li] = ic
            self.valid[li] = True
        self.n_valid = int(self.valid.sum())

    def dump(self):
        """The oracle's dump layout (idx, n, mean, icov) plus the flags."""
        return dict(idx=self.idx, n=self.n, mean=self.mean, cov=self.cov, icov=self.icov, in_tree=self.in_tree, valid=self.valid)


def rot_xyz(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def jang_rows(p):
    cx, sx, cy, sy, cz, sz = np.cos(p[3]), np.sin(p[3]), np.cos(p[4]), np.sin(p[4]), np.cos(p[5]), np.sin(p[5])
    return np.array([
        [-sx * sz + cx * sy * cz, -sx * cz - cx * sy * sz, -cx * cy],
        [cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy],
        [-sy * cz, sy * sz, cy],
        [sx * cy * cz, -sx * cy * sz, sx * sy],
        [-cx * cy * cz, cx * cy * sz, -cx * sy],
        [-cy * sz, -cy * cz, 0],
        [cx * cz - sx * sy * sz, -cx * sz - sx * sy * cz, 0],
        [sx * cz + cx * sy * sz, cx * sy * cz - sx * sz, 0]])


class NumpyNdt:
    """`dump`: an oracle dump or NumpyGrid.dump().  DIRECT lookups use the leaves with n >= min_points; the KDTREE search (search=0)
    queries the kd-tree of every leaf with >= min_points points — invalidated ones (n = -1) included, with their icov of zero: such
    a hit adds exactly -d1 to the score and nothing to the gradient, as pclomp's radiusSearch + computeDerivatives do.
    kd_invalid=False drops them (the pre-fix reading).  After score_grad, `kd_score_only` counts those hits."""

    def __init__(self, dump, min_b, max_b, leaf, d1, d2, search=7, centroids=None, kd_invalid=True):
        self.leaf, self.d1, self.d2 = float(leaf), d1, d2
        self.min_b, self.max_b = np.asarray(min_b, np.int64), np.asarray(max_b, np.int64)
        div = self.max_b - self.min_b + 1
        self.mul = np.array([1, div[0], div[0] * div[1]], np.int64)
        ok = dump["n"] >= 6
        self.table = {int(k): (m, c) for k, m, c in zip(dump["idx"][ok], dump["mean"][ok], dump["icov"][ok])}
        self.kd = None
        self.kd_score_only = 0
        if search == 0:      # KDTREE: a radius search over ALL leaf centroids (brute force: no cell structure is assumed here)
            assert centroids is not None
            tree = ok | (dump["n"] == -1) if kd_invalid else ok
            zero = np.zeros((3, 3))
            self.kd = (np.asarray(centroids, np.float32)[tree],
                       [(m, c if n >= 6 else zero) for m, c, n in zip(dump["mean"][tree], dump["icov"][tree], dump["n"][tree])],
                       np.float32(np.float64(np.float32(leaf)) * np.float64(np.float32(leaf))),
                       dump["n"][tree] < 0)
            self.off = np.zeros((0, 3), np.int64)
        elif search == 1:    # DIRECT1: the cell of the transformed point only
            self.off = np.zeros((1, 3), np.int64)
        elif search == 26:   # DIRECT26: the full 3x3x3 block, centre included (27 cells)
            self.off = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.int64)
        else:                # DIRECT7: centre + the six face neighbours
            self.off = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.int64)

    def score_grad(self, src, p):
        """fp64 score and gradient; cell lookup uses the same fp32 floor(x'/leaf) as the reference so the
        voxel assignment matches at cell faces."""
        p = np.asarray(p, np.float64)
        R = rot_xyz(*p[3:])
        xt = src.astype(np.float64) @ R.T + p[:3]
        ijk = np.floor(xt.astype(np.float32) / np.float32(self.leaf)).astype(np.int64)
        Jr = jang_rows(p)
        score, g = 0.0, np.zeros(6)
        self.kd_score_only = 0
        for n in range(src.shape[0]):
            x = src[n].astype(np.float64)
            ja = Jr @ x
            J = np.array([[1, 0, 0, 0, ja[2], ja[5]], [0, 1, 0, ja[0], ja[3], ja[6]], [0, 0, 1, ja[1], ja[4], ja[7]]])
            leaves = []
            if self.kd is not None:
                # pcl::KdTreeFLANN::radiusSearch on the float point: L2_Simple<float>, strictly inside (float)(r * r)
                diff = np.float32(xt[n]).astype(np.float32) - self.kd[0]
                d = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
                hits = np.nonzero(d < self.kd[2])[0]
                leaves = [self.kd[1][k] for k in hits]
                self.kd_score_only += int(self.kd[3][hits].sum())
            for o in self.off:
                c = ijk[n] + o
                if np.any(c < self.min_b) or np.any(c > self.max_b):
                    continue
                leaf = self.table.get(int(((c - self.min_b) * self.mul).sum()))
                if leaf is not None:
                    leaves.append(leaf)
            for leaf in leaves:
                q = xt[n] - leaf[0]
                Cq = leaf[1] @ q
                e = np.exp(-self.d2 * (q @ Cq) / 2)
                w = self.d2 * e
                if not (0 <= w <= 1):
                    continue
                score += -self.d1 * e
                g += self.d1 * w * (Cq @ J)
        return score, g
