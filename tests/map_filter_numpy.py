"""The map filter restated in numpy (lsr_voxel_grid_filter_map; include/lidarslam_reg.h states the definition): pcl::VoxelGrid with the
leaf index in int64, a stable argsort, float32 sums accumulated one point at a time.  Independent of csrc/map_filter.hip; the CPU test
pins it to the project's oracle where the int32 grid applies."""
import numpy as np

F32 = np.float32
CELL_LIMIT, DIV_LIMIT = 1 << 24, 1 << 21


class IndexOverflow(ValueError):
    pass


def fields(records, layout):
    """(n, point_step) uint8 or (n, point_step / 4) float32 records -> float32 x, y, z, intensity (None without the field)."""
    step, (ox, oy, oz, oi) = layout
    a = np.ascontiguousarray(records)
    w = a.reshape(-1).view(np.uint8).reshape(-1, step).view(np.float32)
    return w[:, ox // 4], w[:, oy // 4], w[:, oz // 4], (None if oi is None else w[:, oi // 4])


def leaf_index(x, y, z, leaf):
    """-> (int64 leaf index of every finite point, mask of the finite points, div_b).  Float arithmetic throughout: one multiply, a
    floor, a subtraction of (float) min_b."""
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    if not finite.any():
        return np.zeros(0, np.int64), finite, (0, 0, 0)
    inv_leaf = F32(1.0) / F32(leaf)
    p = [c[finite] for c in (x, y, z)]
    min_b, div_b = [], []
    for c in p:
        lo, hi = np.floor(c.min() * inv_leaf), np.floor(c.max() * inv_leaf)
        if not (abs(float(lo)) < CELL_LIMIT and abs(float(hi)) < CELL_LIMIT):
            raise IndexOverflow("a cell coordinate reaches 2^24")
        min_b.append(int(lo))
        div_b.append(int(hi) - int(lo) + 1)
        if div_b[-1] > DIV_LIMIT:
            raise IndexOverflow("more than 2^21 cells along an axis")
    cell = [(np.floor(c * inv_leaf) - F32(mb)).astype(np.int32).astype(np.int64) for c, mb in zip(p, min_b)]
    assert all(c.dtype == np.int64 for c in cell)
    return cell[0] + cell[1] * div_b[0] + cell[2] * (div_b[0] * div_b[1]), finite, tuple(div_b)


def index_bits(div_b) -> int:
    """Bits of the largest leaf index (at least 1)."""
    return max(1, int(div_b[0] * div_b[1] * div_b[2] - 1).bit_length())


def voxel_grid_filter_map(records, leaf, layout, out_layout, return_index=False):
    """-> (m, out point_step) uint8 records, one per occupied leaf in ascending leaf index; with return_index also the int64 indices."""
    x, y, z, w = fields(records, layout)
    idx, finite, _ = leaf_index(x, y, z, leaf)
    out_step, (ox, oy, oz, oi) = out_layout
    order = np.argsort(idx, kind="stable")          # ascending leaf index, ascending input index inside a leaf
    keys = idx[order]
    heads = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]]) if keys.size else np.zeros(0, np.int64)
    ends = np.r_[heads[1:], keys.size]
    cols = [c[finite][order] for c in (x, y, z)] + [None if w is None else w[finite][order]]
    out = np.zeros((heads.size, out_step // 4), np.float32)
    for r, (a, b) in enumerate(zip(heads, ends)):
        m = F32(b - a)
        for col, off in zip(cols, (ox, oy, oz, oi)):
            if off is None:
                continue
            s = F32(0.0)
            if col is not None:
                for v in col[a:b]:                  # one float32 addition per point, in input order
                    s = F32(s + v)
                s = F32(s / m)
            out[r, off // 4] = s
    rec = out.view(np.uint8).reshape(heads.size, out_step)
    return (rec, keys[heads]) if return_index else rec


def high_word_cloud():
    """The cloud whose order only the HIGH index word decides (leaf 0.25: inv_leaf is exactly 4; points at (cell + 0.5) * leaf):
    (11, 8) float32 PointXYZI records.  Two points at the cells (0, 0, 0) and (65535, 65535, 3) pin div_b = (65536, 65536, 4); three
    jittered points in (1234, 4321, 2), then three in (1234, 4321, 1) — equal low words 283 182 290, high words 2 and 1, the later
    leaf first in the cloud —; one point each in (9, 7, 1) and (5, 7, 1); a record with a NaN x."""
    rng = np.random.default_rng(2)
    cells = [(0, 0, 0), (65535, 65535, 3)] + [(1234, 4321, 2)] * 3 + [(1234, 4321, 1)] * 3 + [(9, 7, 1), (5, 7, 1), (3, 3, 3)]
    rec = np.zeros((len(cells), 8), np.float32)
    rec[:, :3] = (np.asarray(cells, np.float64) + 0.5) * 0.25
    rec[2:8, :3] += rng.uniform(-0.1, 0.1, (6, 3)).astype(np.float32)
    rec[:, 4] = rng.uniform(0.0, 255.0, len(cells)).astype(np.float32)
    rec[-1, 0] = np.nan
    return rec
