"""The map window restated in numpy float32 (lsr_map_window_around, lsr_crop_map; include/lidarslam_reg.h states the definition, and
this file was written from that text): f = floor(p * (1 / leaf)) in float32, kept iff finite and lo <= f <= hi compared in float32, the
kept records in input order with their four fields moved and every other byte zero.  Independent of csrc/map_window.hip."""
import numpy as np

F32 = np.float32
CELL_LIMIT = 1 << 24


class IndexOverflow(ValueError):
    pass


def fields(records, layout):
    """(n, point_step) uint8 or (n, point_step / 4) float32 records -> float32 x, y, z, intensity (None without the field)."""
    step, (ox, oy, oz, oi) = layout
    w = np.ascontiguousarray(records).reshape(-1).view(np.uint8).reshape(-1, step).view(np.float32)
    return w[:, ox // 4], w[:, oy // 4], w[:, oz // 4], (None if oi is None else w[:, oi // 4])


def cell(p, leaf):
    """The absolute cell of float32 coordinates, as a float32: one multiply by 1.0f / leaf, then the floor."""
    inv_leaf = F32(1.0) / F32(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(p, F32) * inv_leaf)
    assert f.dtype == F32
    return f


def window_around(center, half_extent, leaf):
    """-> (leaf, lo, hi): the difference / sum in double, one conversion to float32, the multiply and the floor."""
    if not F32(leaf) > 0:
        raise ValueError("leaf")
    c, e = np.asarray(center, np.float64), np.asarray(half_extent, np.float64)
    if not (np.isfinite(c).all() and np.isfinite(e).all() and (e >= 0).all()):
        raise ValueError("center / half_extent")
    lo, hi = cell((c - e).astype(F32), leaf), cell((c + e).astype(F32), leaf)
    if not (np.all(np.abs(lo) < F32(CELL_LIMIT)) and np.all(np.abs(hi) < F32(CELL_LIMIT))):
        raise IndexOverflow("a cell of 2^24 or beyond")
    return float(F32(leaf)), tuple(int(v) for v in lo), tuple(int(v) for v in hi)


def keep_mask(x, y, z, window):
    leaf, lo, hi = window
    keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    for c, a, b in zip((x, y, z), lo, hi):
        f = cell(c, leaf)
        with np.errstate(invalid="ignore"):
            keep &= (F32(a) <= f) & (f <= F32(b))
    return keep


def crop(records, window, layout, out_layout, return_mask=False):
    """-> (m, out point_step) uint8: the kept records in ascending input index."""
    x, y, z, w = fields(records, layout)
    keep = keep_mask(x, y, z, window)
    out_step, (ox, oy, oz, oi) = out_layout
    out = np.zeros((int(keep.sum()), out_step // 4), np.uint32)
    for col, off in zip((x, y, z, w), (ox, oy, oz, oi)):
        if off is not None and col is not None:
            out[:, off // 4] = col[keep].view(np.uint32)
    rec = out.view(np.uint8).reshape(out.shape[0], out_step)
    return (rec, keep) if return_mask else rec
