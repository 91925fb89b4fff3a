"""TEST INFRASTRUCTURE: the bytes of an ASCII .pcd file (pcl::PCDWriter::writeASCII at its default precision 8 for a cloud
of width n, height 1 and default viewpoint), restated with Python's own '%.8g' of the float promoted to double — independent of
csrc/pcd_format.hpp.  Every comparison against it is on the raw bytes: there is no tolerance."""
import numpy as np

XYZI = (32, (0, 4, 8, 16))

FLT_MAX, FLT_MIN, DENORM_MIN, DENORM_MAX = 0x7f7fffff, 0x00800000, 0x00000001, 0x007fffff

# the issue's anchors: (value as float32 bits, text)
ANCHORS = [
    (np.float32(1234567.25), "1234567.2"), (np.float32(1234567.75), "1234567.8"), (np.float32(0.1), "0.1"),
    (np.float32(99999992.0), "99999992"), (np.float32(1e8), "1e+08"), (np.float32(1e-4), "9.9999997e-05"),
    (np.uint32(DENORM_MIN).view(np.float32), "1.4012985e-45"), (np.uint32(FLT_MAX).view(np.float32), "3.4028235e+38"),
    (np.uint32(FLT_MIN).view(np.float32), "1.1754944e-38"), (np.float32(123456.789), "123456.79"),
]


def field_text(v) -> str:
    """One float32 as PCL prints it: '%.8g' of the double; any NaN, whatever its sign, is 'nan'."""
    d = float(np.float32(v))
    if d != d:
        return "nan"
    return "%.8g" % d


def bits_to_float(bits) -> np.ndarray:
    return np.asarray(bits, np.uint32).view(np.float32)


def special_bits() -> np.ndarray:
    """+-0, +-inf, NaNs of both signs and several payloads, FLT_MAX, FLT_MIN, the smallest and the largest denormal, and their negatives."""
    pos = [0x00000000, 0x7f800000, 0x7fc00000, 0x7f800001, 0x7fffffff, 0x7fa5a5a5, FLT_MAX, FLT_MIN, DENORM_MIN, DENORM_MAX]
    return np.array(pos + [b | 0x80000000 for b in pos], np.uint32)


def decade_edge_bits() -> np.ndarray:
    """The floats next to 10^k on both sides (and the nearest float itself) for k = -5 .. 9: where %g switches form and digit count."""
    out = []
    for k in range(-5, 10):
        c = np.float32(10.0 ** k)
        out += [np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(np.inf))]
    a = np.array(out, np.float32).view(np.uint32)
    return np.concatenate([a, a | np.uint32(0x80000000)])


def table_bits() -> np.ndarray:
    """Anchors, specials and decade edges: the value table of the CPU and the GPU tests."""
    anchors = np.array([a for a, _ in ANCHORS], np.float32).view(np.uint32)
    return np.concatenate([anchors, anchors | np.uint32(0x80000000), special_bits(), decade_edge_bits()])


def header(n: int, with_intensity: bool = True) -> bytes:
    f, s, t, c = ("x y z intensity", "4 4 4 4", "F F F F", "1 1 1 1") if with_intensity else ("x y z", "4 4 4", "F F F", "1 1 1")
    return (f"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS {f}\nSIZE {s}\nTYPE {t}\nCOUNT {c}\n"
            f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA ascii\n").encode("ascii")


def fields(records, layout=XYZI) -> np.ndarray:
    """(n, 3 or 4) float32: the fields of every record in line order."""
    step, offs = layout
    buf = np.ascontiguousarray(records).reshape(-1).view(np.uint8).reshape(-1, step)
    cols = [buf[:, o:o + 4].copy().view(np.float32).reshape(-1) for o in offs if o is not None and o >= 0]
    return np.stack(cols, 1) if len(buf) else np.zeros((0, len(cols)), np.float32)


def pcd_ascii_bytes(records, layout=XYZI) -> bytes:
    """The whole file image for `records` (any array whose bytes are whole records of `layout`)."""
    F = fields(records, layout)
    nan = np.isnan(F)
    with np.errstate(invalid="ignore"):   # signalling NaNs among the test values
        D = F.astype(np.float64).tolist()
    lines = []
    for row, row_nan in zip(D, nan.tolist()):
        lines.append(" ".join("nan" if m else "%.8g" % v for v, m in zip(row, row_nan)))
    body = ("\n".join(lines) + "\n").encode("ascii") if lines else b""
    return header(len(F), layout[1][3] is not None and layout[1][3] >= 0) + body


def random_records(rng, n: int, step: int = 32, specials: float = 0.01) -> np.ndarray:
    """(n, step / 4) float32: every word log-uniform over 1e-6 .. 1e6 with mixed signs, about `specials` of them special values — line
    lengths vary over the whole range, so a workgroup's text starts at every alignment."""
    w = step // 4
    mag = 10.0 ** rng.uniform(-6.0, 6.0, (n, w))
    a = (mag * rng.choice([-1.0, 1.0], (n, w))).astype(np.float32)
    sp = special_bits()
    mask = rng.random((n, w)) < specials
    a.view(np.uint32)[mask] = sp[rng.integers(0, len(sp), int(mask.sum()))]
    return a


class FakeRegistration:
    """A registration object for the host-side bookkeeping test of MapArray.save_map: saveMapPCDFileASCII is map_numpy's assembly and
    this module's text; every call is recorded."""

    def __init__(self):
        self.calls = []

    def saveMapPCDFileASCII(self, path, submaps, poses=None, in_layout=XYZI):
        import map_numpy

        self.calls.append(("saveMapPCDFileASCII", str(path), len(submaps), poses is not None, in_layout))
        rec, _ = map_numpy.assemble_map(submaps, poses, in_layout, XYZI)
        data = pcd_ascii_bytes(rec, XYZI)
        with open(path, "wb") as f:
            f.write(data)
        return len(data)
