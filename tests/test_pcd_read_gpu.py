"""Reading .pcd files on the device (lsr_decode_pcd, lsr_load_pcd, lsr_set_input_target_pcd): records in HBM against the Python
restatement tests/pcd_read_numpy.py (header parser, line splitter, the C library's strtof).  Every comparison is on raw record bytes:
there is no tolerance.  The shapes are the smallest at which the kernels can go wrong: around the wave (64) and the workgroup (256) of
the parse pass, several workgroups of the line pass (16 KiB of text each), the shortest and the longest line, every alignment of the
body and of the 16-byte loads, pieces cut inside, at and around lines."""
import ctypes as C
import os

import numpy as np
import pytest

import pcd_numpy
import pcd_read_numpy as R
from pcd_numpy import XYZI, pcd_ascii_bytes
from lidarslam_ros2_amd import (GeneralizedIterativeClosestPoint, MapArray, NormalDistributionsTransform, _capi, synth)
from lidarslam_ros2_amd._capi import RegistrationError

pytestmark = pytest.mark.gpu

L16_XYZ = (16, (0, 4, 8, None))
L16_XYZI = (16, (0, 4, 8, 12))
L32_PERM = (32, (20, 0, 28, 8))
LAYOUTS = [XYZI, L16_XYZ, L16_XYZI, L32_PERM]


def _cuda(a):
    import torch

    return torch.from_numpy(np.frombuffer(a, np.uint8).copy() if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)


@pytest.fixture(scope="module")
def reg():
    return NormalDistributionsTransform(device=0)


def check_both(reg, img, layout=XYZI, unresolved=0):
    """decodePCD of a host image and of a device image against the oracle; returns the oracle's records."""
    want = R.decode(img, layout)
    got = reg.decodePCD(img, layout)
    assert isinstance(got, np.ndarray) and got.shape == want.shape and (got == want).all()
    assert (reg.pcdUnresolvedTokens() > 0) == (unresolved > 0)
    got = reg.decodePCD(_cuda(img), layout)
    assert got.is_cuda and (_np(got) == want).all()
    if unresolved == 0:
        assert reg.pcdUnresolvedTokens() == 0
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_round_trip_of_the_writers_image(reg, n):
    rec = pcd_numpy.random_records(np.random.default_rng(900 + n), n)
    img = pcd_ascii_bytes(rec)
    want = check_both(reg, img)
    # what comes back is what "%.8g" keeps of the records: the text of the decoded records is the text again
    assert pcd_ascii_bytes(want.view(np.float32)) == img
    if n == 4099:   # the device formatter's own output closes the chain, text never leaving HBM
        text = reg.formatPCDASCII(_cuda(rec))
        assert (_np(reg.decodePCD(text)) == want).all() and reg.pcdUnresolvedTokens() == 0


@pytest.mark.parametrize("layout", LAYOUTS, ids=["xyzi32", "xyz16", "xyzi16", "permuted32"])
def test_output_layouts_and_the_xyz_header(reg, layout):
    rec = pcd_numpy.random_records(np.random.default_rng(910), 515)
    for img in (pcd_ascii_bytes(rec), pcd_ascii_bytes(rec[:, :4], L16_XYZ)):   # FIELDS x y z intensity, FIELDS x y z
        want = check_both(reg, img, layout)
        if layout == XYZI:
            assert (want.view(np.uint32)[:, [3, 5, 6, 7]] == 0).all()           # every byte outside the fields is zero
            if b"FIELDS x y z\n" in img:
                assert (want.view(np.uint32)[:, 4] == 0).all()                  # no intensity in the file: +0


def test_table_values_in_every_field(reg):
    bits = pcd_numpy.table_bits()
    rec = np.zeros((len(bits), 8), np.float32)
    for k, col in enumerate((0, 1, 2, 4)):
        rec.view(np.uint32)[:, col] = np.roll(bits, -k)
    want = check_both(reg, pcd_ascii_bytes(rec))
    # the file's own nine-digit form gives every finite value back exactly
    with np.errstate(invalid="ignore"):   # signalling NaNs among the table's values
        wide = rec[:, [0, 1, 2, 4]].astype(np.float64)
    lines = [" ".join("%.9g" % float(v) for v in row) for row in wide]
    img9 = pcd_numpy.header(len(rec)) + ("\n".join(lines) + "\n").encode()
    got = _np(reg.decodePCD(_cuda(img9))).view(np.uint32)[:, [0, 1, 2, 4]]
    src = rec.view(np.uint32)[:, [0, 1, 2, 4]]
    nan = np.isnan(rec[:, [0, 1, 2, 4]])
    assert (got[~nan] == src[~nan]).all() and ((got[nan] & 0x7fffffff) == 0x7fc00000).all()
    assert (got == R.decode(img9).view(np.uint32)[:, [0, 1, 2, 4]]).all() and want.shape == (len(bits), 32)


def test_shortest_and_longest_lines_at_every_alignment(reg):
    import torch

    zeros = pcd_ascii_bytes(np.zeros((257, 8), np.float32))
    longest = pcd_ascii_bytes(np.full((257, 8), -np.uint32(pcd_numpy.FLT_MIN).view(np.float32), np.float32))
    assert zeros.endswith(b"0 0 0 0\n") and longest.endswith(b"-1.1754944e-38 -1.1754944e-38 -1.1754944e-38 -1.1754944e-38\n")
    for img in (zeros, longest):
        want = check_both(reg, img)
        buf = torch.full((len(img) + 64,), ord("9"), dtype=torch.uint8, device="cuda")   # digits around the image: reading past it would show
        for shift in range(16):
            buf[shift: shift + len(img)] = _cuda(img)
            assert (_np(reg.decodePCD(buf[shift: shift + len(img)])) == want).all()


def untidy_image():
    """About 300 points of legal but untidy text."""
    rng = np.random.default_rng(920)
    n = 301
    head = (b"# .PCD v0.7\r\nVERSION 0.7\r\nFIELDS intensity rgb x normal y z\r\nSIZE 4 4 4 4 4 4\r\nTYPE F U F F F F\r\nCOUNT 1 1 1 3 1 1\r\n"
            b"WIDTH 301\r\nHEIGHT 1\r\nPOINTS 301\r\nDATA ascii\n")
    forms = [b"+1.5", b"1E2", b"007", b".5", b"5.", b"INF", b"NaN", b"-nan", b"-0", b"1e+05", b"-Infinity", b"0.1", b"3.4028235e38", b"1e-45", b"12345.678"]
    seps = [b" ", b"\t", b"  ", b" \t ", b"\t\t"]
    lines = []
    for k in range(n):
        toks = [forms[rng.integers(len(forms))] if rng.random() < 0.5 else b"%.8g" % rng.normal(0, 100) for _ in range(8)]
        toks[1] = b"4294967295"                                  # rgb: skipped, never parsed as a float
        if k % 7 == 0:
            toks += [b"surplus", b"1,5"]                         # surplus tokens are ignored, whatever they are
        line = b"".join(t + seps[rng.integers(len(seps))] for t in toks[:-1]) + toks[-1]
        lead = [b"", b" ", b"\t ", b"   "][k % 4]
        eol = [b"\n", b"\r\n", b" \r\n", b"\t\n"][rng.integers(4)]
        lines.append(lead + line + eol)
        if k % 11 == 0:
            lines.append([b"\n", b" \t \r\n", b"\r\n"][k % 3])   # empty and blank-only lines between the points
    trailing = [b"this is not a point\n"] * 10 + [b"1 2\n"] * 9 + [b"9 9 9 9 9 9 9 9"]   # 20 lines past POINTS; no final newline
    return head + b"".join(lines) + b"".join(trailing)


def test_legal_but_untidy_text(reg, tmp_path):
    img = untidy_image()
    assert not img.endswith(b"\n")
    for layout in (XYZI, L32_PERM):
        want = check_both(reg, img, layout)
    assert len(want) == 301
    path = tmp_path / "untidy.pcd"
    path.write_bytes(img)
    reg.pcdReadPieceBytes(2048)
    assert (reg.loadPCDFile(path, L32_PERM) == want).all()
    reg.pcdReadPieceBytes(1 << 26)
    # the same points without the trailing lines and without a final newline
    body_end = len(img) - len(b"this is not a point\n" * 10 + b"1 2\n" * 9 + b"9 9 9 9 9 9 9 9")
    cut = img[:body_end].rstrip(b"\r\n\t ")
    assert (reg.decodePCD(cut, L32_PERM) == want).all()


def test_all_tokens_unresolved(reg, tmp_path):
    """300 lines whose every value is a 40-digit text next to the midpoint of two floats: the device leaves them all to the host, and
    the records are strtof's."""
    from fractions import Fraction

    rng = np.random.default_rng(930)
    lines = []
    for _ in range(300):
        toks = []
        for _ in range(4):
            b = int(rng.integers(0x30000000, 0x3a000000))          # 2^-31 .. 2^-11: the midpoints have 30 digits and more
            f0, f1 = (float(np.array([x], np.uint32).view(np.float32)[0]) for x in (b, b + 1))
            mid = (Fraction(f0) + Fraction(f1)) / 2
            e = len(str(mid.numerator // mid.denominator)) - 1 if mid >= 1 else -len(str(mid.denominator // mid.numerator))
            digits = str(int(mid * Fraction(10) ** (39 - e)))   # 40 significant digits, truncated: just below the midpoint or on it
            digits = digits[:39] + ("1" if rng.random() < 0.5 else "0")
            toks.append(("-" if rng.random() < 0.5 else "") + digits[0] + "." + digits[1:] + "e%d" % e)
        lines.append(" ".join(toks))
    img = pcd_numpy.header(300) + ("\n".join(lines) + "\n").encode()
    want = check_both(reg, img, unresolved=1)
    assert reg.pcdUnresolvedTokens() > 1000
    path = tmp_path / "long.pcd"
    path.write_bytes(img)
    reg.pcdReadPieceBytes(4096)
    assert (reg.loadPCDFile(path) == want).all() and reg.pcdUnresolvedTokens() > 1000
    reg.pcdReadPieceBytes(1 << 26)
    reg.decodePCD(pcd_ascii_bytes(np.zeros((3, 8), np.float32)))
    assert reg.pcdUnresolvedTokens() == 0                        # the count is the last call's


def test_piece_independence(reg, tmp_path):
    """A 1000-record file with lines of 1, 60 and 1024 bytes lying across the ends of 2048-, 2049- and 4096-byte pieces."""
    rec = pcd_numpy.random_records(np.random.default_rng(940), 1000)
    lines = pcd_ascii_bytes(rec).split(b"DATA ascii\n")[1].splitlines()
    longest = b"-1.1754944e-38 -1.1754944e-38 -1.1754944e-38 -1.1754944e-38"   # 59 bytes + the newline
    header = pcd_numpy.header(1000)
    out, pos, kinds = [], len(header), []
    for k, line in enumerate(lines):
        room = 2048 - pos % 2048                                  # bytes up to the next multiple of 2048 in the file
        turn = len(kinds) % 3                                     # what lies across the next multiple: by turns
        if turn == 0 and room < 200:                              # 1024 bytes from the first value to the newline: the longest line allowed
            line = line + b" " * (1024 - len(line))
        elif turn == 1 and room < 55:
            line = longest
        elif (turn == 2 and room < 64) or k % 97 == 0:            # a value-less line of one byte in front
            out.append(b"\n")
            pos += 1
        if pos // 2048 != (pos + len(line)) // 2048:
            kinds.append(len(line) + 1)
        out.append(line + b"\n")
        pos += len(line) + 1
    img = header + b"".join(out)
    assert 1025 in kinds and 60 in kinds and len(kinds) >= 20 and b"\n\n" in img
    want = R.decode(img)
    path = tmp_path / "pieces.pcd"
    path.write_bytes(img)
    for piece in (2048, 2049, 4096, 1 << 26):
        assert reg.pcdReadPieceBytes(piece) == piece
        assert (reg.loadPCDFile(path) == want).all(), piece
        assert (_np(reg.loadPCDFile(path, device=True)) == want).all()
    with pytest.raises(RegistrationError):
        reg.pcdReadPieceBytes(2047)
    assert (reg.decodePCD(img) == want).all()


def expect_error(reg, img, status, offset=None, word=None, path=None):
    """decode (host and device image) and load refuse `img` with `status`, name `offset`, and touch neither the records nor the count."""
    lay = reg._layout(*XYZI)
    d_img = _cuda(img)
    for how in ("host", "device", "file"):
        out = np.full((4200, 32), 0xA5, np.uint8)
        n = C.c_size_t(777)
        if how == "file":
            if path is None:
                continue
            path.write_bytes(img)
            st = reg._lib.lsr_load_pcd(reg._h, os.fsencode(path), C.c_void_p(out.ctypes.data), len(out), C.byref(lay), 0, C.byref(n))
        else:
            ptr = img if how == "host" else C.c_void_p(d_img.data_ptr())
            st = reg._lib.lsr_decode_pcd(reg._h, ptr, len(img), int(how == "device"), C.c_void_p(out.ctypes.data), len(out), C.byref(lay), 0, C.byref(n))
        why = reg._lib.lsr_last_error().decode()
        assert st == status, (how, st, why)
        assert n.value == 777 and (out == 0xA5).all()
        if offset is not None:
            assert f"byte offset {offset}" in why, (how, why)
        if word is not None:
            assert word in why, (how, why)
    with pytest.raises(R.PcdError) as e:
        R.decode(img)
    assert e.value.status == status and (offset is None or e.value.offset == offset)


def test_errors_touch_nothing_and_name_the_line(reg, tmp_path):
    rec = pcd_numpy.random_records(np.random.default_rng(950), 1000, specials=0)
    good = pcd_ascii_bytes(rec)
    header = pcd_numpy.header(1000)
    lines = good[len(header):].splitlines(keepends=True)
    starts = np.cumsum([len(header)] + [len(x) for x in lines])
    path = tmp_path / "bad.pcd"
    reg.pcdReadPieceBytes(2048)

    def with_line(k, new):
        return header + b"".join(lines[:k] + [new] + lines[k + 1:])

    for k in (0, 255, 256, 999):                                 # a short line: first, around the workgroup edge, last
        expect_error(reg, with_line(k, b"1 2 3\n"), -1, int(starts[k]), "fewer values", path)
    two = header + b"".join(lines[:100] + [b"1 2 x 4\n"] + lines[101:600] + [b"1 2\n"] + lines[601:])
    expect_error(reg, two, -1, int(starts[100]), "not a number", path)          # the earliest of two bad lines wins
    for tok in (b"0x10", b"1e", b"nan(1)", b"1,5", b"1f"):
        expect_error(reg, with_line(500, b"  1 2 3 " + tok + b"\n"), -1, int(starts[500]) + 2, "not a number")
    expect_error(reg, with_line(300, lines[300][:-1] + b" " * (1025 - len(lines[300]) + 1) + b"\n"), -1, int(starts[300]), "longer than", path)
    expect_error(reg, header + b"".join(lines[:999]), -1, None, "point lines", path)    # too few lines
    expect_error(reg, header + b"".join(lines[:999]) + b"\n \n", -1, None, "point lines", path)
    expect_error(reg, good.replace(b"DATA ascii", b"DATA binary_compressed"), -6, None, "binary_compressed", path)
    expect_error(reg, good.replace(b"SIZE 4 4 4 4", b"SIZE 8 8 8 4"), -6, None, "4-byte float", path)
    reg.pcdReadPieceBytes(1 << 26)
    # capacity too small
    lay, n, out = reg._layout(*XYZI), C.c_size_t(777), np.full((999, 32), 0xA5, np.uint8)
    assert reg._lib.lsr_decode_pcd(reg._h, good, len(good), 0, C.c_void_p(out.ctypes.data), 999, C.byref(lay), 0, C.byref(n)) == -1
    assert b"too small" in reg._lib.lsr_last_error() and n.value == 777 and (out == 0xA5).all()
    # a missing file
    assert reg._lib.lsr_load_pcd(reg._h, os.fsencode(tmp_path / "none.pcd"), C.c_void_p(out.ctypes.data), 999, C.byref(lay), 0, C.byref(n)) == -9
    assert b"none.pcd" in reg._lib.lsr_last_error() and n.value == 777
    assert reg._lib.lsr_set_input_target_pcd(reg._h, os.fsencode(tmp_path / "none.pcd"), C.byref(n)) == -9 and n.value == 777
    # and the good file still reads
    assert (reg.decodePCD(good) == R.decode(good)).all()


def test_binary_bodies(reg, tmp_path):
    rng = np.random.default_rng(960)
    n = 777
    cols = {k: rng.integers(0, 256, (n, 4), dtype=np.uint8) for k in ("x", "y", "z", "intensity")}
    cols["x"][:5] = np.array([0x7fa5a5a5, 0xffc00001, 0x7f800001, 0xff800000, 0x80000000], np.uint32).view(np.uint8).reshape(5, 4)   # NaN payloads
    cases = [(["x", "y", "z", "_", "intensity", "_"], [4, 4, 4, 1, 4, 1], ["F", "F", "F", "U", "F", "U"], [1, 1, 1, 4, 1, 12]),   # 32-byte XYZI with padding
             (["x", "y", "z", "_"], [4, 4, 4, 1], ["F", "F", "F", "U"], [1, 1, 1, 4]),                                           # 16-byte xyz
             (["rgb", "x", "y", "z", "intensity"], [4, 4, 4, 4, 4], ["U", "F", "F", "F", "F"], [1, 1, 1, 1, 1]),                 # a leading uint32
             (["x", "label", "y", "z"], [4, 1, 4, 4], ["F", "U", "F", "F"], [1, 3, 1, 1])]                                       # unaligned fields
    reg.pcdReadPieceBytes(2048)
    seen = set()
    for fields, sizes, types, counts in cases:
        for pad in range(4):                                      # the body starts at offsets = 0, 1, 2, 3 mod 4
            img = R.binary_file(fields, sizes, types, counts, cols, n, pad)
            seen.add((sum(s * c for s, c in zip(sizes, counts)), R.parse_header(img)["data_offset"] % 4))
            for layout in (XYZI, L16_XYZ):
                want = R.decode(img, layout)
                assert (reg.decodePCD(img, layout) == want).all()
                assert (_np(reg.decodePCD(_cuda(img), layout)) == want).all()
            path = tmp_path / "b.pcd"
            path.write_bytes(img + b"trailing bytes are ignored")
            assert (reg.loadPCDFile(path) == R.decode(img)).all()
            if "intensity" in fields:
                got = R.decode(img).view(np.uint32)
                assert (got[:, 0] == cols["x"].view(np.uint32).reshape(-1)).all() and (got[:, 4] == cols["intensity"].view(np.uint32).reshape(-1)).all()
    assert seen == {(s, a) for s in (32, 16, 20, 15) for a in range(4)}
    img = R.binary_file(*cases[0], cols, n)
    expect_error(reg, img[:-1], -1, None, "shorter than", tmp_path / "short.pcd")      # a truncated body
    reg.pcdReadPieceBytes(1 << 26)


def test_target_from_a_file(reg, tmp_path):
    """MapArray.save_map, then setInputTargetPCD(path) on a fresh object against setInputTarget of the oracle-decoded records on
    another: the same voxel grid, the same registration."""
    case = synth.small_case(n_source=1500, n_keyframes=3)
    rng = np.random.default_rng(970)
    ma = MapArray()
    cloud = synth.as_pointxyzi(case.target[:2100])
    cloud[:, 4] = rng.uniform(0, 255, len(cloud)).astype(np.float32)
    for part in np.array_split(cloud, 3):
        ma.append(part, np.eye(4), 1.0)
    path = tmp_path / "map.pcd"
    ma.save_map(reg, path)
    want = R.decode(path.read_bytes())
    assert len(want) == len(cloud)
    source = synth.as_pointxyzi(case.source)

    def run(cls, from_file):
        r = cls(device=0)
        if cls is NormalDistributionsTransform:
            r.setResolution(3.0)
            r.setTransformationEpsilon(0.01)
        if from_file:
            assert r.setInputTargetPCD(path) == len(want) and r.pcdUnresolvedTokens() == 0
        else:
            r.setInputTarget(want.view(np.float32).reshape(-1, 8))
        dump = r.gridDump() if cls is NormalDistributionsTransform else None
        r.setInputSource(source)
        r.align(case.guess)
        return dump, np.asarray(r.getFinalTransformation()).copy(), r.getFinalNumIteration() if cls is NormalDistributionsTransform else None

    a, b = run(NormalDistributionsTransform, True), run(NormalDistributionsTransform, False)
    for key in ("idx", "n", "mean", "icov"):
        assert np.array_equal(a[0][key], b[0][key]), key
    assert np.array_equal(a[1], b[1]) and a[2] == b[2] and a[2] > 0
    a, b = run(GeneralizedIterativeClosestPoint, True), run(GeneralizedIterativeClosestPoint, False)
    assert np.array_equal(a[1], b[1])
    # the loaded records themselves, resident
    assert (_np(reg.loadPCDFile(path, device=True)) == want).all()
