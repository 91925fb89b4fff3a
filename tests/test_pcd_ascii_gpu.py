"""map.pcd from the device (lsr_format_pcd_ascii, lsr_save_pcd_ascii, lsr_save_map_pcd_ascii): the bytes
pcl::io::savePCDFileASCII writes, formatted in HBM, against the Python restatement tests/pcd_numpy.py.  Every comparison is on the raw
bytes: there is no tolerance.  The shapes are the smallest at which the kernels can go wrong: around the wave (64) and the workgroup
(256), more than one workgroup, the shortest and the longest workgroup image, every alignment of a workgroup's text — and one text
past 2^32 bytes, the only size at which a 32-bit offset would show."""
import ctypes as C
import os

import numpy as np
import pytest

import map_numpy
import pcd_numpy
from pcd_numpy import XYZI, pcd_ascii_bytes
from lidarslam_ros2_amd import MapArray, NormalDistributionsTransform, SubMap, _capi, synth

pytestmark = pytest.mark.gpu

L16_XYZ = (16, (0, 4, 8, None))     # 16-byte records, no intensity: the x y z header
L16_XYZI = (16, (0, 4, 8, 12))      # packed x y z intensity
L32_PERM = (32, (20, 0, 28, 8))     # the fields at permuted offsets of a 32-byte record


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(t) -> bytes:
    return (t.cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)).tobytes()


@pytest.fixture(scope="module")
def reg():
    return NormalDistributionsTransform(device=0)


@pytest.fixture(scope="module")
def case4099():
    """4099 random records (17 workgroups, the last of three records) and their file; shared, never modified."""
    rec = pcd_numpy.random_records(np.random.default_rng(701), 4099)
    return rec, pcd_ascii_bytes(rec)


def test_specials_and_anchors_in_every_field(reg):
    bits = pcd_numpy.table_bits()
    rec = np.zeros((len(bits), 8), np.float32)
    for k, col in enumerate((0, 1, 2, 4)):
        rec.view(np.uint32)[:, col] = np.roll(bits, -k)   # value i is field k of record i - k: every value in each of the four fields
    want = pcd_ascii_bytes(rec)
    for value, text in pcd_numpy.ANCHORS:
        assert pcd_numpy.field_text(value) == text
    assert want.split(b"DATA ascii\n")[1].startswith(b"1234567.2 1234567.8 0.1 99999992\n1234567.8 0.1 99999992 1e+08\n")
    assert _bytes(reg.formatPCDASCII(_cuda(rec))) == want
    assert _bytes(reg.formatPCDASCII(rec)) == want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_random_records(reg, n):
    rec = pcd_numpy.random_records(np.random.default_rng(700 + n), n)
    want = pcd_ascii_bytes(rec)
    lens = [len(l) + 1 for l in want.split(b"DATA ascii\n")[1].splitlines()]
    assert min(lens) >= 8 and max(lens) <= _capi.PCD_ASCII_MAX_LINE_BYTES
    assert _bytes(reg.formatPCDASCII(_cuda(rec))) == want


def test_shortest_and_longest_workgroup_image(reg):
    zeros = np.zeros((257, 8), np.float32)
    want = pcd_ascii_bytes(zeros)
    assert want.endswith(b"0 0 0 0\n") and len(want) == len(pcd_numpy.header(257)) + 257 * 8
    assert _bytes(reg.formatPCDASCII(_cuda(zeros))) == want
    longest = np.full((257, 8), -np.uint32(pcd_numpy.FLT_MIN).view(np.float32), np.float32)
    want = pcd_ascii_bytes(longest)
    assert len(want) == len(pcd_numpy.header(257)) + 257 * _capi.PCD_ASCII_MAX_LINE_BYTES
    assert _bytes(reg.formatPCDASCII(_cuda(longest))) == want


@pytest.mark.parametrize("layout", [XYZI, L16_XYZ, L16_XYZI, L32_PERM], ids=["xyzi32", "xyz16", "xyzi16", "permuted32"])
def test_layouts(reg, layout):
    rec = pcd_numpy.random_records(np.random.default_rng(710), 515, layout[0])
    want = pcd_ascii_bytes(rec, layout)
    assert (b"FIELDS x y z\n" in want) == (layout[1][3] is None)
    assert _bytes(reg.formatPCDASCII(_cuda(rec), layout)) == want
    assert _bytes(reg.formatPCDASCII(rec, layout)) == want


def test_residency_size_query_and_capacity(reg, case4099):
    import torch

    rec, want = case4099
    d_rec = _cuda(rec)
    lay = reg._layout(*XYZI)
    size = C.c_size_t(12345)
    for data, dev in ((C.c_void_p(rec.ctypes.data), 0), (C.c_void_p(d_rec.data_ptr()), 1)):
        # out_text == NULL: the size alone
        assert reg._lib.lsr_format_pcd_ascii(reg._h, data, len(rec), C.byref(lay), dev, None, 0, 0, C.byref(size)) == 0
        assert size.value == len(want)
        # host and device output, the device one at every alignment of its first byte
        out = np.full(len(want) + 8, 0xA5, np.uint8)
        assert reg._lib.lsr_format_pcd_ascii(reg._h, data, len(rec), C.byref(lay), dev, C.c_void_p(out.ctypes.data), len(want), 0, C.byref(size)) == 0
        assert out[: len(want)].tobytes() == want and np.all(out[len(want):] == 0xA5)
        for shift in range(4):
            d_out = torch.full((len(want) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            got = reg.formatPCDASCII(d_rec if dev else rec, XYZI, out=d_out[shift: shift + len(want)])
            assert got.is_cuda and _bytes(got) == want
            rest = d_out.cpu().numpy()
            assert np.all(rest[:shift] == 0xA5) and np.all(rest[shift + len(want):] == 0xA5)
        # one byte short: refused, nothing written, *n_bytes untouched
        size.value = 777
        out[:] = 0x5A
        st = reg._lib.lsr_format_pcd_ascii(reg._h, data, len(rec), C.byref(lay), dev, C.c_void_p(out.ctypes.data), len(want) - 1, 0, C.byref(size))
        assert st == -1 and size.value == 777 and np.all(out == 0x5A)
        d_out = torch.full((len(want),), 0x5A, dtype=torch.uint8, device="cuda")
        st = reg._lib.lsr_format_pcd_ascii(reg._h, data, len(rec), C.byref(lay), dev, C.c_void_p(d_out.data_ptr()), len(want) - 1, 1, C.byref(size))
        assert st == -1 and size.value == 777 and bool((d_out == 0x5A).all())
    # an empty cloud is refused, as PCL refuses it
    st = reg._lib.lsr_format_pcd_ascii(reg._h, C.c_void_p(rec.ctypes.data), 0, C.byref(lay), 0, None, 0, 0, C.byref(size))
    assert st == -1 and size.value == 777


def test_save_file_piece_sizes(reg, case4099, tmp_path):
    rec, want = case4099
    default = reg.pcdPieceRecords()
    assert default == 1 << 20
    files = []
    try:
        for piece, data in ((64, rec), (1000, _cuda(rec)), (default, rec), (1000, rec), (64, _cuda(rec))):
            assert reg.pcdPieceRecords(piece) == piece
            path = tmp_path / f"map_{len(files)}.pcd"
            assert reg.savePCDFileASCII(path, data) == len(want)
            files.append(path.read_bytes())
        # the same call twice
        path = tmp_path / "again.pcd"
        assert reg.savePCDFileASCII(path, rec) == len(want)
        first = path.read_bytes()
        assert reg.savePCDFileASCII(path, rec) == len(want)
        assert path.read_bytes() == first == want
        with pytest.raises(_capi.RegistrationError):
            reg.pcdPieceRecords(63)
        with pytest.raises(_capi.RegistrationError):
            reg.pcdPieceRecords((1 << 22) + 1)
    finally:
        reg.pcdPieceRecords(default)
    assert all(f == want for f in files)
    assert _bytes(reg.formatPCDASCII(rec)) == want
    # a directory that does not exist: LSR_ERR_IO, errno's text, no file
    missing = tmp_path / "no_such_directory" / "map.pcd"
    with pytest.raises(_capi.RegistrationError) as e:
        reg.savePCDFileASCII(missing, rec)
    assert e.value.status == _capi.ERR_IO == -9 and os.strerror(2) in str(e.value)
    assert not missing.exists() and not missing.parent.exists()


def test_five_pieces_the_last_partial(reg, tmp_path):
    rec = pcd_numpy.random_records(np.random.default_rng(720), 300000)
    want = pcd_ascii_bytes(rec)
    try:
        reg.pcdPieceRecords(65536)
        path = tmp_path / "mid.pcd"
        assert reg.savePCDFileASCII(path, _cuda(rec)) == len(want)
        assert path.read_bytes() == want
    finally:
        reg.pcdPieceRecords(1 << 20)


def test_text_past_four_gigabytes(reg):
    """72 000 000 packed records of -FLT_MIN in every field, 60-byte lines: 4.32 GB of text, past 2^32 — the workgroup offsets are 64-bit
    from the scan on.  Three records of other lengths (first, middle, last) keep the lines from falling on multiples of 60.  Checked
    on the device, run by run, against the one line."""
    import torch

    n, mid = 72_000_000, 36_000_001
    rec = torch.full((n, 4), float(-np.uint32(pcd_numpy.FLT_MIN).view(np.float32)), dtype=torch.float32, device="cuda")
    rec[0], rec[mid], rec[n - 1] = 0.0, 1.5, 2.0
    text = reg.formatPCDASCII(rec, L16_XYZI)
    head = pcd_numpy.header(n)
    first, middle, last, line = b"0 0 0 0\n", b"1.5 1.5 1.5 1.5\n", b"2 2 2 2\n", b" ".join([b"-1.1754944e-38"] * 4) + b"\n"
    assert len(line) == 60
    size = len(head) + len(first) + len(middle) + len(last) + (n - 3) * 60
    assert size > 2 ** 32 and text.is_cuda and text.numel() == size
    at = 0
    for piece in (head, first):
        assert _bytes(text[at: at + len(piece)]) == piece
        at += len(piece)
    d_line = torch.frombuffer(bytearray(line), dtype=torch.uint8).cuda()
    for count, after in ((mid - 1, middle), (n - 2 - mid, last)):
        run = text[at: at + 60 * count].view(count, 60)
        assert bool((run == d_line).all())
        at += 60 * count
        assert _bytes(text[at: at + len(after)]) == after
        at += len(after)
    assert at == size


def _pose(rng):
    q = rng.normal(size=4)
    return tuple(rng.uniform(-200.0, 200.0, 3)), tuple(q / np.linalg.norm(q))


def test_save_map(reg, tmp_path):
    rng = np.random.default_rng(730)
    sizes = [0, 1, 300, 64, 1000]
    ma_host, ma_dev = MapArray(), MapArray()
    for n in sizes:
        rec = rng.uniform(-60.0, 60.0, (n, 8)).astype(np.float32)
        position, orientation = _pose(rng)
        for ma, cloud in ((ma_host, rec), (ma_dev, _cuda(rec))):
            ma.submaps.append(SubMap(cloud, position, orientation, 0.0))
    given = []
    for _ in sizes:
        position, orientation = _pose(rng)
        given.append(map_numpy.pose_matrix(position, orientation))
    for poses in (None, given):
        records, _ = map_numpy.assemble_map(ma_host.submaps, poses)
        want = pcd_ascii_bytes(records)
        for name, ma in (("host", ma_host), ("device", ma_dev)):
            path = tmp_path / f"{name}_{poses is not None}.pcd"
            assert ma.save_map(reg, path, poses) == len(want)
            assert path.read_bytes() == want
            # ... and what lsr_assemble_map followed by lsr_save_pcd_ascii writes
            assembled, _ = reg.assembleMap(ma.submaps, poses)
            two = tmp_path / "two_calls.pcd"
            assert reg.savePCDFileASCII(two, assembled) == len(want)
            assert two.read_bytes() == want
    empty = MapArray()
    empty.submaps.append(SubMap(np.zeros((0, 8), np.float32), (0, 0, 0), (0, 0, 0, 1), 0.0))
    with pytest.raises(_capi.RegistrationError) as e:
        empty.save_map(reg, tmp_path / "empty.pcd")
    assert e.value.status == -1 and not (tmp_path / "empty.pcd").exists()


def test_a_save_leaves_the_registration_as_it_was(tmp_path):
    case = synth.small_case(n_source=2000, n_keyframes=2)
    ndt = NormalDistributionsTransform(device=0)
    ndt.setResolution(3.0)
    ndt.setInputTarget(synth.as_pointxyzi(case.target))
    ndt.setInputSource(synth.as_pointxyzi(case.source))
    ndt.align(case.guess)
    T, fit = ndt.getFinalTransformation().copy(), ndt.getFitnessScore()
    rec = pcd_numpy.random_records(np.random.default_rng(740), 700)
    want = pcd_ascii_bytes(rec)
    assert ndt.savePCDFileASCII(tmp_path / "a.pcd", rec) == len(want)
    assert _bytes(ndt.formatPCDASCII(_cuda(rec))) == want
    ma = MapArray()
    ma.submaps.append(SubMap(rec, (1.0, 2.0, 3.0), (0.0, 0.0, 0.0, 1.0), 0.0))
    ma.save_map(ndt, tmp_path / "b.pcd")
    assert np.array_equal(ndt.getFinalTransformation(), T)
    assert np.array_equal(np.float64(ndt.getFitnessScore()), np.float64(fit))
    assert (tmp_path / "a.pcd").read_bytes() == want
