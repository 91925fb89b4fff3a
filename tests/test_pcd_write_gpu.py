"""map.pcd as DATA binary and DATA binary_compressed from the device (lsr_format_pcd, lsr_save_pcd, lsr_save_map_pcd, lsr_lzf_deflate;
csrc/pcd_deflate.hip) against the host restatement tests/pcd_write_numpy.py.  Every comparison is on the raw bytes: there is no
tolerance — the stream is a function of the image alone.  The shapes are the smallest at which the kernels can go wrong: around the wave
and the workgroup for the gather kernels; field blocks that end just before, on and just after a chunk boundary (1023, 1024, 1025
points) and chunks that straddle fields (4099) for the compressor; one map of more chunks than the device has compute units."""
import ctypes as C
import os

import numpy as np
import pytest

import map_numpy
import pcd_numpy
import pcd_write_numpy as W
from pcd_numpy import XYZI, pcd_ascii_bytes
from lidarslam_ros2_amd import MapArray, NormalDistributionsTransform, SubMap, _capi, synth

pytestmark = pytest.mark.gpu

L16_XYZ = (16, (0, 4, 8, None))
L16_XYZI = (16, (0, 4, 8, 12))
L32_PERM = (32, (20, 0, 28, 8))
LAYOUTS = {"xyzi32": XYZI, "xyz16": L16_XYZ, "xyzi16": L16_XYZI, "permuted32": L32_PERM}
KINDS = ("binary", "binary_compressed")
RESTATEMENT = {"binary": W.binary_file, "binary_compressed": W.compressed_file, "ascii": pcd_ascii_bytes}


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(t) -> bytes:
    return (t.cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)).tobytes()


def _fields_of(rec, layout) -> np.ndarray:
    """(n, point_step) uint8: the records with every byte outside the layout's fields zero — what the readers return."""
    step, offs = layout
    rec = np.ascontiguousarray(rec).view(np.uint8).reshape(-1, step)
    want = np.zeros_like(rec)
    for o in offs:
        if o is not None:
            want[:, o:o + 4] = rec[:, o:o + 4]
    return want


@pytest.fixture(scope="module")
def reg():
    r = NormalDistributionsTransform(device=0)
    r.pcdReadCompressed(True)
    return r


@pytest.fixture(scope="module")
def case4099():
    """4099 grid-map records and their three images; shared, never modified."""
    rec = W.grid_map(4099, 900)
    return rec, {kind: RESTATEMENT[kind](rec) for kind in ("ascii",) + KINDS}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_gather_kernels(reg, n):
    rng = np.random.default_rng(900 + n)
    for name, layout in LAYOUTS.items():
        rec = rng.integers(0, 256, (n, layout[0]), dtype=np.uint8)        # any bits: NaNs of every payload among them
        for kind in KINDS:
            want = RESTATEMENT[kind](rec, layout)
            assert _bytes(reg.formatPCD(rec, layout, kind)) == want, (name, kind, "host")
            got = reg.formatPCD(_cuda(rec), layout, kind)
            assert got.is_cuda and _bytes(got) == want, (name, kind, "device")


def _contents(n, what, seed):
    if what == "zeros":
        return np.zeros((n, 8), np.float32)
    if what == "grid":
        return W.grid_map(n, seed)
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8).view(np.float32)


@pytest.mark.parametrize("what", ["zeros", "grid", "random"])
@pytest.mark.parametrize("n", [1023, 1024, 1025, 4099])
def test_compressor_at_the_chunk_boundaries(reg, n, what):
    import torch

    rec = _contents(n, what, 910 + n)
    for layout in (XYZI, L16_XYZ):           # images of 16 n and of 12 n bytes
        r = rec.view(np.uint8).reshape(n, 32)[:, :layout[0]].copy()
        want = W.compressed_file(r, layout)
        assert _bytes(reg.formatPCD(r, layout, "binary_compressed")) == want
        d_rec = _cuda(r)
        assert _bytes(reg.formatPCD(d_rec, layout, "binary_compressed")) == want
        # host records into a device buffer and device records into a host buffer, the device one at every alignment
        out = np.full(len(want) + 8, 0xA5, np.uint8)
        got = reg.formatPCD(d_rec, layout, "binary_compressed", out=out)
        assert _bytes(got) == want and np.all(out[len(want):] == 0xA5)
        for shift in range(4):
            d_out = torch.full((len(want) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            got = reg.formatPCD(r, layout, "binary_compressed", out=d_out[shift: shift + len(want)])
            assert got.is_cuda and _bytes(got) == want
            rest = d_out.cpu().numpy()
            assert np.all(rest[:shift] == 0xA5) and np.all(rest[shift + len(want):] == 0xA5)
    if what == "zeros":     # one literal, then overlapping distance-1 references at the 264 cap
        body = want[want.index(b"DATA binary_compressed\n") + 23 + 8:]
        assert body[:2] == b"\x00\x00" and body[2:5] == bytes([7 << 5, 255, 0]) and len(body) < 12 * n / 32


def test_constructed_images(reg):
    """Each image places one case of the rule (tests/test_pcd_write_cpu.py checks which tokens they make): the compressor alone."""
    import torch

    for name, image in W.constructed_images().items():
        want = W.deflate(image)
        assert _bytes(reg.lzfDeflate(image)) == want, name
        got = reg.lzfDeflate(_cuda(np.frombuffer(image, np.uint8).copy()))
        assert got.is_cuda and _bytes(got) == want, name
        # an image that does not start on a word boundary
        d = torch.zeros(len(image) + 3, dtype=torch.uint8, device="cuda")
        d[3:] = _cuda(np.frombuffer(image, np.uint8).copy())
        assert _bytes(reg.lzfDeflate(d[3:])) == want, name
    for image in (b"\x07", b"\x07\x07", b"abc", b"aaaa"):
        assert _bytes(reg.lzfDeflate(image)) == W.deflate(image)
    # ... and as a cloud, where the image's length allows it
    image = W.constructed_images()["period_3_across_chunks"][:16 * 560]
    rec = W.records_of_image(image)
    assert W.field_major_image(rec, L16_XYZI) == image
    assert _bytes(reg.formatPCD(rec, L16_XYZI, "binary_compressed")) == W.compressed_file(rec, L16_XYZI)


@pytest.mark.parametrize("layout", list(LAYOUTS.values()), ids=list(LAYOUTS))
def test_specials_are_copied_bit_for_bit_and_read_back(reg, layout, tmp_path):
    step = layout[0]
    rec = W.special_records(515).view(np.uint8).reshape(-1, 32)[:, :step].copy()
    want_fields = _fields_of(rec, layout)
    for kind in KINDS:
        want = RESTATEMENT[kind](rec, layout)
        img = reg.formatPCD(rec, layout, kind)
        assert _bytes(img) == want, kind
        assert np.array_equal(reg.decodePCD(img, layout), want_fields), kind
        d_img = reg.formatPCD(_cuda(rec), layout, kind)
        assert np.array_equal(reg.decodePCD(d_img, layout).cpu().numpy(), want_fields), kind
        path = tmp_path / f"{kind}.pcd"
        assert reg.savePCDFile(path, rec, layout, kind) == len(want) and path.read_bytes() == want
        assert np.array_equal(reg.loadPCDFile(path, layout), want_fields), kind
        # the points are the same whatever layout they were written from
        assert np.array_equal(reg.loadPCDFile(path, XYZI), _fields_of(_as_xyzi(rec, layout), XYZI))


def _as_xyzi(rec, layout) -> np.ndarray:
    out = np.zeros((len(rec), 32), np.uint8)
    for o_in, o_out in zip(layout[1], XYZI[1]):
        if o_in is not None:
            out[:, o_out:o_out + 4] = rec[:, o_in:o_in + 4]
    return out


def test_round_trip_of_every_kind_of_content(reg, tmp_path):
    for what in ("zeros", "grid", "random"):
        rec = _contents(4099, what, 920)
        for kind in KINDS:
            img = reg.formatPCD(_cuda(rec), XYZI, kind)
            assert np.array_equal(reg.decodePCD(img).cpu().numpy(), _fields_of(rec, XYZI)), (what, kind)
            path = tmp_path / f"{what}_{kind}.pcd"
            reg.savePCDFile(path, rec, XYZI, kind)
            assert np.array_equal(reg.loadPCDFile(path), _fields_of(rec, XYZI)), (what, kind)


def test_a_map_of_more_chunks_than_compute_units(reg, tmp_path):
    """70 001 points: 274 chunks, 69 pieces of 1024 records (a compressed stream: as many bytes a piece)."""
    rec = W.grid_map(70001, 930)
    want = {kind: RESTATEMENT[kind](rec) for kind in KINDS}
    try:
        reg.pcdPieceRecords(1024)
        for kind in KINDS:
            path = tmp_path / f"{kind}.pcd"
            assert reg.savePCDFile(path, _cuda(rec), XYZI, kind) == len(want[kind])
            assert path.read_bytes() == want[kind], kind
            assert np.array_equal(reg.loadPCDFile(path), _fields_of(rec, XYZI)), kind
    finally:
        reg.pcdPieceRecords(1 << 20)
    assert len(want["binary_compressed"]) < 0.95 * len(want["binary"])       # (0.90 on this map: the intensity block shrinks)


def test_target_from_a_saved_compressed_map(tmp_path):
    case = synth.small_case(n_source=1500, n_keyframes=3)
    cloud = synth.as_pointxyzi(case.target[:2100])
    cloud[:, 4] = np.random.default_rng(940).uniform(0, 255, len(cloud)).astype(np.float32)
    a, b = NormalDistributionsTransform(device=0), NormalDistributionsTransform(device=0)
    for r in (a, b):
        r.setResolution(3.0)
    a.savePCDFile(tmp_path / "map.pcd", cloud, XYZI, "binary_compressed")
    a.pcdReadCompressed(True)
    assert a.setInputTargetPCD(tmp_path / "map.pcd") == len(cloud)
    b.setInputTarget(cloud)
    ia, ib = a.gridInfo(), b.gridInfo()
    assert ia["n_leaves"] == ib["n_leaves"] > 10 and ia["n_valid"] == ib["n_valid"]
    assert np.array_equal(ia["min_b"], ib["min_b"]) and np.array_equal(ia["max_b"], ib["max_b"])
    da, db = a.gridDump(), b.gridDump()
    for key in ("idx", "n", "mean", "icov"):
        assert np.array_equal(da[key], db[key]), key


def test_save_file_piece_sizes_and_kinds(reg, case4099, tmp_path):
    rec, want = case4099
    default = reg.pcdPieceRecords()
    assert default == 1 << 20
    try:
        for kind in KINDS:
            assert _bytes(reg.formatPCD(rec, XYZI, kind)) == want[kind]
            for k, (piece, data) in enumerate(((64, rec), (default, _cuda(rec)), (1000, rec), (64, _cuda(rec)), (default, rec))):
                assert reg.pcdPieceRecords(piece) == piece
                path = tmp_path / f"{kind}_{k}.pcd"
                assert reg.savePCDFile(path, data, XYZI, kind) == len(want[kind])
                assert path.read_bytes() == want[kind], (kind, piece)
        # "ascii" through the new entries: the old entries' bytes
        assert _bytes(reg.formatPCD(rec, XYZI, "ascii")) == want["ascii"] == _bytes(reg.formatPCDASCII(rec))
        assert _bytes(reg.formatPCD(_cuda(rec), XYZI, "ascii")) == want["ascii"]
        for piece in (64, default):
            reg.pcdPieceRecords(piece)
            assert reg.savePCDFile(tmp_path / "new.pcd", rec, XYZI, "ascii") == reg.savePCDFileASCII(tmp_path / "old.pcd", rec) == len(want["ascii"])
            assert (tmp_path / "new.pcd").read_bytes() == (tmp_path / "old.pcd").read_bytes() == want["ascii"]
        assert reg.savePCDFile(tmp_path / "default.pcd", rec) == len(want["ascii"])       # ASCII stays the default
    finally:
        reg.pcdPieceRecords(default)


def _pose(rng):
    q = rng.normal(size=4)
    return tuple(rng.uniform(-200.0, 200.0, 3)), tuple(q / np.linalg.norm(q))


def test_save_map(reg, tmp_path):
    rng = np.random.default_rng(950)
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
        for kind in ("ascii",) + KINDS:
            want = RESTATEMENT[kind](records)
            for name, ma in (("host", ma_host), ("device", ma_dev)):
                path = tmp_path / f"{name}_{kind}_{poses is not None}.pcd"
                assert ma.save_map(reg, path, poses, kind) == len(want)
                assert path.read_bytes() == want, (kind, name)
                assert reg.saveMapPCDFile(path, ma.submaps, poses, ma.layout, kind) == len(want) and path.read_bytes() == want
                # ... and what lsr_assemble_map followed by lsr_save_pcd writes
                assembled, _ = reg.assembleMap(ma.submaps, poses)
                two = tmp_path / "two_calls.pcd"
                assert reg.savePCDFile(two, assembled, XYZI, kind) == len(want)
                assert two.read_bytes() == want
    assert ma_host.save_map(reg, tmp_path / "default.pcd") == len(pcd_ascii_bytes(map_numpy.assemble_map(ma_host.submaps, None)[0]))
    empty = MapArray()
    empty.submaps.append(SubMap(np.zeros((0, 8), np.float32), (0, 0, 0), (0, 0, 0, 1), 0.0))
    for kind in KINDS:
        with pytest.raises(_capi.RegistrationError) as e:
            empty.save_map(reg, tmp_path / "empty.pcd", None, kind)
        assert e.value.status == -1 and not (tmp_path / "empty.pcd").exists()


def test_repeatability_and_the_profiling_key(case4099, tmp_path):
    rec, want = case4099
    a, b = NormalDistributionsTransform(device=0), NormalDistributionsTransform(device=0)
    for kind in KINDS:      # the same call twice, and another object: the same bytes
        first = _bytes(a.formatPCD(rec, XYZI, kind))
        assert first == _bytes(a.formatPCD(rec, XYZI, kind)) == _bytes(b.formatPCD(_cuda(rec), XYZI, kind)) == want[kind]
    assert a.pcdDeflateMs() == 0.0                                  # without LSR_PROFILE
    a.setProfiling(True)
    a.formatPCD(rec, XYZI, "binary_compressed")
    assert a.pcdDeflateMs() > 0.0
    a.formatPCD(rec, XYZI, "binary")
    assert a.pcdDeflateMs() == 0.0                                  # the last call's: a binary image
    assert a.savePCDFile(tmp_path / "c.pcd", _cuda(rec), XYZI, "binary_compressed") == len(want["binary_compressed"])
    assert a.pcdDeflateMs() > 0.0
    a.savePCDFile(tmp_path / "a.pcd", rec, XYZI, "ascii")
    assert a.pcdDeflateMs() == 0.0 and a._getf(_capi.PCD_FORMAT_MS) > 0.0
    a.lzfDeflate(W.field_major_image(rec))
    assert a.pcdDeflateMs() > 0.0
    a.setProfiling(False)
    a.formatPCD(rec, XYZI, "binary_compressed")
    assert a.pcdDeflateMs() == 0.0
    assert (tmp_path / "c.pcd").read_bytes() == want["binary_compressed"]


def test_a_save_leaves_the_registration_as_it_was(tmp_path):
    case = synth.small_case(n_source=2000, n_keyframes=2)
    ndt = NormalDistributionsTransform(device=0)
    ndt.setResolution(3.0)
    ndt.setInputTarget(synth.as_pointxyzi(case.target))
    ndt.setInputSource(synth.as_pointxyzi(case.source))
    ndt.align(case.guess)
    T, fit = ndt.getFinalTransformation().copy(), ndt.getFitnessScore()
    rec = W.grid_map(700, 960)
    for kind in KINDS:
        want = RESTATEMENT[kind](rec)
        assert ndt.savePCDFile(tmp_path / "a.pcd", rec, XYZI, kind) == len(want)
        assert _bytes(ndt.formatPCD(_cuda(rec), XYZI, kind)) == want
        ma = MapArray()
        ma.submaps.append(SubMap(rec, (1.0, 2.0, 3.0), (0.0, 0.0, 0.0, 1.0), 0.0))
        ma.save_map(ndt, tmp_path / "b.pcd", None, kind)
    assert np.array_equal(ndt.getFinalTransformation(), T)
    assert np.array_equal(np.float64(ndt.getFitnessScore()), np.float64(fit))


def test_errors_touch_nothing(reg, case4099, tmp_path):
    import torch

    rec, want = case4099
    d_rec = _cuda(rec)
    lay = reg._layout(*XYZI)
    lib, h = reg._lib, reg._h
    size = C.c_size_t(777)
    out = np.full(len(want["binary"]) + 8, 0xA5, np.uint8)
    d_out = torch.full((len(want["binary"]) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    optr, d_optr = C.c_void_p(out.ctypes.data), C.c_void_p(d_out.data_ptr())
    target = tmp_path / "never.pcd"
    path = os.fsencode(target)

    def untouched():
        return size.value == 777 and np.all(out == 0xA5) and bool((d_out == 0xA5).all()) and not target.exists()

    for data, dev in ((C.c_void_p(rec.ctypes.data), 0), (C.c_void_p(d_rec.data_ptr()), 1)):
        # an unknown kind
        for kind in (-1, 3, 99):
            assert lib.lsr_format_pcd(h, data, len(rec), C.byref(lay), dev, kind, optr, out.size, 0, C.byref(size)) == -1
            assert lib.lsr_format_pcd(h, data, len(rec), C.byref(lay), dev, kind, d_optr, out.size, 1, C.byref(size)) == -1
            assert lib.lsr_save_pcd(h, path, data, len(rec), C.byref(lay), dev, kind, C.byref(size)) == -1
            assert b"data_kind" in lib.lsr_last_error() and untouched()
        for kind in (1, 2):
            full = len(want[KINDS[kind - 1]])
            # the size alone
            n_bytes = C.c_size_t(0)
            assert lib.lsr_format_pcd(h, data, len(rec), C.byref(lay), dev, kind, None, 0, 0, C.byref(n_bytes)) == 0 and n_bytes.value == full
            # an empty cloud
            assert lib.lsr_format_pcd(h, data, 0, C.byref(lay), dev, kind, optr, out.size, 0, C.byref(size)) == -1
            assert lib.lsr_save_pcd(h, path, data, 0, C.byref(lay), dev, kind, C.byref(size)) == -1 and untouched()
            # one byte short
            assert lib.lsr_format_pcd(h, data, len(rec), C.byref(lay), dev, kind, optr, full - 1, 0, C.byref(size)) == -1
            assert lib.lsr_format_pcd(h, data, len(rec), C.byref(lay), dev, kind, d_optr, full - 1, 1, C.byref(size)) == -1 and untouched()
            # no path, no data, no count
            assert lib.lsr_save_pcd(h, None, data, len(rec), C.byref(lay), dev, kind, C.byref(size)) == -1
            assert lib.lsr_save_pcd(h, path, None, len(rec), C.byref(lay), dev, kind, C.byref(size)) == -1
            assert lib.lsr_save_pcd(h, path, data, len(rec), C.byref(lay), dev, kind, None) == -1 and untouched()
            # a directory that does not exist: LSR_ERR_IO, errno's text, no file
            missing = tmp_path / "no_such_directory" / "map.pcd"
            assert lib.lsr_save_pcd(h, os.fsencode(missing), data, len(rec), C.byref(lay), dev, kind, C.byref(size)) == _capi.ERR_IO == -9
            assert os.strerror(2).encode() in lib.lsr_last_error() and untouched() and not missing.parent.exists()
            # exactly enough room: written, nothing behind it
            assert lib.lsr_format_pcd(h, data, len(rec), C.byref(lay), dev, kind, optr, full, 0, C.byref(n_bytes)) == 0
            assert out[:full].tobytes() == want[KINDS[kind - 1]] and np.all(out[full:] == 0xA5)
            out[:] = 0xA5
    # the compressor alone
    image = np.frombuffer(W.field_major_image(rec), np.uint8)
    stream = W.deflate(image.tobytes())
    assert lib.lsr_lzf_deflate(h, C.c_void_p(image.ctypes.data), 0, 0, optr, out.size, 0, C.byref(size)) == -1
    assert lib.lsr_lzf_deflate(h, None, image.size, 0, optr, out.size, 0, C.byref(size)) == -1
    assert lib.lsr_lzf_deflate(h, C.c_void_p(image.ctypes.data), image.size, 0, optr, len(stream) - 1, 0, C.byref(size)) == -1
    assert lib.lsr_lzf_deflate(h, C.c_void_p(image.ctypes.data), 2 ** 31, 0, None, 0, 0, C.byref(size)) == _capi.ERR_INDEX_OVERFLOW and untouched()
    # a compressed image of more than 2^31 - 1 bytes is refused before anything runs (the reader's own limit)
    assert lib.lsr_format_pcd(h, C.c_void_p(d_rec.data_ptr()), 2 ** 27, C.byref(lay), 1, 2, None, 0, 0, C.byref(size)) == _capi.ERR_INDEX_OVERFLOW
    assert untouched()
    with pytest.raises(ValueError):
        reg.formatPCD(rec, XYZI, "zip")
