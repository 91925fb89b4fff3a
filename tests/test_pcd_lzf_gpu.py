"""Reading DATA binary_compressed .pcd files on the device (LSR_PCD_READ_COMPRESSED; csrc/pcd_lzf.hip): records in HBM against the Python
restatement tests/pcd_lzf_numpy.py (a literal byte-by-byte lzf_decompress) and against the DATA binary file of the same cloud.  Every
comparison is on raw record bytes: there is no tolerance.  The shapes are the smallest at which the kernels can go wrong: around the wave
(64) and the workgroup (256) of the record pass, streams of one block and of several 4096-byte blocks with a token across every block
boundary at every phase, every reference form, the deepest chain a file of that size can hold."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import pcd_lzf_numpy as Z
import pcd_numpy
import pcd_read_numpy as R
from pcd_numpy import XYZI
from lidarslam_ros2_amd import NormalDistributionsTransform, _capi, synth
from lidarslam_ros2_amd._capi import RegistrationError

pytestmark = pytest.mark.gpu

L16_XYZ = (16, (0, 4, 8, None))
L16_XYZI = (16, (0, 4, 8, 12))
L32_PERM = (32, (20, 0, 28, 8))
LAYOUTS = [XYZI, L16_XYZ, L16_XYZI, L32_PERM]
XYZ_FIELDS = (["x", "y", "z"], [4, 4, 4], ["F", "F", "F"], [1, 1, 1])


def _cuda(a):
    import torch

    return torch.from_numpy(np.frombuffer(a, np.uint8).copy() if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)


@pytest.fixture(scope="module")
def reg():
    r = NormalDistributionsTransform(device=0)
    assert r.pcdReadCompressed() is False and r.pcdReadCompressed(True) is True
    return r


@pytest.fixture(scope="module")
def hand_made():
    return Z.hand_made_streams()


def check_all(reg, img, layout=XYZI, path=None, want=None):
    """decodePCD of a host image and of a device image (and loadPCDFile in 2048-byte pieces) against the oracle; returns its records."""
    if want is None:
        want = Z.decode_compressed(img, layout)
    got = reg.decodePCD(img, layout)
    assert isinstance(got, np.ndarray) and got.shape == want.shape and (got == want).all()
    got = reg.decodePCD(_cuda(img), layout)
    assert got.is_cuda and (_np(got) == want).all()
    if path is not None:
        path.write_bytes(img)
        reg.pcdReadPieceBytes(2048)
        try:
            assert (reg.loadPCDFile(path, layout) == want).all()
        finally:
            reg.pcdReadPieceBytes(1 << 26)
    return want


def call_all(reg, img, path=None, capacity=4200):
    """(how, status, lsr_last_error, records untouched and count untouched) of lsr_decode_pcd on a host and a device image and of
    lsr_load_pcd."""
    lay = reg._layout(*XYZI)
    d_img = _cuda(img)
    out_all = []
    for how in ("host", "device", "file"):
        out = np.full((capacity, 32), 0xA5, np.uint8)
        n = C.c_size_t(777)
        if how == "file":
            if path is None:
                continue
            path.write_bytes(img)
            st = reg._lib.lsr_load_pcd(reg._h, os.fsencode(path), C.c_void_p(out.ctypes.data), len(out), C.byref(lay), 0, C.byref(n))
        else:
            ptr = img if how == "host" else C.c_void_p(d_img.data_ptr())
            st = reg._lib.lsr_decode_pcd(reg._h, ptr, len(img), int(how == "device"), C.c_void_p(out.ctypes.data), len(out), C.byref(lay), 0, C.byref(n))
        out_all.append((how, st, reg._lib.lsr_last_error().decode(), n.value == 777 and bool((out == 0xA5).all())))
    return out_all


def expect_error(reg, img, status, offset=None, word=None, path=None, oracle=True):
    """decode (host and device image) and load refuse `img` with `status`, name `offset` (or no offset at all), touch neither the
    records nor the count — and the oracle refuses it the same way."""
    for how, st, why, untouched in call_all(reg, img, path):
        assert st == status, (how, st, why)
        assert untouched, how
        if offset is not None:
            assert f"byte offset {offset}" in why, (how, why)
        elif status == -1 and oracle:
            assert "byte offset" not in why, (how, why)
        if word is not None:
            assert word in why, (how, why)
    if oracle:
        with pytest.raises(R.PcdError) as e:
            Z.decode_compressed(img)
        assert e.value.status == status and e.value.offset == offset


def test_default_is_unchanged(tmp_path):
    """Without the key a valid compressed image is refused as before, whatever way it comes in."""
    fresh = NormalDistributionsTransform(device=0)
    rec = pcd_numpy.random_records(np.random.default_rng(1000), 300)
    img = Z.compressed_file(*Z.XYZI_FIELDS, Z.xyzi_columns(rec), 300, Z.greedy)
    assert len(Z.decode_compressed(img)) == 300
    assert fresh.pcdReadCompressed() is False
    for how, st, why, untouched in call_all(fresh, img, tmp_path / "c.pcd"):
        assert st == -6 and "binary_compressed" in why and untouched, (how, st, why)
    n = C.c_size_t(777)
    assert fresh._lib.lsr_set_input_target_pcd(fresh._h, os.fsencode(tmp_path / "c.pcd"), C.byref(n)) == -6 and n.value == 777
    with pytest.raises(RegistrationError):
        fresh.decodePCD(img)
    # the key takes 0 and 1 only
    for bad in (2, -1):
        assert fresh._lib.lsr_set_i32(fresh._h, _capi.PCD_READ_COMPRESSED, bad) == -1
    assert fresh.pcdReadCompressed() is False
    assert fresh.pcdReadCompressed(True) is True and (fresh.decodePCD(img) == Z.decode_compressed(img)).all()
    assert fresh.pcdReadCompressed(False) is False
    with pytest.raises(RegistrationError):
        fresh.decodePCD(img)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_sizes_and_encoders(reg, tmp_path, n):
    rng = np.random.default_rng(1100 + n)
    rec = pcd_numpy.random_records(rng, n)
    cols = Z.xyzi_columns(rec)
    binary = R.decode(R.binary_file(*Z.XYZI_FIELDS, cols, n))
    for name, enc in Z.ENCODERS.items():
        img = Z.compressed_file(*Z.XYZI_FIELDS, cols, n, enc, extra=b"bytes behind the stream are ignored")
        want = check_all(reg, img, path=tmp_path / "c.pcd")
        assert (want == binary).all(), name
    # explicit tokens: the cloud is what they inflate to
    stream = Z.from_tokens(Z.random_tokens(rng, 16 * n))
    image = np.frombuffer(Z.lzf_decompress(stream, 16 * n), np.uint8)
    cols = {name: image[4 * n * k: 4 * n * (k + 1)].reshape(n, 4) for k, name in enumerate(("x", "y", "z", "intensity"))}
    want = check_all(reg, Z.xyzi_file_of_stream(stream, n), path=tmp_path / "t.pcd")
    assert (want == R.decode(R.binary_file(*Z.XYZI_FIELDS, cols, n))).all()


@pytest.mark.parametrize("layout", LAYOUTS, ids=["xyzi32", "xyz16", "xyzi16", "permuted32"])
def test_output_layouts_and_the_xyz_header(reg, layout):
    rec = pcd_numpy.random_records(np.random.default_rng(1200), 515)
    cols = Z.xyzi_columns(rec)
    for F in (Z.XYZI_FIELDS, XYZ_FIELDS):
        img = Z.compressed_file(*F, cols, 515, Z.greedy)
        want = check_all(reg, img, layout)
        assert (want == R.decode(R.binary_file(*F, cols, 515), layout)).all()
        if layout == XYZI:
            assert (want.view(np.uint32)[:, [3, 5, 6, 7]] == 0).all()           # every byte outside the fields is zero
            if F is XYZ_FIELDS:
                assert (want.view(np.uint32)[:, 4] == 0).all()                  # no intensity in the file: +0


def test_field_mixes(reg, tmp_path):
    rng = np.random.default_rng(1300)
    n = 777
    cols = {k: rng.integers(0, 256, (n, 4), dtype=np.uint8) for k in ("x", "y", "z", "intensity")}
    cases = [(["x", "y", "z", "_", "intensity", "_"], [4, 4, 4, 1, 4, 1], ["F", "F", "F", "U", "F", "U"], [1, 1, 1, 4, 1, 12]),   # 32-byte XYZI with padding
             (["x", "y", "z", "_"], [4, 4, 4, 1], ["F", "F", "F", "U"], [1, 1, 1, 4]),                                           # 16-byte xyz
             (["rgb", "x", "y", "z", "intensity"], [4, 4, 4, 4, 4], ["U", "F", "F", "F", "F"], [1, 1, 1, 1, 1]),                 # a leading uint32
             (["x", "label", "y", "z"], [4, 1, 4, 4], ["F", "U", "F", "F"], [1, 3, 1, 1])]                                       # unaligned fields
    for fields, sizes, types, counts in cases:
        for pad in range(4):                                      # the stream starts at every offset mod 4
            img = Z.compressed_file(fields, sizes, types, counts, cols, n, Z.greedy, pad)
            twin = R.binary_file(fields, sizes, types, counts, cols, n, pad)
            for layout in (XYZI, L16_XYZ):
                want = check_all(reg, img, layout, tmp_path / "m.pcd" if pad == 1 else None)
                assert (want == R.decode(twin, layout)).all()


def test_hand_made_streams(reg, hand_made, tmp_path):
    assert len(hand_made) == 5 + 32
    for name, stream in hand_made.items():
        img = Z.xyzi_file_of_stream(stream, Z.N_HAND)
        want = Z.decode_compressed(img)
        if name.startswith("first_literal"):                      # 32 phases of the same pattern: the device image alone
            assert (_np(reg.decodePCD(_cuda(img))) == want).all(), name
        else:
            check_all(reg, img, path=tmp_path / "h.pcd", want=want)
        if name.startswith("zeros"):
            assert len(stream) < 800 and not want.any()           # 65584 bytes behind one literal: the chain is as deep as the file


def test_nan_payloads_and_minus_zero(reg):
    bits = np.concatenate([pcd_numpy.special_bits(), np.array([0x7fa5a5a5, 0xffc00001, 0x7f800001, 0xff800000, 0x80000000], np.uint32)])
    n = len(bits)
    rec = np.zeros((n, 8), np.float32)
    for k, col in enumerate((0, 1, 2, 4)):
        rec.view(np.uint32)[:, col] = np.roll(bits, -k)
    for enc in Z.ENCODERS.values():
        want = check_all(reg, Z.compressed_file(*Z.XYZI_FIELDS, Z.xyzi_columns(rec), n, enc))
        assert (want.view(np.uint32)[:, [0, 1, 2, 4]] == rec.view(np.uint32)[:, [0, 1, 2, 4]]).all()   # bit for bit


def test_device_image_at_every_alignment(reg, hand_made):
    import torch

    rec = pcd_numpy.random_records(np.random.default_rng(1400), 257)
    small = Z.compressed_file(*Z.XYZI_FIELDS, Z.xyzi_columns(rec), 257, Z.greedy)
    big = Z.xyzi_file_of_stream(hand_made["lengths_3_8_9_10_264"], Z.N_HAND)
    for img in (small, big):
        want = Z.decode_compressed(img)
        buf = torch.full((len(img) + 64,), ord("9"), dtype=torch.uint8, device="cuda")   # '9' around the image: reading past it would show
        for shift in range(16):
            buf[shift: shift + len(img)] = _cuda(img)
            assert (_np(reg.decodePCD(buf[shift: shift + len(img)])) == want).all(), shift


def test_bad_streams_touch_nothing_and_name_the_token(reg, tmp_path):
    rng = np.random.default_rng(1500)
    n = 1000
    total = 16 * n
    head = Z.header(*Z.XYZI_FIELDS, n)
    first = len(head) + 8                                         # the file offset of the stream's first byte
    path = tmp_path / "bad.pcd"
    reg.pcdReadPieceBytes(2048)

    def image(stream):
        return Z.xyzi_file_of_stream(stream, n)

    good_tokens = Z.random_tokens(rng, total)
    good = image(Z.from_tokens(good_tokens))
    # a reference to before the first output byte: token 0, and a middle token (of the third block of the stream)
    expect_error(reg, image(Z.from_tokens([("ref", 3, 1)] + Z.random_tokens(rng, total - 3))), -1, first, "before the first", path)
    # (a distance is at most 8192: only the first 8192 output bytes can hold such a token; literal runs in front put it in the stream's
    # second 4096-byte block)
    lits = Z._fill([], 5000, rng)
    at = len(Z.from_tokens(lits))
    assert 4096 < at < 8192
    mid = lits + [("ref", 5, 5001)]
    expect_error(reg, image(Z.from_tokens(mid + Z.random_tokens(rng, total - 5005))), -1, first + at, "before the first", path)
    # two bad tokens: the earlier one is named
    two = Z._fill(list(mid), 7000, rng) + [("ref", 9, Z.MAX_DIST)]
    expect_error(reg, image(Z.from_tokens(two + Z.random_tokens(rng, total - 7009))), -1, first + at, "before the first", path)
    # a stream cut inside a literal, and inside a three-byte reference (after its first and after its second byte)
    front = Z.random_tokens(rng, total - 100)
    front_bytes = len(Z.from_tokens(front))
    expect_error(reg, image(Z.from_tokens(front + [("ref", 90, 7), ("lit", b"0123456789")])[:-4]), -1, first + front_bytes + 3, "end of the compressed stream", path)
    for cut in (1, 2):
        expect_error(reg, image(Z.from_tokens(front + [("ref", 100, 7)])[:-cut]), -1, first + front_bytes, "end of the compressed stream", path)
    # output one byte too long (the last token is the one that passes uncompressed_size), one byte too short (no offset to name)
    expect_error(reg, image(Z.from_tokens(front + [("ref", 91, 7), ("lit", b"0123456789")])), -1, first + front_bytes + 3, "past uncompressed_size", path)
    expect_error(reg, image(Z.from_tokens(front + [("ref", 89, 7), ("lit", b"0123456789")])), -1, None, "inflates to 15999 bytes", path)
    # the size words, in the order of the checks
    stream = Z.from_tokens(good_tokens)

    def sized(c, u, tail=stream):
        return head + struct.pack("<II", c, u) + tail

    expect_error(reg, head + b"\x01\x02\x03\x04\x05\x06\x07", -1, None, "size words", path)
    expect_error(reg, sized(2 ** 31, total + 1), -7, None, "2^31", path)            # ahead of the mismatch
    expect_error(reg, sized(0, 2 ** 31), -7, None, "2^31", path)
    expect_error(reg, sized(0, total - 16), -1, None, "uncompressed_size", path)    # ahead of compressed_size 0
    expect_error(reg, sized(0, total), -1, None, "compressed_size is 0", path)
    expect_error(reg, sized(len(stream) + 1, total), -1, None, "bytes follow", path)
    expect_error(reg, sized(2 ** 31 - 1, total), -1, None, "bytes follow", path)
    reg.pcdReadPieceBytes(1 << 26)
    # capacity too small: behind the size words' checks
    lay, cnt, out = reg._layout(*XYZI), C.c_size_t(777), np.full((999, 32), 0xA5, np.uint8)
    for img, word in ((good, b"too small"), (sized(len(stream) + 1, total), b"bytes follow")):
        assert reg._lib.lsr_decode_pcd(reg._h, img, len(img), 0, C.c_void_p(out.ctypes.data), 999, C.byref(lay), 0, C.byref(cnt)) == -1
        assert word in reg._lib.lsr_last_error() and cnt.value == 777 and (out == 0xA5).all()
    path.write_bytes(good)
    assert reg._lib.lsr_load_pcd(reg._h, os.fsencode(path), C.c_void_p(out.ctypes.data), 999, C.byref(lay), 0, C.byref(cnt)) == -1
    assert b"too small" in reg._lib.lsr_last_error() and cnt.value == 777 and (out == 0xA5).all()
    # a missing file
    assert reg._lib.lsr_load_pcd(reg._h, os.fsencode(tmp_path / "none.pcd"), C.c_void_p(out.ctypes.data), 999, C.byref(lay), 0, C.byref(cnt)) == -9
    assert b"none.pcd" in reg._lib.lsr_last_error() and cnt.value == 777
    assert reg._lib.lsr_set_input_target_pcd(reg._h, os.fsencode(tmp_path / "none.pcd"), C.byref(cnt)) == -9 and cnt.value == 777
    # the coordinates' type keeps its precedence over the kind
    expect_error(reg, good.replace(b"SIZE 4 4 4 4", b"SIZE 8 8 8 4"), -6, None, "4-byte float", path, oracle=False)
    # and the good file still reads
    check_all(reg, good, path=path)


def test_target_from_a_compressed_file(tmp_path):
    """setInputTargetPCD of a compressed file against that of the binary file of the same cloud: the same voxel grid."""
    case = synth.small_case(n_source=1500, n_keyframes=3)
    cloud = synth.as_pointxyzi(case.target[:2100])
    cloud[:, 4] = np.random.default_rng(1600).uniform(0, 255, len(cloud)).astype(np.float32)
    n, cols = len(cloud), Z.xyzi_columns(cloud)
    (tmp_path / "c.pcd").write_bytes(Z.compressed_file(*Z.XYZI_FIELDS, cols, n, Z.greedy))
    (tmp_path / "b.pcd").write_bytes(R.binary_file(*Z.XYZI_FIELDS, cols, n))
    dumps = []
    for name in ("c.pcd", "b.pcd"):
        r = NormalDistributionsTransform(device=0)
        r.setResolution(3.0)
        r.pcdReadCompressed(name == "c.pcd")
        r.pcdReadPieceBytes(4096)
        assert r.setInputTargetPCD(tmp_path / name) == n
        dumps.append(r.gridDump())
    assert len(dumps[0]["idx"]) > 10
    for key in ("idx", "n", "mean", "icov"):
        assert np.array_equal(dumps[0][key], dumps[1][key]), key


def test_inflate_profile_key(tmp_path):
    r = NormalDistributionsTransform(device=0)
    r.pcdReadCompressed(True)
    rec = pcd_numpy.random_records(np.random.default_rng(1700), 4099)
    cols = Z.xyzi_columns(rec)
    img = Z.compressed_file(*Z.XYZI_FIELDS, cols, 4099, Z.all_literal)
    r.decodePCD(img)
    assert r._getf(_capi.PCD_INFLATE_MS) == 0.0                   # without LSR_PROFILE
    r.setProfiling(True)
    r.decodePCD(_cuda(img))
    assert r._getf(_capi.PCD_INFLATE_MS) > 0.0
    (tmp_path / "c.pcd").write_bytes(img)
    r.loadPCDFile(tmp_path / "c.pcd")
    assert r._getf(_capi.PCD_INFLATE_MS) > 0.0 and r._getf(_capi.PCD_PARSE_MS) == 0.0
    r.decodePCD(R.binary_file(*Z.XYZI_FIELDS, cols, 4099))
    assert r._getf(_capi.PCD_INFLATE_MS) == 0.0                   # the last call's: a binary file
    r.setProfiling(False)
    r.decodePCD(img)
    assert r._getf(_capi.PCD_INFLATE_MS) == 0.0
