"""CPU: the host side of reading .pcd files on the device — the C ABI's symbols, keys and argument checks; the text -> fp32 arithmetic
and the run-wise line machine of the kernels (csrc/pcd_parse.hpp) compiled for the host (tools/pcd_read_host_emu/harness.cpp) against
the C library's strtof and a plain sequential split; the header parser (lsr_parse_pcd_header needs no handle) against the Python
restatement tests/pcd_read_numpy.py; the Python mirror against a fake library; the INTEGRATION.md 3h snippet.  The kernels themselves:
tests/test_pcd_read_gpu.py."""
import ctypes as C
import os
import re
import subprocess
import textwrap
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

import pcd_numpy
import pcd_read_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tools", "pcd_read_host_emu", "harness.cpp")
NEW = ("lsr_parse_pcd_header", "lsr_decode_pcd", "lsr_load_pcd", "lsr_set_input_target_pcd")
OK, BAD, UNRESOLVED = 0, 1, 2


def test_symbols_keys_and_define_exist():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\bint " + name + r"\(", hdr)
    assert _capi.PCD_PARSE_MS == 13 and re.search(r"LSR_PCD_PARSE_MS\s*=\s*13\b", hdr)
    assert _capi.PCD_READ_PIECE_BYTES == 52 and re.search(r"LSR_PCD_READ_PIECE_BYTES\s*=\s*52\b", hdr)
    assert _capi.PCD_UNRESOLVED_TOKENS == 53 and re.search(r"LSR_PCD_UNRESOLVED_TOKENS\s*=\s*53\b", hdr)
    assert _capi.PCD_READ_MAX_LINE_BYTES == 1024 and re.search(r"#define LSR_PCD_READ_MAX_LINE_BYTES 1024\b", hdr)
    assert "typedef struct lsr_pcd_info" in hdr and C.sizeof(_capi.PcdInfo) == 4 * 8 + 4 * 4 + 7 * 8
    assert lib.lsr_status_string(-6) == b"not implemented"
    # the library exports exactly the names the header declares
    declared = sorted(set(re.findall(r"\b(lsr_[a-z0-9_]+)\s*\(", hdr)))
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\sT\s+([A-Za-z][A-Za-z0-9_]*)$", nm, re.M))) == declared
    assert sorted(_capi.EXPORTED_SYMBOLS) == declared


def test_null_handle_and_null_arguments_touch_nothing():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    n = C.c_size_t(5)
    out = np.full(64, 7, np.uint8)
    lay = _capi.Pc2Layout(32, 0, 4, 8, 16)
    img = pcd_numpy.pcd_ascii_bytes(np.ones((2, 8), np.float32))
    assert lib.lsr_decode_pcd(None, img, len(img), 0, out.ctypes.data, 2, C.byref(lay), 0, C.byref(n)) == -1
    assert b"null handle" in lib.lsr_last_error()
    assert lib.lsr_load_pcd(None, b"never.pcd", out.ctypes.data, 2, C.byref(lay), 0, C.byref(n)) == -1
    assert b"null handle" in lib.lsr_last_error()
    assert lib.lsr_set_input_target_pcd(None, b"never.pcd", C.byref(n)) == -1
    assert b"null handle" in lib.lsr_last_error()
    info = _capi.PcdInfo()
    info.n_points = 99
    assert lib.lsr_parse_pcd_header(None, 10, C.byref(info)) == -1 and lib.lsr_parse_pcd_header(img, len(img), None) == -1
    assert n.value == 5 and (out == 7).all() and info.n_points == 99


# ---- the arithmetic and the line machine, compiled for the host ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcd_read_host_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(d / "libpcdreademu.so"), HARNESS])
    lib = C.CDLL(str(d / "libpcdreademu.so"))
    u32p, llp = C.POINTER(C.c_uint32), C.POINTER(C.c_longlong)
    lib.emu_pcdr_sweep.restype = lib.emu_pcdr_check_list.restype = lib.emu_pcdr_lines.restype = C.c_longlong
    lib.emu_pcdr_sweep.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, u32p, u32p, llp, llp]
    lib.emu_pcdr_check_list.argtypes = [u32p, C.c_longlong, C.c_char_p, u32p, u32p, llp]
    lib.emu_pcdr_lines.argtypes = [C.c_int, C.c_uint32, llp]
    lib.emu_pcdr_batch.restype = None
    lib.emu_pcdr_batch.argtypes = [C.c_char_p, C.c_longlong, C.POINTER(C.c_int), u32p, u32p, C.POINTER(C.c_int)]
    return lib


def batch(emu, tokens):
    """(status, bits, strtof's bits, strtof took the whole token) of every token, through the host build of the device parser."""
    blob = b"".join(t + b"\0" for t in tokens)
    n = len(tokens)
    st, whole = np.zeros(n, np.int32), np.zeros(n, np.int32)
    bits, want = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    u32p, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    emu.emu_pcdr_batch(blob, n, st.ctypes.data_as(ip), bits.ctypes.data_as(u32p), want.ctypes.data_as(u32p), whole.ctypes.data_as(ip))
    return st, bits, want, whole


def _first(text, got, want):
    return f"first mismatch: '{text.value.decode()}': parser 0x{got.value:08x}, strtof 0x{want.value:08x}"


def test_parser_against_strtof_over_every_exponent(emu):
    """256 exponent fields x both signs x (0, 1, 0x400000, 0x7fffff and 2^15 strided mantissas): '%.9g' of every value gives its bits
    back, '%.8g' gives what strtof makes of that text; zero mismatches, zero unresolved."""
    text, got, want, n, unres = C.create_string_buffer(64), C.c_uint32(0), C.c_uint32(0), C.c_longlong(0), C.c_longlong(-1)
    stride = 7919 * 1009
    mism = emu.emu_pcdr_sweep(1 << 15, stride, text, C.byref(got), C.byref(want), C.byref(n), C.byref(unres))
    assert n.value == 2 * 256 * ((1 << 15) + 4)
    assert mism == 0, _first(text, got, want)
    assert unres.value == 0


def test_parser_on_table_edges_and_ties(emu):
    """The writer's value table, the decade edges, FLT_MAX and its overflow neighbours, the denormal floor, exact ties of at most nine
    digits: every result is strtof's, none unresolved."""
    bits = np.ascontiguousarray(pcd_numpy.table_bits())
    text, got, want, unres = C.create_string_buffer(64), C.c_uint32(0), C.c_uint32(0), C.c_longlong(-1)
    assert emu.emu_pcdr_check_list(bits.ctypes.data_as(C.POINTER(C.c_uint32)), len(bits), text, C.byref(got), C.byref(want), C.byref(unres)) == 0, \
        _first(text, got, want)
    assert unres.value == 0
    tokens = [b"3.4028235e38", b"3.4028236e38", b"3.5e38", b"1e39", b"1e400", b"3.40282347e38", b"3.40282357e38", b"340282356e30",
              b"1.4e-45", b"7.1e-46", b"7e-46", b"1e-46", b"1e-400", b"7.00649232e-46", b"7.00649233e-46", b"1.17549435e-38", b"1.17549429e-38",
              b"16777217", b"16777219", b"33554434", b"33554438", b"0.5", b"0.25", b"0.125", b"0.0625", b"8388608.5", b"8388609.5",
              b"4194304.25", b"4194304.75", b"2097152.125", b"2097152.375"]
    for j in range(1000000, 1000000 + 256):                       # j + 0.25, j + 0.75: the patterns of the writer's tie test
        tokens += [b"%d.25" % j, b"%d.75" % j, b"-%d.25" % j]
    for j in range(16777216, 16777216 + 64):                      # integers past 2^24: every odd one is a tie
        tokens += [b"%d" % j, b"-%d" % j, b"%d" % (2 * j + 1), b"%de1" % j]
    tokens += [t.replace(b"e", b"E") for t in tokens[:17]] + [b"-" + t for t in tokens[:31]] + [b"+" + t for t in tokens[:31]]
    st, got, want, whole = batch(emu, tokens)
    assert (st == OK).all() and whole.all()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (tokens[bad[0]], hex(got[bad[0]]), hex(want[bad[0]]))
    want_py = np.array([R.strtof_bits(t) for t in tokens], np.uint32)   # the oracle's own strtof, through ctypes
    assert (want_py == want).all()
    expect = {b"3.4028235e38": 0x7f7fffff, b"3.4028236e38": 0x7f800000, b"1e400": 0x7f800000, b"1.4e-45": 1, b"7.1e-46": 1, b"7e-46": 0,
              b"1e-400": 0, b"16777217": 0x4b800000, b"16777219": 0x4b800002, b"33554434": 0x4c000000, b"-7e-46": 0x80000000}
    for t, b in expect.items():
        assert got[tokens.index(t)] == b, t


def _float_from_bits(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def test_long_tokens_resolve_to_strtof_or_stay_unresolved(emu):
    """2000 random floats: the exact decimal expansion of the midpoint to the next float (a tie: to even), that expansion with its last
    digit +-1, and its truncations to 20, 30 and 60 digits.  A token the device arithmetic decides equals strtof; one it cannot is left
    unresolved (the host entry then asks strtof); none is wrong.  Reported: how many went unresolved."""
    getcontext().prec = 400
    rng = np.random.default_rng(11)
    ex = rng.integers(0, 254, 2000)
    ex[:40] = 0                                                   # denormals
    ex[40:60] = 253
    bits = (ex.astype(np.uint32) << 23) | rng.integers(0, 1 << 23, 2000).astype(np.uint32)
    bits[0] = 0                                                   # the midpoint between 0 and the smallest denormal
    tokens = []
    for b in bits.tolist():
        mid = (Fraction(_float_from_bits(b)) + Fraction(_float_from_bits(b + 1))) / 2
        d = Decimal(mid.numerator) / Decimal(mid.denominator)     # exact: the denominator is a power of two, 400 digits are enough
        assert Fraction(d) == mid
        sign, digits, exp = d.as_tuple()
        digits = list(digits)
        full = "".join(map(str, digits))
        up, dn = digits[:], digits[:]
        up[-1] = (up[-1] + 1) % 10 if up[-1] != 9 else 9          # (a last digit 9 stays: "+1" would need a carry; "-1" still moves it)
        dn[-1] = dn[-1] - 1 if dn[-1] else 1
        forms = [full, "".join(map(str, up)), "".join(map(str, dn))]
        for text in forms:
            tokens.append(f"{text}e{exp}".encode())
        for cut in (20, 30, 60):
            if len(full) > cut:
                tokens.append(f"{full[0]}.{full[1:cut]}e{exp + len(full) - 1}".encode())
            else:
                tokens.append(f"{full}e{exp}".encode())
    st, got, want, whole = batch(emu, tokens)
    assert whole.all() and (st != BAD).all()
    decided = st == OK
    wrong = np.nonzero(decided & (got != want))[0]
    assert len(wrong) == 0, (tokens[wrong[0]], hex(got[wrong[0]]), hex(want[wrong[0]]))
    # the ties themselves go to even, by strtof and, where decided, by the parser
    ties = np.arange(0, len(tokens), 6)
    assert ((want[ties] & 1) == 0).all()
    n_unres = int((st == UNRESOLVED).sum())
    print(f"long tokens: {len(tokens)} checked, {n_unres} unresolved ({int((st[ties] == UNRESOLVED).sum())} of the {len(ties)} exact midpoints), 0 wrong")
    short = np.array([len(t.split(b"e")[0].replace(b".", b"").lstrip(b"0")) <= 19 for t in tokens])
    assert not (short & (st == UNRESOLVED)).any()                 # nothing is dropped from 19 digits: never unresolved


def test_grammar_accepts_and_rejects(emu):
    accept = [b"+1", b"1.", b".5", b"1E5", b"1e+05", b"007", b"-0", b"INF", b"Infinity", b"NaN", b"-nan", b"+nan", b"-iNfInItY", b"0.0e-0", b"1e-05",
              b"00000000000000000000000001", b"0.000000000000000000000000000000000000000000001", b"1" + b"0" * 38, b"1" + b"0" * 39,
              b"12345678901234567890123", b"-.5e1", b"5.e0"]
    reject = [b"0x10", b"1.2.3", b"1e", b"1e+", b"nan(1)", b"1,5", b"--1", b"1f", b"", b".", b"+", b"-", b"e5", b".e5", b"1e5.0", b"in", b"infinit", b"nano",
              b"+-1", b"1 ", b"0x1p3", b"1d5", b"1_000"]
    st, got, want, whole = batch(emu, accept + reject)
    na = len(accept)
    assert (st[:na] == OK).all(), [accept[i] for i in np.nonzero(st[:na] != OK)[0]]
    assert (got[:na] == want[:na]).all() and whole[:na].all()
    assert (st[na:] == BAD).all(), [reject[i] for i in np.nonzero(st[na:] != BAD)[0]]
    pinned = {b"NaN": 0x7fc00000, b"+nan": 0x7fc00000, b"-nan": 0xffc00000, b"INF": 0x7f800000, b"-iNfInItY": 0xff800000, b"-0": 0x80000000,
              b"007": 0x40e00000, b"1" + b"0" * 39: 0x7f800000}
    for t, b in pinned.items():
        assert got[accept.index(t)] == b, t
    for t in accept:
        assert R.token_bits(t) == got[accept.index(t)], t         # the oracle's grammar and value agree
    for t in reject:
        assert R.token_bits(t) is None, t


def test_line_machine_runwise_against_plain_split(emu):
    """500 random texts over {newline, blank, tab, CR, 'a'} of lengths 0 .. 300, each at every start misalignment 0 .. 15 and every run
    length 1 .. 64: run summaries composed in order give the line count, the walk with the composed entry state gives every offset."""
    n = C.c_longlong(0)
    assert emu.emu_pcdr_lines(500, 3, C.byref(n)) == 0
    assert n.value == 500 * 16 * 64


def test_standalone_harness_program(tmp_path):
    """The same harness as a program of its own (its main: a thinner sweep, the grammar's edges, the line machine; the form a host
    sanitizer build takes, see the head of harness.cpp)."""
    exe = str(tmp_path / "pcd_read_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DPCD_READ_HARNESS_MAIN", HARNESS, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and " 0 mismatches, 0 unresolved" in run.stdout, (run.stdout, run.stderr)


# ---- the header parser (no handle, no device) ------------------------------------------------------------------------------------------
def header_of(data: bytes):
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    info = _capi.PcdInfo()
    st = lib.lsr_parse_pcd_header(data, len(data), C.byref(info))
    return st, info, lib.lsr_last_error().decode()


def check_header(data: bytes):
    """lsr_parse_pcd_header against the Python restatement: the same verdict, and for a good header the same numbers."""
    st, info, why = header_of(data)
    try:
        H = R.parse_header(data)
    except R.PcdError as e:
        assert st == e.status, (st, e, why)
        return st, info, why
    assert st == 0, why
    assert (info.n_points, info.width, info.height, info.data_offset) == (H["POINTS"], H["WIDTH"], H["HEIGHT"], H["data_offset"])
    assert (info.point_step, info.n_fields, info.has_intensity) == (H["point_step"], len(H["FIELDS"]), int("intensity" in H["tok"]))
    assert info.data_kind == ["ascii", "binary", "binary_compressed"].index(H["DATA"])
    assert list(info.viewpoint) == [float(v) for v in H["VIEWPOINT"]]
    return st, info, why


def make_header(fields="x y z intensity", size="4 4 4 4", typ="F F F F", count="1 1 1 1", width="7", height="1", points="7", data="ascii",
                version="0.7", viewpoint="0 0 0 1 0 0 0", eol="\n", key="FIELDS"):
    lines = ["# .PCD v0.7 - Point Cloud Data file format"]
    for k, v in (("VERSION", version), (key, fields), ("SIZE", size), ("TYPE", typ), ("COUNT", count), ("WIDTH", width), ("HEIGHT", height),
                 ("VIEWPOINT", viewpoint), ("POINTS", points), ("DATA", data)):
        if v is not None:
            lines.append(f"{k} {v}")
    return (eol.join(lines) + eol).encode()


def test_header_parser_accepts():
    for with_i in (True, False):                                  # the writer's two headers
        data = pcd_numpy.header(12345, with_i) + b"1 2 3 4\n"
        st, info, _ = check_header(data)
        assert st == 0 and info.n_points == 12345 and info.has_intensity == int(with_i) and info.data_offset == len(data) - 8
    st, info, _ = check_header(make_header("rgb z normal x _ intensity y", "4 4 4 4 1 4 4", "U F F F U F F", "1 1 3 1 5 1 1", data="binary"))
    assert st == 0 and info.point_step == 4 + 4 + 12 + 4 + 5 + 4 + 4 and info.n_fields == 7 and info.data_kind == 1 and info.has_intensity == 1
    for gone in ("count", "height", "points", "viewpoint"):       # the entries with a default
        st, info, _ = check_header(make_header(**{gone: None}))
        assert st == 0 and info.n_points == 7 and info.height == 1 and list(info.viewpoint) == [0, 0, 0, 1, 0, 0, 0]
    st, info, _ = check_header(make_header(key="COLUMNS"))
    assert st == 0 and info.n_fields == 4
    st, info, _ = check_header(make_header(eol="\r\n", width="640", height="480", points="307200", viewpoint="1.5 -2 3e0 0.5 0.5 0.5 0.5"))
    assert st == 0 and (info.width, info.height, info.n_points) == (640, 480, 307200) and list(info.viewpoint) == [1.5, -2, 3, 0.5, 0.5, 0.5, 0.5]
    st, info, _ = check_header(b"\n  # a comment\n" + make_header().replace(b"WIDTH 7", b"WIDTH\t 7 ") + b"0 0 0 0\n")
    assert st == 0 and info.width == 7


def test_header_parser_refuses():
    bad = [make_header(version=None), make_header(fields=None), make_header(size=None), make_header(typ=None), make_header(width=None),
           make_header(fields="x y intensity", size="4 4 4", typ="F F F", count="1 1 1"), make_header(fields="x y z x"),
           make_header(points="8"), make_header(width="0", points="0"), make_header(width="0", points=None), make_header(size="4 4 4"),
           make_header(size="4 4 3 4"), make_header(typ="F F G F"), make_header(count="1 1 0 1"), make_header(count="1 3 1 1"),
           make_header(width="-7"), make_header(width="7.0"), make_header(height="1 1"), make_header(data="text"), make_header(data="ascii extra"),
           make_header(viewpoint="0 0 0 1"), make_header(viewpoint="0 0 0 1 0 0 x")]
    for data in bad:
        st, _, why = check_header(data)
        assert st == -1 and why.startswith("PCD header:"), (data, st, why)
    whole = make_header()
    for cut in (0, 10, len(whole) - 1):                           # the bytes end before the DATA line does
        st, _, why = check_header(whole[:cut])
        assert st == -1 and "header incomplete" in why
    for data in (make_header(size="8 8 8 4", typ="F F F F"), make_header(typ="F F F U"), make_header(size="4 4 2 4")):
        st, _, why = check_header(data)
        assert st == -6 and "4-byte float" in why
    st, info, why = check_header(make_header(data="binary_compressed"))
    assert st == -6 and "binary_compressed" in why and info.data_kind == 2 and info.n_points == 7
    st, _, why = check_header(make_header(width=str(2 ** 31), points=str(2 ** 31)))
    assert st == -7
    st, _, _ = check_header(make_header(width=str(2 ** 31 - 1), points=str(2 ** 31 - 1)))
    assert st == 0


# ---- the Python mirror against a fake library ------------------------------------------------------------------------------------------
class FakeLib:
    """Stands in for the ctypes library behind a Registration: records every call, answers lsr_decode_pcd / lsr_load_pcd from the oracle."""

    def __init__(self, files):
        self.calls, self.files = [], files

    def _answer(self, name, data, out, cap, lay, n_out):
        lay = lay._obj if lay is not None else None
        self.calls.append((name, None if out is None or out.value is None else "records", cap, None if lay is None else (lay.point_step, lay.offset_intensity)))
        H = R.parse_header(data)
        if out is not None and out.value is not None:
            layout = (lay.point_step, (lay.offset_x, lay.offset_y, lay.offset_z, lay.offset_intensity))
            rec = R.decode(data, layout)
            assert cap >= len(rec)
            C.memmove(out.value, rec.ctypes.data, rec.nbytes)
        n_out._obj.value = H["POINTS"]
        return 0

    def lsr_decode_pcd(self, h, image, size, dev, out, cap, lay, out_dev, n_out):
        assert dev == 0 and out_dev == 0
        return self._answer("lsr_decode_pcd", C.string_at(image.value, size), out, cap, lay, n_out)

    def lsr_load_pcd(self, h, path, out, cap, lay, out_dev, n_out):
        assert out_dev == 0
        return self._answer("lsr_load_pcd", self.files[path], out, cap, lay, n_out)

    def lsr_set_input_target_pcd(self, h, path, n_out):
        self.calls.append(("lsr_set_input_target_pcd", path))
        n_out._obj.value = R.parse_header(self.files[path])["POINTS"]
        return 0


def test_python_mirror_against_a_fake_library():
    from lidarslam_ros2_amd.registration import Registration

    rec = pcd_numpy.random_records(np.random.default_rng(2), 9)
    img = pcd_numpy.pcd_ascii_bytes(rec)
    reg = Registration.__new__(Registration)
    reg._lib, reg._h, reg._keep, reg._device = FakeLib({b"map.pcd": img}), None, {}, 0
    want = R.decode(img)
    got = reg.decodePCD(img)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (9, 32) and (got == want).all()
    assert reg._lib.calls == [("lsr_decode_pcd", None, 0, None), ("lsr_decode_pcd", "records", 9, (32, 16))]
    got = reg.decodePCD(np.frombuffer(img, np.uint8), layout=(16, (0, 4, 8, None)))
    assert got.shape == (9, 16) and (got == R.decode(img, (16, (0, 4, 8, None)))).all() and reg._lib.calls[-1][3] == (16, -1)
    got = reg.loadPCDFile("map.pcd")
    assert (got == want).all() and reg._lib.calls[-2:] == [("lsr_load_pcd", None, 0, None), ("lsr_load_pcd", "records", 9, (32, 16))]
    assert reg.setInputTargetPCD("map.pcd") == 9 and reg._n_target == 9 and reg._lib.calls[-1] == ("lsr_set_input_target_pcd", b"map.pcd")
    # the oracle reads what the writer's restatement writes
    assert (want.view(np.float32).reshape(9, 8)[:, [0, 1, 2, 4]].view(np.uint32) ==
            np.array([[R.strtof_bits(t) for t in line.split()] for line in img.split(b"DATA ascii\n")[1].splitlines()], np.uint32)).all()


def test_integration_md_pcd_read_snippet_compiles_and_links(tmp_path):
    """the block of tests/cpp/pcd_read_snippets.cpp, compiled against include/lidarslam_reg/pcd_io.hpp and linked
    against the library; the program itself shows the helpers refusing a call without a handle (no device needed, the payload kept)
    and the header parser working without one."""
    src = os.path.join(ROOT, "tests", "cpp", "pcd_read_snippets.cpp")
    libdir = os.path.join(ROOT, "lidarslam_ros2_amd")
    exe = str(tmp_path / "pcd_read_snippets")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir,
                           "-llidarslam_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0 and "PCD_READ_SNIPPETS refused=1 refused_payload=1 kept=1 header=0 points=5 offset=66" in run.stdout, (run.stdout, run.stderr)
    text, doc = open(src).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text.split("// [pcd-snippet begin: load_map]\n")[1].split("// [pcd-snippet end: load_map]")[0]
    assert textwrap.dedent(block).strip("\n").rstrip() in textwrap.dedent(doc.split("### 3h.")[1].split("```cpp\n")[1].split("```")[0])
    assert "lsr_set_input_target_pcd" in doc.split("### 3h.")[1]
