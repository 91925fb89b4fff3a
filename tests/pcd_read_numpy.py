"""TEST INFRASTRUCTURE: reading a .pcd file image (PCD v0.7, DATA ascii / binary, the semantics restated in include/lidarslam_reg.h),
in plain Python — a header parser, a line splitter and the C library's own strtof through ctypes — independent of csrc/pcd_parse.hpp and
csrc/pcd_read.hip.  Every comparison against it is on raw record bytes: there is no tolerance."""
import ctypes as C
import re

import numpy as np

XYZI = (32, (0, 4, 8, 16))
INVALID, NOT_IMPLEMENTED, INDEX_OVERFLOW, IO = -1, -6, -7, -9
MAX_LINE = 1024

_libc = C.CDLL(None)
_libc.strtof.restype = C.c_float
_libc.strtof.argtypes = [C.c_char_p, C.POINTER(C.c_char_p)]

_NUMBER = re.compile(rb"[+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[iI][nN][fF](?:[iI][nN][iI][tT][yY])?|[nN][aA][nN])\Z")
_BLANKS = b" \t\r"


def _words(line: bytes):
    return [w for w in line.replace(b"\t", b" ").replace(b"\r", b" ").split(b" ") if w]


class PcdError(Exception):
    def __init__(self, status, why, offset=None):
        super().__init__(f"{why} (status {status}, offset {offset})")
        self.status, self.why, self.offset = status, why, offset


def strtof_bits(token: bytes) -> int:
    """glibc's strtof of a whole token, as fp32 bits; a NaN is the quiet NaN of the token's sign."""
    v = _libc.strtof(token, None)
    if v != v:
        return 0xffc00000 if token.startswith(b"-") else 0x7fc00000
    return int(np.array([v], np.float32).view(np.uint32)[0])


def token_bits(token: bytes):
    """fp32 bits of a token of the accepted grammar, None for anything else."""
    return strtof_bits(token) if _NUMBER.match(token) else None


def parse_header(data: bytes) -> dict:
    pos, H = 0, {"COUNT": None, "HEIGHT": 1, "VIEWPOINT": [0.0, 0, 0, 1, 0, 0, 0], "POINTS": None}
    while True:
        nl = data.find(b"\n", pos)
        if nl < 0:
            raise PcdError(INVALID, "header incomplete")
        words = _words(data[pos:nl])
        pos = nl + 1
        if not words or words[0].startswith(b"#"):
            continue
        key, vals = words[0].decode(), [w.decode() for w in words[1:]]
        if key == "COLUMNS":
            key = "FIELDS"
        if key in ("SIZE", "COUNT", "WIDTH", "HEIGHT", "POINTS"):
            if not vals or not all(re.fullmatch(r"[0-9]{1,19}", v) for v in vals) or (key in ("WIDTH", "HEIGHT", "POINTS") and len(vals) != 1):
                raise PcdError(INVALID, "malformed " + key)
            H[key] = [int(v) for v in vals] if key in ("SIZE", "COUNT") else int(vals[0])
        elif key in ("FIELDS", "TYPE"):
            if not vals:
                raise PcdError(INVALID, "malformed " + key)
            H[key] = vals
        elif key == "VERSION":
            if len(vals) != 1:
                raise PcdError(INVALID, "malformed VERSION")
            H[key] = vals[0]
        elif key == "VIEWPOINT":
            try:
                H[key] = [float(v) for v in vals]
            except ValueError:
                raise PcdError(INVALID, "malformed VIEWPOINT")
            if len(vals) != 7:
                raise PcdError(INVALID, "malformed VIEWPOINT")
        elif key == "DATA":
            if len(vals) != 1 or vals[0] not in ("ascii", "binary", "binary_compressed"):
                raise PcdError(INVALID, "malformed DATA")
            H["DATA"], H["data_offset"] = vals[0], pos
            break
    for key in ("VERSION", "FIELDS", "SIZE", "TYPE", "WIDTH"):
        if key not in H:
            raise PcdError(INVALID, "no " + key)
    nf = len(H["FIELDS"])
    if H["COUNT"] is None:
        H["COUNT"] = [1] * nf
    if not (len(H["SIZE"]) == len(H["TYPE"]) == len(H["COUNT"]) == nf):
        raise PcdError(INVALID, "entries differ in length")
    tok = off = 0
    H["tok"], H["src"], not_float = {}, {}, []
    for name, s, t, c in zip(H["FIELDS"], H["SIZE"], H["TYPE"], H["COUNT"]):
        if s not in (1, 2, 4, 8) or t not in ("I", "U", "F") or c < 1:
            raise PcdError(INVALID, "bad SIZE / TYPE / COUNT")
        if name in ("x", "y", "z", "intensity"):
            if name in H["tok"] or c != 1:
                raise PcdError(INVALID, "field twice or with a COUNT")
            H["tok"][name], H["src"][name] = tok, off
            if (s, t) != (4, "F"):
                not_float.append(name)
        tok += c
        off += s * c
    if not all(k in H["tok"] for k in "xyz"):
        raise PcdError(INVALID, "x, y and z are required")
    wh = H["WIDTH"] * H["HEIGHT"]
    if H["POINTS"] is None:
        H["POINTS"] = wh
    if H["POINTS"] != wh or wh == 0:
        raise PcdError(INVALID, "POINTS")
    if wh > 2 ** 31 - 1:
        raise PcdError(INDEX_OVERFLOW, "too many points")
    H["n_tokens"], H["point_step"] = tok, off
    if not_float:
        raise PcdError(NOT_IMPLEMENTED, "not a 4-byte float")
    if H["DATA"] == "binary_compressed":
        raise PcdError(NOT_IMPLEMENTED, "binary_compressed")
    return H


def point_lines(data: bytes, start: int):
    """(offset of the first non-blank byte, tokens, bytes from there to the newline) of every line with a token, from `start` on."""
    out, pos, n = [], start, len(data)
    while pos < n:
        nl = data.find(b"\n", pos)
        end = n if nl < 0 else nl
        line = data[pos:end]
        lead = len(line) - len(line.lstrip(_BLANKS))
        if lead < len(line):
            out.append((pos + lead, _words(line), len(line) - lead))
        pos = end + 1
    return out


def decode(data, layout=XYZI) -> np.ndarray:
    """(POINTS, point_step) uint8: the records of the file image `data`.  Raises PcdError (status, and for a bad line its offset)."""
    data = bytes(data)
    H = parse_header(data)
    step, offs = layout
    n = H["POINTS"]
    names = ["x", "y", "z", "intensity"]
    out = np.zeros((n, step // 4), np.uint32)
    if H["DATA"] == "binary":
        body = np.frombuffer(data, np.uint8, offset=H["data_offset"])
        if len(body) < n * H["point_step"]:
            raise PcdError(INVALID, "short body")
        rec = body[: n * H["point_step"]].reshape(n, H["point_step"])
        for name, o in zip(names, offs):
            if o is None or o < 0 or name not in H["src"]:
                continue
            s = H["src"][name]
            out[:, o // 4] = rec[:, s:s + 4].copy().view(np.uint32).reshape(-1)
        return out.view(np.uint8).reshape(n, step)
    lines = point_lines(data, H["data_offset"])
    for k, (offset, toks, length) in enumerate(lines[:n]):
        if length > MAX_LINE:
            raise PcdError(INVALID, "line too long", offset)
        if len(toks) < H["n_tokens"]:
            raise PcdError(INVALID, "short line", offset)
        for name, o in zip(names, offs):
            if o is None or o < 0 or name not in H["tok"]:
                continue
            bits = token_bits(toks[H["tok"][name]])
            if bits is None:
                raise PcdError(INVALID, "bad token", offset)
            out[k, o // 4] = bits
    if len(lines) < n:
        raise PcdError(INVALID, "too few lines", len(data))
    return out.view(np.uint8).reshape(n, step)


def binary_file(fields, sizes, types, counts, columns: dict, n: int, pad_header: int = 0, extra=b"") -> bytes:
    """A DATA binary image: `columns` maps a field name to its (n, size * count) uint8 bytes; other fields are filled with 0xA5.
    pad_header: extra bytes in a comment line, to move the body's first byte."""
    rec = []
    for name, s, c in zip(fields, sizes, counts):
        rec.append(columns[name] if name in columns else np.full((n, s * c), 0xA5, np.uint8))
    body = np.concatenate(rec, 1).tobytes()
    head = (f"# .PCD v0.7{'#' * pad_header}\nVERSION 0.7\nFIELDS {' '.join(fields)}\nSIZE {' '.join(map(str, sizes))}\nTYPE {' '.join(types)}\n"
            f"COUNT {' '.join(map(str, counts))}\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n").encode()
    return head + body + extra
