"""TEST INFRASTRUCTURE: DATA binary_compressed .pcd images in plain Python (the format restated in include/lidarslam_reg.h) — a literal
byte-by-byte lzf_decompress, three encoders that write valid LZF streams, the file image around a stream, the oracle of the records,
and the hand-made streams both test files use.  Independent of csrc/pcd_lzf.hip.  Every comparison against it is on raw bytes."""
import struct

import numpy as np

import pcd_read_numpy as R
from pcd_read_numpy import INDEX_OVERFLOW, INVALID, XYZI, PcdError

MAX_LEN, MAX_DIST = 264, 8192
XYZI_FIELDS = (["x", "y", "z", "intensity"], [4, 4, 4, 4], ["F", "F", "F", "F"], [1, 1, 1, 1])


class LzfError(Exception):
    """A bad stream: `offset` of the offending token's control byte inside the stream (None: the stream ends short)."""

    def __init__(self, offset, why):
        super().__init__(f"{why} (token at stream offset {offset})")
        self.offset, self.why = offset, why


def lzf_decompress(stream: bytes, n_out: int) -> bytes:
    """liblzf's lzf_decompress, byte by byte."""
    ip, n, out = 0, len(stream), bytearray()
    while ip < n:
        at = ip
        c = stream[ip]
        ip += 1
        if c < 32:
            if ip + c + 1 > n:
                raise LzfError(at, "a literal run passes the end of the stream")
            if len(out) + c + 1 > n_out:
                raise LzfError(at, "output past uncompressed_size")
            for _ in range(c + 1):
                out.append(stream[ip])
                ip += 1
            continue
        length = c >> 5
        if length == 7:
            if ip >= n:
                raise LzfError(at, "a reference passes the end of the stream")
            length += stream[ip]
            ip += 1
        if ip >= n:
            raise LzfError(at, "a reference passes the end of the stream")
        distance = (((c & 0x1f) << 8) | stream[ip]) + 1
        ip += 1
        if len(out) + length + 2 > n_out:
            raise LzfError(at, "output past uncompressed_size")
        if distance > len(out):
            raise LzfError(at, "a reference to before the first output byte")
        for _ in range(length + 2):
            out.append(out[-distance])
    if len(out) < n_out:
        raise LzfError(None, "the stream ends short")
    return bytes(out)


# ---- encoders --------------------------------------------------------------------------------------------------------------------------
def _literals(data: bytes) -> bytes:
    return b"".join(bytes([len(data[i:i + 32]) - 1]) + data[i:i + 32] for i in range(0, len(data), 32))


def _reference(length: int, distance: int) -> bytes:
    assert 3 <= length <= MAX_LEN and 1 <= distance <= MAX_DIST
    l, d = length - 2, distance - 1
    if l < 7:
        return bytes([(l << 5) | (d >> 8), d & 255])
    return bytes([(7 << 5) | (d >> 8), l - 7, d & 255])


def all_literal(data: bytes) -> bytes:
    """Literal runs of 32 (the last one shorter)."""
    return _literals(bytes(data))


def greedy(data: bytes) -> bytes:
    """A simple hash matcher: the last place the next three bytes were seen, extended as far as it goes."""
    data = bytes(data)
    n, i, start, seen, out = len(data), 0, 0, {}, []
    while i < n:
        key = data[i:i + 3]
        p = seen.get(key)
        seen[key] = i
        if p is not None and len(key) == 3 and i - p <= MAX_DIST:
            length = 3
            while length < MAX_LEN and i + length < n and data[p + length] == data[i + length]:
                length += 1
            out.append(_literals(data[start:i]))
            out.append(_reference(length, i - p))
            i += length
            start = i
        else:
            i += 1
    out.append(_literals(data[start:]))
    return b"".join(out)


def from_tokens(tokens) -> bytes:
    """Explicit tokens: ("lit", bytes of 1 .. 32) or ("ref", length 3 .. 264, distance 1 .. 8192)."""
    out = []
    for t in tokens:
        if t[0] == "lit":
            assert 1 <= len(t[1]) <= 32
            out.append(bytes([len(t[1]) - 1]) + bytes(t[1]))
        else:
            out.append(_reference(t[1], t[2]))
    return b"".join(out)


def tokens_out(tokens) -> int:
    return sum(len(t[1]) if t[0] == "lit" else t[1] for t in tokens)


ENCODERS = {"all_literal": all_literal, "greedy": greedy}


# ---- the file image --------------------------------------------------------------------------------------------------------------------
def header(fields, sizes, types, counts, n: int, pad_header: int = 0, data: str = "binary_compressed") -> bytes:
    return (f"# .PCD v0.7{'#' * pad_header}\nVERSION 0.7\nFIELDS {' '.join(fields)}\nSIZE {' '.join(map(str, sizes))}\nTYPE {' '.join(types)}\n"
            f"COUNT {' '.join(map(str, counts))}\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA {data}\n").encode()


def body_of_stream(stream: bytes, n_out: int, extra: bytes = b"") -> bytes:
    return struct.pack("<II", len(stream), n_out) + stream + extra


def field_major_image(fields, sizes, counts, columns: dict, n: int) -> bytes:
    """The inflated image: per field a block of n * size * count bytes; fields not in `columns` are filled with 0xA5."""
    return b"".join((columns[name] if name in columns else np.full((n, s * c), 0xA5, np.uint8)).tobytes() for name, s, c in zip(fields, sizes, counts))


def compressed_file(fields, sizes, types, counts, columns: dict, n: int, encoder, pad_header: int = 0, extra: bytes = b"") -> bytes:
    """A DATA binary_compressed image of the cloud pcd_read_numpy.binary_file gives the same arguments."""
    image = field_major_image(fields, sizes, counts, columns, n)
    return header(fields, sizes, types, counts, n, pad_header) + body_of_stream(encoder(image), len(image), extra)


def xyzi_file_of_stream(stream: bytes, n: int, n_out=None, extra: bytes = b"") -> bytes:
    """FIELDS x y z intensity, n points, around a given stream (n_out: what the size word says; default n * 16)."""
    return header(*XYZI_FIELDS, n) + body_of_stream(stream, 16 * n if n_out is None else n_out, extra)


def xyzi_columns(rec: np.ndarray) -> dict:
    """(n, 8) float32 pcl::PointXYZI records -> the four columns' bytes."""
    u = np.ascontiguousarray(rec).view(np.uint32)
    return {name: np.ascontiguousarray(u[:, c:c + 1]).view(np.uint8) for name, c in zip(("x", "y", "z", "intensity"), (0, 1, 2, 4))}


def decode_compressed(img, layout=XYZI) -> np.ndarray:
    """(POINTS, point_step) uint8: the records of the DATA binary_compressed image.  Raises PcdError: the status, and for a bad token
    the FILE offset of its control byte."""
    img = bytes(img)
    word = b"DATA binary_compressed\n"
    at = img.index(word)
    H = R.parse_header(img[:at] + b"DATA binary\n" + img[at + len(word):])
    body_off = H["data_offset"] + len(b"_compressed")
    n, step_in = H["POINTS"], H["point_step"]
    body = img[body_off:]
    if len(body) < 8:
        raise PcdError(INVALID, "no size words")
    c_size, u_size = struct.unpack("<II", body[:8])
    if c_size > 2 ** 31 - 1 or u_size > 2 ** 31 - 1:
        raise PcdError(INDEX_OVERFLOW, "a size above 2^31 - 1")
    if u_size != n * step_in:
        raise PcdError(INVALID, "uncompressed_size")
    if c_size == 0 or c_size > len(body) - 8:
        raise PcdError(INVALID, "compressed_size")
    try:
        image = np.frombuffer(lzf_decompress(body[8:8 + c_size], u_size), np.uint8)
    except LzfError as e:
        raise PcdError(INVALID, e.why, None if e.offset is None else body_off + 8 + e.offset)
    step, offs = layout
    out = np.zeros((n, step // 4), np.uint32)
    for name, o in zip(["x", "y", "z", "intensity"], offs):
        if o is None or o < 0 or name not in H["src"]:
            continue
        first = n * H["src"][name]                                # the field's block; SIZE 4, COUNT 1: point i at 4 * i
        out[:, o // 4] = image[first:first + 4 * n].copy().view(np.uint32)
    return out.view(np.uint8).reshape(n, step)


# ---- hand-made streams -----------------------------------------------------------------------------------------------------------------
N_HAND = 4099
HAND_BYTES = 16 * N_HAND          # FIELDS x y z intensity: four blocks of 16396 bytes


def _fill(tokens, total, rng):
    """Literal runs of 32 random bytes (then what is left) until the tokens put out `total` bytes."""
    left = total - tokens_out(tokens)
    assert left >= 0
    while left > 0:
        k = min(32, left)
        tokens.append(("lit", rng.integers(0, 256, k, dtype=np.uint8).tobytes()))
        left -= k
    return tokens


def hand_made_streams() -> dict:
    """name -> stream; every one inflates to HAND_BYTES bytes: a cloud of N_HAND x y z intensity points."""
    rng = np.random.default_rng(1234)
    S = {}

    def lit(k):
        return ("lit", rng.integers(0, 256, k, dtype=np.uint8).tobytes())

    # all zero: one literal byte, then distance-1 references of length 264: the chain is as deep as the file
    toks, left = [("lit", b"\0")], HAND_BYTES - 1
    while left:
        k = min(MAX_LEN, left)
        if left - k in (1, 2):
            k -= 3
        toks.append(("ref", k, 1))
        left -= k
    S["zeros_depth_of_the_file"] = toks
    # distances 8192 and 1
    toks = [lit(32) for _ in range(256)]
    for k in range(200):
        toks += [("ref", 3 + (k * 37) % 262, MAX_DIST), lit(1 + k % 32), ("ref", 3 + (k * 11) % 262, 1)]
    S["distance_8192_and_1"] = _fill(toks, HAND_BYTES, rng)
    # lengths 3, 8, 9 (the first with a length byte), 10, 264 at many distances
    toks = [lit(32), lit(32)]
    for k in range(600):
        toks += [("ref", (3, 8, 9, 10, MAX_LEN)[k % 5], 1 + (k * 7) % 64), lit(1 + k % 7)]
    S["lengths_3_8_9_10_264"] = _fill(toks, HAND_BYTES, rng)
    # literal runs of 1 and of 32
    toks = []
    for k in range(1500):
        toks += [lit(1), lit(32)] if k % 3 else [lit(1), lit(1), lit(32)]
    S["literal_runs_1_and_32"] = _fill(toks, HAND_BYTES, rng)
    # references into referenced output, three levels deep, from the x block (it ends at 16396) into the y block
    toks = _fill([], 16300, rng)
    toks += [("ref", 200, 5000), ("ref", 200, 150), ("ref", MAX_LEN, 100), ("ref", MAX_LEN, 300)]
    S["three_levels_across_a_field"] = _fill(toks, HAND_BYTES, rng)
    # a first literal of every length in front of a fixed pattern: a token lies across every block boundary at every phase
    pattern = []
    for k in range(2200):
        pattern += [("lit", bytes([(k + j) & 255 for j in range(32)])), ("ref", 4 + k % 5, 33), ("ref", 9 + k % 200, 7 + k % 90), ("lit", bytes([k & 255] * 5))]
    for first in range(1, 33):
        toks, have = [lit(first)], first
        for t in pattern:
            have += tokens_out([t])
            if have > HAND_BYTES:
                break
            toks.append(t)
        S[f"first_literal_{first:02d}"] = _fill(toks, HAND_BYTES, rng)
    return {name: from_tokens(t) for name, t in S.items()}


def random_tokens(rng, n_out: int) -> list:
    """Valid tokens that put out exactly n_out bytes: literal runs of every length, references of every length with distances near and
    far, into literals and into referenced output alike."""
    toks, out = [], 0
    while out < n_out:
        left = n_out - out
        if out == 0 or left < 3 or rng.integers(0, 4) == 0:
            k = min(left, int(rng.integers(1, 33)) if rng.random() < 0.7 else int(rng.choice([1, 32])))
            toks.append(("lit", rng.integers(0, 256, k, dtype=np.uint8).tobytes()))
        else:
            k = min(left, int(rng.choice([3, 4, 8, 9, 10, MAX_LEN])) if rng.random() < 0.5 else int(rng.integers(3, MAX_LEN + 1)))
            far = min(out, MAX_DIST)
            toks.append(("ref", k, int(rng.choice([1, min(2, far), far])) if rng.random() < 0.4 else int(rng.integers(1, far + 1))))
        out += k
    return toks
