"""TEST INFRASTRUCTURE: the DATA binary and DATA binary_compressed .pcd images lsr_format_pcd writes, in plain Python — the formats and
the chunked LZF rule restated from include/lidarslam_reg.h, independent of csrc/pcd_deflate.hip.  Headers and field-major images come
from pcd_read_numpy / pcd_lzf_numpy.  Every comparison against it is on raw bytes: there is no tolerance."""
import numpy as np

import pcd_lzf_numpy as Z
import pcd_read_numpy as R
from pcd_read_numpy import XYZI

CHUNK = 4096          # LSR_PCD_LZF_CHUNK_BYTES
MAX_LEN = Z.MAX_LEN   # 264
NAMES = ("x", "y", "z", "intensity")


def columns(records, layout=XYZI) -> dict:
    """field name -> (n, 4) uint8, the field's bytes of every record; no "intensity" for a layout without one."""
    step, offs = layout
    rec = np.ascontiguousarray(records).view(np.uint8).reshape(-1, step)
    return {name: np.ascontiguousarray(rec[:, o:o + 4]) for name, o in zip(NAMES, offs) if o is not None and o >= 0}


def _fields(cols):
    names = [n for n in NAMES if n in cols]
    k = len(names)
    return names, [4] * k, ["F"] * k, [1] * k


def header(n: int, with_intensity: bool, data: str) -> bytes:
    """The ASCII file's header (pcd_numpy.header: the text the library writes) with another last line."""
    import pcd_numpy

    head = pcd_numpy.header(n, with_intensity)
    assert head.endswith(b"DATA ascii\n")
    return head[: -len(b"ascii\n")] + data.encode() + b"\n"


def binary_file(records, layout=XYZI) -> bytes:
    """The DATA binary image: header, then n packed records of 12 or 16 bytes."""
    cols = columns(records, layout)
    n = len(cols["x"])
    body = R.binary_file(*_fields(cols), cols, n).split(b"DATA binary\n", 1)[1]      # the helper's packed records behind its own header
    return header(n, "intensity" in cols, "binary") + body


def field_major_image(records, layout=XYZI) -> bytes:
    cols = columns(records, layout)
    names, sizes, _, counts = _fields(cols)
    return Z.field_major_image(names, sizes, counts, cols, len(cols["x"]))


def deflate_chunk(data: bytes) -> bytes:
    """One chunk under the rule: candidate = the nearest earlier position with the same three bytes (compared exactly), length = the
    common extension capped at 264 and at the chunk's end, greedy parse from the first byte, literal runs of at most 32."""
    n, i, start, last, out = len(data), 0, 0, {}, []
    cand = [None] * n
    for q in range(n - 2):             # every position's candidate, whether the parse visits it or not
        key = data[q:q + 3]
        cand[q] = last.get(key)
        last[key] = q
    while i < n:
        p = cand[i]
        if p is None:
            i += 1
            continue
        length = 3
        while length < MAX_LEN and i + length < n and data[p + length] == data[i + length]:
            length += 1
        out.append(Z._literals(data[start:i]))
        out.append(Z._reference(length, i - p))
        i += length
        start = i
    out.append(Z._literals(data[start:]))
    return b"".join(out)


def deflate(image) -> bytes:
    """The stream of an image: its chunks of CHUNK bytes (the last may be shorter), each compressed on its own, back to back."""
    image = bytes(image)
    return b"".join(deflate_chunk(image[a:a + CHUNK]) for a in range(0, len(image), CHUNK))


def chunk_bound(n_image: int) -> int:
    """Sum over the chunks of c + ceil(c / 32): what literal runs of 32 alone take."""
    return sum(c + (c + 31) // 32 for c in (min(CHUNK, n_image - a) for a in range(0, n_image, CHUNK)))


def compressed_file(records, layout=XYZI) -> bytes:
    """The DATA binary_compressed image: header, the two size words, deflate(field-major image)."""
    cols = columns(records, layout)
    image = field_major_image(records, layout)
    return header(len(cols["x"]), "intensity" in cols, "binary_compressed") + Z.body_of_stream(deflate(image), len(image))


# ---- maps and constructed images ---------------------------------------------------------------------------------------------------------
def grid_map(n: int, seed: int, intensity="random") -> np.ndarray:
    """(n, 8) float32 pcl::PointXYZI records, the map of tools/pcd_compressed_timing.py: coordinates of a few hundred metres on a
    centimetre grid (what a voxel-filtered map holds), intensities whole numbers 0 .. 255 ("random") or one constant."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 8), np.float32)
    rec[:, 0:3] = np.round(rng.uniform(-300.0, 300.0, (n, 3)), 2).astype(np.float32)
    rec[:, 2] *= np.float32(0.05)
    rec[:, 3] = 1.0
    rec[:, 4] = rng.integers(0, 256, n).astype(np.float32) if intensity == "random" else np.float32(intensity)
    return rec


def special_records(n: int = 96) -> np.ndarray:
    """(n, 8) float32 records with NaN payloads, -0, +-inf and denormals in every field (and in the bytes between the fields)."""
    bits = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffbfffff, 0x7fffffff, 0x80000000, 0x00000000, 0x7f800000, 0xff800000,
                     0x00000001, 0x807fffff, 0x00800000, 0x3f800000, 0xc2f6e979, 0x7fa5a5a5, 0xff812345], np.uint32)
    rec = np.zeros((n, 8), np.uint32)
    for c in range(8):
        rec[:, c] = bits[(np.arange(n) * (c + 1) + 3 * c) % len(bits)]
    return rec.view(np.float32)


def records_of_image(image: bytes) -> np.ndarray:
    """(n, 4) float32 packed x y z intensity records whose field-major image is `image` (16 n bytes)."""
    assert len(image) % 16 == 0
    return np.ascontiguousarray(np.frombuffer(image, np.uint32).reshape(4, -1).T).view(np.float32)


def constructed_images() -> dict:
    """name -> image bytes of any length (the compressor alone takes them: lsr_lzf_deflate), each placing one case of the rule;
    tests/test_pcd_write_cpu.py checks that the tokens meant are the tokens made."""
    rng = np.random.default_rng(4321)

    def unique(k, salt):
        """k random bytes whose 3-byte windows are all distinct (checked)."""
        for attempt in range(100):
            b = np.random.default_rng(salt * 1000 + attempt).integers(0, 256, k, dtype=np.uint8).tobytes()
            if len({b[i:i + 3] for i in range(k - 2)}) == k - 2:
                return b
        raise AssertionError("no such bytes")

    S = {}
    for m in (8, 9, 264, 265):
        # `m` bytes, a separator, the same m bytes again and a byte that differs: the second copy matches over exactly m (265: capped at 264)
        block = unique(m, m)
        S[f"match_{m}"] = block + bytes([block[m - 1] ^ 1, block[0] ^ 2, block[1] ^ 4, block[2] ^ 8]) + block + bytes([block[m - 1] ^ 16])
    for run in (32, 33):
        head = unique(run, 50 + run)          # `run` literals, then a match with the head's first bytes
        S[f"literals_{run}_then_match"] = head + head[:12]
    # the same 300 bytes on both sides of a chunk boundary: the match in front stops at the chunk's end, none reaches back across it
    block = unique(300, 77)
    S["same_bytes_across_a_chunk_boundary"] = unique(CHUNK - 300 - 200, 78) + block + block[:200] + block[200:] + block + unique(96, 79)
    S["chunk_of_one_byte_behind_a_full_one"] = rng.integers(0, 256, CHUNK, dtype=np.uint8).tobytes() + b"\x07"
    S["chunk_of_two_bytes_behind_a_full_one"] = bytes(CHUNK) + b"\x07\x07"
    S["period_3"] = b"abc" * 700
    S["period_3_across_chunks"] = b"xyz" * 3000
    return S
