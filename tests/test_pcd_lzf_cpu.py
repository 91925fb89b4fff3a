"""CPU: reading DATA binary_compressed .pcd files — the test helper's own encoders against its literal decoder; the formulation the
kernels of csrc/pcd_lzf.hip follow (per block of the stream a 33-entry transition map, the maps composed in order, a source word per
output byte, pointer doubling), written here in numpy for blocks of 64 and of 4096 bytes, against that decoder on every hand-made stream
and on 200 random token streams; the keys; lsr_parse_pcd_header's unchanged answer.  The size-word checks need an object, so a device:
they are in tests/test_pcd_lzf_gpu.py with the kernels themselves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pcd_lzf_numpy as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITERAL = 0x80000000
ENTRIES = 33


@pytest.fixture(scope="module")
def hand_made():
    return Z.hand_made_streams()


def sample_bytes():
    rng = np.random.default_rng(5)
    text = b"".join(b"%.8g %.8g\n" % (x, y) for x, y in rng.normal(0, 10, (400, 2)))
    return {"random": rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(), "zeros": bytes(9000), "period_3": b"abc" * 1500,
            "text": text, "floats": np.round(rng.normal(0, 50, 2000), 1).astype(np.float32).tobytes(), "one": b"x", "two": b"xy",
            "few_values": rng.integers(0, 3, 6000, dtype=np.uint8).tobytes()}


def test_encoders_round_trip_through_the_literal_decoder():
    for name, data in sample_bytes().items():
        for enc_name, enc in Z.ENCODERS.items():
            stream = enc(data)
            assert Z.lzf_decompress(stream, len(data)) == data, (name, enc_name)
        assert len(Z.all_literal(data)) == len(data) + (len(data) + 31) // 32
    assert len(Z.greedy(bytes(9000))) < 200 and len(Z.greedy(b"abc" * 1500)) < 100       # the matcher does find runs and patterns
    toks = [("lit", b"abcdefgh"), ("ref", 3, 8), ("ref", 9, 1), ("ref", 264, 5), ("lit", b"z"), ("ref", 8, 280), ("ref", 10, 2)]
    want = bytearray(b"abcdefgh")
    for t in toks[1:]:
        if t[0] == "lit":
            want += t[1]
        else:
            for _ in range(t[1]):
                want.append(want[-t[2]])
    stream = Z.from_tokens(toks)
    assert Z.lzf_decompress(stream, len(want)) == bytes(want) and len(want) == Z.tokens_out(toks)
    assert stream[:9] == b"\x07abcdefgh" and stream[9:11] == bytes([1 << 5, 7]) and stream[11:14] == bytes([7 << 5, 0, 0])   # the two reference forms


def test_literal_decoder_names_the_bad_token():
    good = Z.from_tokens([("lit", b"abcd"), ("ref", 5, 2), ("lit", b"xy"), ("ref", 20, 3)])
    n = 4 + 5 + 2 + 20
    assert len(Z.lzf_decompress(good, n)) == n
    cases = [(Z.from_tokens([("ref", 3, 1)]), 3, 0), (Z.from_tokens([("lit", b"abcd"), ("ref", 3, 5)]), 7, 5),
             (good[:-1], n, 10), (good[:-2], n, 10), (good[:3], n, 0), (good, n - 1, 10), (good, n + 1, None)]
    for stream, n_out, offset in cases:
        with pytest.raises(Z.LzfError) as e:
            Z.lzf_decompress(stream, n_out)
        assert e.value.offset == offset, (stream, n_out)


# ---- the kernels' formulation, in numpy ------------------------------------------------------------------------------------------------
def block_inflate(stream: bytes, n_out: int, block: int, threads: int = 7):
    """csrc/pcd_lzf.hip step by step.  Returns (bytes, doubling passes); raises Z.LzfError like the literal decoder."""
    s = np.frombuffer(stream, np.uint8).astype(np.int64)
    n = len(s)
    nb = (n + block - 1) // block
    # every byte as a control byte: the token's length in the stream and in the output (a length byte behind the stream reads as 0)
    ext = np.concatenate([s[1:], [0]])
    long_form = (s >> 5) == 7
    t_len = np.where(s < 32, s + 2, np.where(long_form, 3, 2))
    o_len = np.where(s < 32, s + 1, np.where(long_form, 9 + ext, (s >> 5) + 2))
    # a. + b.  per block and entry: where the walk leaves into the next block, how many bytes it puts out
    exit_map, out_count = np.zeros((nb, ENTRIES), np.int64), np.zeros((nb, ENTRIES), np.int64)
    for b in range(nb):
        base = b * block
        L = min(block, n - base)
        leave, total = list(range(L + ENTRIES + 1)), [0] * (L + ENTRIES + 1)      # from block byte p on: (position reached - 0, output)
        for p in range(L - 1, -1, -1):
            q = p + int(t_len[base + p])
            leave[p], total[p] = leave[q], total[q] + int(o_len[base + p])
        for e in range(ENTRIES):
            exit_map[b, e], out_count[b, e] = leave[e] - L, total[e]
    assert exit_map.min() >= 0 and exit_map.max() < ENTRIES
    # the scan: each thread composes the maps of its chunk of blocks, one thread the chunks; the stream is entered at byte 0
    chunk = (nb + threads - 1) // threads
    composed = []
    for t in range(threads):
        m = np.arange(ENTRIES)
        for b in range(min(t * chunk, nb), min((t + 1) * chunk, nb)):
            m = exit_map[b][m]
        composed.append(m)
    entry, out_start, e, run = np.zeros(nb, np.int64), np.zeros(nb + 1, np.int64), 0, 0
    for t in range(threads):
        e_t = e
        for b in range(min(t * chunk, nb), min((t + 1) * chunk, nb)):
            entry[b], out_start[b] = e_t, run
            run += out_count[b, e_t]
            e_t = exit_map[b, e_t]
        assert e_t == composed[t][e]
        e = e_t
    out_start[nb] = run
    # c.  the source words, and the bad tokens
    src = np.zeros(n_out, np.int64)
    first_error = None
    for b in range(nb):
        base = b * block
        L = min(block, n - base)
        pos, o = int(entry[b]), int(out_start[b])
        while pos < L:
            g = base + pos
            c, tl, ol = int(s[g]), int(t_len[g]), int(o_len[g])
            bad = g + tl > n or o + ol > n_out
            dist = 0
            if not bad and c >= 32:
                dist = (((c & 31) << 8) | int(s[g + tl - 1])) + 1
                bad = dist > o
            if bad:
                first_error = g if first_error is None else min(first_error, g)
            hi = min(o + ol, n_out)
            if o < hi:
                k = np.arange(o, hi)
                if bad:
                    src[k] = LITERAL
                elif c < 32:
                    src[k] = LITERAL | (g + 1 + k - o)
                else:
                    src[k] = k - dist
            pos += tl
            o += ol
    if first_error is not None:
        raise Z.LzfError(first_error, "bad token")
    if run != n_out:
        raise Z.LzfError(None, "short")
    # d.  src[k] = src[src[k]], four hops a pass, until nothing points at output any more
    passes = 0
    while True:
        todo = np.nonzero(src < LITERAL)[0]
        new = src[todo]
        for _ in range(4):
            live = new < LITERAL
            new[live] = src[new[live]]
        src[todo] = new
        passes += 1
        assert passes <= 32
        if not (new < LITERAL).any():
            break
    assert (src >= LITERAL).all()
    return s[src - LITERAL].astype(np.uint8).tobytes(), passes


def random_tokens(rng, n_stream_bytes):
    toks, out, size = [], 0, 0
    while size < n_stream_bytes:
        kind = rng.integers(0, 4)
        if out == 0 or kind == 0:
            k = int(rng.integers(1, 33)) if rng.random() < 0.7 else int(rng.choice([1, 32]))
            toks.append(("lit", rng.integers(0, 256, k, dtype=np.uint8).tobytes()))
            out, size = out + k, size + 1 + k
        else:
            length = int(rng.choice([3, 4, 8, 9, 10, 264])) if rng.random() < 0.5 else int(rng.integers(3, 265))
            far = min(out, Z.MAX_DIST)
            distance = int(rng.choice([1, min(2, far), far])) if rng.random() < 0.4 else int(rng.integers(1, far + 1))
            toks.append(("ref", length, distance))
            out, size = out + length, size + (3 if length >= 9 else 2)
    return toks, out


def test_block_formulation_on_hand_made_streams(hand_made):
    deepest = 0
    for name, stream in hand_made.items():
        want = Z.lzf_decompress(stream, Z.HAND_BYTES)
        for block in (64, 4096):
            got, passes = block_inflate(stream, Z.HAND_BYTES, block)
            assert got == want, (name, block)
            deepest = max(deepest, passes)
    assert Z.lzf_decompress(hand_made["zeros_depth_of_the_file"], Z.HAND_BYTES) == bytes(Z.HAND_BYTES)
    # a chain as deep as the file (65583 hops): a pass multiplies what a word spans by 5 (its own hop and four more), 5^7 >= 65583
    assert deepest == 7


def test_block_formulation_on_random_token_streams():
    rng = np.random.default_rng(77)
    for k in range(200):
        toks, n_out = random_tokens(rng, int(rng.integers(100, 9000)))
        stream = Z.from_tokens(toks)
        want = Z.lzf_decompress(stream, n_out)
        for block in (64, 4096):
            got, _ = block_inflate(stream, n_out, block, threads=int(rng.integers(1, 9)))
            assert got == want, (k, block)


def test_block_formulation_names_the_literal_decoders_bad_token():
    rng = np.random.default_rng(78)
    for k in range(40):
        toks, n_out = random_tokens(rng, int(rng.integers(200, 3000)))
        stream = Z.from_tokens(toks)
        cut = int(rng.integers(1, len(stream)))
        bad_at = int(rng.integers(1, len(toks)))
        early = Z.from_tokens(toks[:bad_at] + [("ref", 3, min(Z.tokens_out(toks[:bad_at]) + 1 + int(rng.integers(0, 50)), Z.MAX_DIST))] + toks[bad_at:])
        for bad, size in ((stream[:cut], n_out), (stream, n_out - 1), (stream, n_out + 1), (early, n_out + 3)):
            try:
                Z.lzf_decompress(bad, size)
                want = "good"
            except Z.LzfError as e:
                want = e.offset
            for block in (64, 4096):
                try:
                    block_inflate(bad, size, block)
                    got = "good"
                except Z.LzfError as e:
                    got = e.offset
                assert got == want, (k, block, size - n_out)


# ---- the keys and the header parser ----------------------------------------------------------------------------------------------------
def test_keys_exist_and_agree():
    from lidarslam_ros2_amd import _capi
    from lidarslam_ros2_amd.registration import Registration

    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    assert _capi.PCD_READ_COMPRESSED == 54 and re.search(r"LSR_PCD_READ_COMPRESSED\s*=\s*54\b", hdr)
    assert _capi.PCD_INFLATE_MS == 14 and re.search(r"LSR_PCD_INFLATE_MS\s*=\s*14\b", hdr)
    assert callable(Registration.pcdReadCompressed)
    assert "pcdReadCompressed" in open(os.path.join(ROOT, "include", "lidarslam_reg", "pcd_io.hpp")).read()
    lib = _capi.load()
    v = C.c_int(7)
    assert lib.lsr_set_i32(None, 54, 1) == -1 and lib.lsr_get_i32(None, 54, C.byref(v)) == -1 and v.value == 7   # no handle: refused


def test_parse_pcd_header_keeps_its_answer():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    rec = np.arange(40, dtype=np.float32).reshape(5, 8)
    img = Z.compressed_file(*Z.XYZI_FIELDS, Z.xyzi_columns(rec), 5, Z.greedy)
    info = _capi.PcdInfo()
    assert lib.lsr_parse_pcd_header(img, len(img), C.byref(info)) == -6
    assert b"binary_compressed" in lib.lsr_last_error()
    assert (info.data_kind, info.n_points, info.point_step, info.has_intensity) == (2, 5, 16, 1)
    assert info.data_offset == img.index(b"DATA binary_compressed\n") + len(b"DATA binary_compressed\n")
    # the oracle reads the same image: the records of the cloud
    want = np.zeros((5, 8), np.float32)
    want[:, [0, 1, 2, 4]] = rec[:, [0, 1, 2, 4]]
    assert (Z.decode_compressed(img) == want.view(np.uint8).reshape(5, 32)).all()


# ---- the stand-alone C++ codec of the timing tool --------------------------------------------------------------------------------------
def test_cpp_greedy_codec_against_the_literal_decoder(hand_made):
    """tests/cpp/lzf_greedy.cpp: what its encoder writes is a valid stream to the Python decoder, and its decoder agrees with the Python
    one on good streams and names the same bad token."""
    import lzf_codec

    lib = lzf_codec.load_codec()
    for name, data in sample_bytes().items():
        stream = lzf_codec.compress(lib, data).tobytes()
        assert Z.lzf_decompress(stream, len(data)) == data, name
        st, out = lzf_codec.decompress(lib, stream, len(data))
        assert st == len(data) and out.tobytes() == data
    assert len(lzf_codec.compress(lib, bytes(100000))) < 1300     # runs are found: 264 bytes per 3-byte token
    for name in ("zeros_depth_of_the_file", "lengths_3_8_9_10_264", "three_levels_across_a_field", "first_literal_17"):
        st, out = lzf_codec.decompress(lib, hand_made[name], Z.HAND_BYTES)
        assert st == Z.HAND_BYTES and out.tobytes() == Z.lzf_decompress(hand_made[name], Z.HAND_BYTES), name
    good = hand_made["distance_8192_and_1"]
    for stream, n_out in ((good[:-1], Z.HAND_BYTES), (good[:5000], Z.HAND_BYTES), (good, Z.HAND_BYTES - 1), (good, Z.HAND_BYTES + 1),
                          (Z.from_tokens([("lit", b"ab"), ("ref", 3, 3)]), 5)):
        with pytest.raises(Z.LzfError) as e:
            Z.lzf_decompress(stream, n_out)
        st, _ = lzf_codec.decompress(lib, stream, n_out)
        assert st == -1 - (len(stream) if e.value.offset is None else e.value.offset)
