"""TEST AND TOOL INFRASTRUCTURE: builds tests/cpp/lzf_greedy.cpp — the stand-alone greedy LZF encoder and literal decoder — once per
checkout and binds it through ctypes (tests/test_pcd_lzf_cpu.py, tools/pcd_compressed_timing.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lzf_greedy.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "liblzf_greedy.so")


def build_codec() -> str:
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < os.path.getmtime(SRC):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        tmp = OUT + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", tmp])
        os.replace(tmp, OUT)
    return OUT


def load_codec():
    lib = C.CDLL(build_codec())
    lib.lzfg_bound.restype = C.c_size_t
    lib.lzfg_bound.argtypes = [C.c_size_t]
    lib.lzfg_compress.restype = lib.lzfg_decompress.restype = C.c_longlong
    lib.lzfg_compress.argtypes = lib.lzfg_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    return lib


def compress(lib, data) -> np.ndarray:
    """uint8 array: the greedy encoder's stream for `data` (bytes or a contiguous uint8 array)."""
    src = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    out = np.empty(lib.lzfg_bound(src.size), np.uint8)
    size = lib.lzfg_compress(src.ctypes.data, src.size, out.ctypes.data, out.size)
    assert size >= 0
    return out[:size]


def decompress(lib, stream, n_out: int):
    """(status, uint8 array): lzfg_decompress's return value and the buffer it filled."""
    src = np.frombuffer(stream, np.uint8) if isinstance(stream, (bytes, bytearray)) else np.ascontiguousarray(stream)
    out = np.zeros(n_out, np.uint8)
    return int(lib.lzfg_decompress(src.ctypes.data, src.size, out.ctypes.data, n_out)), out
