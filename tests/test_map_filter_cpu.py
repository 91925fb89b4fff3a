"""CPU: the host side of the map filter (lsr_voxel_grid_filter_map, lsr_assemble_map_filtered, lsr_save_map_pcd_filtered) — the numpy
restatement tests/map_filter_numpy.py pinned to the project's oracle where the int32 grid applies, the C ABI's symbols, keys and null
handle check, the C++ adapter's snippets.  The kernels: tests/test_map_filter_gpu.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import map_filter_numpy as mfn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XYZI = (32, (0, 4, 8, 16))
PACKED = (16, (0, 4, 8, 12))


@pytest.fixture(scope="module")
def cloud():
    """3 000 points in +-60 m x +-60 m x +-5 m with an intensity: (n, 4) float32; shared, never modified."""
    rng = np.random.default_rng(7)
    return np.column_stack([rng.uniform(-60, 60, 3000), rng.uniform(-60, 60, 3000), rng.uniform(-5, 5, 3000),
                            rng.uniform(0, 255, 3000)]).astype(np.float32)


@pytest.mark.parametrize("leaf", [0.5, 0.1])
def test_restatement_equals_the_oracle_on_an_int32_grid(cloud, leaf):
    from oracle import oracle as O

    want = O.voxel_grid_filter_xyzi(cloud, leaf, 3)
    got = mfn.voxel_grid_filter_map(cloud, leaf, PACKED, PACKED).view(np.float32).reshape(-1, 4)
    assert got.shape == want.shape and 0 < got.shape[0] <= cloud.shape[0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_restatement_on_the_wide_index_of_the_gpu_test():
    """The cloud of the GPU suite's high-word test: six leaves, these indices, 34 bits."""
    rec = mfn.high_word_cloud()
    out, idx = mfn.voxel_grid_filter_map(rec, 0.25, XYZI, XYZI, return_index=True)
    assert idx.tolist() == [0, 4295426053, 4295426057, 4578149586, 8873116882, 17179869183] and out.shape == (6, 32)
    x, y, z, _ = mfn.fields(rec, XYZI)
    _, _, div_b = mfn.leaf_index(x, y, z, 0.25)
    assert div_b == (65536, 65536, 4) and mfn.index_bits(div_b) == 34
    assert (4578149586 & 0xFFFFFFFF) == (8873116882 & 0xFFFFFFFF) == 283182290


def test_restatement_refuses_what_is_beyond_the_limits():
    far = np.array([[0, 0, 0, 0], [3.0e5, 0, 0, 0]], np.float32)
    with pytest.raises(mfn.IndexOverflow):
        mfn.voxel_grid_filter_map(far, 0.1, PACKED, PACKED)
    with pytest.raises(mfn.IndexOverflow):
        mfn.voxel_grid_filter_map(np.array([[2.0e6, 0, 0, 0]], np.float32), 0.1, PACKED, PACKED)


def test_symbols_and_keys_exist():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    for name in ("lsr_voxel_grid_filter_map", "lsr_assemble_map_filtered", "lsr_save_map_pcd_filtered"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes
    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    assert _capi.MAP_FILTER_KEY_BITS == 55 and re.search(r"LSR_MAP_FILTER_KEY_BITS\s*=\s*55\b", hdr)
    assert _capi.MAP_FILTER_BBOX_MS == 16 and re.search(r"LSR_MAP_FILTER_BBOX_MS\s*=\s*16\b", hdr)
    assert _capi.MAP_FILTER_WRITE_MS == 21 and re.search(r"LSR_MAP_FILTER_WRITE_MS\s*=\s*21\b", hdr)
    assert "scanmatcher_component.cpp:529-552" in hdr and "graph_based_slam_component.cpp:321-369" in hdr


def test_null_handle_is_refused():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    assert lib.lsr_voxel_grid_filter_map(None, None, 0, None, 0, 0.1, None, 0, None, 0, None) == -1
    assert b"null handle" in lib.lsr_last_error()
    assert lib.lsr_assemble_map_filtered(None, None, 0, None, 0, None, 0.1, None, 0, None, 0, None) == -1
    assert b"null handle" in lib.lsr_last_error()
    assert lib.lsr_save_map_pcd_filtered(None, b"/dev/null", None, 0, None, 0, None, 0.1, 0, None, None) == -1
    assert b"null handle" in lib.lsr_last_error()


def test_cpp_adapter_snippets_compile(tmp_path):
    """the blocks of tests/cpp/map_filter_snippets.cpp, compiled against include/lidarslam_reg/map_assembly.hpp and
    pcd_io.hpp and linked against the library, like the other snippet files; the program shows every helper with a leaf refusing a
    call without a handle (no device needed), the payload emptied and no file left behind."""
    import textwrap

    src = os.path.join(ROOT, "tests", "cpp", "map_filter_snippets.cpp")
    libdir = os.path.join(ROOT, "lidarslam_ros2_amd")
    exe = str(tmp_path / "map_filter_snippets")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir,
                           "-llidarslam_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0 and "MAP_FILTER_SNIPPETS refused=6 emptied=1 payload=0 file=0" in run.stdout, (run.stdout, run.stderr)
    text, doc = open(src).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc.split("### 3i.")[1]
    for k, name in enumerate(("publish_map", "save_map")):
        block = text.split(f"// [map-filter-snippet begin: {name}]\n")[1].split(f"  // [map-filter-snippet end: {name}]")[0]
        assert textwrap.dedent(block).strip("\n").rstrip() in textwrap.dedent(section.split("```cpp\n")[k + 1].split("```")[0])
