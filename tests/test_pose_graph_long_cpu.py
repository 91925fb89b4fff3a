"""The host side of `lsr_optimize_pose_graph_long` (pose graphs with up to 1024 edges outside the band): the symbol, its binding and its
limit against include/lidarslam_reg.h, the old entry's limit unchanged, every link line of csrc/Makefile.  No device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()


def test_long_limit_macro_equals_the_binding_constant():
    from lidarslam_ros2_amd import _capi

    hdr = _header()
    assert int(re.search(r"#define LSR_POSE_GRAPH_LONG_MAX_OFFBAND_EDGES (\d+)", hdr).group(1)) == _capi.POSE_GRAPH_LONG_MAX_OFFBAND_EDGES == 1024


def test_old_limit_is_still_64():
    from lidarslam_ros2_amd import _capi

    assert int(re.search(r"#define LSR_POSE_GRAPH_MAX_OFFBAND_EDGES (\d+)", _header()).group(1)) == _capi.POSE_GRAPH_MAX_OFFBAND_EDGES == 64


def test_long_symbol_has_nine_argtypes_and_refuses_a_null_handle():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    assert "lsr_optimize_pose_graph_long" in _capi.EXPORTED_SYMBOLS and re.search(r"\blsr_optimize_pose_graph_long\s*\(", _header())
    assert len(lib.lsr_optimize_pose_graph_long.argtypes) == 9
    assert list(lib.lsr_optimize_pose_graph_long.argtypes) == list(lib.lsr_optimize_pose_graph.argtypes)
    assert lib.lsr_optimize_pose_graph_long(None, None, 0, None, 0, None, None, None, None) == -1
    assert b"null handle" in lib.lsr_last_error()


def test_stage_time_keys_mirror_the_header():
    from lidarslam_ros2_amd import _capi

    hdr = _header()
    for name in ("POSE_GRAPH_BAND_SOLVE_MS", "POSE_GRAPH_DENSE_MS", "POSE_GRAPH_COMBINE_MS"):
        assert int(re.search(r"LSR_%s = (\d+)," % name, hdr).group(1)) == getattr(_capi, name)


def test_the_dense_object_is_on_every_link_line():
    mk = open(os.path.join(ROOT, "lidarslam_ros2_amd", "csrc", "Makefile")).read()
    links = [l for l in mk.splitlines() if "-shared" in l]
    assert len(links) == 3
    for l in links:
        assert "pose_graph_dense.o" in l or "$(OBJS)" in l
    assert "pose_graph_dense.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
