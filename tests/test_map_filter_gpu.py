"""The VoxelGrid filter for map-sized clouds on the device (lsr_voxel_grid_filter_map, lsr_assemble_map_filtered,
lsr_save_map_pcd_filtered; csrc/map_filter.hip) against the numpy restatement tests/map_filter_numpy.py and, where the int32 grid
applies, against the existing filter lsr_voxel_grid_filter_pc2.  Every comparison is np.array_equal on the raw bytes of the records:
there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import map_filter_numpy as mfn
from lidarslam_ros2_amd import MapArray, NormalDistributionsTransform, SubMap, _capi

pytestmark = pytest.mark.gpu

XYZI = (32, (0, 4, 8, 16))
L16 = (16, (0, 4, 8, None))       # packed xyzw, no intensity
L48 = (48, (8, 12, 16, 4))        # fields in the middle of a longer record, intensity first
ERR_INVALID_ARGUMENT = -1


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)


@pytest.fixture(scope="module")
def reg():
    return NormalDistributionsTransform(device=0)


def _records(rng, n, layout, extent=60.0):
    """n records of `layout`: every word a finite float in +-extent, padding words included (the output must not carry them)."""
    return rng.uniform(-extent, extent, (n, layout[0] // 4)).astype(np.float32)


# ---- 1. the same bytes as the int32 filter where it applies ---------------------------------------------------------------------
@pytest.mark.parametrize("layout", [XYZI, L16, L48], ids=["xyzi", "packed16", "wide48"])
def test_same_bytes_as_the_int32_filter(reg, layout):
    """5 000 records in +-60 m at leaf 0.5 (240^3 cells: int32), 1 % of them with a NaN or an inf coordinate: restatement == existing
    kernel == new kernel, from host and from device input."""
    rng = np.random.default_rng(301)
    rec = _records(rng, 5000, layout)
    step, offs = layout
    bad = rng.choice(5000, 50, replace=False)
    for k, i in enumerate(bad):
        rec[i, offs[k % 3] // 4] = [np.nan, np.inf, -np.inf][(k // 3) % 3]
    want = mfn.voxel_grid_filter_map(rec, 0.5, layout, layout)
    old = reg.voxelGridFilterPointCloud2(rec.view(np.uint8).reshape(-1), 5000, step, offs, 0.5, step, offs)
    assert 0 < want.shape[0] <= 4950 and np.array_equal(old, want)
    got_host = reg.voxelGridFilterMap(rec, 0.5, layout, layout)
    assert isinstance(got_host, np.ndarray) and got_host.shape == want.shape and np.array_equal(got_host, want)
    assert 1 <= reg.mapFilterKeyBits() <= 31
    got_dev = reg.voxelGridFilterMap(_cuda(rec), 0.5, layout, layout)
    assert got_dev.is_cuda and np.array_equal(_host(got_dev), want)
    # another output layout: the same centroids at other offsets, every other byte zero
    other = reg.voxelGridFilterMap(_cuda(rec), 0.5, layout, L48)
    assert np.array_equal(_host(other), mfn.voxel_grid_filter_map(rec, 0.5, layout, L48))


# ---- 2. the high word decides the order -----------------------------------------------------------------------------------------
def test_high_word_decides_the_order(reg):
    rec = mfn.high_word_cloud()
    want, idx = mfn.voxel_grid_filter_map(rec, 0.25, XYZI, XYZI, return_index=True)
    assert idx.tolist() == [0, 4295426053, 4295426057, 4578149586, 8873116882, 17179869183]
    # the existing filter refuses the cloud ...
    lay = _capi.Pc2Layout(32, 0, 4, 8, 16)
    out = np.zeros((rec.shape[0], 32), np.uint8)
    n_out = C.c_size_t(12345)
    st = reg._lib.lsr_voxel_grid_filter_pc2(reg._h, C.c_void_p(rec.ctypes.data), rec.shape[0], C.byref(lay), C.c_float(0.25),
                                            C.c_void_p(out.ctypes.data), out.shape[0], C.byref(lay), C.byref(n_out))
    assert st == _capi.ERR_INDEX_OVERFLOW
    # ... the new one orders it by both words
    for src in (rec, _cuda(rec)):
        got = reg.voxelGridFilterMap(src, 0.25)
        assert got.shape == (6, 32) and np.array_equal(_host(got), want)
        assert reg.mapFilterKeyBits() == 34


# ---- 3. map-scale extents at a leaf that is no power of two ---------------------------------------------------------------------
def test_map_scale_extents(reg):
    """600 leaf centres over 30 000 x 30 000 x 3 000 cells of 0.1 m, 4 096 points dealt to them at random with +-0.03 m of jitter."""
    rng = np.random.default_rng(303)
    centres = (np.column_stack([rng.integers(0, 30000, 600), rng.integers(0, 30000, 600), rng.integers(0, 3000, 600)]) + 0.5) * 0.1
    rec = np.zeros((4096, 8), np.float32)
    rec[:, :3] = (centres[rng.integers(0, 600, 4096)] + rng.uniform(-0.03, 0.03, (4096, 3))).astype(np.float32)
    rec[:, 4] = rng.uniform(0.0, 255.0, 4096).astype(np.float32)
    want = mfn.voxel_grid_filter_map(rec, 0.1, XYZI, XYZI)
    x, y, z, _ = mfn.fields(rec, XYZI)
    bits = mfn.index_bits(mfn.leaf_index(x, y, z, 0.1)[2])
    assert 590 <= want.shape[0] <= 600 and 40 <= bits <= 42
    got = reg.voxelGridFilterMap(rec, 0.1)
    assert np.array_equal(got, want) and reg.mapFilterKeyBits() == bits
    import torch

    out = torch.full((4096, 32), 0xAB, dtype=torch.uint8, device="cuda")
    got = reg.voxelGridFilterMap(_cuda(rec), 0.1, out=out)
    assert got.is_cuda and got.data_ptr() == out.data_ptr() and np.array_equal(_host(got), want)
    assert bool((out[want.shape[0]:] == 0xAB).all())     # nothing behind the last leaf's record is written
    again = reg.voxelGridFilterMap(_cuda(rec), 0.1)
    assert np.array_equal(_host(again), want)            # bit-identical from call to call


# ---- 4. run lengths and block seams ---------------------------------------------------------------------------------------------
def test_run_lengths_and_block_seams(reg):
    """2 * 2048 + 17 points: leaves of 2, 3, 4, 5, 7, 8 and 300 points — the 300 spread over the whole cloud —, every other point a leaf
    of its own; the leaves lie over 60 000 x 60 000 x 4 cells of 0.25 m, so both index words are sorted.  The sort's 2 048-key
    workgroups, the run finder's 256-key chunks, the four-way gather's remainders and the float summation order."""
    rng = np.random.default_rng(304)
    n = 2 * 2048 + 17
    sizes = [2, 3, 4, 5, 7, 8, 300]
    n_leaves = len(sizes) + n - sum(sizes)
    flat = rng.choice(60000 * 60000 * 4, n_leaves, replace=False)
    cells = np.column_stack([flat % 60000, (flat // 60000) % 60000, flat // (60000 * 60000)])
    leaf_of = np.concatenate([np.repeat(np.arange(len(sizes)), sizes), np.arange(len(sizes), n_leaves)])
    leaf_of = leaf_of[rng.permutation(n)]
    rec = np.zeros((n, 8), np.float32)
    rec[:, :3] = ((cells[leaf_of] + 0.5) * 0.25 + rng.uniform(-0.1, 0.1, (n, 3))).astype(np.float32)
    rec[:, 4] = rng.uniform(0.0, 255.0, n).astype(np.float32)
    big = np.flatnonzero(leaf_of == len(sizes) - 1)
    assert big.size == 300 and big.min() < 256 and big.max() > n - 256
    want = mfn.voxel_grid_filter_map(rec, 0.25, XYZI, XYZI)
    assert want.shape[0] == n_leaves
    for src in (rec, _cuda(rec)):
        got = reg.voxelGridFilterMap(src, 0.25)
        assert np.array_equal(_host(got), want)
        assert reg.mapFilterKeyBits() > 32


def test_one_point_and_no_finite_point(reg):
    one = np.array([[1.0, -2.0, 3.0, 9.0, 7.5, 9.0, 9.0, 9.0]], np.float32)
    got = reg.voxelGridFilterMap(one, 0.1)
    assert got.shape == (1, 32) and np.array_equal(got.view(np.float32)[0], [1.0, -2.0, 3.0, 0.0, 7.5, 0.0, 0.0, 0.0])
    none = np.full((300, 8), np.nan, np.float32)
    none[::2, 1] = np.inf
    for src in (none, _cuda(none)):
        got = reg.voxelGridFilterMap(src, 0.1)
        assert got.shape == (0, 32)
    empty = reg.voxelGridFilterMap(np.zeros((0, 8), np.float32), 0.1)
    assert empty.shape == (0, 32)


def test_a_workgroup_without_a_finite_point_and_a_run_over_the_chunk_seam(reg):
    """2 049 records: the bounding-box passes of both filters walk them with three workgroups (workgroup b takes the records i with
    (i mod 768) // 256 == b), the second of which meets nothing but NaN x, so its record is the empty box; the third is partly
    filled.  The finite records: a leaf of 250 points, then one of 20 — sorted positions 250..269, over the run finder's 256-key
    seam — then a leaf each.  The int32 filter (twice on a fresh object: grid dimensions on the host, then folded on the device from
    the ingest's records) and the map filter against the restatement."""
    rng = np.random.default_rng(305)
    n = 2049
    finite = np.flatnonzero((np.arange(n) % 768) // 256 != 1)
    assert finite.size == 1281
    cell_x = np.concatenate([np.zeros(250), np.ones(20), 2 + np.arange(finite.size - 270)])
    rec = np.zeros((n, 8), np.float32)
    rec[:, 0] = np.nan
    rec[:, 1:3] = rng.uniform(-5.0, 5.0, (n, 2)).astype(np.float32)     # finite y, z beside the NaN x: the test is on all three
    rec[finite, :3] = (np.column_stack([cell_x[rng.permutation(finite.size)], np.zeros(finite.size), np.zeros(finite.size)])
                       + rng.uniform(0.1, 0.9, (finite.size, 3))).astype(np.float32)
    rec[:, 4] = rng.uniform(0.0, 255.0, n).astype(np.float32)
    want = mfn.voxel_grid_filter_map(rec, 1.0, XYZI, XYZI)
    assert want.shape[0] == finite.size - 268
    fresh = NormalDistributionsTransform(device=0)
    for _ in range(2):
        old = fresh.voxelGridFilterPointCloud2(rec.view(np.uint8).reshape(-1), n, 32, XYZI[1], 1.0, 32, XYZI[1])
        assert np.array_equal(old.reshape(-1, 32), want.view(np.uint8).reshape(-1, 32))
    for src in (rec, _cuda(rec)):
        assert np.array_equal(_host(reg.voxelGridFilterMap(src, 1.0)).view(np.uint8).reshape(-1, 32), want.view(np.uint8).reshape(-1, 32))


def test_records_behind_two_gib(reg):
    """2^26 + 4096 records of 32 bytes: the byte offset of the last 4 096 passes 2^31, and they are the only finite ones (the records
    in front have a NaN x and are dropped), so the bounding box, the keys and the centroids all come from behind that offset.  The
    result is the restatement's of those 4 096 records alone."""
    import torch

    rng = np.random.default_rng(308)
    tail = np.zeros((4096, 8), np.float32)
    tail[:, :3] = rng.uniform(-30.0, 30.0, (4096, 3)).astype(np.float32)
    tail[:, 4] = rng.uniform(0.0, 255.0, 4096).astype(np.float32)
    n = (1 << 26) + 4096
    rec = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    rec[: 1 << 26, 0] = float("nan")
    rec[1 << 26:] = torch.from_numpy(tail).cuda()
    want = mfn.voxel_grid_filter_map(tail, 2.0, XYZI, XYZI)
    got = reg.voxelGridFilterMap(rec, 2.0)
    assert 1000 < want.shape[0] < 4096 and np.array_equal(_host(got), want)


# ---- 5. composition -------------------------------------------------------------------------------------------------------------
def _pose(rng):
    q = rng.normal(size=4)
    return tuple(rng.uniform(-2000.0, 2000.0, 3)), tuple(q / np.linalg.norm(q))


def _on_device(submaps):
    return [SubMap(_cuda(s.cloud), s.position, s.orientation, s.distance) for s in submaps]


@pytest.fixture(scope="module")
def drive():
    """Three submaps of 700 / 0 / 1 300 records within +-60 m of poses spread over +-2 000 m: at leaf 0.1 the index needs more than 32
    bits.  And the optimiser's poses for them.  Shared, never modified."""
    rng = np.random.default_rng(305)
    sm = [SubMap(_records(rng, n, XYZI), *_pose(rng)) for n in (700, 0, 1300)]
    poses = []
    for _ in sm:
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        x, y, z, w = q
        P = np.eye(4)
        P[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        P[:3, 3] = rng.uniform(-2000.0, 2000.0, 3)
        poses.append(P)
    return sm, poses


@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
@pytest.mark.parametrize("with_poses", [False, True], ids=["own_poses", "optimised_poses"])
def test_assemble_filtered_equals_the_two_steps(reg, drive, resident, with_poses):
    sm, poses = drive
    sm = _on_device(sm) if resident else sm
    poses = poses if with_poses else None
    raw, first = reg.assembleMap(sm, poses)
    assert raw.shape == (2000, 32) and first.tolist() == [0, 700, 700, 2000]
    want = reg.voxelGridFilterMap(raw, 0.1)
    assert reg.mapFilterKeyBits() > 32
    got, none = reg.assembleMap(sm, poses, leaf=0.1)
    assert none is None and hasattr(got, "is_cuda") == resident
    assert 0 < got.shape[0] <= 2000 and np.array_equal(_host(got), _host(want))
    # ... and the two steps are what the restatement makes of the raw map
    assert np.array_equal(_host(want), mfn.voxel_grid_filter_map(_host(raw), 0.1, XYZI, XYZI))


# ---- 6. save --------------------------------------------------------------------------------------------------------------------
def _map_array(submaps):
    ma = MapArray()
    ma.submaps = list(submaps)
    return ma


@pytest.mark.parametrize("kind", ["ascii", "binary", "binary_compressed"])
def test_save_map_filtered(reg, drive, tmp_path, kind):
    sm, poses = drive
    ma = _map_array(_on_device(sm))
    thin, _ = ma.modified_map(reg, poses, leaf=0.1)
    a, b = str(tmp_path / "filtered.pcd"), str(tmp_path / "apart.pcd")
    size = ma.save_map(reg, a, poses, data=kind, leaf=0.1)
    assert reg.getSavedMapPoints() == thin.shape[0]
    assert reg.savePCDFile(b, thin, XYZI, kind) == size
    assert open(a, "rb").read() == open(b, "rb").read()
    if kind == "binary":
        return
    was = reg.pcdReadCompressed()
    reg.pcdReadCompressed(True)
    try:
        back = reg.loadPCDFile(a)
    finally:
        reg.pcdReadCompressed(was)
    want = _host(thin).copy()
    if kind == "ascii":   # the text carries eight significant digits: the records of the file are those of the text
        f = want.view(np.float32)
        for col in (0, 1, 2, 4):
            f[:, col] = [np.float32("%.8g" % v) for v in f[:, col]]
    assert np.array_equal(back, want)


# ---- 7. contract ----------------------------------------------------------------------------------------------------------------
def _call(reg, rec, leaf, out, capacity, n_out):
    lay = _capi.Pc2Layout(32, 0, 4, 8, 16)
    return reg._lib.lsr_voxel_grid_filter_map(reg._h, C.c_void_p(rec.ctypes.data), rec.shape[0], C.byref(lay), 0, C.c_float(leaf),
                                              None if out is None else C.c_void_p(out.ctypes.data), capacity, C.byref(lay), 0,
                                              C.byref(n_out))


def test_contract(reg):
    rng = np.random.default_rng(307)
    rec = _records(rng, 500, XYZI)
    target = _records(rng, 800, XYZI)[:, :3].copy()
    reg.setInputTarget(target)
    T_before = reg.getFinalTransformation().copy()
    n_out = C.c_size_t(777)
    out = np.full((500, 32), 0xCD, np.uint8)
    for leaf in (0.0, -0.5, float("nan")):
        assert _call(reg, rec, leaf, out, 500, n_out) == ERR_INVALID_ARGUMENT
    assert n_out.value == 777 and bool((out == 0xCD).all())
    # beyond the limits: refused on the host, before any launch that depends on them
    far = np.zeros((2, 8), np.float32)
    far[1, 0] = 3.0e5                                   # div_b > 2^21 at leaf 0.1
    assert _call(reg, far, 0.1, out, 500, n_out) == _capi.ERR_INDEX_OVERFLOW and b"2^21" in reg._lib.lsr_last_error()
    far = np.zeros((1, 8), np.float32)
    far[0, 1] = 2.0e6                                   # a cell coordinate >= 2^24
    assert _call(reg, far, 0.1, out, 500, n_out) == _capi.ERR_INDEX_OVERFLOW and b"2^24" in reg._lib.lsr_last_error()
    assert n_out.value == 777 and bool((out == 0xCD).all())
    # out_data = NULL: the count
    want = mfn.voxel_grid_filter_map(rec, 0.5, XYZI, XYZI)
    assert _call(reg, rec, 0.5, None, 0, n_out) == 0 and n_out.value == want.shape[0]
    # a capacity one short: the count, and the buffer untouched
    n_out = C.c_size_t(777)
    assert _call(reg, rec, 0.5, out, want.shape[0] - 1, n_out) == ERR_INVALID_ARGUMENT
    assert n_out.value == want.shape[0] and bool((out == 0xCD).all())
    assert _call(reg, rec, 0.5, out, want.shape[0], n_out) == 0
    assert np.array_equal(out[: want.shape[0]], want) and bool((out[want.shape[0]:] == 0xCD).all())
    # what the object otherwise answers is unchanged
    assert np.array_equal(reg.getFinalTransformation(), T_before)
    score_source = target[:100].copy()
    reg.setInputSource(score_source)
    assert reg.getFitnessScore() < 1e-6                  # the target is still those 800 points: every source point lies on one
