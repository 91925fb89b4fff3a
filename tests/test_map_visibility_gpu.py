"""Visibility votes on the device: the depth images, their erosion, the votes and the static map bit for bit against
the numpy float32 restatement (tests/map_visibility_numpy.py) — array_equal throughout, the definition is exact — and the behaviour test
of the definition on the device."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from lidarslam_ros2_amd import MapArray, NormalDistributionsTransform, SubMap, VisibilityParams, _capi, visibilityPairs
from lidarslam_ros2_amd.posemath import matrix_from_pose, quaternion_from_matrix
from lidarslam_ros2_amd.synth import pose_matrix

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_visibility_numpy as MV  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
XYZI32 = (32, (0, 4, 8, 16))
XYZI20 = (20, (8, 0, 4, 16))     # z first in memory order, intensity last
XYZ12 = (12, (0, 4, 8, None))    # an output layout without intensity
SHAPES = ((8, 4), (128, 32))


@pytest.fixture(scope="module")
def reg():
    return NormalDistributionsTransform(0)


def _u32(a):
    a = a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _cloud(n, seed):
    """n records in a +-20 m box, one in sixteen of them with a NaN or an infinity in one coordinate; columns x y z intensity."""
    rng = np.random.default_rng(1000 + seed)
    pts = np.concatenate([rng.uniform(-20, 20, (n, 2)), rng.uniform(-3, 6, (n, 1)), rng.uniform(0, 255, (n, 1))], axis=1).astype(F)
    bad = np.arange(5, n, 16)
    pts[bad, bad % 3] = np.array([np.nan, np.inf, -np.inf], F)[(bad // 16) % 3]
    return pts


def _records(pts, layout):
    """(n, 4) x y z intensity -> float records of `layout`; every other word holds something that must not be read."""
    out = np.full((pts.shape[0], layout[0] // 4), 9.0, F)
    for k in range(4):
        if layout[1][k] is not None:
            out[:, layout[1][k] // 4] = pts[:, k]
    return out


def _sm(cloud, position=(0.0, 0.0, 0.0)):
    return SubMap(cloud, position)


_scenes = {}


def _scene(name):
    """A table of submaps with poses a few metres apart, built once: dict(pts: the (n_i, 4) clouds, subs(layout, device): the SubMaps,
    poses: other poses (what an optimiser would hand back))."""
    if name in _scenes:
        return _scenes[name]
    sizes, far = {"one": ((5000,), None), "two": ((5000, 3000), None), "six": ((5000, 0, 1, 63, 64, 65), 4),
                  "big": ((5000, 65), None)}[name]
    rng = np.random.default_rng(len(name))
    pts = [_cloud(n, 10 * len(name) + i) for i, n in enumerate(sizes)]
    stored, other = [], []
    for i in range(len(sizes)):
        for out in (stored, other):
            x, y, z = (200.0, 50.0, 0.0) if i == far else rng.uniform(-4, 4, 3) * (1.0, 1.0, 0.1)
            out.append(pose_matrix(x, y, z, rng.uniform(-0.4, 0.4), rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03)))

    def subs(layout=XYZI32, device=False):
        import torch

        out = []
        for c, M in zip(pts, stored):
            rec = _records(c, layout)
            out.append(SubMap(torch.from_numpy(rec).cuda() if device else rec, tuple(M[:3, 3]), tuple(quaternion_from_matrix(M[:3, :3])), 0.0))
        return out

    _scenes[name] = dict(pts=pts, subs=subs, poses=np.stack(other), refs={})
    return _scenes[name]


def _ref(name, p, poses=False):
    """The restatement on a scene, computed once per parameter set: (E, votes) with the pair table of the host entry."""
    sc = _scene(name)
    key = (tuple(p), poses)
    if key not in sc["refs"]:
        first, other, rel = visibilityPairs(sc["subs"](), sc["poses"] if poses else None, p)
        E = MV.images(sc["pts"], p)
        sc["refs"][key] = (E, MV.votes(sc["pts"], first, other, rel, E, p), first)
    return sc["refs"][key]


def _params(W=128, H=32, **kw):
    return VisibilityParams(face_width=W, height=H, **kw)


# ---- images ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (0.4, -0.25, 1.1)])
def test_image_bits(reg, W, H, origin):
    import torch

    p = _params(W, H, sensor_origin=origin)
    sizes = (0, 1, 63, 64, 65, 5000, 9000)        # 9000: more than two workgroups' slices of one image
    pts = [_cloud(n, n) for n in sizes]
    D = MV.images(pts, p, eroded=False)
    E = MV.images(pts, p)
    assert np.isinf(D[0]).all() and np.isfinite(D[-1]).sum() > min(100, W * H) and not np.array_equal(D, E)
    for layout in (XYZI32, XYZI20):
        host = [_sm(_records(c, layout)) for c in pts]
        dev = [_sm(torch.from_numpy(h.cloud).cuda()) for h in host]
        got = reg.depthImages(host, p, layout, eroded=False)
        assert got.dtype == np.float32 and got.shape == (len(sizes), H, 4 * W)
        assert np.array_equal(_u32(got), _u32(D)), layout
        assert np.array_equal(_u32(reg.depthImages(host, p, layout)), _u32(E))
        got_dev = reg.depthImages(dev, p, layout)
        assert got_dev.is_cuda and np.array_equal(_u32(got_dev), _u32(E))
        assert np.array_equal(_u32(reg.depthImages(dev, p, layout, eroded=False)), _u32(D))
        out_host = np.full((len(sizes), H, 4 * W), 5.0, F)           # device input, host output, into a buffer that held something
        reg.depthImages(dev, p, layout, out_host)
        assert np.array_equal(_u32(out_host), _u32(E))
        out_dev = torch.full((len(sizes), H, 4 * W), 5.0, dtype=torch.float32, device="cuda")   # host input, device output
        reg.depthImages(host, p, layout, out_dev, eroded=False)
        assert np.array_equal(_u32(out_dev), _u32(D))
    rev = reg.depthImages([_sm(_records(c[::-1].copy(), XYZI32)) for c in pts], p)     # another order: the same bytes
    assert np.array_equal(_u32(rev), _u32(E))


def test_appending_images_writes_the_bytes_of_the_whole_call(reg):
    import torch

    p = _params()
    sizes = (300, 0, 4097, 65, 0, 5000, 1, 8193, 64)
    pts = [_cloud(n, 50 + i) for i, n in enumerate(sizes)]
    E = MV.images(pts, p)
    for device in (False, True):
        subs = [_sm(torch.from_numpy(_records(c, XYZI32)).cuda() if device else _records(c, XYZI32)) for c in pts]
        assert np.array_equal(_u32(reg.depthImages(subs, p)), _u32(E))
        for k in (1, 4, 8):
            table = torch.zeros((9, 32, 512), dtype=torch.float32, device="cuda") if device else np.zeros((9, 32, 512), F)
            reg.depthImages(subs[:k], p, XYZI32, table)
            reg.depthImages(subs[k:], p, XYZI32, table[k:])
            assert np.array_equal(_u32(table), _u32(E)), (device, k)


def test_map_array_extends_its_image_table_by_the_new_keyframes(reg):
    import torch

    p = _params()
    sc = _scene("six")
    E = _ref("six", p)[0]
    for device in (False, True):
        ma = MapArray()
        tables = []
        for k, s in enumerate(sc["subs"](XYZI32, device)):
            ma.submaps.append(s)
            got = ma.depth_images(reg, p)
            tables.append(ma._di_table)
            assert got.shape[0] == k + 1 and np.array_equal(_u32(got), _u32(E[: k + 1])), (device, k)
        assert len({id(t) for t in tables}) == 4               # capacity 1, 2, 4, 8: the table grew geometrically
        assert ma.depth_images(reg, p) is not None and ma._di_table is tables[-1]
        q = _params(margin=0.1, min_votes=1, keyframe_range=5.0, max_neighbours=2)      # what no image depends on: the table stays
        assert ma.depth_images(reg, q) is not None and ma._di_table is tables[-1]
        small = ma.depth_images(reg, _params(8, 4))           # other images: the table starts again
        assert small.shape == (6, 4, 32) and np.array_equal(_u32(small), _u32(MV.images(sc["pts"], _params(8, 4))))


# ---- votes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "two", "six"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_vote_bits(reg, name, W, H):
    import torch

    sc = _scene(name)
    for kw in (dict(), dict(max_neighbours=1), dict(sensor_origin=(0.4, -0.25, 1.1), margin=0.2)):
        p = _params(W, H, **kw)
        for poses in (False, True):
            E, votes, first_pair = _ref(name, p, poses)
            P = sc["poses"] if poses else None
            if name == "one":
                assert first_pair[-1] == 0 and not votes.any()
            elif name == "six":
                assert first_pair[5] == first_pair[4] and 4 not in visibilityPairs(sc["subs"](), P, p)[1]      # nobody sees the far one
            if not kw and (name, W) in (("two", 128), ("six", 8)):
                assert (votes == 0).sum() > 100 and (votes >= 1).sum() > 100       # the comparison below is not about zeros
            for layout, device, img_dev, out_dev in ((XYZI32, False, False, False), (XYZI20, True, True, True), (XYZI32, True, False, False),
                                                     (XYZI20, False, True, True)):
                subs = sc["subs"](layout, device)
                images = torch.from_numpy(E).cuda() if img_dev else E
                got, first = reg.visibilityVotes(subs, images, p, P, layout, device_out=out_dev)
                assert (got.is_cuda if out_dev else got.dtype == np.int32) and got.shape == votes.shape
                got = got.cpu().numpy() if out_dev else got
                assert np.array_equal(got, votes), (kw, poses, layout, device)
                assert list(first) == [0] + list(np.cumsum([len(c) for c in sc["pts"]]))
            # and with the images the device made itself
            got, _ = reg.visibilityVotes(sc["subs"](), reg.depthImages(sc["subs"](), p), p, P)
            assert np.array_equal(got, votes)


def test_large_images_two_submaps(reg):
    """1024 x 512: 8 MB an image, far beyond what LDS holds — the one launch form serves it."""
    p = _params(1024, 512, min_votes=1)
    sc = _scene("big")
    E, votes, _ = _ref("big", p)
    subs = sc["subs"]()
    got = reg.depthImages(subs, p)
    assert got.shape == (2, 512, 4096) and np.array_equal(_u32(got), _u32(E))
    assert np.array_equal(_u32(reg.depthImages(subs, p, eroded=False)), _u32(MV.images(sc["pts"], p, eroded=False)))
    v, _ = reg.visibilityVotes(sc["subs"](XYZI32, True), got, p)
    assert np.array_equal(v, votes)


def test_host_clouds_cut_across_staging_pieces(reg):
    """Host clouds staged 1 000 records (and 37: not even a workgroup's share) at a time: a submap is cut across pieces, its image
    lowered by several launches, its votes written piece by piece — the bytes of the one-piece call."""
    sc = _scene("six")
    p = _params(min_votes=1)
    E, votes, _ = _ref("six", p)
    D = MV.images(sc["pts"], p, eroded=False)
    raw, _ = reg.assembleMap(sc["subs"]())
    default = reg.visibilityPieceBytes()
    assert default == 1 << 26
    try:
        for layout, records in ((XYZI32, 1000), (XYZI20, 37), (XYZI32, 8)):
            assert reg.visibilityPieceBytes(records * layout[0]) == records * layout[0]
            subs = sc["subs"](layout)
            assert np.array_equal(_u32(reg.depthImages(subs, p, layout, eroded=False)), _u32(D)), records
            assert np.array_equal(_u32(reg.depthImages(subs, p, layout)), _u32(E))
            got, first = reg.visibilityVotes(subs, E, p, None, layout)
            assert np.array_equal(got, votes) and first[-1] == votes.size
            rec, first, removed = reg.assembleMapStatic(subs, E, p, None, layout, XYZI32)
            assert np.array_equal(rec, raw[votes < 1]) and removed == int((votes >= 1).sum())
        for bad in (255, (1 << 30) + 1, 0, -4):
            with pytest.raises(_capi.RegistrationError):
                reg.visibilityPieceBytes(bad)
        assert reg.visibilityPieceBytes() == 8 * 32
    finally:
        reg.visibilityPieceBytes(default)


# ---- the static map --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("two", dict(min_votes=1)), ("six", dict(min_votes=1)), ("two", dict()), ("six", dict(W=8, H=4, max_neighbours=1))])
def test_static_map_is_the_assembled_map_masked_by_the_votes(reg, name, kw):
    import torch

    sc = _scene(name)
    p = _params(**kw)
    for poses in (False, True):
        E, votes, _ = _ref(name, p, poses)
        P = sc["poses"] if poses else None
        keep = votes < p.min_votes
        sizes = [len(c) for c in sc["pts"]]
        bounds = np.concatenate([[0], np.cumsum(sizes)])
        want_first = [int(keep[:b].sum()) for b in bounds]
        if kw == dict(min_votes=1):
            assert 100 < keep.sum() < keep.size - 100
        for in_layout, out_layout, device in ((XYZI32, XYZI32, False), (XYZI32, XYZI32, True), (XYZI20, XYZ12, True), (XYZI20, XYZI32, False),
                                              (XYZI32, XYZI20, True)):
            subs = sc["subs"](in_layout, device)
            raw, raw_first = reg.assembleMap(subs, P, in_layout, out_layout)
            raw = raw.cpu().numpy() if device else raw
            images = torch.from_numpy(E).cuda() if device else E
            got, first, removed = reg.assembleMapStatic(subs, images, p, P, in_layout, out_layout)
            assert (got.is_cuda if device else isinstance(got, np.ndarray)) and got.dtype in (np.uint8, torch.uint8)
            got = got.cpu().numpy() if device else got
            assert np.array_equal(got, raw[keep]), (poses, in_layout, out_layout, device)
            assert list(first) == want_first and removed == int((~keep).sum())
            # count only: the same figures, nothing written
            none, first0, removed0 = reg.assembleMapStatic(subs, images, p, P, in_layout, out_layout, count_only=True)
            assert none is None and list(first0) == want_first and removed0 == removed
        # a host buffer for device clouds, a device buffer for host clouds, and one with exactly the room it needs
        n_keep = int(keep.sum())
        out = np.full((n_keep, 32), 7, np.uint8)
        got, _, _ = reg.assembleMapStatic(sc["subs"](XYZI32, True), E, p, P, out=out)
        raw, _ = reg.assembleMap(sc["subs"](), P)
        assert np.array_equal(got, raw[keep]) and got.shape[0] == n_keep
        out = torch.full((keep.size, 32), 7, dtype=torch.uint8, device="cuda")
        got, _, _ = reg.assembleMapStatic(sc["subs"](), E, p, P, out=out)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), raw[keep]) and bool((out[n_keep:] == 7).all())


def test_static_map_refusals_leave_the_outputs_alone(reg):
    sc = _scene("two")
    p = _params(min_votes=1)
    E, votes, _ = _ref("two", p)
    n_keep = int((votes < 1).sum())
    lib = _capi.load()
    arr, keep, residency, total, _ = reg._submap_table(sc["subs"](), None, 32)
    li = reg._layout(*XYZI32)
    out = np.full((total, 32), 7, np.uint8)
    first = (C.c_size_t * 3)(9, 9, 9)
    n_out, n_removed = C.c_size_t(99), C.c_size_t(99)
    cp = p.struct()

    def call(params=cp, images=E, cap=total, layout=li, n=2, table=arr):
        return lib.lsr_assemble_map_static(reg._h, table, n, C.byref(layout), 0, None, C.c_void_p(images.ctypes.data) if images is not None else None, 0,
                                           C.byref(params) if params is not None else None, C.c_void_p(out.ctypes.data), cap, C.byref(li), 0,
                                           first, C.byref(n_out), C.byref(n_removed))

    assert call(cap=n_keep - 1) == -1                                         # capacity too small
    assert call(params=None) == -1 and call(images=None) == -1 and call(n=0) == -1
    assert call(params=_params(min_votes=0).struct()) == -1 and call(params=_params(9, 32).struct()) == -1
    assert call(layout=reg._layout(10, (0, 4, 8, None))) == -1
    huge = (_capi.SubMap * 2)()
    for i in range(2):
        huge[i].orientation[3] = 1.0
        huge[i].cloud = out.ctypes.data
        huge[i].n_points = 2 ** 30 + 1
    assert call(table=huge) == _capi.ERR_INDEX_OVERFLOW                       # past INT32_MAX records, before anything is read
    votes_out = np.full(8, 7, np.int32)
    n_rec = C.c_size_t(99)
    assert lib.lsr_visibility_votes(reg._h, huge, 2, C.byref(li), 0, None, C.c_void_p(E.ctypes.data), 0, C.byref(cp),
                                    C.c_void_p(votes_out.ctypes.data), 0, None, C.byref(n_rec)) == _capi.ERR_INDEX_OVERFLOW
    img_out = np.full(8, 7.0, F)
    assert lib.lsr_depth_images_build(reg._h, huge, 2, C.byref(li), 0, C.byref(cp), 1, C.c_void_p(img_out.ctypes.data), 0) == _capi.ERR_INDEX_OVERFLOW
    assert lib.lsr_depth_images_build(reg._h, arr, 2, C.byref(li), 0, C.byref(_params(128, 3).struct()), 1, C.c_void_p(img_out.ctypes.data), 0) == -1
    assert (out == 7).all() and list(first) == [9, 9, 9] and n_out.value == 99 and n_removed.value == 99
    assert (votes_out == 7).all() and n_rec.value == 99 and (img_out == 7.0).all()
    assert call(cap=n_keep) == 0 and n_out.value == n_keep and n_removed.value == total - n_keep and first[2] == n_keep


def test_one_submap_or_an_empty_pair_table_gives_the_assembled_bytes(reg):
    p = _params(min_votes=1)
    one = _scene("one")
    raw, _ = reg.assembleMap(one["subs"]())
    got, first, removed = reg.assembleMapStatic(one["subs"](), reg.depthImages(one["subs"](), p), p)
    assert np.array_equal(got, raw) and list(first) == [0, 5000] and removed == 0
    six = _scene("six")
    alone = _params(min_votes=1, keyframe_range=1e-3)                 # nobody within range of anybody
    assert visibilityPairs(six["subs"](), None, alone)[1].size == 0
    raw, raw_first = reg.assembleMap(six["subs"]())
    got, first, removed = reg.assembleMapStatic(six["subs"](), reg.depthImages(six["subs"](), alone), alone)
    assert np.array_equal(got, raw) and np.array_equal(first, raw_first) and removed == 0
    empty = [_sm(np.zeros((0, 8), F)), _sm(np.zeros((0, 8), F), (1.0, 0.0, 0.0))]
    got, first, removed = reg.assembleMapStatic(empty, reg.depthImages(empty, p), p)
    assert got.shape == (0, 32) and list(first) == [0, 0, 0] and removed == 0


# ---- MapArray ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_map_array_publishes_and_saves_the_static_map(reg, tmp_path, device):
    sc = _scene("two")
    p = _params(min_votes=1)
    ma = MapArray()
    ma.submaps = sc["subs"](XYZI32, device)
    raw, _ = reg.assembleMap(sc["subs"]())
    keep = _ref("two", p)[1] < 1
    got, first = ma.publish_map(reg, remove_moving=p)
    got = got.cpu().numpy() if device else got
    assert np.array_equal(got, raw[keep]) and first[-1] == keep.sum() and ma.last_static == (int(keep.sum()), int((~keep).sum()))
    # the optimiser's poses
    raw_p, _ = reg.assembleMap(sc["subs"](), sc["poses"])
    keep_p = _ref("two", p, True)[1] < 1
    got, _ = ma.modified_map(reg, sc["poses"], remove_moving=p)
    assert np.array_equal(got.cpu().numpy() if device else got, raw_p[keep_p])
    # through the existing leaf filter: the filter's records of the static map
    thin, none = ma.publish_map(reg, leaf=0.5, remove_moving=p)
    assert none is None and thin.is_cuda                       # the static map stays on the device
    assert np.array_equal(thin.cpu().numpy(), reg.voxelGridFilterMap(raw[keep], 0.5))
    # map.pcd: the static assembly and the save-from-device-buffer entry
    for data in ("binary", "ascii", "binary_compressed"):
        path = str(tmp_path / f"map_{data}.pcd")
        size = ma.save_map(reg, path, data=data, remove_moving=p)
        assert size == os.path.getsize(path)
        if data == "ascii":     # text does not carry a float's bits: the file is the text of exactly those records
            assert open(path, "rb").read() == reg.formatPCDASCII(raw[keep]).tobytes()
            assert reg.loadPCDFile(path).shape[0] == int(keep.sum())
            continue
        if data == "binary_compressed":
            reg.pcdReadCompressed(True)
        back = reg.loadPCDFile(path)
        assert np.array_equal(_u32(back.view(F)[:, [0, 1, 2, 4]]), _u32(raw[keep].view(F)[:, [0, 1, 2, 4]])), data
    path = str(tmp_path / "thin.pcd")
    ma.save_map(reg, path, sc["poses"], "binary", leaf=0.5, remove_moving=p)
    assert np.array_equal(reg.loadPCDFile(path), reg.voxelGridFilterMap(raw_p[keep_p], 0.5))
    # without remove_moving every call is what it was
    assert np.array_equal(_u32(ma.publish_map(reg)[0]), _u32(raw))
    ma.save_map(reg, str(tmp_path / "raw.pcd"), data="binary")
    assert np.array_equal(reg.loadPCDFile(str(tmp_path / "raw.pcd")), raw)


# ---- behaviour and timing ------------------------------------------------------------------------------------------------------------------
def test_the_car_goes_and_the_world_stays_on_the_device(reg):
    """The CPU behaviour test's assertions on the device's votes, which are the restatement's: 0 of 208 671 static records and 352 of
    488 car records removed, 0 of 209 505 without the car."""
    import torch

    p = VisibilityParams()
    votes = []
    for with_car in (True, False):
        scene = MV.car_scene(with_car)
        ma = MapArray()
        for s in scene["ma"].submaps:
            ma.submaps.append(SubMap(torch.from_numpy(s.cloud).cuda(), s.position, s.orientation, s.distance))
        v, _ = reg.visibilityVotes(ma.submaps, ma.depth_images(reg, p), p, device_out=True)
        ref, _ = MV.static_votes(scene["clouds"], scene["ma"].submaps, p)
        assert np.array_equal(v.cpu().numpy(), ref)
        votes.append(v.cpu().numpy())
        if with_car:
            records, first = ma.publish_map(reg, remove_moving=p)
            car = scene["is_car"]
            assert records.shape[0] == int((ref < 2).sum()) and ma.last_static[1] == int((ref >= 2).sum()) >= 0.6 * car.sum()
    MV.assert_behaviour(MV.behaviour(votes[0], votes[1], p.min_votes))


def test_timing_keys_report_the_launches(reg):
    p = _params()
    sc = _scene("two")
    subs = sc["subs"]()
    assert reg.visibilityMs() is not None
    reg.setProfiling(True)
    try:
        E = reg.depthImages(subs, p)
        images_ms, _ = reg.visibilityMs()
        reg.visibilityVotes(subs, E, p)
        _, votes_ms = reg.visibilityMs()
        reg.assembleMapStatic(subs, E, p)
        _, static_ms = reg.visibilityMs()
    finally:
        reg.setProfiling(False)
    assert 0.0 < images_ms < 1000.0 and 0.0 < votes_ms < 1000.0 and 0.0 < static_ms < 1000.0
    reg.depthImages(subs, p)
    reg.visibilityVotes(subs, E, p)
    assert reg.visibilityMs() == (0.0, 0.0)
