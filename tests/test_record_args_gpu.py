"""The malformed-argument table of tests/record_args_cases.py through the C ABI, against every entry that takes a buffer of records.
A refused call must give the status the table states (read off the per-entry checks as they stood before they were merged), must come
before any copy — the over-limit counts are passed with a 300-record HOST buffer, a copy of 2^30 records from it could not succeed —
and must leave the object working: after EACH refusal one good call at n = 300 gives the bytes it gave before the refusals.
The differences between the entries are part of the table: an empty cloud is fine for the ingest and the transform, still reports for
the de-skew and is refused by the PCD writer; the ingest entries stop at INT32_MAX / 2 records with INVALID_ARGUMENT, the map and PCD
entries at INT32_MAX with INDEX_OVERFLOW; the de-skew does not look at the intensity offset; only the records -> records and the map /
PCD entries demand 4-byte aligned pointers."""
import ctypes as C

import numpy as np
import pytest

import deskew_cases as DC
import record_args_cases as RC
from record_args_cases import FULL, HALF, INVALID, OK, OVERFLOW

pytestmark = pytest.mark.gpu
F = np.float32
N, STEP = 300, 32
GOOD = (32, 0, 4, 8, 16)


@pytest.fixture(scope="module")
def entries():
    from lidarslam_ros2_amd import DIRECT7, NormalDistributionsTransform, _capi
    from lidarslam_ros2_amd.registration import _sensor_transform

    reg = NormalDistributionsTransform(device=0)
    reg.setResolution(20.0); reg.setTransformationEpsilon(0.01); reg.setMaximumIterations(5); reg.setNeighborhoodSearchMethod(DIRECT7)
    lib, h = reg._lib, reg._h
    rng = np.random.default_rng(5)
    samples = DC.imu_samples(DC.stamps_200hz(DC.T0 - 0.05, DC.T0 + 0.15), rng)
    xyz = DC.make_scan(N, rng, [s[3] for s in samples])
    raw = np.zeros((N, STEP), np.uint8)
    raw.view(F)[:, :3] = xyz
    raw.view(F)[:, 4] = rng.uniform(0, 255, N).astype(F)
    shifted = np.zeros(N * STEP + 16, np.uint8)             # the same records one byte off a 4-byte boundary: "pointer + 1"
    shifted[1:1 + N * STEP] = raw.reshape(-1)
    two = np.zeros(64, np.uint8)                            # room for 2 records of 16 bytes read and 2 written: the range cases
    out = np.zeros((N + 1) * 64, np.uint8)                  # results: records of up to 48 bytes, or the PCD text (<= 64 bytes a line)
    p, po, p1, p2 = raw.ctypes.data, out.ctypes.data, shifted.ctypes.data + 1, two.ctypes.data
    assert p % 16 == 0 and po % 16 == 0 and p1 % 4 == 1 and p2 % 4 == 0
    tf = _sensor_transform((0.6, -0.3, 1.1), (0.02, -0.04, 0.15, 0.98))
    n_out = C.c_size_t()
    ident = np.eye(4, dtype=F).reshape(16)
    fp = C.POINTER(C.c_float)

    def lay(t):
        return C.byref(_capi.Pc2Layout(*t))

    def source_bytes():
        reg._n_source = N
        return reg.getInputSourcePointCloud2().tobytes()

    def out_bytes(n_bytes):
        return out[:n_bytes].tobytes()

    def pc2(data=p, n=N, layout=GOOD):
        return lib.lsr_set_input_source_pc2(h, data, n, lay(layout), 0.5, 90.0, C.c_float(1.0), 0, C.byref(n_out))

    def pc2_tf(data=p, n=N, layout=GOOD):
        return lib.lsr_set_input_source_pc2_tf(h, data, n, lay(layout), C.byref(tf), 0.5, 90.0, C.c_float(1.0), 0, C.byref(n_out))

    def frontend(data=p, n=N, stride=STEP):
        return lib.lsr_set_input_source_frontend(h, data, stride, n, 0.5, 90.0, C.c_float(1.0), 0, C.byref(n_out))

    def filtered(data=p, n=N, stride=STEP):
        return lib.lsr_set_input_source_filtered(h, data, stride, n, C.c_float(1.0), 0, C.byref(n_out))

    def vgf_pc2(data=p, n=N, layout=GOOD, out_layout=GOOD, dst=po, cap=N):
        out[:] = 0
        return lib.lsr_voxel_grid_filter_pc2(h, data, n, lay(layout), C.c_float(1.0), dst, cap, lay(out_layout), C.byref(n_out))

    def transform(data=p, n=N, layout=GOOD, dst=po):
        out[:] = 0
        return lib.lsr_transform_pc2(h, data, n, lay(layout), C.byref(tf), 0, dst)

    def deskew(data=p, n=N, layout=GOOD, dst=po, ring=True):
        out[:] = 0
        reg.imuReset(0.1)                                   # the same ring for every call: a de-skew moves its cursor
        for ang, acc, quat, stamp in samples if ring else ():
            a, b, c = (np.ascontiguousarray(v, F) for v in (ang, acc, quat))
            assert lib.lsr_imu_push(h, a.ctypes.data_as(fp), b.ctypes.data_as(fp), c.ctypes.data_as(fp), float(stamp)) == 0
        return lib.lsr_deskew_pc2(h, data, n, lay(layout), DC.T0, 0, dst, None)

    def pcd(data=p, n=N, layout=GOOD):
        out[:] = 0
        return lib.lsr_format_pcd_ascii(h, data, n, lay(layout), 0, po, out.nbytes, 0, C.byref(n_out))

    def submaps(clouds):
        arr = (_capi.SubMap * max(len(clouds), 1))()
        for i, (ptr, cnt) in enumerate(clouds):
            arr[i].position[:] = [1.0 + i, -2.0, 0.5]
            arr[i].orientation[:] = [0.0, 0.0, 0.1, 0.995]
            arr[i].cloud, arr[i].n_points = ptr, cnt
        return arr

    def amap(clouds=((p, 100), (p + 100 * STEP, 200)), num=None, layout=GOOD, out_layout=GOOD, dst=po, cap=N):
        out[:] = 0
        return lib.lsr_assemble_map(h, submaps(clouds), len(clouds) if num is None else num, lay(layout), 0, None, dst, cap, lay(out_layout),
                                    0, None, C.byref(n_out))

    def frame_lists(frames):
        nf = max(len(frames), 1)
        ptrs, counts = (C.c_void_p * nf)(*[f[0] for f in frames]), (C.c_size_t * nf)(*[f[1] for f in frames])
        return ptrs, counts, np.tile(ident, nf).ctypes.data_as(fp)

    def frames(fr=((p, 100), (p + 100 * STEP, 200)), nf=None, stride=STEP, lists=True):
        ptrs, counts, poses = frame_lists(fr)
        nf = len(fr) if nf is None else nf
        return lib.lsr_set_input_target_frames(h, nf, ptrs if lists else None, counts if lists else None, stride, poses if lists else None, 0)

    def frames_filtered(fr=((p, 100), (p + 100 * STEP, 200)), nf=None, stride=STEP, lists=True):
        ptrs, counts, poses = frame_lists(fr)
        nf = len(fr) if nf is None else nf
        return lib.lsr_set_input_target_frames_filtered(h, nf, ptrs if lists else None, counts if lists else None, stride,
                                                        poses if lists else None, 0, C.c_float(0.5), C.byref(n_out))

    def aligned_pose():     # what a target is good for: a registration of the same scan against it
        assert filtered() == OK
        reg.align(np.eye(4, dtype=F))
        return np.asarray(reg.getFinalTransformation(), F).tobytes() + bytes([reg.getFinalNumIteration()])

    null2 = dict(data=None, n=2)
    bad_layouts = [dict(layout=t) for t in RC.BAD_LAYOUTS]
    bad_strides = [dict(stride=s) for s, st in RC.STRIDES if st != OK]
    in_out = [(dict(n=2, layout=(16, 0, 4, 8, -1), data=a - RC.P + p2, dst=b - RC.P + p2), st) for (a, b, n, _), st in RC.IN_OUT
              if n == 2 and a >= RC.P and b >= RC.P]
    assert len(in_out) == 6 and sorted(st for _, st in in_out) == [INVALID] * 3 + [OK] * 3
    bad_frames = [(dict(nf=0), INVALID), (dict(lists=False), INVALID), (dict(fr=((p, 5), (None, 3))), INVALID), (dict(stride=10), INVALID),
                  (dict(stride=30), INVALID), (dict(fr=((p, HALF + 1),)), INVALID), (dict(fr=((p, HALF), (p, 1))), INVALID)]
    # name -> (call, the bytes a good call leaves behind, [(arguments, status) ...]); yielded: the calls hold addresses, not the arrays,
    # and the arrays live in this frame until the module's tests are done
    yield {
        "lsr_set_input_source_pc2": (pc2, source_bytes, [(a, INVALID) for a in bad_layouts + [null2, dict(n=HALF + 1), dict(n=FULL + 1)]]
                                     + [(dict(data=None, n=0), OK), (dict(data=p1), OK)]),
        "lsr_set_input_source_pc2_tf": (pc2_tf, source_bytes, [(a, INVALID) for a in bad_layouts + [null2, dict(n=HALF + 1)]]
                                        + [(dict(data=p1), OK)]),
        "lsr_set_input_source_frontend": (frontend, source_bytes, [(a, INVALID) for a in bad_strides + [null2, dict(n=HALF + 1)]]
                                          + [(dict(data=p1), OK)]),
        "lsr_set_input_source_filtered": (filtered, source_bytes, [(a, INVALID) for a in bad_strides + [null2, dict(n=HALF + 1)]]
                                          + [(dict(data=p1), OK)]),
        "lsr_voxel_grid_filter_pc2": (vgf_pc2, lambda: out_bytes(n_out.value * STEP),
                                      [(a, INVALID) for a in bad_layouts + [dict(out_layout=t) for t in RC.BAD_LAYOUTS]
                                       + [null2, dict(n=HALF + 1), dict(cap=0)]] + [(dict(data=p1), OK)]),
        "lsr_transform_pc2": (transform, lambda: out_bytes(N * STEP),
                              [(a, INVALID) for a in bad_layouts + [null2, dict(dst=None, n=2), dict(data=p1), dict(dst=po + 1), dict(n=HALF + 1)]]
                              + in_out + [(dict(data=None, dst=None, n=0), OK)]),
        "lsr_deskew_pc2": (deskew, lambda: out_bytes(N * STEP),
                           [(dict(layout=t), INVALID) for t in RC.BAD_XYZ_LAYOUTS]
                           + [(a, INVALID) for a in [null2, dict(dst=None, n=2), dict(data=p1), dict(dst=po + 1), dict(data=p1, n=0), dict(n=HALF + 1)]]
                           + in_out + [(dict(ring=False, **a), st) for a, st in in_out]
                           + [(dict(layout=(32, 0, 4, 8, 30)), OK), (dict(data=None, dst=None, n=0), OK)]),
        "lsr_format_pcd_ascii": (pcd, lambda: out_bytes(n_out.value),
                                 [(a, INVALID) for a in bad_layouts + [null2, dict(n=0), dict(data=None, n=0), dict(data=p1)]]
                                 + [(dict(n=FULL + 1), OVERFLOW), (dict(data=p1, n=FULL + 1), INVALID)]),
        "lsr_assemble_map": (amap, lambda: out_bytes(n_out.value * STEP),
                             [(a, INVALID) for a in bad_layouts + [dict(out_layout=t) for t in RC.BAD_OUT_LAYOUTS]
                              + [dict(clouds=((p, 100), (None, 2))), dict(clouds=((p1, 100),)), dict(dst=None), dict(dst=po + 1), dict(num=0),
                                 dict(cap=N - 1), dict(clouds=((p1, FULL + 1),))]]
                             + [(dict(clouds=((p, FULL + 1),)), OVERFLOW), (dict(clouds=((p, FULL // 2 + 1), (p, FULL // 2 + 1))), OVERFLOW),
                                (dict(clouds=((p, 100), (None, 0), (p + 100 * STEP, 200))), OK)]),
        "lsr_set_input_target_frames": (frames, aligned_pose, bad_frames),
        "lsr_set_input_target_frames_filtered": (frames_filtered, aligned_pose, bad_frames),
    }


ENTRIES = ["lsr_set_input_source_pc2", "lsr_set_input_source_pc2_tf", "lsr_set_input_source_frontend", "lsr_set_input_source_filtered",
           "lsr_voxel_grid_filter_pc2", "lsr_transform_pc2", "lsr_deskew_pc2", "lsr_format_pcd_ascii", "lsr_assemble_map",
           "lsr_set_input_target_frames", "lsr_set_input_target_frames_filtered"]


@pytest.mark.parametrize("name", ENTRIES)
def test_malformed_record_arguments(entries, name):
    assert sorted(entries) == sorted(ENTRIES)
    call, result, table = entries[name]
    assert call() == OK
    before = result()
    assert len(before) > 16 and any(before)
    refused = 0
    for args, status in table:
        assert call(**args) == status, (name, args)
        if status == OK:
            continue
        refused += 1
        assert call() == OK, (name, args)
        assert result() == before, (name, args)          # the object still works, and gives the same bytes
    assert refused >= 5
