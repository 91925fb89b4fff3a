"""CPU tests of the host side: the C-ABI library loads and exports every symbol include/lidarslam_reg.h
declares (no compute without a GPU), workload generator, pose maths, and the multi-process sharding
path (gloo, world_size 2)."""
import ctypes as C
import os
import re
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_exports_every_declared_symbol():
    from lidarslam_ros2_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    declared = sorted(set(re.findall(r"\b(lsr_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 25
    lib = _capi.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/lidarslam_reg.h but not exported"
    assert set(_capi.EXPORTED_SYMBOLS) == set(declared)
    assert b"gfx950" in lib.lsr_version()
    assert lib.lsr_status_string(0) == b"ok"
    assert lib.lsr_status_string(-2) == b"no usable gfx950 device"


def test_table_driven_angle_coefficients_equal_the_scalar_formulas():
    """The device builds j_ang / h_ang (NDT eq. 6.19 / 6.21) one table entry per lane; the host-side self check evaluates
    the same 72 entries next to the scalar formulas — including the 1e-4 small-angle snap and both
    settings of the h_ang d1 sign quirk.  No device needed."""
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    rng = np.random.default_rng(5)
    for t in range(600):
        ang = rng.uniform(-3.2, 3.2, 3) if t % 3 else rng.uniform(-2e-4, 2e-4, 3)
        p = np.concatenate([rng.normal(size=3), ang])
        for sign in (1, -1):
            jr, hr, jt, ht = (np.zeros(24, np.float32), np.zeros(48, np.float32), np.zeros(24, np.float32), np.zeros(48, np.float32))
            assert lib.lsr_debug_angle_tables(p.ctypes.data_as(dp), sign, jr.ctypes.data_as(fp), hr.ctypes.data_as(fp),
                                              jt.ctypes.data_as(fp), ht.ctypes.data_as(fp)) == 0
            assert np.array_equal(jr, jt), (t, sign)
            assert np.array_equal(hr, ht), (t, sign)
    # cross-check one entry against the closed form: j_ang row c = (-sy cz, sy sz, cy)
    p = np.array([0, 0, 0, 0.3, -0.4, 0.5])
    jr, hr, jt, ht = (np.zeros(24, np.float32), np.zeros(48, np.float32), np.zeros(24, np.float32), np.zeros(48, np.float32))
    lib.lsr_debug_angle_tables(p.ctypes.data_as(dp), 1, jr.ctypes.data_as(fp), hr.ctypes.data_as(fp), jt.ctypes.data_as(fp),
                               ht.ctypes.data_as(fp))
    sy, cy, sz, cz = np.sin(-0.4), np.cos(-0.4), np.sin(0.5), np.cos(0.5)
    assert np.allclose(jt[6:9], [-sy * cz, sy * sz, cy], atol=1e-7)
    assert ht[20] == np.float32(sy)


def test_c_shard_range_is_the_python_partition():
    """lsr_shard_range (C ABI, device-free) and sharding.shard_range (torch.distributed path) must cut a batch the same way:
    contiguous shares in rank order, sizes differing by at most one, nothing lost."""
    from lidarslam_ros2_amd.sharding import c_shard_range, shard_range

    for n in (0, 1, 7, 8, 63, 64, 65):
        for world in (1, 2, 3, 8):
            cover = []
            for r in range(world):
                a, b = c_shard_range(n, world, r), shard_range(n, world, r)
                assert (a.start, a.stop) == (b.start, b.stop), (n, world, r)
                cover += list(a)
            assert cover == list(range(n))


def test_comm_entry_points_fail_cleanly_without_a_device():
    import torch

    from lidarslam_ros2_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.lsr_comm_create(None, 0, 1, 0, C.byref(h)) == -2          # LSR_ERR_NO_DEVICE
    assert lib.lsr_comm_create(None, 1, 1, 0, C.byref(h)) == -1          # rank out of range
    assert lib.lsr_comm_create(None, 0, 2, 0, C.byref(h)) == -1          # world 2 needs a unique id
    assert lib.lsr_comm_destroy(None) == 0
    recs = (_capi.ShardRecord * 1)()
    assert lib.lsr_align_batch_sharded(None, None, 0, 1, None, 0, recs) == -1


def test_no_cpu_fallback_without_a_device():
    """Without a GPU lsr_create must fail loudly (LSR_ERR_NO_DEVICE) — there is no CPU path."""
    import torch

    from lidarslam_ros2_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    from lidarslam_ros2_amd import NormalDistributionsTransform

    with pytest.raises(_capi.RegistrationError) as ei:
        NormalDistributionsTransform(device=0)
    assert ei.value.status == -2


def test_product_package_never_imports_the_oracle():
    """The product path may not import, link, dlopen or include anything under oracle/."""
    pkg = os.path.join(ROOT, "lidarslam_ros2_amd")
    bad = re.compile(r"(import\s+oracle|from\s+oracle|liboracle|#include\s+[\"<][^\">]*oracle|oracle\.py|orc_[a-z_]+\s*\()")
    for base in (pkg, os.path.join(ROOT, "include")):
        for dirpath, _, files in os.walk(base):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".h", "Makefile")):
                    txt = open(os.path.join(dirpath, f)).read()
                    assert not bad.search(txt), (dirpath, f, bad.search(txt).group(0))


def test_synth_is_deterministic_and_exact():
    from lidarslam_ros2_amd import synth

    a, b = synth.small_case(n_source=1500, n_keyframes=2), synth.small_case(n_source=1500, n_keyframes=2)
    assert np.array_equal(a.source, b.source) and np.array_equal(a.target, b.target) and np.array_equal(a.guess, b.guess)
    assert a.source.shape == (1500, 3) and a.source.dtype == np.float32
    xyzi = synth.as_pointxyzi(a.source)
    assert xyzi.shape == (1500, 8) and xyzi.strides[0] == 32 and np.all(xyzi[:, 3] == 1.0)
    # VoxelGrid stand-in: one centroid per occupied leaf, inside its leaf
    pts = a.target[:5000]
    d = synth.voxel_downsample(pts, 0.5)
    assert len(np.unique(np.floor(d / np.float32(0.5)).astype(np.int64), axis=0)) == d.shape[0]
    assert d.shape[0] == len(np.unique(np.floor(pts * (np.float32(1) / np.float32(0.5))).astype(np.int64), axis=0))


def test_cfg2_workload_has_exact_point_counts():
    from lidarslam_ros2_amd import synth

    c = synth.cfg_ndt_30k()
    assert c.source.shape == (30000, 3)
    assert c.target.shape[0] > 300000
    from lidarslam_ros2_amd.posemath import pose_delta

    dt, ang = pose_delta(c.guess, c.truth)   # guess = previous scan pose: 0.5 m behind
    assert 0.45 < dt < 0.55 and ang < 2e-3


def test_pose_delta_is_accurate_for_tiny_rotations():
    from lidarslam_ros2_amd import synth
    from lidarslam_ros2_amd.posemath import pose_delta

    A = synth.pose_matrix(1, 2, 3, 0.1).astype(np.float32)
    B = synth.pose_matrix(1, 2, 3.001, 0.10002).astype(np.float32)
    dt, ang = pose_delta(A, B)
    assert dt == pytest.approx(1e-3, rel=1e-3) and ang == pytest.approx(2e-5, abs=2e-7)


def test_shard_range_partitions_every_batch():
    from lidarslam_ros2_amd.sharding import pack_record, shard_range, unpack_record

    for n in (0, 1, 7, 64, 65):
        for world in (1, 2, 3, 8):
            got = [i for r in range(world) for i in shard_range(n, world, r)]
            assert got == list(range(n))
            sizes = [len(shard_range(n, world, r)) for r in range(world)]
            assert max(sizes) - min(sizes) <= 1
    assert [len(shard_range(64, 8, r)) for r in range(8)] == [8] * 8   # cfg 4: 64 candidates over 8 GPUs
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (1, 2, 3)
    r = unpack_record(pack_record(T, 13.5, 7, True, 0.25))
    assert np.array_equal(r["T"], T) and r["iterations"] == 7 and r["converged"] and r["score"] == 13.5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ring_gate_costs(n_items):
    """Sizes as the ring gate produces them: a few full submaps, many small ones (cost in point visits)."""
    from lidarslam_ros2_amd.sharding import registration_cost

    rng = np.random.default_rng(77)
    n_target = np.where(rng.random(n_items) < 0.25, 661_000, rng.integers(4_000, 120_000, n_items))
    return np.array([registration_cost(int(t), 33_000) for t in n_target])


def _gloo_worker(rank, world, port, n_items, out_dir, planned=False):
    import torch.distributed as dist

    sys.path.insert(0, ROOT)
    from lidarslam_ros2_amd.sharding import pack_record, register_sharded

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def register_local(indices):   # stands in for the per-GPU registrations: result encodes (item, rank)
        recs = []
        for i in indices:
            T = np.eye(4, dtype=np.float32)
            T[:3, 3] = (i, 10 * i, rank)
            recs.append(pack_record(T, score=float(i) / 2, iterations=i % 5, converged=(i % 2 == 0), fitness=0.1 * i))
        return recs

    seen = []

    def register_seen(indices):
        seen.extend(indices)
        return register_local(indices)

    res = register_sharded(n_items, register_seen, costs=_ring_gate_costs(n_items) if planned else None)
    np.save(os.path.join(out_dir, f"rank{rank}.npy"), np.array([[r["T"][0, 3], r["T"][1, 3], r["T"][2, 3], r["score"],
                                                                   r["iterations"], r["converged"]] for r in res]))
    np.save(os.path.join(out_dir, f"seen{rank}.npy"), np.array(seen, np.int64))
    dist.destroy_process_group()


def _gloo_bcast_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    from lidarslam_ros2_amd.sharding import broadcast_target

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    class Rec:   # stands in for a registration object: records what setInputTarget was given
        def setInputTarget(self, cloud):
            self.cloud = np.asarray(cloud).copy()

    r = Rec()
    cloud = None
    if rank == 1:   # the submap lives on rank 1
        cloud = np.random.default_rng(7).normal(size=(1234, 4)).astype(np.float32)
    got = broadcast_target(r, cloud, src=1)
    np.save(os.path.join(out_dir, f"tgt{rank}.npy"), r.cloud)
    assert np.array_equal(np.asarray(got), r.cloud)
    dist.destroy_process_group()


def test_target_broadcast_gloo_world2(tmp_path):
    """SURVEY.md 8e "N keyframes vs. one submap" across ranks: the rank that holds the submap broadcasts it (shape, then the records)
    and every rank sets the same bytes as its input target (sharding.broadcast_target; the C ABI's lsr_set_input_target_bcast does the
    same with ncclBroadcast — exercised on hardware by tests/test_multigpu_gpu.py)."""
    import torch.multiprocessing as mp

    world, port = 2, _free_port()
    mp.spawn(_gloo_bcast_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    a, b = np.load(tmp_path / "tgt0.npy"), np.load(tmp_path / "tgt1.npy")
    assert a.shape == (1234, 4) and np.array_equal(a, b)
    assert np.array_equal(b, np.random.default_rng(7).normal(size=(1234, 4)).astype(np.float32))


@pytest.mark.parametrize("n_items", [7, 64])
def test_sharded_batch_all_gather_gloo_world2(tmp_path, n_items):
    """N>1 path on CPU: two processes, static partition, one all-gather of 64-byte records."""
    import torch.multiprocessing as mp

    from lidarslam_ros2_amd.sharding import shard_range

    world, port = 2, _free_port()
    mp.spawn(_gloo_worker, args=(world, port, n_items, str(tmp_path)), nprocs=world, join=True)
    a, b = np.load(tmp_path / "rank0.npy"), np.load(tmp_path / "rank1.npy")
    assert np.array_equal(a, b)                       # every rank ends with the full, identical table
    assert np.array_equal(a[:, 0], np.arange(n_items)) and np.array_equal(a[:, 1], 10 * np.arange(n_items))
    owner = np.zeros(n_items)
    owner[list(shard_range(n_items, world, 1))] = 1
    assert np.array_equal(a[:, 2], owner)             # each item was registered by the rank that owns it
    assert np.array_equal(a[:, 4], np.arange(n_items) % 5)


def test_shard_plan_is_longest_first_and_the_c_plan_is_the_python_plan():
    """lsr_shard_plan (C ABI, device-free) == sharding.shard_plan; every rank's list is longest first; the plan's makespan is
    never worse than the block partition's and within the LPT bound of the trivial lower bounds."""
    from lidarslam_ros2_amd.sharding import block_plan, c_shard_plan, shard_plan

    rng = np.random.default_rng(5)
    for n in (0, 1, 7, 64, 65):
        for world in (1, 2, 3, 8):
            for costs in (_ring_gate_costs(n), np.ones(n), rng.integers(1, 4, n).astype(np.float64)):
                P, Q = shard_plan(costs, world), c_shard_plan(costs, world)
                assert np.array_equal(P.owner, Q.owner) and np.array_equal(P.order, Q.order) and np.array_equal(P.rank_first, Q.rank_first)
                assert sorted(P.order.tolist()) == list(range(n))
                for r in range(world):
                    it = P.items(r)
                    assert all(P.owner[i] == r for i in it)
                    assert all(costs[a] >= costs[b] for a, b in zip(it, it[1:]))
                if n:
                    span, lower = P.loads(costs).max(), max(costs.sum() / world, costs.max())
                    assert span <= block_plan(n, world).loads(costs).max() + 1e-9
                    assert span <= (4.0 / 3.0 - 1.0 / (3.0 * world)) * lower + costs.max() * (world > 1) + 1e-9
    P = shard_plan(np.ones(64), 8)                       # costs the model cannot tell apart: the block partition, 8 each (cfg 4 over 8 GPUs)
    assert [len(P.items(r)) for r in range(8)] == [8] * 8 and P.items(1)[:3] == [8, 9, 10]
    near = 661000.0 + 300.0 * np.sin(np.arange(64.0))    # ... and so are costs within 2 % of each other (cfg 4's own candidates)
    Pn, Qn = shard_plan(near, 8), c_shard_plan(near, 8)
    assert Pn.items(3) == list(range(24, 32)) and np.array_equal(Pn.order, Qn.order) and np.array_equal(Pn.rank_first, Qn.rank_first)
    assert np.array_equal(c_shard_plan(64, 8).order, np.arange(64))   # no costs at all: the same
    costs = _ring_gate_costs(64)                         # the case it is for: block partition vs plan on ring-gate sizes
    assert shard_plan(costs, 8).loads(costs).max() < 0.8 * block_plan(64, 8).loads(costs).max()
    with pytest.raises(ValueError):
        shard_plan([1.0, float("nan")], 2)
    from lidarslam_ros2_amd import _capi
    with pytest.raises(_capi.RegistrationError):
        c_shard_plan(np.array([1.0, -2.0]), 2)


@pytest.mark.parametrize("n_items", [7, 64])
def test_planned_batch_all_gather_gloo_world2(tmp_path, n_items):
    """N>1 path on CPU with the cost-aware plan: each rank registers plan.items(rank) longest first, the table comes back in
    batch order on both ranks."""
    import torch.multiprocessing as mp

    from lidarslam_ros2_amd.sharding import shard_plan

    world, port = 2, _free_port()
    mp.spawn(_gloo_worker, args=(world, port, n_items, str(tmp_path), True), nprocs=world, join=True)
    a, b = np.load(tmp_path / "rank0.npy"), np.load(tmp_path / "rank1.npy")
    assert np.array_equal(a, b)
    assert np.array_equal(a[:, 0], np.arange(n_items)) and np.array_equal(a[:, 1], 10 * np.arange(n_items))
    plan = shard_plan(_ring_gate_costs(n_items), world)
    assert np.array_equal(a[:, 2], plan.owner)
    for r in range(world):
        assert np.load(tmp_path / f"seen{r}.npy").tolist() == plan.items(r)


def _build_adapter(tmp_path):
    import subprocess

    exe = str(tmp_path / "adapter_smoke")
    libdir = os.path.join(ROOT, "lidarslam_ros2_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "adapter_smoke.cpp"), "-o", exe, "-L" + libdir,
                           "-llidarslam_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_adapter_compiles_against_the_c_abi(tmp_path):
    """include/lidarslam_reg/registration.hpp (the pcl::Registration-shaped adapter) compiles with plain
    g++ against the C ABI; on a CPU-only host construction fails loudly instead of falling back."""
    import subprocess

    import torch

    exe = _build_adapter(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    if torch.cuda.is_available():
        assert out.startswith("OK converged=1"), out
    else:
        assert out.startswith("NO_DEVICE"), out


@pytest.mark.gpu
def test_cpp_adapter_runs_the_frontend_call_sequence(tmp_path):
    import subprocess

    exe = _build_adapter(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    assert out.startswith("OK converged=1"), out
    assert "OUTPUT fields_ok=1" in out, out      # align(output): xyz transformed, intensity etc. kept (PCL semantics)
    assert "BATCH ok=1" in out, out               # candidate set through setInputTargets / alignBatch / getFitnessScores
    assert "LOOP st=0 n=1 from=0 to=3 accepted=1" in out, out


def _build_binding(tmp_path):
    import subprocess

    exe = str(tmp_path / "binding_smoke")
    libdir = os.path.join(ROOT, "lidarslam_ros2_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp", "mock"),
                           os.path.join(ROOT, "tests", "cpp", "binding_smoke.cpp"), "-o", exe, "-L" + libdir,
                           "-llidarslam_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pcl_binding_compiles_and_fails_loudly_without_a_device(tmp_path):
    """include/lidarslam_reg/gfx950_registration.hpp against the PCL stand-in whose align() keeps pcl::Registration's
    initCompute() contract; without a device the program reports it (no CPU path)."""
    import subprocess

    import torch

    out = subprocess.run([_build_binding(tmp_path)], capture_output=True, text=True, timeout=120).stdout
    assert out.startswith("NO_TARGET" if torch.cuda.is_available() else "NO_DEVICE"), out


@pytest.mark.gpu
def test_pcl_binding_never_builds_a_host_kdtree_over_the_target(tmp_path):
    """pcl::Registration::align() -> initCompute() rebuilds a FLANN kd-tree over target_ after every
    setInputTarget (scanmatcher_component.cpp:307,353) — the binding opts out with setSearchMethodTarget(tree,
    force_no_recompute = true).  Three frontend cycles through the base-class pointer: converged, zero kd-tree builds;
    align() before setInputTarget() is refused by initCompute() the PCL way."""
    import subprocess

    out = subprocess.run([_build_binding(tmp_path)], capture_output=True, text=True, timeout=120).stdout
    assert "NO_TARGET converged=0" in out, out
    assert "OK converged=1" in out, out
    assert "KDTREE builds=0 points_indexed=0" in out, out


@pytest.mark.gpu
def test_pcl_binding_answers_getFitnessScore_left_on_the_base_pointer(tmp_path):
    """VERDICT r04 #7 / ADVICE r04 (medium): pcl::Registration::getFitnessScore is NOT virtual.  The reference's own call sites
    (graph_based_slam_component.cpp:231, scanmatcher_component.cpp:376) go through the base pointer; with force_no_recompute the
    base class's tree_ never sees a cloud, so a call site a maintainer forgot to edit would search an empty FLANN index.  The
    binding installs Gfx950FitnessTree as tree_: PCL's own loop (the stand-in's getFitnessScore mirrors registration.hpp: transform
    input_, one nearestKSearch per point) is answered from ONE device search.  Asserted: the base-pointer score equals the derived
    call's, twice in a row and again after a new align; no search ever reached an un-indexed kd-tree; a search that is not that
    walk is refused with 0 neighbours and distance FLT_MAX (a fitness built from it cannot pass a loop gate)."""
    import re
    import subprocess

    run = subprocess.run([_build_binding(tmp_path)], capture_output=True, text=True, timeout=120)
    out = run.stdout
    m = re.search(r"BASE_FITNESS base=(\S+) again=(\S+) derived=(\S+) unindexed_searches=(\d+)", out)
    assert m, out
    base, again, derived, unindexed = float(m.group(1)), float(m.group(2)), float(m.group(3)), int(m.group(4))
    assert unindexed == 0, out
    assert derived > 0 and abs(base - derived) <= 1e-6 * derived and abs(again - derived) <= 1e-6 * derived, out
    m2 = re.search(r"BASE_FITNESS_AFTER_ALIGN base=(\S+) derived=(\S+)", out)
    assert m2, out
    b2, d2 = float(m2.group(1)), float(m2.group(2))
    assert d2 > 0 and abs(b2 - d2) <= 1e-6 * d2, out
    assert "FOREIGN_SEARCH found=0 d2_is_max=1" in out, out
    assert "called through pcl::Registration*" in run.stderr and "not getFitnessScore's walk" in run.stderr, run.stderr


def test_reference_dumper_is_well_formed():
    """oracle/ref_recipe/dump_fixtures.cpp — the program that, on a machine with PCL 1.12 and a checkout of rsasaki0109/ndt_omp_ros2,
    dumps the REFERENCE's own numbers for every committed fixture (README there) — compiled with -fsyntax-only against stand-in
    pcl / pclomp headers (tests/cpp/mock), and the recipe's Python steps parse: the one-command pin cannot rot unnoticed."""
    import ast
    import subprocess

    rec = os.path.join(ROOT, "oracle", "ref_recipe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"),
                           os.path.join(rec, "dump_fixtures.cpp")])
    for f in ("export_inputs.py", "import_results.py"):
        ast.parse(open(os.path.join(rec, f)).read())
    cm = open(os.path.join(rec, "CMakeLists.txt")).read()
    assert "dump_fixtures.cpp" in cm and "src/pclomp" in cm
    assert "ref:" in open(os.path.join(ROOT, "oracle", "Makefile")).read()
    # round 6: the two SEQUENCES are part of the dump — the frontend drive (receiveCloud + updateMap) and the loop gate (searchLoop) —
    # and the import step turns them into the files tests/golden_fixtures.py:load_reference() looks for
    src = open(os.path.join(rec, "dump_fixtures.cpp")).read()
    assert '"frontend_stream"' in src.replace("\\", "") and '"loop_gate"' in src.replace("\\", "")
    # the degenerate-voxel scene is exported and dumped, and kd-tree membership comes from the tree's own cloud (getCentroids())
    assert '"ndt_degenerate"' in src.replace("\\", "") and "getCentroids()" in src and "nr_points >= 6" not in src
    assert '"ndt_degenerate"' in open(os.path.join(rec, "export_inputs.py")).read()
    import importlib.util
    import json
    import tempfile
    spec = importlib.util.spec_from_file_location("import_results", os.path.join(rec, "import_results.py"))
    imp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(imp)
    eye = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 2.5, 0, 0, 1]   # column-major, x = 2.5
    fake = {"frontend_stream": {"scans": [{"final": eye, "iterations": 6, "points_kept": 100}, {"final": eye, "iterations": 7, "points_kept": 90}], "update_at": [1]},
            "loop_gate": {"pair_id": [1, 20], "final": eye, "fitness": 0.1, "accepted": 1, "n_target_points": 1234, "iterations": 5}}
    # a degenerate-scene dump shaped like the reference's: the kd-tree cloud holds the in-tree leaves in leaf-map order
    import degenerate_scene as DS
    from ndt_numpy import NumpyGrid
    G = NumpyGrid(DS.make().target, DS.RES)
    npose = len(DS.POSES)
    fake["ndt_degenerate"] = dict(resolution=DS.RES, leaf_idx=G.idx.tolist(), leaf_n=G.n.tolist(), min_b=G.min_b.tolist(), max_b=G.max_b.tolist(),
                                  kd_cloud=G.centroid[G.in_tree].astype(np.float64).ravel().tolist())
    for t in ("d7", "kdtree"):
        fake["ndt_degenerate"].update({"score_" + t: [1.0] * npose, "grad_" + t: [0.5] * (6 * npose), "hess_" + t: [0.25] * (36 * npose),
                                       "final_" + t: eye, "iters_" + t: 4})
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "results.json"), "w") as f:
            json.dump(fake, f)
        wrote = imp.main(os.path.join(d, "results.json"), d)
        assert "ref_frontend_stream.npz" in wrote and "ref_loop_gate.npz" in wrote and "ref_ndt_degenerate.npz" in wrote
        dg = np.load(os.path.join(d, "ref_ndt_degenerate.npz"))
        # each kd-tree point is placed in its own leaf: the "point" leaves (n = -1) get their centroid, the 5-point leaf stays NaN
        assert np.array_equal(~np.isnan(dg["leaf_centroid"][:, 0]), G.in_tree) and (dg["leaf_n"] == -1).sum() >= 8
        assert np.array_equal(dg["leaf_centroid"][G.in_tree], G.centroid[G.in_tree])
        assert dg["grad_kdtree"].shape == (npose, 6) and dg["hess_d7"].shape == (npose, 6, 6) and dg["final_d7"][0, 3] == 2.5
        with pytest.raises(AssertionError):   # two tree points in one leaf cannot be placed
            imp.leaf_centroids_from_kd_cloud(np.repeat(G.centroid[:1], 2, 0).ravel(), G.idx, G.min_b, G.max_b, DS.RES)
        os.environ["LSR_GOLDEN_DIR"] = d
        try:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from golden_fixtures import load_reference
            fs, lg = load_reference("frontend_stream"), load_reference("loop_gate")
        finally:
            del os.environ["LSR_GOLDEN_DIR"]
        assert fs["poses"].shape == (2, 4, 4) and fs["poses"][0][0, 3] == 2.5 and fs["update_at"].tolist() == [1] and fs["points_kept"].tolist() == [100, 90]
        assert lg["pair_id"].tolist() == [1, 20] and bool(lg["accepted"]) and int(lg["n_target_points"]) == 1234 and lg["final"][0, 3] == 2.5
        assert load_reference("no_such_dump") is None


def test_c_abi_argument_validation_needs_no_device():
    """Error conventions of the boundary: status codes, never an exception or a crash — checked on
    the paths that do not need a device (null handles, invalid method, status strings)."""
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    lib.lsr_status_string.restype = C.c_char_p
    lib.lsr_last_error.restype = C.c_char_p
    names = {0: b"ok", -1: b"invalid argument", -3: b"HIP runtime error", -4: b"input target not set",
             -5: b"input source not set", -6: b"not implemented", -7: b"voxel index overflow", -8: b"too few points",
             -99: b"unknown status"}
    for code, text in names.items():
        assert lib.lsr_status_string(code) == text
    null = C.c_void_p(None)
    out16 = (C.c_float * 16)()
    dbl, i32 = C.c_double(), C.c_int()
    assert lib.lsr_destroy(null) == 0                                   # destroying nothing is fine
    assert lib.lsr_set_f64(null, _capi.RESOLUTION, C.c_double(1.0)) == -1
    assert b"null handle" in lib.lsr_last_error()
    assert lib.lsr_set_i32(null, _capi.MAX_ITERATIONS, 3) == -1
    assert lib.lsr_get_f64(null, _capi.RESOLUTION, C.byref(dbl)) == -1
    assert lib.lsr_get_i32(null, _capi.MAX_ITERATIONS, C.byref(i32)) == -1
    assert lib.lsr_set_input_target(null, None, 32, 0) == -1
    assert lib.lsr_set_input_source(null, None, 32, 0) == -1
    assert lib.lsr_align(null, None, out16, None, None, 0) == -1
    assert lib.lsr_get_final_transformation(null, out16) == -1
    assert lib.lsr_has_converged(null, C.byref(i32)) == -1
    assert lib.lsr_get_fitness_score(null, C.c_double(1.0), C.byref(dbl)) == -1
    assert lib.lsr_align_batch(None, 0, None, None, None) == -1
    # the controller's inspection entries: pointers and counts first, then the handle (test_ndt_controller_cpu.py has every argument)
    d6 = (C.c_double * 64)()
    assert lib.lsr_debug_ndt_controller_replay(null, d6, 0.1, 0.01, 35, 10, d6, 1, d6, C.byref(i32)) == -1
    assert lib.lsr_debug_ndt_controller_replay(null, d6, 0.1, 0.01, 35, 10, d6, 513, d6, C.byref(i32)) == -1
    assert lib.lsr_debug_ndt_controller_replay(null, None, 0.1, 0.01, 35, 10, None, 1, None, None) == -1
    assert lib.lsr_debug_ndt_solve6(null, d6, d6, 1, d6) == -1 and lib.lsr_debug_ndt_solve6(null, None, None, 0, None) == -1
    assert lib.lsr_debug_mt_math(null, d6, d6, 1, d6, d6) == -1 and lib.lsr_debug_mt_math(null, None, None, 0, None, None) == -1
    # the sort / scan / run inspection entries likewise (test_sort_primitives_cpu.py has every argument)
    u8, i8, f8 = (C.c_uint32 * 8)(), (C.c_int32 * 8)(), (C.c_float * 8)()
    assert lib.lsr_debug_sort_pairs_u32(null, u8, i8, 8, 12, 0, u8, i8, C.byref(i32)) == -1
    assert lib.lsr_debug_exclusive_scan_i32(null, i8, 8, 0, 0, i8) == -1
    assert lib.lsr_debug_sorted_runs(null, u8, i8, 8, f8, f8, f8, None, 9, 0, u8, i8, f8, f8, f8, None, C.byref(i32), C.byref(i32)) == -1
    assert lib.lsr_debug_lsd_plan(0, 12, i8) == -1 and lib.lsr_debug_lsd_plan(8, 12, None) == -1
    h = C.c_void_p()
    assert lib.lsr_create(7, 0, None, C.byref(h)) == -1 and not h.value  # registration_method neither NDT nor GICP
    assert lib.lsr_create(_capi.METHOD_NDT, 0, None, None) == -1
    n = C.c_int(-5)
    st = lib.lsr_device_count(C.byref(n))
    assert (st == 0 and n.value >= 0) or (st == -2 and n.value == 0)


def test_cfg4_fixture_is_well_formed():
    """tests/golden/cfg4_candidates_oracle.npz (CPU oracle on the 64 cfg-4 candidates; bench.py and the GPU tests compare with it)."""
    import os

    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg4_candidates_oracle.npz"))
    assert fx["final"].shape == (64, 4, 4) and fx["iterations"].shape == (64,) and fx["fitness"].shape == (64,)
    R = fx["final"][:, :3, :3]
    assert np.abs(R @ np.transpose(R, (0, 2, 1)) - np.eye(3)).max() < 1e-5      # fp32-composed rotations
    assert np.all(fx["converged"]) and fx["iterations"].min() >= 1 and fx["iterations"].max() <= 100
    assert np.all(fx["fitness"] > 0) and np.all(np.isfinite(fx["fitness"]))


def _snippets(path):
    """{name: text} of the blocks between '[snippet: NAME]' and '[end snippet]' marker lines (markers excluded; leading
    indentation and trailing blanks normalised)."""
    import re
    import textwrap

    out, name, buf = {}, None, []
    for line in open(path).read().splitlines():
        m = re.search(r"\[snippet: (\w+)\]", line)
        if m:
            name, buf = m.group(1), []
        elif "[end snippet]" in line and name:
            out[name] = textwrap.dedent("\n".join(buf)).strip("\n")
            name = None
        elif name:
            buf.append(line.rstrip())
    return out


def test_integration_md_snippets_compile_against_the_header(tmp_path):
    """Every code block of INTEGRATION.md that touches the C ABI lives verbatim in a file this test COMPILES and LINKS against
    include/lidarslam_reg.h + liblidarslam_reg.so: the pcl::Registration binding (include/lidarslam_reg/gfx950_registration.hpp,
    against tests/cpp/mock/pcl — virtual setInput*, non-virtual getFitnessScore, as in PCL 1.12) and tests/cpp/integration_snippets.cpp
    (construction sites, searchLoop in one call, PointCloud2 codec, sharded candidate set)."""
    import subprocess

    libdir = os.path.join(ROOT, "lidarslam_ros2_amd")
    exe = str(tmp_path / "integration_snippets")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "cpp", "mock"), os.path.join(ROOT, "tests", "cpp", "integration_snippets.cpp"),
                           "-o", exe, "-L" + libdir, "-llidarslam_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    doc = _snippets(os.path.join(ROOT, "INTEGRATION.md"))
    src = {}
    src.update(_snippets(os.path.join(ROOT, "include", "lidarslam_reg", "gfx950_registration.hpp")))
    src.update(_snippets(os.path.join(ROOT, "tests", "cpp", "integration_snippets.cpp")))
    assert set(src) == {"binding", "construction", "fitness", "search_loop", "pc2", "sharded", "planned"}
    assert set(doc) == set(src), (sorted(doc), sorted(src))
    for name in src:
        assert doc[name] == src[name], f"INTEGRATION.md block '{name}' differs from the compiled source"


def test_cfg4_tight_fixture_is_well_formed():
    """tests/golden/cfg4_candidates_oracle_tight.npz (make_cfg4_tight_fixture.py): tight-epsilon results and the CPU-vs-CPU
    spread of the eps-0.01 schedule under fp32-ulp perturbations.  The perturbed CPU runs take the same number of Newton
    iterations as the committed result on every candidate; only a short list of candidates moves by more than half the
    north_star bar — the list the GPU test bounds by its spread instead of the bar."""
    import os

    here = os.path.dirname(os.path.abspath(__file__))
    fx = np.load(os.path.join(here, "golden", "cfg4_candidates_oracle.npz"))
    fxt = np.load(os.path.join(here, "golden", "cfg4_candidates_oracle_tight.npz"))
    assert fxt["final_tight"].shape == (64, 4, 4) and fxt["final_fma"].shape == (64, 4, 4) and fxt["final_jitter"].shape[:2] == (64, 4)
    assert np.all(fxt["converged_tight"]) and fxt["iterations_tight"].max() <= 102
    assert np.array_equal(fxt["iterations_fma"], fx["iterations"])
    sp_t, sp_r = fxt["cpu_spread_translation_m"], fxt["cpu_spread_rotation_rad"]
    sensitive = [c for c in range(64) if sp_t[c] > 5e-4 or sp_r[c] > 5e-5]
    assert 1 <= len(sensitive) <= 6 and 34 in sensitive, sensitive
    from lidarslam_ros2_amd.posemath import pose_delta

    # where the eps-0.01 schedule stops short of the optimum (up to the 0.01 m termination tolerance) the two fixtures differ
    d = np.array([pose_delta(fx["final"][c], fxt["final_tight"][c])[0] for c in range(64)])
    assert np.median(d) < 0.02 and d.max() < 1.5


def test_c_ray_caster_is_bit_identical_to_the_numpy_one(monkeypatch):
    """lidarslam_ros2_amd/synth_raycast.c (workload generation only) restates raycast_geometry()'s IEEE double arithmetic
    operation for operation: the same rays hit, at the same ranges, to the last bit — the committed fixtures were generated
    with the numpy code and stay valid."""
    from lidarslam_ros2_amd import synth

    w = synth.make_world()
    for sensor, x in ((synth.vlp32(), 3.1), (synth.hdl64(), 41.7)):
        T = synth.trajectory_pose(x)
        synth._RAYCAST_C = None
        monkeypatch.delenv("LSR_SYNTH_NUMPY", raising=False)
        if synth._raycast_c() is None:
            pytest.skip("gcc could not build synth_raycast.c here")
        k1, t1 = synth.raycast_geometry(w, sensor, T)
        synth._RAYCAST_C = None
        monkeypatch.setenv("LSR_SYNTH_NUMPY", "1")
        k2, t2 = synth.raycast_geometry(w, sensor, T)
        synth._RAYCAST_C = None
        assert np.array_equal(k1, k2) and np.array_equal(t1, t2)
