"""Degenerate target voxels (tests/degenerate_scene.py) on the device: the grid builders against the independent numpy grid
(plane / line leaves clamped, "point" leaves invalidated but in the kd-tree), every launch variant of every neighbourhood against
the oracle, registrations, candidate sets and shared targets.  KDTREE keeps pclomp's invalidated leaves as score-only neighbours."""
import numpy as np
import pytest

import degenerate_scene as DS
from lidarslam_ros2_amd.posemath import pose_delta
from ndt_numpy import NumpyGrid, NumpyNdt
from ndt_variants import POSE_R_TOL, POSE_T_TOL, VARIANTS, tune

pytestmark = pytest.mark.gpu

METHODS = ["DIRECT1", "DIRECT7", "DIRECT26", "KDTREE"]
SEARCH = {"DIRECT1": 1, "DIRECT7": 7, "DIRECT26": 26, "KDTREE": 0}
FAR = np.float32([3000.0, 3000.0, 0.0])      # a far copy of the scene: > 4 Mi cells, the compact leaf table


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def sc():
    return DS.make()


def make_ndt(method="DIRECT7", eps=0.01, max_iter=None):
    import lidarslam_ros2_amd as L

    ndt = L.NormalDistributionsTransform(device=0)
    ndt.setResolution(DS.RES)
    ndt.setTransformationEpsilon(eps)
    ndt.setNeighborhoodSearchMethod(getattr(L, method))
    if max_iter is not None:
        ndt.setMaximumIterations(max_iter)
    return ndt


@pytest.mark.parametrize("builder", ["auto", "radix", "compact"])
def test_grid_matches_numpy(sc, builder):
    tgt = sc.target if builder != "compact" else np.concatenate([sc.target, sc.target + FAR])
    G = NumpyGrid(tgt, DS.RES)
    ndt = make_ndt("KDTREE")
    if builder == "radix":
        ndt.setTuning(grid_builder=1)
    ndt.setInputTarget(tgt)
    info, d = ndt.gridInfo(), ndt.gridDump()
    if builder == "compact":
        assert np.prod((info["max_b"] - info["min_b"] + 1).astype(np.int64)) > 4 * 2**20
    assert np.array_equal(info["min_b"], G.min_b) and np.array_equal(info["max_b"], G.max_b)
    assert np.array_equal(d["idx"], G.idx) and np.array_equal(d["n"], G.n)
    assert (d["n"] == -1).sum() >= 8 and info["n_valid"] == G.n_valid
    # every sum of this scene is exact: the device's tree-order fp64 sums give numpy's means bit for bit
    assert np.array_equal(d["mean"], G.mean)
    # the covariances of the power-of-two leaves are exact too; a 6-point leaf's rounded mean enters the single-pass covariance,
    # whose cancellation 3 km out (compact) leaves the summation order's trace
    exact = (G.count & (G.count - 1)) == 0
    num = np.abs(d["icov"] - G.icov).max(axis=(1, 2))
    rel = num / np.maximum(np.abs(G.icov).max(axis=(1, 2)), 1e-300)
    assert rel[G.valid & exact].max() < 1e-12 and rel[G.valid].max() < 1e-6
    assert not d["icov"][~G.valid].any()
    cen = ndt.gridCentroids()
    assert np.array_equal(cen[G.in_tree], G.centroid[G.in_tree])                     # "point" leaves included
    assert np.isnan(cen[~G.in_tree]).all() and (G.count[~G.in_tree] == 5).all()                # the 5-point leaf: in nothing


@pytest.mark.parametrize("method", METHODS)
def test_every_launch_variant_matches_the_oracle(O, sc, method):
    """Derivatives through every kernel instantiation against the oracle, at test_ndt_gpu's tolerances; within the method every variant
    gives the same bits.  For KDTREE the oracle's value is the one WITH the score-only neighbours: the pre-fix kernels miss k * -d1."""
    grid = O.VoxelGridCovariance(sc.target, DS.RES)
    d1, d2, _ = O.gauss_constants(DS.RES)
    poses = [sc.truth + np.array([0.05, -0.03, 0.02, 0.004, -0.002, 0.006]), sc.truth * 0.5]
    ref = [O.ndt_derivatives(grid, sc.source, p, compute_hessian=h, resolution=DS.RES, search=SEARCH[method])
           for p, h in zip(poses, (True, False))]
    if method == "KDTREE":
        G = NumpyGrid(sc.target, DS.RES)
        wo = NumpyNdt(G.dump(), G.min_b, G.max_b, DS.RES, d1, d2, search=0, centroids=G.centroid, kd_invalid=False)
        w = NumpyNdt(G.dump(), G.min_b, G.max_b, DS.RES, d1, d2, search=0, centroids=G.centroid)
        for p, (rs, _, _) in zip(poses, ref):
            w.score_grad(sc.source, p)
            so = wo.score_grad(sc.source, p)[0]
            assert w.kd_score_only >= 50 and abs((rs - so) - w.kd_score_only * -d1) < 1e-3 * w.kd_score_only * -d1
    first = None
    for v in VARIANTS:
        ndt = make_ndt(method)
        tune(ndt, v)
        ndt.setInputTarget(sc.target)
        ndt.setInputSource(sc.source)
        got = [ndt.derivatives(p, compute_hessian=h) for p, h in zip(poses, (True, False))]
        for (s, g, H), (rs, rg, rH), hess in zip(got, ref, (True, False)):
            assert abs(s - rs) <= 1e-5 * abs(rs), (v, s, rs, (s - rs) / d1)
            assert np.abs(g - rg).max() <= 2e-5 * np.abs(rg).max(), v
            if hess:
                assert np.abs(H - rH).max() <= 2e-5 * np.abs(rH).max(), v
        if first is None:
            first = got
        for (s, g, H), (s0, g0, H0) in zip(got, first):
            assert s == s0 and np.array_equal(g, g0) and np.array_equal(H, H0), v


@pytest.mark.parametrize("method", METHODS)
def test_align_matches_the_oracle(O, sc, method):
    grid = O.VoxelGridCovariance(sc.target, DS.RES)
    guess = np.eye(4, dtype=np.float32)
    for eps, mi in ((0.01, 35), (1e-6, 30)):
        ndt = make_ndt(method, eps, mi)
        ndt.setInputTarget(sc.target)
        ndt.setInputSource(sc.source)
        ndt.align(guess)
        ref = O.ndt_align(grid, sc.source, guess, resolution=DS.RES, trans_eps=eps, max_iterations=mi, search=SEARCH[method])
        dt, ang = pose_delta(ndt.getFinalTransformation(), ref["final"])
        assert dt <= POSE_T_TOL and ang <= POSE_R_TOL, (eps, dt, ang)
        if eps == 0.01:
            assert ndt.getFinalNumIteration() == ref["iterations"] and ndt.hasConverged() == ref["converged"]


def test_batch_and_shared_target_equal_single_aligns(sc):
    """Objects sharing one target, KDTREE and DIRECT7 ones: a candidate set of each method (a set shares its method) returns for each
    member the pose and iteration count its own align() gives, bit for bit."""
    from lidarslam_ros2_amd import align_batch

    rng = np.random.default_rng(4)
    lead = make_ndt("KDTREE")
    lead.setInputTarget(sc.target)
    regs, guesses, singles = [], [], []
    for b in range(6):
        r = lead if b == 0 else make_ndt("KDTREE" if b % 2 == 0 else "DIRECT7")
        if b:
            r.shareTargetOf(lead)
        r.setInputSource(sc.source[: len(sc.source) - 97 * b])
        g = np.eye(4, dtype=np.float32)
        g[:3, 3] = rng.uniform(-0.05, 0.05, 3)
        regs.append(r)
        guesses.append(g)
    for r, g in zip(regs, guesses):
        r.align(g)
        singles.append((r.getFinalTransformation().copy(), r.getFinalNumIteration()))
    for members in ([0, 2, 4], [1, 3, 5]):
        finals, results = align_batch([regs[b] for b in members], [guesses[b] for b in members])
        for k, b in enumerate(members):
            assert np.array_equal(finals[k], singles[b][0]), (b, pose_delta(finals[k], singles[b][0]))
            assert results[k]["iterations"] == singles[b][1], b
