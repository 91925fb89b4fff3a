"""Degenerate target voxels (tests/degenerate_scene.py) on the CPU: the scene is exact, the oracle's grid equals an independent fp64
numpy build from the raw points (NumpyGrid), and the oracle's derivatives equal numpy's for all four neighbourhoods — KDTREE
included, where pclomp keeps the leaves its eigen check invalidated in the kd-tree as score-only neighbours (icov 0)."""
from fractions import Fraction

import numpy as np
import pytest

import degenerate_scene as DS
from ndt_numpy import NumpyGrid, NumpyNdt
from oracle import oracle as O

POSES = DS.POSES


@pytest.fixture(scope="module")
def scene():
    sc = DS.make()
    G = NumpyGrid(sc.target, DS.RES)
    og = O.VoxelGridCovariance(sc.target, DS.RES)
    kinds = np.array([sc.kinds[int(i)] for i in G.idx])
    return sc, G, og, kinds


def test_scene_kinds_are_what_geometry_says(scene):
    sc, G, _, kinds = scene
    assert np.array_equal(G.idx, np.array(sorted(sc.kinds), np.int32))
    expect = {"ordinary": (32, True, True, 0), "plane": (16, True, True, 1), "line": (16, True, True, 2),
              "point": (-1, True, False, 0), "five": (5, False, False, 0), "six": (6, True, True, 0)}
    for kind, (n, tree, valid, clamped) in expect.items():
        m = kinds == kind
        assert m.any(), kind
        assert (G.n[m] == n).all() and (G.in_tree[m] == tree).all() and (G.valid[m] == valid).all(), kind
        assert (G.clamped[m] == clamped).all(), kind
    assert (G.count[kinds == "point"] >= 8).all()
    # nothing rounding-decided: every ordinary leaf is far from the clamp threshold
    w = np.linalg.eigvalsh(G.cov[kinds == "ordinary"])
    assert (w[:, 0] > 0.05 * w[:, 2]).all()
    assert (~np.isfinite(sc.target).all(1)).sum() >= 3          # the non-finite run of the builders


def test_scene_covariances_are_exact(scene):
    """Per power-of-two leaf, the fp64 single-pass covariance (before the clamp) equals the exact rational one."""
    sc, G, _, kinds = scene
    fin = sc.target[np.isfinite(sc.target).all(1)]
    inv = np.float32(1) / np.float32(DS.RES)
    ijk = (np.floor(fin * inv) - G.min_b.astype(np.float32)).astype(np.int64)
    div = G.max_b - G.min_b + 1
    key = ijk @ np.array([1, div[0], div[0] * div[1]])
    checked = 0
    for li, k in enumerate(G.idx):
        if int(k) not in sc.exact:
            continue
        P = [[Fraction(float(v)) for v in q] for q in fin[key == k]]
        n = len(P)
        s = [sum(q[a] for q in P) for a in range(3)]
        m = [v / n for v in s]
        exact = [[((sum(q[a] * q[b] for q in P) - 2 * s[a] * m[b]) / n + m[a] * m[b]) * Fraction(n - 1, n) for b in range(3)]
                 for a in range(3)]
        mean64 = G.sum[li] / n
        cov64 = ((G.sq[li] - 2.0 * np.outer(G.sum[li], mean64)) / n + np.outer(mean64, mean64)) * ((n - 1.0) / n)
        assert all(Fraction(float(mean64[a])) == m[a] for a in range(3)), li
        assert all(Fraction(float(cov64[a, b])) == exact[a][b] for a in range(3) for b in range(3)), (li, kinds[li])
        if kinds[li] in ("plane", "line", "point"):
            assert all(exact[a][b] == 0 for a in range(3) for b in range(3) if a != b)     # diagonal: eigensolvers are exact
        checked += 1
    assert checked == len(sc.exact) == (kinds != "six").sum() - (kinds == "five").sum()


def test_oracle_grid_equals_numpy_grid(scene):
    sc, G, og, kinds = scene
    d = og.dump()
    assert np.array_equal(og.min_b, G.min_b) and np.array_equal(og.max_b, G.max_b)
    assert np.array_equal(d["idx"], G.idx) and np.array_equal(d["n"], G.n)
    assert (d["n"] == -1).sum() == (kinds == "point").sum() and og.n_valid == G.n_valid
    assert np.array_equal(d["mean"], G.mean)
    v = G.valid
    num = np.abs(d["icov"][v] - G.icov[v]).max(axis=(1, 2))
    assert (num / np.abs(G.icov[v]).max(axis=(1, 2))).max() < 1e-12
    assert not d["icov"][~v].any()
    # the clamp: the dumped covariance of a plane / line leaf is its diagonal with the zero eigenvalues raised to 0.01 * lambda2
    for li in np.nonzero((kinds == "plane") | (kinds == "line"))[0]:
        c = d["cov"][li]
        assert np.array_equal(c, np.diag(np.diag(c))) and np.array_equal(c, G.cov[li])
        w = np.sort(np.diag(c))
        assert w[0] == 0.01 * w[2] and (w[1] == 0.01 * w[2]) == (kinds[li] == "line")
    cen = og.centroids()
    assert np.array_equal(cen[G.in_tree], G.centroid[G.in_tree])
    pt = kinds == "point"   # a "point" leaf's centroid is its point
    assert np.array_equal(cen[pt], G.mean[pt].astype(np.float32))


@pytest.mark.parametrize("search", [1, 7, 26, 0])
def test_oracle_derivatives_equal_numpy(scene, search):
    sc, G, og, _ = scene
    d1, d2, _ = O.gauss_constants(DS.RES)
    ref = NumpyNdt(G.dump(), G.min_b, G.max_b, DS.RES, d1, d2, search=search, centroids=G.centroid)
    for p in POSES:
        p = sc.truth + p
        s, g, _ = O.ndt_derivatives(og, sc.source, p, resolution=DS.RES, search=search)
        s64, g64 = ref.score_grad(sc.source, p)
        assert abs(s - s64) <= 2e-5 * abs(s64)
        assert np.abs(g - g64).max() <= 1e-4 * np.abs(g64).max()


def test_kdtree_keeps_invalidated_leaves_as_score_only_neighbours(scene):
    """pclomp pushes a leaf's centroid into the kd-tree before its eigen check; radiusSearch() and computeDerivatives() never test
    nr_points.  A "point" leaf (cov = 0, nr_points = -1) within `resolution` of a source point is a neighbour with icov 0: exp(0) = 1,
    d2 * 1 passes the [0, 1] test, the pair adds exactly -d1 to the score and nothing to the gradient."""
    sc, G, og, _ = scene
    d1, d2, _ = O.gauss_constants(DS.RES)
    assert 0 < d2 <= 1
    kw = dict(search=0, centroids=G.centroid)
    with_ = NumpyNdt(G.dump(), G.min_b, G.max_b, DS.RES, d1, d2, kd_invalid=True, **kw)
    without = NumpyNdt(G.dump(), G.min_b, G.max_b, DS.RES, d1, d2, kd_invalid=False, **kw)
    for p in POSES:
        p = sc.truth + p
        sw, gw = with_.score_grad(sc.source, p)
        so, go = without.score_grad(sc.source, p)
        k = with_.kd_score_only
        assert k >= 50 and without.kd_score_only == 0
        assert abs((sw - so) - k * -d1) <= 1e-9 * abs(sw) and np.array_equal(gw, go)
        s, g, H = O.ndt_derivatives(og, sc.source, p, resolution=DS.RES, search=0)
        assert abs(s - sw) <= 2e-5 * abs(sw) and abs(s - sw) < 0.01 * k * abs(d1)     # the "with" value, not the "without" one
        assert np.abs(g - gw).max() <= 1e-4 * np.abs(gw).max()
        # computeHessian's fp64 path takes the same neighbours (score-only ones add exactly nothing there either)
        _, _, H64 = O.ndt_derivatives(og, sc.source, p, resolution=DS.RES, search=0, fp64_hessian=True)
        assert np.abs(H - H64).max() <= 1e-4 * np.abs(H64).max()


@pytest.mark.parametrize("search", [7, 0])
def test_oracle_registers_the_degenerate_scene(scene, search):
    """Registration from the identity finds `truth` with every neighbourhood; the KDTREE score-only terms move no step."""
    sc, _, og, _ = scene
    r = O.ndt_align(og, sc.source, np.eye(4, dtype=np.float32), resolution=DS.RES, search=search)
    e = O.matrix_to_pose(r["final"]) - sc.truth
    assert r["converged"] and np.abs(e[:3]).max() < 0.03 and np.abs(e[3:]).max() < 0.005


def test_oracle_equals_the_reference_dump_when_there_is_one(scene):
    """oracle/ref_recipe dumps this scene through pclomp itself (tests/golden/ref_ndt_degenerate.npz, made on a machine with PCL).
    Once that file exists the oracle is held to it: leaf counts with the -1 entries, kd-tree membership as the tree's own cloud shows
    it (not inferred from nr_points), the centroids bit for bit, and the D7 / KDTREE derivatives."""
    from golden_fixtures import load_reference

    sc, G, og, _ = scene
    ref = load_reference("ndt_degenerate")
    if ref is None:   # no reference dump on this machine: the oracle is held to the numpy build above
        return
    d = og.dump()
    assert np.array_equal(ref["leaf_idx"], d["idx"]) and np.array_equal(ref["leaf_n"], d["n"])
    assert np.array_equal(ref["min_b"], og.min_b) and np.array_equal(ref["max_b"], og.max_b)
    in_tree = ~np.isnan(ref["leaf_centroid"][:, 0])
    assert np.array_equal(in_tree, G.in_tree) and np.array_equal(ref["leaf_centroid"][in_tree], og.centroids()[in_tree])
    for tag, search in (("d7", 7), ("kdtree", 0)):
        for k, dp in enumerate(POSES):
            s, g, H = O.ndt_derivatives(og, sc.source, sc.truth + dp, resolution=DS.RES, search=search)
            assert abs(s - ref["score_" + tag][k]) <= 1e-5 * abs(ref["score_" + tag][k]), (tag, k)
            assert np.abs(g - ref["grad_" + tag][k]).max() <= 2e-5 * np.abs(ref["grad_" + tag][k]).max(), (tag, k)
            assert np.abs(H - ref["hess_" + tag][k]).max() <= 2e-5 * np.abs(ref["hess_" + tag][k]).max(), (tag, k)
