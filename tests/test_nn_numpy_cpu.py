"""The nearest-neighbour reference and the inputs of tests/test_nn_forms_gpu.py, checked without a GPU: brute_nn equals the oracle's
grid search bit for bit on every adversarial cloud, and every property the GPU tests rely on to reach a search form BY SHAPE —
how many queries the capped walk proves, defers, finds outside the grid; which members of a fitness group fill the work list;
which builder a wide target takes — is asserted here with brute force and the numpy grid."""
import numpy as np
import pytest

import nn_numpy as N

F = np.float32


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.mark.parametrize("name", [n for n, _ in N.clouds()])
def test_brute_nn_equals_the_oracle(O, name):
    pts = N.cloud(name)
    nn = O.NearestNeighbour(pts, cell=1.0)
    for cell in (0.5, 0.4625, 0.37):
        q = N.query_mix(pts, cell, nonfinite=False)      # (the oracle's ring walk is defined for finite queries only)
        for T in (None, N.yaw_pose()):
            idx, d2 = N.brute_nn(pts, q, T)
            ridx, rd2 = nn.search(q, T)
            assert np.array_equal(d2, rd2) and np.array_equal(idx, ridx), (name, cell, T is None)
            if T is None:   # the one-query reference the host emulation tests use
                for i in range(0, len(q), 7):
                    j, dj = N.brute_nn1(pts, q[i])
                    assert idx[i] == j and d2[i] == dj
            assert N.brute_fitness(pts, q, T, 1.0) == pytest.approx(nn.fitness_score(q, T if T is not None else np.eye(4), 1.0), rel=N.fitness_rel_tol(len(q)))


def test_brute_nn_edges():
    pts = np.vstack([N.cloud("duplicates"), np.full((1, 3), np.nan, F)])
    q = N.query_mix(N.cloud("duplicates"), 0.5)
    idx, d2 = N.brute_nn(pts, q)
    assert np.array_equal(idx[-3:], [-1, -1, -1]) and np.all(np.isinf(d2[-3:]))          # nan, inf, and 1e30 (every d2 overflows)
    assert idx[:-3].min() >= 0 and idx.max() < len(pts) - 1                                # the non-finite target point is never an answer
    hits = slice(200, 230)
    assert np.array_equal(idx[hits], np.arange(30)) and np.all(d2[hits] == 0)             # duplicates: the lowest index
    assert np.array_equal(N.brute_nn(pts[-1:], q)[0], np.full(len(q), -1))                # no finite target point at all
    e = N.brute_nn(pts, np.zeros((0, 3), F))
    assert e[0].shape == (0,) and N.brute_fitness(pts, np.zeros((0, 3), F), None) == N.DBL_MAX
    assert N.brute_fitness(pts, q[-3:], None) == N.DBL_MAX
    # max_range is inclusive (PCL tests <=)
    one = np.float32([[0, 0, 0]])
    assert N.brute_fitness(one, np.float32([[0.5, 0, 0], [0, 2, 0]]), None, 0.25) == 0.25
    # chunking does not change the answer
    a, b = N.brute_nn(pts, q, N.yaw_pose(), chunk=4096), N.brute_nn(pts, q, N.yaw_pose(), chunk=7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_query_mix_holds_what_it_says():
    beyond = at_edge = 0
    for name, pts in N.clouds():
        for cell in (0.5, 0.4625, 0.37):
            q = N.query_mix(pts, cell)
            assert q.shape == (150 + 50 + 30 + 12 + 12 + 3, 3) and q.dtype == F
            org, cdim = N.grid_dims(pts, cell)
            faces = q[230:242]
            lo, hi = pts.min(0), pts.max(0)
            for k, p in enumerate(faces):
                a, side, c = (k % 6) // 2, k % 2, (1, 6)[k // 6]
                assert p[a] == (lo[a] - F(c) * F(cell) if side == 0 else hi[a] + F(c) * F(cell))
            out = N.cells_outside(faces, cell, org, cdim)
            assert np.array_equal(N.cells_outside(q[242:254], cell, org, cdim), [1] * 6 + [6] * 6)
            fg = N.fine_cell(q[242:248], cell, org)
            assert all(fg[2 * a, a] == -1 and fg[2 * a + 1, a] == 8 * cdim[a] for a in range(3))
            beyond += int((out > N.NN_MAX_FINE_RINGS).sum())       # (the grid box is aligned to 8 cells: up to 7 wider than the bounding box)
            at_edge += int(((out >= 1) & (out <= N.NN_MAX_FINE_RINGS)).sum())
            idx, d2 = N.brute_nn(pts, q)
            assert np.all(d2[200:230] == 0)
    assert beyond >= 20 and at_edge >= 20      # queries outside the grid within the fine shells' reach, and beyond it
    pile = N.cloud("pile")
    g = N.build_grid(pile, 0.37)
    assert np.unique(g["rel"], axis=0, return_counts=True)[1].max() >= 300                                  # several waves' worth of candidates in ONE fine cell
    assert len(N.cloud("single")) == 1 and np.array_equal(N.cloud("pair")[0], N.cloud("pair")[1])


@pytest.mark.parametrize("n", [N.NN_WAVE_MAX_QUERIES + 1, N.NN_WAVE_MAX_QUERIES + 4096 + 3])
def test_large_query_set_conditions(n):
    """More than 262 144 queries: nn_search_device takes nn1_kernel (ring_cap = 2) + nn1_coop_kernel.  The shares below are what
    makes both halves do real work."""
    tgt = N.large_target()
    assert len(tgt) <= 2048 and np.isfinite(tgt).all()
    org, cdim = N.grid_dims(tgt, N.LARGE_CELL)
    assert cdim[0] <= 16 and cdim[1] <= 16 and cdim[2] <= 4
    others = np.linalg.norm(tgt[:-1].astype(np.float64) - N.ISOLATED[None, :], axis=1)
    assert np.array_equal(tgt[-1], N.ISOLATED) and others.min() > 3.0
    for posed in ((False, True) if n == N.NN_WAVE_MAX_QUERIES + 1 else (False,)):
        T = N.yaw_pose() if posed else None
        src = N.large_source(n, posed)
        assert src.shape == (n, 3) and n > N.NN_WAVE_MAX_QUERIES
        idx, d2 = N.large_brute(n, posed)
        q = N.transform_rn(src, T)
        found = idx >= 0
        d = np.sqrt(d2.astype(np.float64))
        assert (~np.isfinite(q).all(1)).sum() == 64 and (~found).sum() == 64
        assert (d[found] <= 0.5).sum() >= 0.5 * n                       # proven by the capped walk
        assert (d[found] > 3 * N.LARGE_CELL).sum() >= 20000             # certainly deferred: after shell 2 the bound is <= 3 cells
        assert (N.cells_outside(q[found], N.LARGE_CELL, org, cdim) > N.NN_MAX_FINE_RINGS).sum() >= 5000
        if not posed:
            assert (d2 == 0).sum() >= 1000
            gate = (d2 == F(0.25)) & (idx == len(tgt) - 1)
            assert gate.sum() >= 100                                    # exactly ON max_range = 0.25: counted, PCL tests <=
            with_gate, without = N.brute_fitness(tgt, src, T, 0.25, (idx, d2)), N.brute_fitness(tgt, src, T, np.nextafter(0.25, 0), (idx, d2))
            assert with_gate != without


def test_all_deferred_shift():
    """+1 000 m in x: every finite query is hundreds of cells outside the grid, the work list is full to its last slot but 64."""
    n = N.NN_WAVE_MAX_QUERIES + 1
    tgt = N.large_target()
    org, cdim = N.grid_dims(tgt, N.LARGE_CELL)
    q = N.large_source(n) + np.float32([1000.0, 0, 0])
    fin = np.isfinite(q).all(1)
    assert fin.sum() == n - 64
    assert (N.cells_outside(q[fin], N.LARGE_CELL, org, cdim) > N.NN_MAX_FINE_RINGS).all()


def test_group_member_conditions():
    tgt = N.group_target()
    assert tgt.shape == (3000, 3) and np.isfinite(tgt).all()
    members = N.group_members()
    assert len(members) == 13
    names = [m[0] for m in members]
    assert names[7] == "empty" and members[7][2].shape == (0, 3) and names[8] == "pose_1e30"
    org, cdim = N.grid_dims(tgt, N.GROUP_CELL)
    for k, (name, T, src) in enumerate(members):
        assert len(src) <= 4400 and src.dtype == F
        defer = N.must_defer(tgt, src, T, N.GROUP_CELL)
        idx, d2 = N.brute_nn(tgt, src, T)
        if name.startswith(("half_out", "far", "ball")):
            assert defer.sum() >= 1000, (name, defer.sum())
        if name.startswith("on"):
            assert (np.sqrt(d2) < 0.1).all()
        if name.startswith("shifted"):
            fq = N.fine_cell(N.transform_rn(src, T), N.GROUP_CELL, org)
            ft = N.fine_cell(tgt, N.GROUP_CELL, org)
            occupied = set(map(tuple, ft))
            own_empty = sum(tuple(c) not in occupied for c in fq)
            assert own_empty >= 1000                                    # the 3 x 3 x 3 seed runs
        if name == "faces":
            fq = N.fine_cell(N.transform_rn(src, T), N.GROUP_CELL, org)
            fdim = cdim * 8
            assert len(src) == 2400 and ((fq == -1).any(1)).sum() >= 300 and (fq < -1).any(1).sum() >= 300
            assert (fq == fdim[None, :]).any(1).sum() >= 300 and (fq > fdim[None, :]).any(1).sum() >= 300
        if name == "ball":
            d = np.sqrt(d2.astype(np.float64))
            assert d.min() >= 2.0 and d.max() <= 3.0 and (N.cells_outside(N.transform_rn(src, T), N.GROUP_CELL, org, cdim) == 0).all()
        if name == "nonfinite":
            assert (~np.isfinite(src).all(1)).sum() == 64 and (idx < 0).sum() == 64
        if name == "pose_1e30":
            assert (idx < 0).all() and N.brute_fitness(tgt, src, T) == N.DBL_MAX


def test_wide_target_takes_the_sort_builder_and_the_widest_overflows():
    tgt = N.wide_target(600.0)
    assert len(tgt) == 4000 and np.isfinite(tgt).all()
    org, cdim = N.grid_dims(tgt, N.WIDE_CELL)
    assert cdim[0] >= 150 and cdim[1] >= 150 and cdim[2] >= 3
    assert int(np.prod(cdim)) > 32768 and int(np.prod(cdim)) * 512 > N.NN_BUCKET_MAX_KEYS       # nkeys > 16 Mi: sorted, not bucketed
    assert int(np.prod(cdim)) * 512 < 0xFFFFFFFF
    q = N.wide_queries(600.0)
    assert q.shape == (4200, 3) and len(q) <= N.NN_WAVE_MAX_QUERIES
    d = np.sqrt(N.brute_nn(tgt, q)[1].astype(np.float64))
    assert d.max() <= 40.0 and (d[4000:] > 2.0).sum() >= 50           # nothing in the empty middle, some well off the copies
    org, cdim = N.grid_dims(N.wide_target(12000.0), N.WIDE_CELL)
    assert cdim[0] >= 3000 and cdim[1] >= 3000 and int(np.prod(cdim)) * 512 >= 2 ** 32        # LSR_ERR_INDEX_OVERFLOW
