"""The numpy restatement of one GICP linearisation (tests/gicp_numpy.py) against itself by finite differences, and the C++
oracle's cost / gradient against it — so that the reference the device pass is held to (tests/test_gicp_linearize_gpu.py) is
checked by something that shares no code with either."""
import numpy as np
import pytest

import gicp_numpy as GN
from lidarslam_ros2_amd import synth

# every angle non-zero, both signs, small and large
STATES = [(0.3, -0.2, 0.1, 0.05, -0.08, 0.12), (-1.2, 0.7, 0.4, -0.6, 0.35, -1.1), (0.02, 0.01, -0.03, 1.3, -0.9, 2.4),
          (0.0, 0.0, 0.0, 1e-3, -2e-3, 3e-3)]


@pytest.fixture(scope="module")
def pairs():
    """400 real correspondences with real Mahalanobis matrices: scan points, their neighbours in the filtered map, the oracle's
    regularised covariances."""
    from oracle import oracle as O

    c = synth.small_case(n_source=400, n_keyframes=2)
    tgt = synth.voxel_downsample(c.target, 0.4)
    nn = O.NearestNeighbour(tgt)
    p = O.transform_point_cloud(c.source, c.guess)
    idx, _ = nn.search(p)
    C1 = O.gicp_covariances(O.NearestNeighbour(p), p)
    C2 = O.gicp_covariances(nn, tgt)[idx]
    R = np.asarray(c.guess, np.float64)[:3, :3]
    M = np.asarray(GN.mahalanobis(C1, C2, R), np.float64)
    return p, tgt[idx], M


def test_mahalanobis_is_the_inverse():
    rng = np.random.default_rng(3)
    A, B = rng.normal(size=(2, 50, 3, 3))
    C1, C2 = A @ np.swapaxes(A, 1, 2) + 1e-3 * np.eye(3), B @ np.swapaxes(B, 1, 2) + 1e-3 * np.eye(3)
    R, _ = GN.state([0, 0, 0, 0.4, -0.3, 1.0])
    M = GN.mahalanobis(C1, C2, R)
    S = C2 + R @ C1 @ R.T
    # the longdouble inverse of a matrix of condition <= ~1e6, tested in fp64: cond * 2^-53 ~ 1e-10
    assert np.abs(np.asarray(M, np.float64) @ S - np.eye(3)).max() < 1e-9
    # transposing R or swapping the roles of C1 and C2 is a different matrix
    assert np.abs(np.asarray(GN.mahalanobis(C1, C2, R.T) - M, np.float64)).max() > 1e-3
    assert np.abs(np.asarray(GN.mahalanobis(C2, C1, R) - M, np.float64)).max() > 1e-3


@pytest.mark.parametrize("x", STATES)
def test_state_derivatives_are_central_differences_of_R(x):
    x = np.asarray(x, np.float64)
    R, dR = GN.state(x)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
    h = 1e-6
    for k in range(3):
        e = np.zeros(6)
        e[3 + k] = h
        fd = (GN.state(x + e)[0] - GN.state(x - e)[0]) / (2 * h)
        # every entry of R carries a few 2^-53 of rounding: / 2h -> < 5e-10; truncation h^2 / 6 = 2e-13
        assert np.abs(fd - dR[k]).max() < 1e-9, k
    assert np.abs(dR[2][2]).max() == 0.0          # the bottom row of Rz(psi) Ry Rx does not depend on psi
    assert np.abs(dR[0][:, 0]).max() < 1e-16      # the first column of Rz Ry Rx(phi) does not depend on phi


@pytest.mark.parametrize("x", STATES)
def test_gradient_sums_are_the_gradient_of_the_cost(pairs, x):
    """2/m (J^T M r) = grad of 1/m sum r^T M r, by central differences with an fp64 step of 1e-6: 1e-6 relative, per component."""
    p, q, M = pairs
    x = np.asarray(x, np.float64)
    R, dR = GN.state(x)
    res = p.astype(np.float64) @ R.T + x[:3] - q.astype(np.float64)
    sums, _ = GN.system(res, p, M, dR)
    m = p.shape[0]
    assert abs(float(sums[0] / m - GN.cost(x, p, q, M))) <= 1e-15 * float(sums[0] / m)
    g = np.asarray(2 * sums[1:7] / m, np.float64)
    h = 1e-6
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        fd = float((GN.cost(x + e, p, q, M) - GN.cost(x - e, p, q, M)) / (2 * h))
        assert abs(fd - g[k]) <= 1e-6 * abs(g[k]), (k, fd, g[k])
    # the 21 packed entries are the upper triangle of a symmetric positive semi-definite matrix: J^T M J with M > 0
    H = np.zeros((6, 6))
    for k, (i, j) in enumerate(GN.TRIU):
        H[i, j] = H[j, i] = float(sums[7 + k])
    assert np.linalg.eigvalsh(H).min() > -1e-9 * np.abs(H).max()
    # ... and its translation block is sum M
    assert np.abs(H[:3, :3] - M.sum(0)).max() <= 1e-12 * np.abs(M.sum(0)).max()


@pytest.mark.parametrize("x", STATES)
def test_oracle_cost_and_gradient_agree_with_the_numpy_system(pairs, x):
    """oracle.gicp_cost forms its residuals in fp32 (applyState's float matrix, the float transform, the float subtraction); the
    numpy system is fed fp64 residuals.  Each residual component then differs by at most
        d_i = 8 * 2^-24 * (|p_i|_1 + |t|_inf + |q_i|_inf)
    (matrix entries good to 2 ulp times the coordinates, three roundings of the sum, one of the subtraction), hence
        |f - f_ref| <= 1/m sum_i (2 |M_i r_i|_1 d_i + |M_i|_sum d_i^2),   |g - g_ref|_k <= 2/m sum_i |J_i|^T |M_i| 1 d_i."""
    from oracle import oracle as O

    p, q, M = pairs
    x = np.asarray(x, np.float64)
    R, dR = GN.state(x)
    res = p.astype(np.float64) @ R.T + x[:3] - q.astype(np.float64)
    sums, _ = GN.system(res, p, M, dR)
    m = p.shape[0]
    f_ref, g_ref = float(sums[0] / m), np.asarray(2 * sums[1:7] / m, np.float64)
    f, g = O.gicp_cost(p, q, M.reshape(-1, 9), x)
    d = 8 * 2.0 ** -24 * (np.abs(p).sum(1) + np.abs(x[:3]).max() + np.abs(q).max(1)).astype(np.float64)
    Mr1 = np.abs(np.einsum("nij,nj->ni", M, res)).sum(1)
    bound_f = float((2 * Mr1 * d + np.abs(M).sum((1, 2)) * d * d).sum() / m)
    J = np.zeros((m, 3, 6))
    J[:, :, :3] = np.eye(3)
    for k in range(3):
        J[:, :, 3 + k] = p.astype(np.float64) @ dR[k].T
    bound_g = 2 * np.einsum("nak,nab,n->k", np.abs(J), np.abs(M), d) / m
    print("f %.6e ref %.6e |diff| %.2e bound %.2e" % (f, f_ref, abs(f - f_ref), bound_f))
    print("g diff", np.abs(g - g_ref), "bound", bound_g)
    assert abs(f - f_ref) <= bound_f
    assert np.all(np.abs(g - g_ref) <= bound_g)
    assert bound_f < 1e-3 * f_ref and np.all(bound_g < 1e-2 * np.abs(g_ref).max())   # the bars mean something
