"""Plain numpy restatement of one GICP linearisation (Segal, Haehnel, Thrun 2009, eq. 2; the cost pclomp's
GeneralizedIterativeClosestPoint minimises), written from the definition:

    r_i = R(x) p_i + t - q_i,   M_i = (C2_j + Rm C1_i Rm^T)^-1,   f(x) = 1/m sum r_i^T M_i r_i,
    x = (t, phi, theta, psi),   R = Rz(psi) Ry(theta) Rx(phi),    J_i = dr_i/dx = [I | dR/dphi p_i, dR/dtheta p_i, dR/dpsi p_i]

the "maths truth" the device's correspondence / Gauss-Newton pass (lsr_gicp_linearize) and the C++ oracle are held to.
Sums are formed in np.longdouble (64-bit mantissa on x86).  Test infrastructure only."""
import numpy as np

LD = np.longdouble


def _elementary(axis, a):
    """-> (rotation about `axis` by a, its derivative with respect to a), fp64."""
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]        # the plane the rotation turns, in right-handed order
    E, dE = np.eye(3), np.zeros((3, 3))
    E[i, i] = E[j, j] = c
    E[j, i], E[i, j] = s, -s
    dE[i, i] = dE[j, j] = -s
    dE[j, i], dE[i, j] = c, -c
    return E, dE


def state(x):
    """x = (t, phi, theta, psi) -> (R, dR): R = Rz(psi) Ry(theta) Rx(phi) and dR[k] = dR/d(phi, theta, psi)[k], as products of
    the elementary rotations and their derivatives (fp64)."""
    x = np.asarray(x, np.float64)
    Rx, dRx = _elementary(0, x[3])
    Ry, dRy = _elementary(1, x[4])
    Rz, dRz = _elementary(2, x[5])
    return Rz @ Ry @ Rx, np.stack([Rz @ Ry @ dRx, Rz @ dRy @ Rx, dRz @ Ry @ Rx])


def mahalanobis(C1, C2, R):
    """inv(C2 + R C1 R^T) in np.longdouble; C1, C2: (..., 3, 3)."""
    C1, C2, R = np.asarray(C1, LD), np.asarray(C2, LD), np.asarray(R, LD)
    S = C2 + R @ C1 @ R.T
    adj = np.empty_like(S)
    for i in range(3):                            # inverse = adjugate / determinant
        for j in range(3):
            a, b, c, d = (j + 1) % 3, (j + 2) % 3, (i + 1) % 3, (i + 2) % 3
            adj[..., i, j] = S[..., a, c] * S[..., b, d] - S[..., a, d] * S[..., b, c]
    det = S[..., 0, 0] * adj[..., 0, 0] + S[..., 0, 1] * adj[..., 1, 0] + S[..., 0, 2] * adj[..., 2, 0]
    return adj / det[..., None, None]


TRIU = [(i, j) for i in range(6) for j in range(i, 6)]   # the 21 entries of the upper triangle, row by row


def system(res, p, M, dR):
    """The 28 sums of one Gauss-Newton linearisation over the pairs (res_i, p_i, M_i), J_i = [I | dR_k p_i]:
    [0] sum r^T M r, [1..6] sum J^T M r, [7..27] the upper triangle of sum J^T M J row by row — and, second, the sum of the
    ABSOLUTE values of the per-pair terms of each (the scale any summation order's rounding error is proportional to).
    res, p: (m, 3); M: (m, 3, 3); dR: (3, 3, 3).  Both results np.longdouble (28,)."""
    res, p, M, dR = np.asarray(res, LD), np.asarray(p, LD), np.asarray(M, LD), np.asarray(dR, LD)
    m = res.shape[0]
    J = np.zeros((m, 3, 6), LD)
    J[:, :, :3] = np.eye(3, dtype=LD)
    for k in range(3):
        J[:, :, 3 + k] = p @ dR[k].T
    Jt = np.swapaxes(J, 1, 2)
    Mr = (M @ res[:, :, None])[:, :, 0]
    terms = np.empty((m, 28), LD)
    terms[:, 0] = (res * Mr).sum(1)
    terms[:, 1:7] = (Jt @ Mr[:, :, None])[:, :, 0]
    H = Jt @ M @ J
    for k, (i, j) in enumerate(TRIU):
        terms[:, 7 + k] = H[:, i, j]
    return terms.sum(0), np.abs(terms).sum(0)


def cost(x, p, q, M):
    """f(x) = 1/m sum r^T M r with the residuals formed in fp64 from x (smooth in x), summed in longdouble."""
    R, _ = state(x)
    r = np.asarray(p, np.float64) @ R.T + np.asarray(x, np.float64)[:3] - np.asarray(q, np.float64)
    r, M = np.asarray(r, LD), np.asarray(M, LD)
    return ((r * (M @ r[:, :, None])[:, :, 0]).sum() / LD(r.shape[0]))


def xform32(rows, p):
    """fp32 point transform in the reference's order, ((m0 x + m1 y) + m2 z) + m3, every operation rounded to float32 on its
    own (what the device's xform_rn does with __fmul_rn / __fadd_rn).  rows: (3, 4) — a row-major 3x4 or the top of a 4x4."""
    rows, p = np.asarray(rows, np.float32), np.asarray(p, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty((p.shape[0], 3), np.float32)
    for r in range(3):
        out[:, r] = ((rows[r, 0] * x + rows[r, 1] * y) + rows[r, 2] * z) + rows[r, 3]
    return out


def sym6_to_33(M6):
    """(n, 6) = 00 01 02 11 12 22 -> (n, 3, 3)."""
    M6 = np.asarray(M6)
    M = np.empty(M6.shape[:-1] + (3, 3), M6.dtype)
    for k, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        M[..., i, j] = M6[..., k]
        M[..., j, i] = M6[..., k]
    return M
