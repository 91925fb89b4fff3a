"""TEST INFRASTRUCTURE: a dense fp64 numpy restatement of the pose-graph optimisation of GraphBasedSlamComponent::doPoseAdjustment
(graph_based_slam_component.cpp:267-319) — g2o's VertexSE3 / EdgeSE3 with identity information under its Levenberg-Marquardt
controller, ten iterations — written from the specification (DESIGN.md 4 "Pose-graph optimisation"), independently of csrc/pose_graph*.  The linear system is
dense and solved by numpy.linalg.solve; the device's band + Woodbury solve is compared with it, not derived from it.

Poses are 4x4 float64 matrices.  An edge is (from, to, Z) with Z the measurement from^-1 * to.
"""
import numpy as np

NUM_ADJACENT = 5     # num_adjacent_pose_cnstraints (graph_based_slam_component.cpp:40)
STOP_MAX_ITERATIONS, STOP_TRIALS, STOP_RHO_ZERO, STOP_LAMBDA = 0, 1, 2, 3


def q2R(w, v):
    x, y, z = v
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R2q_raw(R):
    """unit quaternion (w, x, y, z) of a rotation matrix; the sign is not fixed"""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1) * 2
        w = s / 4
        v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / s
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1 + R[i, i] - R[j, j] - R[k, k]) * 2
        v = np.zeros(3)
        v[i] = s / 4
        v[j] = (R[j, i] + R[i, j]) / s
        v[k] = (R[k, i] + R[i, k]) / s
        w = (R[k, j] - R[j, k]) / s
    q = np.array([w, *v])
    return q / np.linalg.norm(q)


def R2q(R):
    q = R2q_raw(R)
    return -q if q[0] < 0 else q


def qmul(a, b):
    w1, v1, w2, v2 = a[0], a[1:], b[0], b[1:]
    cx = np.array([v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]])
    return np.concatenate([[w1 * w2 - v1 @ v2], w1 * v2 + w2 * v1 + cx])


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def from_mqt(d):
    """fromVectorMQT: (dt, dq) -> 4x4; |dq|^2 > 1 gives the identity rotation"""
    d = np.asarray(d, np.float64)
    T = np.eye(4)
    T[:3, 3] = d[:3]
    w = 1.0 - d[3:] @ d[3:]
    if not w < 0:
        T[:3, :3] = q2R(np.sqrt(w), d[3:])
    return T


def to_mqt(T):
    return np.concatenate([T[:3, 3], R2q(T[:3, :3])[1:]])


def inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def oplus(X, d):
    return X @ from_mqt(d)


def error(Z, Xi, Xj):
    return to_mqt(inv(Z) @ inv(Xi) @ Xj)


def jacobians(Z, Xi, Xj):
    """-> (de/d delta_from, de/d delta_to), 6x6 each, exact at delta = 0"""
    Zi = inv(Z)
    A = inv(Xi) @ Xj
    E = Zi @ A
    qz, qa = R2q_raw(Zi[:3, :3]), R2q_raw(A[:3, :3])
    qe = qmul(qz, qa)
    s = 1.0 if qe[0] >= 0 else -1.0
    qe = s * qe
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Jj[:3, :3] = E[:3, :3]
    Jj[3:, 3:] = qe[0] * np.eye(3) + skew(qe[1:])
    Ji[:3, :3] = -Zi[:3, :3]
    Ji[:3, 3:] = 2 * Zi[:3, :3] @ skew(A[:3, 3])
    for a in range(3):
        u = np.zeros(4)
        u[1 + a] = 1
        Ji[3:, 3 + a] = -s * qmul(qmul(qz, u), qa)[1:]
    return Ji, Jj


def raw_product_w(Z, Xi, Xj):
    """w of q_z (x) q_a before the sign is fixed (the tests want an edge where it is negative)"""
    return float(qmul(R2q_raw(inv(Z)[:3, :3]), R2q_raw((inv(Xi) @ Xj)[:3, :3]))[0])


def numeric_jacobians(Z, Xi, Xj, h=1e-6):
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    for a in range(6):
        d = np.zeros(6)
        d[a] = h
        Ji[:, a] = (error(Z, oplus(Xi, d), Xj) - error(Z, oplus(Xi, -d), Xj)) / (2 * h)
        Jj[:, a] = (error(Z, Xi, oplus(Xj, d)) - error(Z, Xi, oplus(Xj, -d))) / (2 * h)
    return Ji, Jj


def chi2(X, edges):
    c = 0.0
    for i, j, Z in edges:
        e = error(Z, X[i], X[j])
        c += float(e @ e)
    return c


def build(X, edges):
    """H (vertex 0 removed), b = -sum J^T e, chi2"""
    N = len(X)
    H, b, c = np.zeros((6 * N, 6 * N)), np.zeros(6 * N), 0.0
    for i, j, Z in edges:
        e = error(Z, X[i], X[j])
        c += float(e @ e)
        Ji, Jj = jacobians(Z, X[i], X[j])
        for a, Ja in ((i, Ji), (j, Jj)):
            b[6 * a:6 * a + 6] -= Ja.T @ e
            for cc, Jc in ((i, Ji), (j, Jj)):
                H[6 * a:6 * a + 6, 6 * cc:6 * cc + 6] += Ja.T @ Jc
    return H[6:, 6:], b[6:], c


def adjacent_edges(poses, k=NUM_ADJACENT):
    """the odometry edges of graph_based_slam_component.cpp:289-303, in its order: for i > k (strictly), j = 0 .. k-1:
    (i - k + j -> i) measured from the incoming poses"""
    out = []
    for i in range(len(poses)):
        if i > k:
            for j in range(k):
                out.append((i - k + j, i, inv(poses[i - k + j]) @ poses[i]))
    return out


def optimize(poses, edges, max_iterations=10, history=None):
    """-> (poses, trace, result); trace: one dict per iteration (trials, chi2, lam, rho, and per trial rhos: the gain ratio, gains:
    (cur - tmp) / cur, the relative change of chi2 whose sign decides accept or reject).
    history: a list that receives the accepted poses after every iteration."""
    X = [np.array(x, np.float64) for x in poses]
    N = len(X)
    result = dict(iterations=0, trials=0, chi2_before=chi2(X, edges), chi2_after=None, lam=0.0, stop=STOP_MAX_ITERATIONS)
    trace = []
    if N < 2 or not edges:
        result["chi2_after"] = result["chi2_before"]
        return X, trace, result
    lam, nu = 0.0, 2.0
    for it in range(max_iterations):
        H, b, cur = build(X, edges)
        if it == 0:
            lam, nu = 1e-5 * float(np.max(np.diag(H))), 2.0
        q, rho, rhos, gains = 0, 0.0, [], []
        while True:
            try:
                x = np.linalg.solve(H + lam * np.eye(len(b)), b)
                Xn = [X[0]] + [oplus(X[v], x[6 * (v - 1):6 * v]) for v in range(1, N)]
                tmp = chi2(Xn, edges)
            except np.linalg.LinAlgError:
                x, Xn, tmp = np.zeros(len(b)), X, np.finfo(np.float64).max
            rho = (cur - tmp) / (float(x @ (lam * x + b)) + 1e-3)
            rhos.append(rho)
            gains.append((cur - tmp) / cur if cur > 0 else 0.0)
            if rho > 0 and np.isfinite(tmp):
                lam *= max(1.0 / 3.0, min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0))
                nu, cur, X = 2.0, tmp, Xn
            else:
                lam *= nu
                nu *= 2.0
            q += 1
            if not (rho < 0 and q < 10):
                break
        trace.append(dict(trials=q, chi2=cur, lam=lam, rho=rho, rhos=rhos, gains=gains))
        if history is not None:
            history.append([x.copy() for x in X])
        result["iterations"] += 1
        result["trials"] += q
        if q == 10 or rho == 0 or not np.isfinite(lam):
            result["stop"] = STOP_TRIALS if q == 10 else (STOP_RHO_ZERO if rho == 0 else STOP_LAMBDA)
            break
    result["chi2_after"] = trace[-1]["chi2"] if trace else result["chi2_before"]
    result["lam"] = lam
    return X, trace, result
