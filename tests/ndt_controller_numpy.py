"""TEST INFRASTRUCTURE: the NDT controller (Newton step + More-Thuente line search) apart from the derivative pass.

Three pieces:

* `run_oracle`: the ORACLE's own loop (oracle.ndt_align(deriv_cb=...), ndt_oracle.cpp DerivCb) driven by a Python callback that evaluates a
  synthetic objective and logs every call.  The reference trajectory of a case is this log, not anything computed here.
* `rows_from_log`: the log as the rows lsr_debug_ndt_controller_replay takes (the sums of one derivative pass each).
* `replay`: a plain float64 restatement of the same loop, written from ndt_oracle.cpp / linalg.h (std::min / std::max, svd6_solve), that
  consumes the rows.  It yields what the oracle does not expose (the interval, a_t of every trial, dir), one expected trace row per
  consumed row, names the branch every step took and records how close every deciding comparison was.  test_ndt_controller_cpu.py holds it
  to the oracle's logged poses bit for bit.

Row mapping.  One row per mode-3/1/0 call.  A mode-2 call (computeHessian after trial steps) is a row of its own, consumed by the
device in PH_MT_HESS, except after the tenth trial of a search, where its Hessian joins that trial's row (PH_MT_LAST, the fused pass).
What the device must not read is NaN: H on gradient-only rows, score and gradient on mode-2 rows."""
import ctypes as C
import numpy as np

F = np.float64
NAN = F(np.nan)
PH_INIT, PH_MT_FIRST, PH_MT_TRIAL, PH_MT_HESS, PH_DIAG, PH_MT_LAST = 0, 1, 2, 3, 4, 5
MU, NU = F(1.0e-4), F(0.9)
MAX_STEP_ITERATIONS = 10
EPS = 2.220446049250313e-16

# the trace row of lsr_debug_ndt_controller_replay (include/lidarslam_reg.h)
INT_FIELDS = ["phase", "want_hessian", "request", "done", "converged", "nr_iterations", "n_evals", "n_passes", "step_iterations",
              "open_interval", "interval_converged"]
TRACE_FIELDS = INT_FIELDS + ["a_t", "a_l", "f_l", "g_l", "a_u", "f_u", "g_u", "phi_0", "d_phi_0"] + \
    ["p%d" % i for i in range(6)] + ["x_t%d" % i for i in range(6)] + ["dir%d" % i for i in range(6)] + ["score"] + \
    ["g%d" % i for i in range(6)] + ["trans_probability", "last_pairs"]
TRACE_WIDTH = len(TRACE_FIELDS)   # 47
COL = {n: i for i, n in enumerate(TRACE_FIELDS)}

IU = np.triu_indices(6)


def upper21(H):
    return np.asarray(H, F)[IU]


def full_from_upper(u):
    H = np.zeros((6, 6))
    H[IU] = u
    return H + np.triu(H, 1).T


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle under a Python callback
# ---------------------------------------------------------------------------------------------------------------------------
_CB = C.CFUNCTYPE(C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_double),
                  C.POINTER(C.c_double))


class _NoGrid:
    """oracle.ndt_align wants a grid; under a derivative callback the loop never looks at it."""
    h = None
    leaf = 1.0


def run_oracle(O, objective, p_start, step_size, trans_eps, max_iterations, n_points):
    """objective(p or None, mode) -> (score, grad[6], H[6,6] or None).  Returns (log, result): log = one dict per callback call
    {mode, p (None for mode 2), score, grad, hess}."""
    log = []

    def cb(user, p, T16, mode, grad, hess):
        pv = None if not p else np.array([p[i] for i in range(6)], F)
        score, g, H = objective(pv, mode)
        if mode != 2:
            for i in range(6):
                grad[i] = g[i]
        if mode != 0:
            Hf = np.asarray(H, F).reshape(36)
            for i in range(36):
                hess[i] = Hf[i]
        log.append(dict(mode=int(mode), p=pv, score=F(score), grad=None if g is None else np.array(g, F),
                        hess=None if (H is None or mode == 0) else np.array(H, F).reshape(6, 6)))
        return float(score)

    fn = _CB(cb)
    guess = O.pose_to_matrix(np.asarray(p_start, F))
    src = np.zeros((n_points, 3), np.float32)
    res = O.ndt_align(_NoGrid(), src, guess, resolution=1.0, step_size=step_size, trans_eps=trans_eps, max_iterations=max_iterations,
                      trace=True, deriv_cb=(C.cast(fn, C.c_void_p).value, None))
    return log, res


def rows_from_log(log):
    """(rows [n, 29], kinds [n]): kinds = the phase in which the device consumes the row."""
    rows, kinds = [], []
    trials = 0
    for k, e in enumerate(log):
        mode = e["mode"]
        if mode == 2:
            if trials == MAX_STEP_ITERATIONS:   # the fused pass: the Hessian rides on the tenth trial's row
                rows[-1][8:29] = upper21(e["hess"])
                kinds[-1] = PH_MT_LAST
                continue
            r = np.full(29, np.nan)
            r[8:29] = upper21(e["hess"])
            kinds.append(PH_MT_HESS)
        else:
            r = np.full(29, np.nan)
            r[0] = e["score"]
            r[1:7] = e["grad"]
            if mode in (3, 1):
                r[8:29] = upper21(e["hess"])
                trials = 0
                kinds.append(PH_INIT if mode == 3 else PH_MT_FIRST)
            else:
                trials += 1
                kinds.append(PH_MT_TRIAL)
        r[7] = 100.0 + len(rows)   # the pair count: any number, a different one per row
        rows.append(r)
    return np.array(rows), kinds


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
class Arith:
    """Division and square root of the restatement: IEEE, or pushed one ulp up or down at random (rng given)."""

    def __init__(self, rng=None):
        self.rng = rng

    def _nudge(self, r):
        if self.rng is None or not np.isfinite(r) or r == 0:
            return r
        k = int(self.rng.integers(0, 3))
        return r if k == 0 else np.nextafter(r, F(np.inf) if k == 1 else F(-np.inf))

    def div(self, a, b):
        return self._nudge(F(a) / F(b))

    def sqrt(self, x):
        return self._nudge(np.sqrt(F(x)))


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


def svd6_solve(H, b):
    """oracle/linalg.h svd6_solve, operation for operation (one-sided Jacobi, singular values <= 6 eps s_max are zero)."""
    n = 6
    U = [[F(H[i][j]) for j in range(n)] for i in range(n)]
    V = [[F(1.0) if i == j else F(0.0) for j in range(n)] for i in range(n)]
    for _sweep in range(60):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                alpha = beta = gamma = F(0.0)
                for k in range(n):
                    alpha = alpha + U[k][p] * U[k][p]
                    beta = beta + U[k][q] * U[k][q]
                    gamma = gamma + U[k][p] * U[k][q]
                if gamma == 0.0:
                    continue
                if abs(gamma) <= F(1e-15) * np.sqrt(alpha * beta):
                    continue
                rotated = True
                zeta = (beta - alpha) / (F(2.0) * gamma)
                t = (F(1.0) if zeta >= 0 else F(-1.0)) / (abs(zeta) + np.sqrt(F(1.0) + zeta * zeta))
                c = F(1.0) / np.sqrt(F(1.0) + t * t)
                s = c * t
                for k in range(n):
                    up, uq = U[k][p], U[k][q]
                    U[k][p] = c * up - s * uq
                    U[k][q] = s * up + c * uq
                    vp, vq = V[k][p], V[k][q]
                    V[k][p] = c * vp - s * vq
                    V[k][q] = s * vp + c * vq
        if not rotated:
            break
    sv, smax = [], F(0.0)
    for j in range(n):
        s = F(0.0)
        for k in range(n):
            s = s + U[k][j] * U[k][j]
        sv.append(np.sqrt(s))
        smax = std_max(smax, sv[j])
    thr = F(6.0) * F(EPS) * smax
    y = []
    for j in range(n):
        if sv[j] > thr and sv[j] > 0:
            d = F(0.0)
            for k in range(n):
                d = d + U[k][j] * F(b[k])
            y.append(d / (sv[j] * sv[j]))
        else:
            y.append(F(0.0))
    x = []
    for i in range(n):
        s = F(0.0)
        for j in range(n):
            s = s + V[i][j] * y[j]
        x.append(s)
    return np.array(x, F)


def longdouble_solve(H, b):
    """Gaussian elimination with partial pivoting in numpy.longdouble; None when a pivot vanishes."""
    A = np.array(H, np.longdouble)
    x = np.array(b, np.longdouble)
    n = len(x)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if not (np.abs(A[piv, k]) > 0):
            return None
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            x[[k, piv]] = x[[piv, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]
            x[i] -= f * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - np.dot(A[k, k + 1:], x[k + 1:])) / A[k, k]
    return x


class Replay:
    """What `replay` returns: trace [n_used, 47] (expected trace rows of the device), branches (set of names), per_row (the branch
    names row by row), margins (list of (name, relative margin) of every deciding comparison that is not an exact tie), poses (x_t of
    every evaluation the rows stand for, in the order of the oracle's callback calls), solves (the (H, g, delta) of every Newton
    solve), and the result fields converged / iterations / p / trans_probability / n_evals."""


def replay(rows, p_start, step_size, trans_eps, max_iterations, n_points, rng=None):
    with np.errstate(all="ignore"):
        return _replay(np.asarray(rows, F), np.asarray(p_start, F), F(step_size), F(trans_eps), int(max_iterations), int(n_points), rng)


def _replay(rows, p_start, step_max, eps, max_iter, n_points, rng):
    ar = Arith(rng)
    out = Replay()
    out.branches, out.per_row, out.margins, out.poses, out.solves = set(), [], [], [], []
    trace = []
    st = dict(phase=PH_INIT, want_hessian=1, request=0, done=0, converged=0, nr_iterations=0, n_evals=0, n_passes=0, step_iterations=0,
              open_interval=0, interval_converged=0, a_t=F(0), a_l=F(0), f_l=F(0), g_l=F(0), a_u=F(0), f_u=F(0), g_u=F(0), phi_0=F(0),
              d_phi_0=F(0), p=p_start.copy(), x_t=p_start.copy(), dir=np.zeros(6), score=F(0), g=np.zeros(6), trans_probability=F(0),
              last_pairs=F(0))
    step_min = eps / F(2)
    cursor = [0]
    row_tags = []

    def tag(name):
        out.branches.add(name)
        row_tags.append(name)

    def margin(name, lhs, rhs, scale=None, tie_ok=False):
        """record how far apart the two sides of a deciding comparison are, relative to `scale` (default: the larger side)"""
        lhs, rhs = F(lhs), F(rhs)
        if not (np.isfinite(lhs) and np.isfinite(rhs)):
            return   # NaN / inf operands compare the same way everywhere
        if lhs == rhs and tie_ok:
            return
        s = max(abs(lhs), abs(rhs)) if scale is None else F(scale)
        out.margins.append((name, float(abs(lhs - rhs) / s) if s > 0 else 0.0))

    def snapshot():
        """the trace row after the row just consumed"""
        t = np.zeros(TRACE_WIDTH)
        for k, n in enumerate(INT_FIELDS):
            t[k] = st[n]
        for n in ("a_t", "a_l", "f_l", "g_l", "a_u", "f_u", "g_u", "phi_0", "d_phi_0", "score", "trans_probability", "last_pairs"):
            t[COL[n]] = st[n]
        for i in range(6):
            t[COL["p%d" % i]] = st["p"][i]
            t[COL["x_t%d" % i]] = st["x_t"][i]
            t[COL["dir%d" % i]] = st["dir"][i]
            t[COL["g%d" % i]] = st["g"][i]
        trace.append(t)
        out.per_row.append(list(row_tags))
        del row_tags[:]
        st["request"] = 0

    def request(phase):
        st["phase"] = phase
        st["want_hessian"] = {PH_MT_FIRST: 1, PH_MT_TRIAL: 0, PH_MT_LAST: 2, PH_MT_HESS: 1}[phase]
        st["request"] = {PH_MT_FIRST: 3, PH_MT_TRIAL: 1, PH_MT_LAST: 1, PH_MT_HESS: 0}[phase]
        snapshot()

    def take(with_score, with_hessian, evals=1):
        """the next row = the next derivative evaluation; only what the evaluation delivers is read"""
        if cursor[0] >= len(rows):
            raise IndexError("the rows ran out before the controller finished")
        r = rows[cursor[0]]
        cursor[0] += 1
        st["n_evals"] += evals
        st["n_passes"] += 1
        st["last_pairs"] = r[7]
        if with_score:
            st["score"] = r[0]
            st["g"] = r[1:7].copy()
            out.poses.append(st["x_t"].copy())
        else:
            out.poses.append(None)
        return full_from_upper(r[8:29]) if with_hessian else None

    def finish(converged):
        st["converged"] = converged
        st["trans_probability"] = st["score"] / F(n_points)
        st["done"] = 1
        snapshot()

    def trial_value(a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t):
        margin("tv:f_t>f_l", f_t, f_l, scale=abs(st["phi_0"]) + abs(f_t) + abs(f_l), tie_ok=True)   # a tie: f_l is a copy of f_t
        if f_t > f_l:
            z = ar.div(F(3) * (f_t - f_l), a_t - a_l) - g_t - g_l
            w = ar.sqrt(z * z - g_t * g_l)
            a_c = a_l + ar.div((a_t - a_l) * (w - g_l - z), g_t - g_l + F(2) * w)
            a_q = a_l - ar.div(F(0.5) * (a_l - a_t) * g_l, g_l - ar.div(f_l - f_t, a_l - a_t))
            margin("tv1:|a_c-a_l|<|a_q-a_l|", abs(a_c - a_l), abs(a_q - a_l))
            if abs(a_c - a_l) < abs(a_q - a_l):
                tag("tv1_cubic")
                return a_c
            tag("tv1_average_nan" if np.isnan(a_c) else "tv1_average")
            return F(0.5) * (a_q + a_c)
        margin("tv:g_t*g_l<0", min(abs(g_t), abs(g_l)), 0.0, scale=max(abs(g_t), abs(g_l), abs(st["d_phi_0"])), tie_ok=True)
        if g_t * g_l < 0:
            z = ar.div(F(3) * (f_t - f_l), a_t - a_l) - g_t - g_l
            w = ar.sqrt(z * z - g_t * g_l)
            a_c = a_l + ar.div((a_t - a_l) * (w - g_l - z), g_t - g_l + F(2) * w)
            a_s = a_l - ar.div(a_l - a_t, g_l - g_t) * g_l
            margin("tv2:|a_c-a_t|>=|a_s-a_t|", abs(a_c - a_t), abs(a_s - a_t))
            if abs(a_c - a_t) >= abs(a_s - a_t):
                tag("tv2_cubic")
                return a_c
            tag("tv2_secant")
            return a_s
        margin("tv:|g_t|<=|g_l|", abs(g_t), abs(g_l), tie_ok=True)
        if abs(g_t) <= abs(g_l):
            z = ar.div(F(3) * (f_t - f_l), a_t - a_l) - g_t - g_l
            w = ar.sqrt(z * z - g_t * g_l)
            a_c = a_l + ar.div((a_t - a_l) * (w - g_l - z), g_t - g_l + F(2) * w)
            a_s = a_l - ar.div(a_l - a_t, g_l - g_t) * g_l
            a_n = a_c if abs(a_c - a_t) < abs(a_s - a_t) else a_s
            if np.isfinite(a_c) and np.isfinite(a_s):
                margin("tv3:|a_c-a_t|<|a_s-a_t|", abs(a_c - a_t), abs(a_s - a_t))
                tag("tv3_proper")
            else:
                tag("tv3_degenerate")   # a_t == a_l: 0/0, the interpolants are NaN
            lim = a_t + F(0.66) * (a_u - a_t)
            margin("tv3:a_t>a_l", a_t, a_l, tie_ok=True)
            if a_t > a_l:
                return std_min(lim, a_n)
            return std_max(lim, a_n)
        tag("tv4_nan" if not (np.isfinite(g_t) and np.isfinite(f_t)) else "tv4_proper")
        z = ar.div(F(3) * (f_t - f_u), a_t - a_u) - g_t - g_u
        w = ar.sqrt(z * z - g_t * g_u)
        return a_u + ar.div((a_t - a_u) * (w - g_u - z), g_t - g_u + F(2) * w)

    def update_interval(a_t, f_t, g_t):
        margin("ui:f_t>f_l", f_t, st["f_l"], scale=abs(st["phi_0"]) + abs(f_t) + abs(st["f_l"]))
        if f_t > st["f_l"]:
            tag("ui_upper")
            st["a_u"], st["f_u"], st["g_u"] = a_t, f_t, g_t
            return False
        v = g_t * (st["a_l"] - a_t)
        margin("ui:g_t*(a_l-a_t)", abs(g_t), 0.0, scale=max(abs(g_t), abs(st["d_phi_0"])), tie_ok=True)
        margin("ui:a_l-a_t", st["a_l"], a_t, tie_ok=True)
        if v > 0:
            tag("ui_lower")
            st["a_l"], st["f_l"], st["g_l"] = a_t, f_t, g_t
            return False
        if v < 0:
            tag("ui_swap")
            st["a_u"], st["f_u"], st["g_u"] = st["a_l"], st["f_l"], st["g_l"]
            st["a_l"], st["f_l"], st["g_l"] = a_t, f_t, g_t
            return False
        tag("ui_converged")
        return True

    def dphi(direction):
        d = F(0)
        for i in range(6):
            d = d + st["g"][i] * direction[i]
        return -d

    def line_search(nrm):
        """compute_step_length_mt; returns (a_t, hess) with hess = the Hessian the next Newton step uses"""
        direction = st["dir"]
        phi_0 = -st["score"]
        d_phi_0 = dphi(direction)
        st["phi_0"] = phi_0
        gsc = F(sum(abs(st["g"][i] * direction[i]) for i in range(6)))
        margin("ls:d_phi_0>=0", d_phi_0, 0.0, scale=gsc, tie_ok=True)
        if d_phi_0 >= 0:
            if d_phi_0 == 0:
                tag("zero_slope")
                st["d_phi_0"] = d_phi_0
                st["a_t"] = F(0)
                return F(0), None
            tag("reversed")
            d_phi_0 = -d_phi_0
            direction = -direction
            st["dir"] = direction
        margin("ls:nrm<step_max", nrm, step_max, tie_ok=True)
        margin("ls:nrm>step_min", nrm, step_min, tie_ok=True)
        a_t = std_max(std_min(nrm, step_max), step_min)
        if nrm > step_max:
            tag("first_clamped_down")
        elif nrm < step_min:
            tag("first_clamped_up")
        st["d_phi_0"] = d_phi_0
        st["a_l"] = st["a_u"] = st["f_l"] = st["f_u"] = F(0)
        st["g_l"] = st["g_u"] = d_phi_0 - MU * d_phi_0
        st["interval_converged"] = 1 if (step_max - step_min) < 0 else 0
        st["open_interval"] = 1
        st["step_iterations"] = 0
        st["a_t"] = a_t
        st["x_t"] = st["p"] + direction * a_t
        request(PH_MT_FIRST)
        hess = take(True, True)
        while True:
            phi_t = -st["score"]
            d_phi_t = dphi(direction)
            psi_t = phi_t - phi_0 - MU * d_phi_0 * a_t
            d_psi_t = d_phi_t - MU * d_phi_0
            fsc = abs(phi_t) + abs(phi_0) + abs(MU * d_phi_0 * a_t)
            gsc = F(sum(abs(st["g"][i] * direction[i]) for i in range(6))) + abs(d_phi_0)
            if st["step_iterations"] > 0:   # bookkeeping of a trial
                margin("ls:close psi_t<=0", psi_t, 0.0, scale=fsc)
                margin("ls:close d_psi_t>=0", d_psi_t, 0.0, scale=gsc)
                if st["open_interval"] and (psi_t <= 0 and d_psi_t >= 0):
                    tag("interval_closed")
                    st["open_interval"] = 0
                    st["f_l"] = st["f_l"] + phi_0 - MU * d_phi_0 * st["a_l"]
                    st["g_l"] = st["g_l"] + MU * d_phi_0
                    st["f_u"] = st["f_u"] + phi_0 - MU * d_phi_0 * st["a_u"]
                    st["g_u"] = st["g_u"] + MU * d_phi_0
                if st["open_interval"]:
                    st["interval_converged"] = 1 if update_interval(a_t, psi_t, d_psi_t) else 0
                else:
                    st["interval_converged"] = 1 if update_interval(a_t, phi_t, d_phi_t) else 0
            margin("ls:psi_t<=0", psi_t, 0.0, scale=fsc)
            margin("ls:d_phi_t<=-nu*d_phi_0", d_phi_t, -NU * d_phi_0, scale=gsc)
            if st["interval_converged"] or st["step_iterations"] >= MAX_STEP_ITERATIONS or (psi_t <= 0 and d_phi_t <= -NU * d_phi_0):
                break
            if st["open_interval"]:
                a_new = trial_value(st["a_l"], st["f_l"], st["g_l"], st["a_u"], st["f_u"], st["g_u"], a_t, psi_t, d_psi_t)
            else:
                a_new = trial_value(st["a_l"], st["f_l"], st["g_l"], st["a_u"], st["f_u"], st["g_u"], a_t, phi_t, d_phi_t)
            margin("ls:trial<step_max", a_new, step_max, tie_ok=True)
            margin("ls:trial>step_min", a_new, step_min, tie_ok=True)
            a_t = std_max(std_min(a_new, step_max), step_min)
            if np.isnan(a_t):
                tag("trial_nan")
            elif a_new > step_max:
                tag("trial_clamped_down")
            elif a_new < step_min:
                tag("trial_clamped_up")
            st["a_t"] = a_t
            st["x_t"] = st["p"] + direction * a_t
            last = st["step_iterations"] + 1 >= MAX_STEP_ITERATIONS
            request(PH_MT_LAST if last else PH_MT_TRIAL)
            h_last = take(True, last, evals=2 if last else 1)
            st["step_iterations"] += 1
            if last:
                hess = h_last
        if st["step_iterations"] >= MAX_STEP_ITERATIONS:
            tag("cap_ten_trials")
            out.poses.append(None)   # the oracle's computeHessian call, fused into the tenth trial's row
        elif st["step_iterations"]:
            tag("exit_after_trials")
            request(PH_MT_HESS)
            hess = take(False, True)
        else:
            tag("exit_first_evaluation")
        return a_t, hess

    hess = take(True, True)
    while True:
        delta = svd6_solve(hess, -st["g"])
        out.solves.append((hess.copy(), st["g"].copy(), delta.copy()))
        if rng is not None:
            delta = np.array([ar._nudge(d) for d in delta], F)
        nrm = F(0)
        for i in range(6):
            nrm = nrm + delta[i] * delta[i]
        nrm = ar.sqrt(nrm)
        if nrm == 0 or nrm != nrm:
            tag("newton_zero_step" if nrm == 0 else "newton_nan_step")
            finish(1 if nrm == nrm else 0)
            break
        st["dir"] = np.array([ar.div(delta[i], nrm) for i in range(6)], F)
        a_t, h_new = line_search(nrm)
        if h_new is not None:
            hess = h_new
        st["p"] = st["p"] + st["dir"] * a_t
        nr = st["nr_iterations"]
        margin("newton:|a_t|<eps", abs(a_t), eps)
        done = nr > max_iter or (nr and abs(a_t) < eps)
        if nr == 0 and abs(a_t) < eps:
            tag("small_step_at_iteration_0")
        st["nr_iterations"] = nr + 1
        if done:
            tag("end_by_max_iterations" if nr > max_iter else "end_by_trans_eps")
            finish(1)
            break
    out.trace = np.array(trace)
    out.n_used = cursor[0]
    out.converged, out.iterations = st["converged"], st["nr_iterations"]
    out.p, out.trans_probability, out.n_evals = st["p"].copy(), st["trans_probability"], st["n_evals"]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# comparing traces
# ---------------------------------------------------------------------------------------------------------------------------
def _groups(ref_row, step_min):
    """(name, columns, scale) of the compared float fields of one trace row"""
    c = COL
    gnorm = float(np.sqrt(np.nansum(ref_row[c["g0"]:c["g0"] + 6] ** 2)))
    phi0 = abs(ref_row[c["phi_0"]])
    vec = lambda n: list(range(c[n + "0"], c[n + "0"] + 6))   # noqa: E731
    amax = lambda cols, floor: max([abs(float(v)) for v in ref_row[cols] if v == v] + [floor])   # noqa: E731
    return [("a", [c["a_t"], c["a_l"], c["a_u"]], amax([c["a_t"], c["a_l"], c["a_u"]], float(step_min))),
            ("f", [c["f_l"], c["f_u"]], amax([c["f_l"], c["f_u"]], phi0)),
            ("g", [c["g_l"], c["g_u"], c["d_phi_0"]], amax([c["g_l"], c["g_u"], c["d_phi_0"]], gnorm)),
            ("phi_0", [c["phi_0"]], phi0),
            ("dir", vec("dir"), 1.0),
            ("x_t", vec("x_t"), amax(vec("x_t"), float(step_min))),
            ("p", vec("p"), amax(vec("p"), float(step_min))),
            ("trans_probability", [c["trans_probability"]], abs(ref_row[c["trans_probability"]]))]


def trace_deviation(got, ref, step_min):
    """largest deviation of the compared float fields of `got` from `ref`, relative to the field's scale; a NaN on one side only is inf"""
    worst = 0.0
    for r in range(len(ref)):
        for _name, cols, scale in _groups(ref[r], step_min):
            a, b = got[r][cols], ref[r][cols]
            if np.any(np.isnan(a) != np.isnan(b)):
                return float("inf")
            ok = ~np.isnan(b)
            if not np.any(ok):
                continue
            inf_differs = np.isinf(a[ok]) | np.isinf(b[ok])
            if np.any(inf_differs):
                if not np.array_equal(a[ok][inf_differs], b[ok][inf_differs]):
                    return float("inf")
            d = np.abs(a[ok][~inf_differs] - b[ok][~inf_differs])
            if d.size and scale > 0:
                worst = max(worst, float(d.max() / scale))
            elif d.size and d.max() > 0:
                return float("inf")
    return worst


EXACT_COLS = list(range(len(INT_FIELDS))) + [COL["score"], COL["last_pairs"]] + [COL["g%d" % i] for i in range(6)]


def solve_gap(solves):
    """largest gap between svd6_solve and a longdouble elimination over the Newton solves of a case, relative to |delta|_inf"""
    worst = 0.0
    for H, g, delta in solves:
        if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g)) and np.all(np.isfinite(delta))):
            continue
        sv = np.linalg.svd(H, compute_uv=False)
        if sv.min() <= 6 * EPS * sv.max():
            continue   # the reference drops a direction there: no plain solve to compare with
        x = longdouble_solve(H, -g)
        if x is None:
            continue
        scale = float(np.max(np.abs(delta)))
        if scale > 0:
            worst = max(worst, float(np.max(np.abs(np.asarray(x - delta.astype(np.longdouble), np.float64))) / scale))
    return worst


ULP64 = 64 * EPS


def measure_bar(rows, base, p_start, step_size, trans_eps, max_iterations, n_points, seeds=32):
    """(bar, branches_stable): 8 x the larger of the one-ulp perturbation's deviation and the solve gap, never below 64 ulp; whether
    every perturbed run took the branches of the unperturbed one, row by row."""
    dev, stable = 0.0, True
    for seed in range(seeds):
        try:
            r = replay(rows, p_start, step_size, trans_eps, max_iterations, n_points, rng=np.random.default_rng(1000 + seed))
        except IndexError:   # took another way and asked for more rows than the case has
            stable = False
            continue
        if r.per_row != base.per_row or r.n_used != base.n_used or not np.array_equal(r.trace[:, :len(INT_FIELDS)], base.trace[:, :len(INT_FIELDS)]):
            stable = False
            continue
        dev = max(dev, trace_deviation(r.trace, base.trace, trans_eps / 2))
    return max(8 * max(dev, solve_gap(base.solves)), ULP64), stable


# ---------------------------------------------------------------------------------------------------------------------------
# the 6x6 solve and the fast division / square root
# ---------------------------------------------------------------------------------------------------------------------------
def gauss_jordan6(H, g, details=False):
    """The device's elimination (csrc/ndt.hip solve6_wave) in float64 without fused multiply-adds: Gauss-Jordan with partial pivoting on
    [H | -g]; a column whose pivot (at most 6 eps max|H_ij|) is dropped leaves its unknown 0.  details: also the dropped columns and `order`,
    order[k] = the equation (row of H) that ended in position k; the equations in the positions of the kept columns are the ones solved."""
    A = np.zeros((6, 7))
    A[:, :6] = H
    A[:, 6] = -np.asarray(g, F)
    with np.errstate(all="ignore"):
        scale = np.nanmax(np.abs(A[:, :6])) if np.any(~np.isnan(A[:, :6])) else 0.0
        dropped, order = [], list(range(6))
        for k in range(6):
            best, piv = abs(A[k, k]), k
            for i in range(k + 1, 6):
                if abs(A[i, k]) > best:
                    best, piv = abs(A[i, k]), i
            if best <= 6 * EPS * scale:
                dropped.append(k)
                continue
            A[[k, piv]] = A[[piv, k]]
            order[k], order[piv] = order[piv], order[k]
            for r in range(6):
                if r != k:
                    A[r] = A[r] - (A[r, k] * (1.0 / A[k, k])) * A[k]
        x = np.array([0.0 if k in dropped else A[k, 6] / A[k, k] for k in range(6)])
        return (x, dropped, order) if details else x


def reference_solve6(H, g):
    """-H^+ g in numpy.longdouble: elimination where H is regular; where it is singular, the minimum-norm least-squares answer with the
    singular values at or below 6 eps s_max dropped (the contract of JacobiSVD::solve).  None where H or g is not finite."""
    H, g = np.asarray(H, F), np.asarray(g, F)
    if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g))):
        return None
    sv = np.linalg.svd(H, compute_uv=False)
    if sv.max() > 0 and sv.min() > 6 * EPS * sv.max():
        return np.asarray(longdouble_solve(H, -g), np.longdouble)
    return np.asarray(np.linalg.lstsq(H, -g, rcond=6 * EPS)[0], np.longdouble)


def solve6_bar(H):
    """16 cond(H) 2^-53, cond over the singular values the reference keeps"""
    sv = np.linalg.svd(np.asarray(H, F), compute_uv=False)
    keep = sv[sv > 6 * EPS * sv.max()] if sv.max() > 0 else sv[:0]
    return 16.0 * (keep.max() / keep.min() if keep.size else 1.0) * 2.0 ** -53


def ulp_distance(a, b):
    """distance of two float64 arrays in units in the last place, counted in integers along the ordered bit patterns (so across zero,
    the denormals and up to the infinities; -0 and +0 are 0 apart); 0 for NaN against NaN, 2^64 - 1 for a NaN on one side only.
    Returns uint64."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    top = np.uint64(1) << np.uint64(63)

    def key(x):   # monotone in the value: negative patterns mirrored below 2^63, non-negative ones moved above it; -0 and +0 share 2^63
        u = x.view(np.uint64)
        return np.where(u >= top, top - (u - top), u + top)

    ka, kb = key(a), key(b)
    d = np.where(ka > kb, ka - kb, kb - ka)
    d = np.where(np.isnan(a) & np.isnan(b), np.uint64(0), d)
    return np.where(np.isnan(a) != np.isnan(b), np.uint64(2 ** 64 - 1), d)


def same_bits(a, b):
    """elementwise: the same float64 bit pattern, or NaN on both sides"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


MT_GUARD_LO, MT_GUARD_HI = 1e-290, 1e290


MT_GUARD_DIVIDEND = 1e18


def mt_div_takes_ieee_path(a, b):
    """the divisor outside (1e-290, 1e290) in magnitude, or the dividend at or above 1e18 (the fast quotient could overflow) or NaN"""
    a, b = np.abs(np.asarray(a, F)), np.abs(np.asarray(b, F))
    with np.errstate(invalid="ignore"):
        return ~((b > MT_GUARD_LO) & (b < MT_GUARD_HI) & (a < MT_GUARD_DIVIDEND))


def mt_sqrt_takes_ieee_path(x):
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        return ~((x > MT_GUARD_LO) & (x < MT_GUARD_HI))
