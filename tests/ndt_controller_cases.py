"""The cases of the NDT controller tests (test_ndt_controller_cpu.py, test_ndt_controller_gpu.py): synthetic objectives for the oracle's
Newton / More-Thuente loop (ndt_controller_numpy.run_oracle), 6 unknowns, at most 40 rows each.

Two families.

* SMOOTH: score(p) = -sum_i t_i(u_i), u = Q^T (p - c), Q a random orthogonal matrix, t_i one of: quadratic, quartic, 1 - cos, log cosh.
  The REPORTED Hessian is the true one times k: a Newton step that is too long (k < 1) or too short is what makes the search iterate.
  Everything about a case follows from its seed (smooth_case).
* SCRIPTED: the callback ignores the pose and returns listed (score, g_1, c) triples call by call: gradient g_1 e_1, Hessian -c I.  Along
  e_1 these are line profiles (phi, phi') = (-score, -g_1) that no smooth function need produce: NaN scores, slopes that jump.

What the structure of the loop makes unreachable (checked by test_reachability_of_case_3_and_4 with the restatement over random
scripted profiles).  After the first evaluation of a search a selection is always preceded by an update of the interval with the same
(a_t, f_t, g_t).  If the update moved a_l to a_t (its second and third outcome), the selection sees f_t == f_l and g_t == g_l: not case 1
(f_t > f_l), not case 2 (g_t g_l = g_t^2 is not negative), so case 3 with a_t == a_l, where 0/0 makes both interpolants NaN and the result
is a_t + 0.66 (a_u - a_t).  If the update moved a_u (first outcome), then f_t > f_l: case 1.  If the update found the interval converged,
no selection follows.  At the FIRST selection (no update before it) a_l = 0, f_l = 0, g_l = (1 - mu) phi'(0) < 0: cases 3 and 4 need
f_t <= f_l = 0, that is psi_t <= 0, and g_t g_l >= 0, that is psi'_t <= 0, hence phi'_t <= mu phi'(0) <= -nu phi'(0) — the sufficient
decrease and curvature test that ends the search before it selects.  So with finite operands neither the proper case 3 (a_t != a_l) nor
case 4 is reachable; case 3 is covered in its degenerate form and case 4 through a NaN score, which fails every comparison on the way.

Every case carries its bar: the relative deviation allowed between the device's trace and the restatement's (ndt_controller_numpy.
measure_bar: 8 x the larger of what a one-ulp perturbation of every division and square root does to the trace and of the gap between
svd6_solve and a longdouble elimination on the case's Hessians, never below 64 ulp = 1.42e-14).  test_ndt_controller_cpu.py measures
them again and holds the figures below to the measurement."""
import numpy as np

N_POINTS = 1000   # trans_probability = score / N_POINTS

KS = [0.2, 0.5, 1.0, 2.0, 5.0]
STEP_SIZES = [0.1, 1.0, 10.0]
TRANS_EPS = [0.01, 0.1]
MAX_ITERATIONS = [3, 35]
TERMS = ["quadratic", "quartic", "one_minus_cos", "log_cosh"]


def _term(kind, w, u):
    """(t, t', t'') of one separable term"""
    if kind == "quadratic":
        return 0.5 * w * u * u, w * u, w
    if kind == "quartic":
        return 0.25 * w * u ** 4, w * u ** 3, 3.0 * w * u * u
    if kind == "one_minus_cos":
        return w * (1.0 - np.cos(u)), w * np.sin(u), w * np.cos(u)
    return w * np.log(np.cosh(u)), w * np.tanh(u), w / np.cosh(u) ** 2


def smooth_case(seed):
    """dict(objective, p_start, step_size, trans_eps, max_iterations) of the smooth case `seed`"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    kinds = [TERMS[int(i)] for i in rng.integers(0, 4, 6)]
    w = 10.0 ** rng.uniform(-1.0, 2.0, 6)
    c = rng.standard_normal(6) * 0.3
    p_start = c + rng.standard_normal(6) * 10.0 ** rng.uniform(-2.0, 0.3)
    p_start[3:] = np.clip(p_start[3:], -1.2, 1.2)
    k = KS[int(rng.integers(0, len(KS)))]
    last = [np.zeros(6)]

    def objective(p, mode):
        if p is None:
            p = last[0]
        last[0] = p.copy()
        u = Q.T @ (p - c)
        t = [_term(kinds[i], w[i], u[i]) for i in range(6)]
        score = -float(sum(x[0] for x in t))
        grad = -(Q @ np.array([x[1] for x in t]))
        H = -k * ((Q * np.array([x[2] for x in t])) @ Q.T)
        return score, grad, 0.5 * (H + H.T)

    return dict(objective=objective, p_start=p_start, step_size=STEP_SIZES[int(rng.integers(0, 3))],
                trans_eps=TRANS_EPS[int(rng.integers(0, 2))], max_iterations=MAX_ITERATIONS[int(rng.integers(0, 2))])


def scripted_objective(entries, hessians=None):
    """entries: (score, g_1, c) per callback call; hessians: {call: 6x6} replaces -c I at that call.  Once the entries are used up
    the profile goes on downhill (score + 0.1 per call, slope 0.001): every further search accepts its first step, which is below
    trans_eps, and the align ends."""
    calls = [0]

    def objective(p, mode):
        k = calls[0]
        calls[0] += 1
        e = entries[min(k, len(entries) - 1)]
        score, g = e[0], e[1]
        if k >= len(entries):
            score, g = _last_finite_score(entries) + 0.1 * (k - len(entries) + 1), 0.001
        grad = np.array(g, float) if np.ndim(g) else np.array([g, 0, 0, 0, 0, 0], float)
        H = -float(e[2]) * np.eye(6)
        if hessians and k in hessians:
            H = np.array(hessians[k], float)
        return score, grad, H

    return objective


def _last_finite_score(entries):
    return [e[0] for e in entries if e[0] == e[0]][-1]


def random_scripted_entries(seed, n=14):
    """a random line profile: a first point with phi'(0) < 0, then values and slopes of either sign at a few scales"""
    rng = np.random.default_rng(seed)
    c = 10.0 ** rng.uniform(-1.0, 1.0)
    g1 = 10.0 ** rng.uniform(-1.0, 1.0)
    out = [(-10.0, g1, c)]
    for _ in range(n):
        phi = 10.0 + rng.standard_normal() * 10.0 ** rng.uniform(-3.0, 0.5)
        dphi = rng.standard_normal() * 10.0 ** rng.uniform(-2.0, 1.0)
        out.append((-phi, -dphi, c))
    return out


def scripted_case(entries, step_size, trans_eps, max_iterations, hessians=None):
    return dict(objective=scripted_objective(entries, hessians), p_start=np.array([0.5, -0.25, 0.125, 0.1, -0.2, 0.3]),
                step_size=step_size, trans_eps=trans_eps, max_iterations=max_iterations)


def random_scripted_case(seed):
    rng = np.random.default_rng(seed + 7)
    return scripted_case(random_scripted_entries(seed), STEP_SIZES[int(rng.integers(0, 3))], TRANS_EPS[int(rng.integers(0, 2))], 3)


NAN = float("nan")
_H_ZERO_SLOPE = np.diag([1.0, -1.0, -1.0, -1.0, -1.0, -1.0])
_H_NAN = -np.eye(6)
_H_NAN[0, 1] = _H_NAN[1, 0] = NAN

# name -> (builder, bar).  The bars are measured (module docstring); the smooth and random scripted cases were picked from 3000 and
# 10 000 draws so that every branch of the restatement is taken by at least two cases with every deciding comparison at least 1e-9
# (relative) away from a tie (test_ndt_controller_cpu.py holds the set to both).
HAND = {
    # g = (1,1,0,0,0,0), H = diag(1,-1,...): delta = (-1, 1, 0..), g . delta = 0 exactly: no search, converged at iteration 2, p unchanged
    "exact_zero_slope": (lambda: scripted_case([(-10.0, [1.0, 1.0, 0, 0, 0, 0], 1.0)], 0.1, 0.01, 35, {0: _H_ZERO_SLOPE}), 1.42e-14),
    "zero_gradient": (lambda: scripted_case([(-10.0, 0.0, 1.0)], 0.1, 0.01, 35), 1.42e-14),
    "nan_in_hessian": (lambda: scripted_case([(-10.0, 1.0, 1.0)], 0.1, 0.01, 35, {0: _H_NAN}), 1.42e-14),
    # the same endings a second time, at other sizes: g . delta = -8 + 8 (powers of two on purpose: the device fuses the multiply-adds
    # of g . dir, so the tie holds there when the products g_i dir_i are exact; with inexact ones the fused sum keeps the rounding
    # error of the first product, a slope of 1e-16 relative, where the reference's two rounded products cancel), a zero gradient at a scaled Hessian, a Hessian of NaN alone
    # (before the pivot rule was fixed the device took every NaN pivot for a vanishing one: a zero step, converged = 1)
    "exact_zero_slope_2": (lambda: scripted_case([(-4.0, [4.0, 0, 0, 0, 4.0, 0], 1.0)], 1.0, 0.1, 3,
                                                 {0: np.diag([2.0, -1.0, -1.0, -1.0, -2.0, -1.0])}), 1.42e-14),
    "zero_gradient_2": (lambda: scripted_case([(-3.0, 0.0, 250.0)], 10.0, 0.1, 3), 1.42e-14),
    "all_nan_hessian": (lambda: scripted_case([(-10.0, 1.0, 1.0)], 0.1, 0.01, 35, {0: np.full((6, 6), NAN)}), 1.42e-14),
    # iteration 0 steps a_t = 0.02 < trans_eps = 0.1 and is accepted at once: must go on (`nr_iterations &&`); iteration 1 ends it
    "small_step_at_iteration_0": (lambda: scripted_case([(-10.0, 0.02, 1.0), (-9.9, 0.01, 1.0), (-9.8, 0.005, 1.0)], 1.0, 0.1, 35),
                                  1.42e-14),
    # the same with a step above trans_eps at iteration 1: a third iteration
    "small_step_then_large": (lambda: scripted_case([(-10.0, 0.02, 1.0), (-9.9, 0.5, 1.0), (-9.8, 0.01, 1.0), (-9.7, 0.001, 1.0)],
                                                    1.0, 0.1, 35), 1.42e-14),
    # A NaN trial value from finite operands (max_iterations = 2).  The recipe "case 1 with a_t > a_l, both slopes positive and
    # z^2 < g_t g_l" is not reachable: g_l > 0 only after the update's third outcome, which leaves a_u < a_l and every later trial
    # between them, and with a_t < a_l, f_t > f_l and positive slopes z <= -(g_t + g_l), so z^2 > g_t g_l.  What the random scripted
    # profiles do reach is case 1 with a_t == a_l: two trials clamped to step_min where the profile returns a higher value the second
    # time; 3 (f_t - f_l) / 0 is inf, the cubic's 0 * inf is NaN and so is the average.  std::min / std::max keep the NaN and the
    # next pose is NaN.
    "nan_trial_value": (lambda: scripted_case([(-10.0, 0.8, 10.0), (-10.01, 0.2, 10.0), (-9.99, -1.0, 10.0), (-10.06, -0.02, 10.0),
                                               (-10.05, -0.03, 10.0), (-10.0, 0.05, 10.0), (-9.9, 0.01, 10.0)], 0.1, 0.1, 2), 1.42e-14),
    # a NaN score at the first evaluation: every comparison fails, the selection falls through to case 4
    "nan_score_case_4": (lambda: scripted_case([(-10.0, 2.0, 1.0), (NAN, 5.0, 1.0), (-10.2, 0.1, 1.0), (-10.3, 0.01, 1.0)],
                                               1.0, 0.01, 3), 1.42e-14),
    "nan_score_and_slope_case_4": (lambda: scripted_case([(-10.0, 2.0, 1.0), (NAN, NAN, 1.0), (-10.2, 0.1, 1.0), (-10.3, 0.01, 1.0)],
                                                         1.0, 0.01, 3), 1.42e-14),
}

SMOOTH = {1348: 8.57e-13, 1871: 3.14e-14, 303: 1.98e-13, 2759: 3.1e-12, 2275: 1.35e-13}

SCRIPTED_RANDOM = {2425: 1.42e-14, 5067: 1.42e-14}


# cases that are ABOUT an exact tie (g . delta == 0): a perturbed division breaks the tie by construction
EXACT_TIE_CASES = {"exact_zero_slope", "exact_zero_slope_2"}


def all_cases():
    """{name: (builder, bar)}"""
    out = dict(HAND)
    out.update({"smooth_%d" % s: ((lambda s=s: smooth_case(s)), bar) for s, bar in SMOOTH.items()})
    out.update({"scripted_%d" % s: ((lambda s=s: random_scripted_case(s)), bar)
                for s, bar in SCRIPTED_RANDOM.items()})
    return out


_built = {}


def build(name, O):
    """Run the oracle on a case once: dict(log, result, rows, kinds, p0, replay, bar, and the align parameters)."""
    if name in _built:
        return _built[name]
    from ndt_controller_numpy import replay, rows_from_log, run_oracle

    builder, bar = all_cases()[name]
    c = builder()
    log, res = run_oracle(O, c["objective"], c["p_start"], c["step_size"], c["trans_eps"], c["max_iterations"], N_POINTS)
    rows, kinds = rows_from_log(log)
    p0 = log[0]["p"]
    rp = replay(rows, p0, c["step_size"], c["trans_eps"], c["max_iterations"], N_POINTS)
    _built[name] = dict(name=name, log=log, result=res, rows=rows, kinds=kinds, p0=p0, replay=rp, bar=bar, step_size=c["step_size"],
                        trans_eps=c["trans_eps"], max_iterations=c["max_iterations"], n_points=N_POINTS)
    return _built[name]


# ---------------------------------------------------------------------------------------------------------------------------
# the systems of the 6x6 solve test and the operands of the division / square root test
# ---------------------------------------------------------------------------------------------------------------------------
def solve6_systems():
    """[(name, kind, H, g)]; kind: "regular" (compare with the longdouble elimination), "singular" (with the minimum-norm answer: the
    singular part is decoupled), "residual" (H delta = -g only), "bounded" (finding 2, rotated: residual and a bounded step), "nan"."""
    rng = np.random.default_rng(66)
    out = []

    def negdef():
        A = rng.standard_normal((6, 6))
        return -(A @ A.T + np.eye(6))

    for k in range(8):
        out.append(("negative_definite_%d" % k, "regular", negdef(), rng.standard_normal(6)))
    D = np.sqrt(np.array([1e2, 1e2, 1e2, 1e5, 1e5, 1e5]))
    for k in range(4):   # NDT-like scales: translation block 1e2, rotation block 1e5
        out.append(("ndt_scales_%d" % k, "regular", D[:, None] * negdef() * D[None, :], rng.standard_normal(6) * D))
    for k in range(2):   # zero leading pivots: rows must be swapped
        B = rng.standard_normal((3, 3)) + 3.0 * np.eye(3)
        H = np.zeros((6, 6))
        H[:3, 3:] = B
        H[3:, :3] = B.T
        out.append(("zero_leading_pivots_%d" % k, "regular", H, rng.standard_normal(6)))
    for k in (0, 3, 5):   # an exact zero row and column: that unknown is 0 (the minimum-norm answer), whatever g says there
        H = negdef()
        H[k, :] = 0.0
        H[:, k] = 0.0
        out.append(("zero_row_and_column_%d" % k, "singular", H, rng.standard_normal(6)))
    out.append(("all_zero", "singular", np.zeros((6, 6)), rng.standard_normal(6)))
    H = negdef()
    H[1, 4] = H[4, 1] = float("nan")
    out.append(("nan_entry", "nan", H, rng.standard_normal(6)))
    out.append(("all_nan", "nan", np.full((6, 6), float("nan")), np.full(6, float("nan"))))
    # finding 2: one direction unobserved to 1e-18 relative; the reference ignores it
    Hd = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 1e-18])
    out.append(("unobserved_direction", "singular", Hd, np.array([0.3, -0.2, 0.5, 0.1, -0.4, 0.25])))
    Q, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((6, 6)))
    Hr = Q @ Hd @ Q.T
    out.append(("unobserved_direction_rotated", "bounded", 0.5 * (Hr + Hr.T), np.array([0.3, -0.2, 0.5, 0.1, -0.4, 0.25])))
    # two identical rows (and columns): singular and consistent; the minimum-norm answer is not promised, H delta = -g is
    A = rng.standard_normal((5, 5))
    M = -(A @ A.T + np.eye(5))
    E = np.zeros((6, 5))
    E[0, 0] = E[1, 0] = 1.0
    for i in range(1, 5):
        E[i + 1, i] = 1.0
    H = E @ M @ E.T
    g = -(H @ rng.standard_normal(6))
    g[1] = g[0]
    out.append(("two_identical_rows", "residual", H, g))
    return out


def mt_operands():
    """(a, b), 4096 pairs: random over 600 binades, the guards at 1e-290 / 1e290 (and 1e18 for the dividend) and their neighbours, denormals, zeros, infinities, NaN,
    negative radicands"""
    rng = np.random.default_rng(4096)
    lo, hi = 1e-290, 1e290
    edge = [lo, np.nextafter(lo, 0.0), np.nextafter(lo, 1.0), hi, np.nextafter(hi, 0.0), np.nextafter(hi, np.inf),
            5e-324, 1e-310, 2.2250738585072014e-308, 1e18, np.nextafter(1e18, 0.0), np.nextafter(1e18, np.inf), -1e18, 1.7976931348623157e308, 0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.0, 1e-300,
            1e300, -lo, -hi, -np.nextafter(lo, 0.0), -np.nextafter(hi, np.inf), -5e-324, -2.0, 0.1]
    a = [x for x in edge for _ in edge]
    b = [y for _ in edge for y in edge]
    n = 4096 - len(a)
    sign = lambda: np.where(rng.random(n) < 0.25, -1.0, 1.0)   # noqa: E731
    a = np.concatenate([a, sign() * np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-300, 301, n))])
    b = np.concatenate([b, sign() * np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-300, 301, n))])
    return a.astype(np.float64), b.astype(np.float64)
