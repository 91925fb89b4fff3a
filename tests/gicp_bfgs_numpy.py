"""Plain nested-loop restatement of the BFGS inner optimiser of GICP — PCL's port of GSL vector_bfgs2 as
pclomp::GeneralizedIterativeClosestPoint drives it, after oracle/gicp_oracle.cpp (struct Bfgs and the solver == 0
branch of orc_gicp_align) — written for readability: the loops are loops, the wrapper caches f and df separately and sometimes asks
for f alone, exactly as the original.  What the flattened automaton of csrc/gicp_bfgs.hpp is held to (tests/test_gicp_bfgs_cpu.py):
both do the same IEEE operations in the same order (python floats are fp64, one rounding per operation).  Test infrastructure only.

`fn(x) -> (f, g)` is the cost; every call is logged in `calls` as (alpha, x): the automaton asks for the same points, once each."""
import math

RHO, SIGMA, TAU1, TAU2, TAU3, STEP = 0.01, 0.01, 9.0, 0.05, 0.5, 1.0
DBL_EPSILON = 2.220446049250313e-16
NAN = float("nan")
RUNNING, NO_PROGRESS, GRADIENT_TOL, MAX_INNER, NONFINITE = 0, 1, 2, 3, 4


class NonFinite(Exception):
    pass


def nrm(v):
    s = 0.0
    for a in v:
        s += a * a
    return math.sqrt(s)


def dot(a, b):
    s = 0.0
    for u, v in zip(a, b):
        s += u * v
    return s


def interp_quad(f0, fp0, f1, zl, zh):
    fl = f0 + zl * (fp0 + zl * (f1 - f0 - fp0))
    fh = f0 + zh * (fp0 + zh * (f1 - f0 - fp0))
    c = 2 * (f1 - f0 - fp0)
    zmin, fmin = zl, fl
    if fh < fmin:
        zmin, fmin = zh, fh
    if c > 0:
        z = -fp0 / c
        if zl < z < zh:
            f = f0 + z * (fp0 + z * (f1 - f0 - fp0))
            if f < fmin:
                zmin, fmin = z, f
    return zmin


def cubic(c0, c1, c2, c3, z):
    return c0 + z * (c1 + z * (c2 + z * c3))


def solve_quadratic(a, b, c):
    """-> the real roots in ascending order (a double root twice)"""
    if a == 0:
        return [] if b == 0 else [-c / b]
    disc = b * b - 4 * a * c
    if disc > 0:
        if b == 0:
            r = math.sqrt(-c / a)
            return [-r, r]
        sgnb = 1 if b > 0 else -1
        temp = -0.5 * (b + sgnb * math.sqrt(disc))
        r1, r2 = temp / a, c / temp
        return [r1, r2] if r1 < r2 else [r2, r1]
    if disc == 0:
        return [-0.5 * b / a, -0.5 * b / a]
    return []


def interp_cubic(f0, fp0, f1, fp1, zl, zh):
    eta = 3 * (f1 - f0) - 2 * fp0 - fp1
    xi = fp0 + fp1 - 2 * (f1 - f0)
    c0, c1, c2, c3 = f0, fp0, eta, xi
    zmin, fmin = zl, cubic(c0, c1, c2, c3, zl)
    candidates = [zh] + [z for z in solve_quadratic(3 * c3, 2 * c2, c1) if zl < z < zh]
    for z in candidates:
        y = cubic(c0, c1, c2, c3, z)
        if y < fmin:
            zmin, fmin = z, y
    return zmin


class Bfgs:
    def __init__(self, fn):
        self.fn = fn
        self.calls = []          # (alpha, x) of every functor call
        self.orders = set()      # interpolation orders taken: 2, 3
        self.branches = set()    # line-search branches taken

    # ---- the function wrapper (f and df cached separately)
    def _call(self, alpha, x):
        self.calls.append((alpha, list(x)))
        f, g = self.fn(list(x))
        f, g = float(f), [float(v) for v in g]
        if not (math.isfinite(f) and all(math.isfinite(v) for v in g)):
            raise NonFinite        # the automaton's stated deviation: end at once (the original spins its 100 trials)
        return f, g

    def moveto(self, alpha):
        if alpha == self.x_key:
            return
        self.x_alpha = [a + alpha * b for a, b in zip(self.x0, self.p)]
        self.x_key = alpha

    def slope(self):
        return dot(self.g_alpha, self.p)

    def eval_f(self, alpha):
        if alpha == self.f_key:
            return self.f_alpha
        self.moveto(alpha)
        self.f_alpha, _ = self._call(alpha, self.x_alpha)
        self.f_key = alpha
        return self.f_alpha

    def eval_df(self, alpha):
        if alpha == self.df_key:
            return self.df_alpha
        self.moveto(alpha)
        if alpha != self.g_key:
            _, self.g_alpha = self._call(alpha, self.x_alpha)
            self.g_key = alpha
        self.df_alpha = self.slope()
        self.df_key = alpha
        return self.df_alpha

    def eval_fdf(self, alpha):
        if alpha == self.f_key and alpha == self.df_key:
            return self.f_alpha, self.df_alpha
        if alpha == self.f_key or alpha == self.df_key:
            return self.eval_f(alpha), self.eval_df(alpha)
        self.moveto(alpha)
        self.f_alpha, self.g_alpha = self._call(alpha, self.x_alpha)
        self.f_key = self.g_key = alpha
        self.df_alpha = self.slope()
        self.df_key = alpha
        return self.f_alpha, self.df_alpha

    # ---- the minimiser
    def init(self, x):
        self.delta_f = 0.0
        f, gradient = self._call(0.0, x)
        self.x0, self.g0 = list(x), list(gradient)
        self.g0norm = nrm(self.g0)
        with_zero = self.g0norm == 0.0
        self.p = [(-g / self.g0norm) if not with_zero else NAN for g in gradient]
        self.pnorm = nrm(self.p)
        self.fp0 = -self.g0norm
        self.x_alpha, self.g_alpha = list(self.x0), list(self.g0)
        self.f_alpha, self.df_alpha = f, self.slope()
        self.f_key = self.df_key = self.x_key = self.g_key = 0.0
        return f, gradient

    def interpolate(self, a, fa, fpa, b, fb, fpb, xmin, xmax):
        zmin, zmax = (xmin - a) / (b - a), (xmax - a) / (b - a)
        if zmin > zmax:
            zmin, zmax = zmax, zmin
        if math.isfinite(fpb):
            self.orders.add(3)
            z = interp_cubic(fa, fpa * (b - a), fb, fpb * (b - a), zmin, zmax)
        else:
            self.orders.add(2)
            z = interp_quad(fa, fpa * (b - a), fb, zmin, zmax)
        return a + z * (b - a)

    def line_search(self, alpha1):
        """-> (status, alpha): status 0 success (alpha None when the iteration cap ran out), 1 no progress"""
        alpha, alpha_prev = alpha1, 0.0
        f0, fp0 = self.eval_fdf(0.0)
        falpha_prev, fpalpha_prev = f0, fp0
        a, b, fa, fb, fpa, fpb = 0.0, alpha, f0, 0.0, fp0, 0.0
        i = 0
        while i < 100:                      # bracketing
            i += 1
            falpha = self.eval_f(alpha)
            if falpha > f0 + alpha * RHO * fp0 or falpha >= falpha_prev:
                self.branches.add("bracket_armijo")
                a, fa, fpa = alpha_prev, falpha_prev, fpalpha_prev
                b, fb, fpb = alpha, falpha, NAN
                break
            fpalpha = self.eval_df(alpha)
            if abs(fpalpha) <= -SIGMA * fp0:
                self.branches.add("bracket_accept")
                return 0, alpha
            if fpalpha >= 0:
                self.branches.add("bracket_uphill")
                a, fa, fpa = alpha, falpha, fpalpha
                b, fb, fpb = alpha_prev, falpha_prev, fpalpha_prev
                break
            self.branches.add("bracket_extend")
            delta = alpha - alpha_prev
            alpha_next = self.interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, alpha + delta,
                                          alpha + TAU1 * delta)
            alpha_prev, falpha_prev, fpalpha_prev, alpha = alpha, falpha, fpalpha, alpha_next
        else:
            i += 1                          # `while (i++ < 100)`: the failing test increments too
        while i < 100:                      # sectioning: the same counter
            i += 1
            delta = b - a
            alpha = self.interpolate(a, fa, fpa, b, fb, fpb, a + TAU2 * delta, b - TAU3 * delta)
            falpha = self.eval_f(alpha)
            if (a - alpha) * fpa <= DBL_EPSILON:
                self.branches.add("section_no_progress")
                return 1, None
            if falpha > f0 + RHO * alpha * fp0 or falpha >= fa:
                self.branches.add("section_shrink")
                b, fb, fpb = alpha, falpha, NAN
            else:
                fpalpha = self.eval_df(alpha)
                if abs(fpalpha) <= -SIGMA * fp0:
                    self.branches.add("section_accept")
                    return 0, alpha
                self.branches.add("section_move")
                if ((b - a) >= 0 and fpalpha >= 0) or ((b - a) <= 0 and fpalpha <= 0):
                    b, fb, fpb = a, fa, fpa
                a, fa, fpa = alpha, falpha, fpalpha
        self.branches.add("cap")
        return 0, None

    def one_step(self, x, f, gradient):
        """-> (status, x, f, gradient)"""
        f0 = f
        if self.pnorm == 0.0 or self.g0norm == 0.0 or self.fp0 == 0:
            return 1, x, f, gradient
        if self.delta_f < 0:
            dl = max(-self.delta_f, 10 * DBL_EPSILON * abs(f0))
            alpha1 = min(1.0, 2.0 * dl / (-self.fp0))
        else:
            alpha1 = abs(STEP)
        status, alpha = self.line_search(alpha1)
        if status:
            return status, x, f, gradient
        if alpha is None:
            alpha = 0.0
        # update_position
        f, _ = self.eval_fdf(alpha)
        x, gradient = list(self.x_alpha), list(self.g_alpha)
        self.delta_f = f - f0
        dx0 = [a - b for a, b in zip(x, self.x0)]
        dg0 = [a - b for a, b in zip(gradient, self.g0)]
        dxg, dgg, dxdg, dgnorm = dot(dx0, gradient), dot(dg0, gradient), dot(dx0, dg0), nrm(dg0)
        if dxdg != 0:
            B = dxg / dxdg
            A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg
        else:
            A = B = 0.0
        self.p = [g - A * u - B * v for g, u, v in zip(gradient, dx0, dg0)]
        self.g0, self.x0 = list(gradient), list(x)
        self.g0norm = nrm(self.g0)
        self.pnorm = nrm(self.p)
        pg = dot(self.p, gradient)
        direction = -1.0 if pg >= 0.0 else 1.0
        self.p = [v * (direction / self.pnorm) for v in self.p]
        self.pnorm = nrm(self.p)
        self.fp0 = dot(self.p, self.g0)
        # change_direction
        self.x_alpha, self.g_alpha = list(self.x0), list(self.g0)
        self.x_key = 0.0
        self.f_alpha, self.f_key, self.g_key = f, 0.0, 0.0
        self.df_alpha, self.df_key = self.slope(), 0.0
        return 0, x, f, gradient


def minimize(fn, x_start, max_inner, gradient_tol=1e-2):
    """The driver of orc_gicp_align's solver == 0 branch.  -> dict(x, f, g, n_inner, reason, points, alphas, orders, branches):
    points / alphas = the distinct evaluation points in the order they were first asked for (a functor call at the point of the
    call before it — f, then df — is the same evaluation)."""
    bf = Bfgs(fn)
    x = [float(v) for v in x_start]
    f, grad, inner, reason = 0.0, [0.0] * 6, 0, RUNNING
    try:
        f, grad = bf.init(x)
        while True:
            inner += 1
            status, x, f, grad = bf.one_step(x, f, grad)
            if status:
                reason = NO_PROGRESS
                break
            if nrm(grad) < gradient_tol:
                reason = GRADIENT_TOL
                break
            if not inner < max_inner:
                reason = MAX_INNER if inner == max_inner else RUNNING
                break
    except NonFinite:
        reason = NONFINITE
        x = list(getattr(bf, "x0", x))
    points, alphas = [], []
    for alpha, xa in bf.calls:
        if points and xa == points[-1]:
            continue
        points.append(xa)
        alphas.append(alpha)
    return dict(x=x, f=f, g=grad, n_inner=inner, reason=reason, points=points, alphas=alphas, orders=bf.orders,
                branches=bf.branches)
