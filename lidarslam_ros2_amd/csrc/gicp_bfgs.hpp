// The BFGS inner optimiser of GICP — PCL's port of GSL vector_bfgs2 as pclomp::GeneralizedIterativeClosestPoint drives it
// (SURVEY.md §9.7), restated line by line after oracle/gicp_oracle.cpp (struct Bfgs and the solver == 0 branch of orc_gicp_align) —
// as a RESUMABLE AUTOMATON: the nested loops (driver do-while > one_step > Fletcher line search: bracketing, sectioning) are
// flattened so that the automaton stops wherever the original asks for a cost/gradient evaluation and goes on when it is handed the
// result.  One evaluation per launch on the device (csrc/gicp.hip: gicp_bfgs_step_kernel runs this on lane 0 of its controller
// wave); compiled for the host under LSR_HOST_EMU by tools/gicp_bfgs_host_emu (tests/test_gicp_bfgs_cpu.py).  Everything is fp64;
// no FMA contraction (the host build and the device build then run the same operations).
//
//   bfgs_begin(S, x, max_inner)   -> BFGS_EVAL: evaluate (f, g) at S.x_req (= x)
//   bfgs_consume(S, f, g)         -> BFGS_EVAL: evaluate at S.x_req;  BFGS_DONE: S.x0 / S.f / S.g0 are the result, S.reason why
//
// Evaluation caching.  The GSL wrapper caches f and df of the last alpha separately and sometimes evaluates f alone (eval_f in the
// line search, eval_df only when the Armijo test passed).  Here EVERY evaluation yields f and g together, and the automaton keeps
// the last one (cur_alpha, cur_f, cur_g): a request at the alpha it already holds costs no evaluation.  That is equivalent, because
// an evaluation is a deterministic function of x (fixed-order sums): f or g asked for later at the same alpha have the bits they
// would have had.  Only the NUMBER of evaluations differs from the wrapper's number of calls.
//
// The one deviation: a non-finite f or g ends the loop at once (BFGS_NONFINITE) with the last accepted — finite — x; the original
// would spend its 100 line-search trials there.
#pragma once
#ifndef LSR_HOST_EMU
#include <hip/hip_runtime.h>
#endif

namespace lsr {

enum { BFGS_EVAL = 0, BFGS_DONE = 1 };
// why the inner loop ended; BFGS_RUNNING is the driver's "max_inner_iterations < 1 and one step did not finish the job" (the
// reference then throws: the align ends unconverged)
enum { BFGS_RUNNING = 0, BFGS_NO_PROGRESS = 1, BFGS_GRADIENT_TOL = 2, BFGS_MAX_INNER = 3, BFGS_NONFINITE = 4 };
// which line-search branches an align (a test function) has taken: BfgsState::visited
enum {
  BFGS_V_BRACKET_ARMIJO = 1,      // bracketing: trial fails the descent test (overshoot) -> section [alpha_prev, alpha]
  BFGS_V_BRACKET_ACCEPT = 2,      // bracketing: curvature test passed
  BFGS_V_BRACKET_UPHILL = 4,      // bracketing: slope >= 0 -> section [alpha, alpha_prev]
  BFGS_V_BRACKET_EXTEND = 8,      // bracketing: extrapolated to a larger alpha
  BFGS_V_SECTION_SHRINK = 16,     // sectioning: trial fails the descent test -> b = alpha
  BFGS_V_SECTION_ACCEPT = 32,     // sectioning: curvature test passed
  BFGS_V_SECTION_MOVE = 64,       // sectioning: a = alpha
  BFGS_V_CUBIC = 128,             // interpolation by the cubic
  BFGS_V_QUADRATIC = 256,         // interpolation by the quadratic (fpb not finite)
  BFGS_V_SECTION_NO_PROGRESS = 512,
  BFGS_V_CAP = 1024               // the shared iteration cap (100) ran out
};

constexpr double BFGS_RHO = 0.01, BFGS_SIGMA = 0.01, BFGS_TAU1 = 9, BFGS_TAU2 = 0.05, BFGS_TAU3 = 0.5, BFGS_STEP = 1.0;
constexpr double BFGS_GRADIENT_TOL_VALUE = 1e-2, BFGS_DBL_EPSILON = 2.220446049250313e-16;
constexpr int BFGS_LINE_ITERS = 100;

struct BfgsState {
  double x0[6], g0[6], p[6];      // the accepted point, its gradient, the search direction (unit length)
  double f;                       // cost at x0
  double delta_f, fp0, pnorm, g0norm;
  double df0;                     // slope at alpha = 0 as the wrapper caches it (dot(g0, p); init's fp0 is -|g0| instead)
  double cur_alpha, cur_f, cur_g[6];   // the last evaluation along p
  double req_alpha, x_req[6];     // the evaluation asked for
  // line search
  double ls_f0, ls_fp0, alpha, alpha_prev, falpha_prev, fpalpha_prev, a, b, fa, fb, fpa, fpb;
  int ls_i;
  int stage;
  int inner, max_inner;           // one_step calls so far
  int reason;
  int n_evals;                    // evaluations consumed
  int visited;
  int pad;
};
static_assert(sizeof(BfgsState) % 8 == 0, "BfgsState travels inside IterBlock (8-byte words)");

namespace bfgs_detail {
enum { ST_INIT = 0, ST_BRACKET_EVAL = 1, ST_SECTION_EVAL = 2, ST_UPDATE_EVAL = 3 };
// where the automaton goes on without an evaluation
enum { GO_START_STEP = 16, GO_BRACKET_HEAD, GO_SECTION_HEAD, GO_BRACKET_EVAL, GO_SECTION_EVAL, GO_UPDATE };

__host__ __device__ inline bool finite_d(double v) { return (v - v) == 0.0; }   // false for NaN and +-inf
__host__ __device__ inline double nrm6(const double* v) {
#pragma clang fp contract(off)
  double s = 0;
  for (int i = 0; i < 6; i++) s += v[i] * v[i];
  return sqrt(s);
}
__host__ __device__ inline double dot6(const double* a, const double* b) {
#pragma clang fp contract(off)
  double s = 0;
  for (int i = 0; i < 6; i++) s += a[i] * b[i];
  return s;
}

__host__ __device__ inline double interp_quad(double f0, double fp0, double f1, double zl, double zh) {
#pragma clang fp contract(off)
  const double fl = f0 + zl * (fp0 + zl * (f1 - f0 - fp0));
  const double fh = f0 + zh * (fp0 + zh * (f1 - f0 - fp0));
  const double c = 2 * (f1 - f0 - fp0);
  double zmin = zl, fmin = fl;
  if (fh < fmin) { zmin = zh; fmin = fh; }
  if (c > 0) {
    const double z = -fp0 / c;
    if (z > zl && z < zh) {
      const double f = f0 + z * (fp0 + z * (f1 - f0 - fp0));
      if (f < fmin) { zmin = z; fmin = f; }
    }
  }
  return zmin;
}

__host__ __device__ inline double cubic(double c0, double c1, double c2, double c3, double z) {
#pragma clang fp contract(off)
  return c0 + z * (c1 + z * (c2 + z * c3));
}

__host__ __device__ inline int solve_quadratic(double a, double b, double c, double* x0, double* x1) {
#pragma clang fp contract(off)
  if (a == 0) {
    if (b == 0) return 0;
    *x0 = -c / b;
    return 1;
  }
  const double disc = b * b - 4 * a * c;
  if (disc > 0) {
    if (b == 0) {
      const double r = sqrt(-c / a);
      *x0 = -r; *x1 = r;
    } else {
      const double sgnb = (b > 0 ? 1 : -1);
      const double temp = -0.5 * (b + sgnb * sqrt(disc));
      const double r1 = temp / a, r2 = c / temp;
      if (r1 < r2) { *x0 = r1; *x1 = r2; } else { *x0 = r2; *x1 = r1; }
    }
    return 2;
  } else if (disc == 0) {
    *x0 = -0.5 * b / a; *x1 = -0.5 * b / a;
    return 2;
  }
  return 0;
}

__host__ __device__ inline double interp_cubic(double f0, double fp0, double f1, double fp1, double zl, double zh) {
#pragma clang fp contract(off)
  const double eta = 3 * (f1 - f0) - 2 * fp0 - fp1;
  const double xi = fp0 + fp1 - 2 * (f1 - f0);
  const double c0 = f0, c1 = fp0, c2 = eta, c3 = xi;
  double zmin = zl, fmin = cubic(c0, c1, c2, c3, zl), z0 = 0, z1 = 0;
  { const double y = cubic(c0, c1, c2, c3, zh); if (y < fmin) { zmin = zh; fmin = y; } }
  const int n = solve_quadratic(3 * c3, 2 * c2, c1, &z0, &z1);
  if (n == 2) {
    if (z0 > zl && z0 < zh) { const double y = cubic(c0, c1, c2, c3, z0); if (y < fmin) { zmin = z0; fmin = y; } }
    if (z1 > zl && z1 < zh) { const double y = cubic(c0, c1, c2, c3, z1); if (y < fmin) { zmin = z1; fmin = y; } }
  } else if (n == 1) {
    if (z0 > zl && z0 < zh) { const double y = cubic(c0, c1, c2, c3, z0); if (y < fmin) { zmin = z0; fmin = y; } }
  }
  return zmin;
}

__host__ __device__ inline double interpolate(BfgsState& S, double a, double fa, double fpa, double b, double fb, double fpb, double xmin,
                                              double xmax) {
#pragma clang fp contract(off)
  double zmin = (xmin - a) / (b - a), zmax = (xmax - a) / (b - a);
  if (zmin > zmax) { const double t = zmin; zmin = zmax; zmax = t; }
  double z;
  if (finite_d(fpb)) {   // order 3
    S.visited |= BFGS_V_CUBIC;
    z = interp_cubic(fa, fpa * (b - a), fb, fpb * (b - a), zmin, zmax);
  } else {
    S.visited |= BFGS_V_QUADRATIC;
    z = interp_quad(fa, fpa * (b - a), fb, zmin, zmax);
  }
  return a + z * (b - a);
}

__host__ __device__ inline double quiet_nan() { return __builtin_nan(""); }
}  // namespace bfgs_detail

__host__ __device__ inline int bfgs_begin(BfgsState& S, const double* x, int max_inner) {
  for (int i = 0; i < 6; i++) { S.x_req[i] = x[i]; S.x0[i] = x[i]; S.g0[i] = 0; S.p[i] = 0; S.cur_g[i] = 0; }
  S.f = 0; S.delta_f = 0; S.fp0 = 0; S.pnorm = 0; S.g0norm = 0; S.df0 = 0;
  S.cur_alpha = 0; S.cur_f = 0; S.req_alpha = 0;
  S.ls_f0 = S.ls_fp0 = S.alpha = S.alpha_prev = S.falpha_prev = S.fpalpha_prev = 0;
  S.a = S.b = S.fa = S.fb = S.fpa = S.fpb = 0;
  S.ls_i = 0;
  S.stage = bfgs_detail::ST_INIT;
  S.inner = 0; S.max_inner = max_inner;
  S.reason = BFGS_RUNNING;
  S.n_evals = 0; S.visited = 0; S.pad = 0;
  return BFGS_EVAL;
}

__host__ __device__ inline int bfgs_consume(BfgsState& S, double f, const double* g) {
#pragma clang fp contract(off)
  using namespace bfgs_detail;
  S.n_evals++;
  bool ok = finite_d(f);
  for (int i = 0; i < 6; i++) ok = ok && finite_d(g[i]);
  if (!ok) {   // (the stated deviation) x0 is the last accepted point — the start x when nothing has been accepted yet
    S.reason = BFGS_NONFINITE;
    return BFGS_DONE;
  }
  int go = S.stage;
  if (go == ST_INIT) {   // Bfgs::init
    S.delta_f = 0;
    S.f = f;
    for (int i = 0; i < 6; i++) { S.x0[i] = S.x_req[i]; S.g0[i] = g[i]; }
    S.g0norm = nrm6(S.g0);
    for (int i = 0; i < 6; i++) S.p[i] = -g[i] / S.g0norm;
    S.pnorm = nrm6(S.p);
    S.fp0 = -S.g0norm;
    S.cur_alpha = 0; S.cur_f = f;
    for (int i = 0; i < 6; i++) S.cur_g[i] = g[i];
    S.df0 = dot6(S.cur_g, S.p);
    S.inner = 0;
    go = GO_START_STEP;
  } else {
    S.cur_alpha = S.req_alpha; S.cur_f = f;
    for (int i = 0; i < 6; i++) S.cur_g[i] = g[i];
    go = (go == ST_BRACKET_EVAL) ? GO_BRACKET_EVAL : (go == ST_SECTION_EVAL) ? GO_SECTION_EVAL : GO_UPDATE;
  }
  for (;;) {
    int want = -1;   // the stage that needs (f, g) at S.alpha next
    switch (go) {
      case GO_START_STEP: {   // the driver's do { inner++; one_step ... : one_step up to its line search
        S.inner++;
        if (S.pnorm == 0.0 || S.g0norm == 0.0 || S.fp0 == 0) { S.reason = BFGS_NO_PROGRESS; return BFGS_DONE; }
        double alpha1;
        if (S.delta_f < 0) {
          const double m1 = -S.delta_f, m2 = 10 * BFGS_DBL_EPSILON * fabs(S.f);
          const double del = (m1 < m2) ? m2 : m1;
          const double c = 2.0 * del / (-S.fp0);
          alpha1 = (c < 1.0) ? c : 1.0;
        } else {
          alpha1 = fabs(BFGS_STEP);
        }
        // line_search: eval_fdf(0.0) is the cached pair
        S.ls_f0 = S.f; S.ls_fp0 = S.df0;
        S.alpha = alpha1; S.alpha_prev = 0.0;
        S.falpha_prev = S.ls_f0; S.fpalpha_prev = S.ls_fp0;
        S.a = 0.0; S.b = S.alpha; S.fa = S.ls_f0; S.fb = 0.0; S.fpa = S.ls_fp0; S.fpb = 0.0;
        S.ls_i = 0;
        go = GO_BRACKET_HEAD;
        break;
      }
      case GO_BRACKET_HEAD:
        if (S.ls_i++ < BFGS_LINE_ITERS) want = ST_BRACKET_EVAL;
        else go = GO_SECTION_HEAD;
        break;
      case GO_BRACKET_EVAL: {
        const double falpha = S.cur_f;
        if (falpha > S.ls_f0 + S.alpha * BFGS_RHO * S.ls_fp0 || falpha >= S.falpha_prev) {
          S.visited |= BFGS_V_BRACKET_ARMIJO;
          S.a = S.alpha_prev; S.fa = S.falpha_prev; S.fpa = S.fpalpha_prev;
          S.b = S.alpha; S.fb = falpha; S.fpb = quiet_nan();
          go = GO_SECTION_HEAD;
          break;
        }
        const double fpalpha = dot6(S.cur_g, S.p);
        if (fabs(fpalpha) <= -BFGS_SIGMA * S.ls_fp0) { S.visited |= BFGS_V_BRACKET_ACCEPT; go = GO_UPDATE; break; }
        if (fpalpha >= 0) {
          S.visited |= BFGS_V_BRACKET_UPHILL;
          S.a = S.alpha; S.fa = falpha; S.fpa = fpalpha;
          S.b = S.alpha_prev; S.fb = S.falpha_prev; S.fpb = S.fpalpha_prev;
          go = GO_SECTION_HEAD;
          break;
        }
        S.visited |= BFGS_V_BRACKET_EXTEND;
        const double delta = S.alpha - S.alpha_prev;
        const double alpha_next = interpolate(S, S.alpha_prev, S.falpha_prev, S.fpalpha_prev, S.alpha, falpha, fpalpha, S.alpha + delta,
                                              S.alpha + BFGS_TAU1 * delta);
        S.alpha_prev = S.alpha; S.falpha_prev = falpha; S.fpalpha_prev = fpalpha; S.alpha = alpha_next;
        go = GO_BRACKET_HEAD;
        break;
      }
      case GO_SECTION_HEAD:
        if (S.ls_i++ < BFGS_LINE_ITERS) {
          const double delta = S.b - S.a;
          S.alpha = interpolate(S, S.a, S.fa, S.fpa, S.b, S.fb, S.fpb, S.a + BFGS_TAU2 * delta, S.b - BFGS_TAU3 * delta);
          want = ST_SECTION_EVAL;
        } else {   // line_search returns success with alpha_new untouched: one_step's alpha = 0.0
          S.visited |= BFGS_V_CAP;
          S.alpha = 0.0;
          want = ST_UPDATE_EVAL;
        }
        break;
      case GO_SECTION_EVAL: {
        const double falpha = S.cur_f;
        if ((S.a - S.alpha) * S.fpa <= BFGS_DBL_EPSILON) {
          S.visited |= BFGS_V_SECTION_NO_PROGRESS;
          S.reason = BFGS_NO_PROGRESS;
          return BFGS_DONE;
        }
        if (falpha > S.ls_f0 + BFGS_RHO * S.alpha * S.ls_fp0 || falpha >= S.fa) {
          S.visited |= BFGS_V_SECTION_SHRINK;
          S.b = S.alpha; S.fb = falpha; S.fpb = quiet_nan();
        } else {
          const double fpalpha = dot6(S.cur_g, S.p);
          if (fabs(fpalpha) <= -BFGS_SIGMA * S.ls_fp0) { S.visited |= BFGS_V_SECTION_ACCEPT; go = GO_UPDATE; break; }
          S.visited |= BFGS_V_SECTION_MOVE;
          if (((S.b - S.a) >= 0 && fpalpha >= 0) || ((S.b - S.a) <= 0 && fpalpha <= 0)) {
            S.b = S.a; S.fb = S.fa; S.fpb = S.fpa;
            S.a = S.alpha; S.fa = falpha; S.fpa = fpalpha;
          } else {
            S.a = S.alpha; S.fa = falpha; S.fpa = fpalpha;
          }
        }
        go = GO_SECTION_HEAD;
        break;
      }
      case GO_UPDATE: {   // update_position at S.alpha (= cur_alpha), the direction update, change_direction, the driver's tests
        const double f0 = S.f;
        double x[6], dx0[6], dg0[6];
        const double* gradient = S.cur_g;
        for (int i = 0; i < 6; i++) x[i] = S.x_req[i];
        S.f = S.cur_f;
        S.delta_f = S.f - f0;
        for (int i = 0; i < 6; i++) { dx0[i] = x[i] - S.x0[i]; dg0[i] = gradient[i] - S.g0[i]; }
        const double dxg = dot6(dx0, gradient), dgg = dot6(dg0, gradient), dxdg = dot6(dx0, dg0), dgnorm = nrm6(dg0);
        double A, B;
        if (dxdg != 0) {
          B = dxg / dxdg;
          A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg;
        } else {
          B = 0; A = 0;
        }
        for (int i = 0; i < 6; i++) S.p[i] = gradient[i] - A * dx0[i] - B * dg0[i];
        for (int i = 0; i < 6; i++) { S.g0[i] = gradient[i]; S.x0[i] = x[i]; }
        S.g0norm = nrm6(S.g0);
        S.pnorm = nrm6(S.p);
        const double pg = dot6(S.p, gradient);
        const double dir = (pg >= 0.0) ? -1.0 : +1.0;
        for (int i = 0; i < 6; i++) S.p[i] *= dir / S.pnorm;
        S.pnorm = nrm6(S.p);
        S.fp0 = dot6(S.p, S.g0);
        S.cur_alpha = 0; S.req_alpha = 0;   // cur_f / cur_g / x_req stay: they are the evaluation at the new x0
        S.df0 = dot6(S.cur_g, S.p);
        if (nrm6(S.g0) < BFGS_GRADIENT_TOL_VALUE) { S.reason = BFGS_GRADIENT_TOL; return BFGS_DONE; }
        if (S.inner < S.max_inner) { go = GO_START_STEP; break; }
        S.reason = (S.inner == S.max_inner) ? BFGS_MAX_INNER : BFGS_RUNNING;
        return BFGS_DONE;
      }
    }
    if (want >= 0) {
      if (S.alpha == S.cur_alpha) {   // held already: no evaluation
        go = (want == ST_BRACKET_EVAL) ? GO_BRACKET_EVAL : (want == ST_SECTION_EVAL) ? GO_SECTION_EVAL : GO_UPDATE;
        continue;
      }
      for (int i = 0; i < 6; i++) S.x_req[i] = S.x0[i] + S.alpha * S.p[i];   // moveto
      S.req_alpha = S.alpha;
      S.stage = want;
      return BFGS_EVAL;
    }
  }
}

// the align goes on with the result (NoProgress / Success / the iteration cap reached); otherwise the reference's solver throws
__host__ __device__ inline bool bfgs_accepted(const BfgsState& S) {
  return S.reason == BFGS_NO_PROGRESS || S.reason == BFGS_GRADIENT_TOL || S.reason == BFGS_MAX_INNER;
}

// One cost/gradient evaluation from the 13 sums of a pass over the m pairs (OptimizationFunctorWithIndices::fdf as
// oracle/gicp_oracle.cpp: cost_grad restates it): sums[0] = sum r^T M r, sums[1..3] = sum M r, sums[4 + 3a + b] = sum p_a (M r)_b;
// dR27 = dR/dphi, dR/dtheta, dR/dpsi at the evaluated x (row-major 3x3 each).  f = sums[0] / m; g_t = 2/m sum M r;
// g_r[k] = tr(dR_k * Rm) with Rm = 2/m sum p (M r)^T.
__host__ __device__ inline void bfgs_cost_gradient(const double* sums, int m, const double* dR27, double* f, double* g) {
#pragma clang fp contract(off)
  const double s = 2.0 / m;
  double Rm[9];
  for (int a = 0; a < 3; a++) g[a] = sums[1 + a] * s;
  for (int a = 0; a < 9; a++) Rm[a] = sums[4 + a] * s;
  for (int k = 0; k < 3; k++) {
    const double* D = dR27 + 9 * k;
    double r = 0;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) r += D[j * 3 + i] * Rm[i * 3 + j];
    g[3 + k] = r;
  }
  *f = sums[0] / m;
}

}  // namespace lsr
