// TEST INFRASTRUCTURE.  csrc/gicp_bfgs.hpp compiled for the CPU: the BFGS automaton exactly as lane 0 of gicp_bfgs_step_kernel runs
// it, driven by a C callback for (f, g), checked against the plain nested-loop restatement (tests/gicp_bfgs_numpy.py) without a
// GPU (tests/test_gicp_bfgs_cpu.py); and the analytic test functions both sides evaluate (one shared implementation: the same bits).
//   g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off harness.cpp -o libgicpbfgsemu.so
#include <cmath>

#define __device__
#define __host__
#define LSR_HOST_EMU 1
#include "../../lidarslam_ros2_amd/csrc/gicp_bfgs.hpp"

using namespace lsr;

extern "C" {

typedef void (*emu_bfgs_fn)(const double* x6, double* f, double* g6, void* user);

// Runs one inner loop from x_start.  Per evaluation e < capacity: xs[6 e ..] the point asked for, alphas[e] its step along the
// direction of its line search (0 for the start x), inner[e] the step it belonged to.  -> the automaton's reason.
int emu_bfgs_run(const double* x_start, int max_inner, emu_bfgs_fn fn, void* user, int capacity, double* xs, double* alphas, int* inner,
                 int* n_evals, int* n_inner, int* visited, double* x_final, double* f_final, double* g_final) {
  BfgsState S;
  int r = bfgs_begin(S, x_start, max_inner);
  int e = 0;
  while (r == BFGS_EVAL) {
    if (e < capacity) {
      for (int k = 0; k < 6; k++) xs[6 * e + k] = S.x_req[k];
      alphas[e] = S.req_alpha;
      inner[e] = S.inner;
    }
    e++;
    double f = 0, g[6] = {0, 0, 0, 0, 0, 0};
    fn(S.x_req, &f, g, user);
    r = bfgs_consume(S, f, g);
  }
  if (n_evals) *n_evals = S.n_evals;
  if (n_inner) *n_inner = S.inner;
  if (visited) *visited = S.visited;
  for (int k = 0; k < 6; k++) {
    if (x_final) x_final[k] = S.x0[k];
    if (g_final) g_final[k] = S.g0[k];
  }
  if (f_final) *f_final = S.f;
  return S.reason;
}

void emu_bfgs_cost_gradient(const double* sums13, int m, const double* dR27, double* f, double* g6) {
  bfgs_cost_gradient(sums13, m, dR27, f, g6);
}

// ---- analytic functions in six variables (which = *(int*)user)
//   0  convex quadratic, condition number 1e4: 1/2 sum d_i (x_i - c_i)^2, d = 1 .. 1e4
//   1  Rosenbrock chain: sum_{i<5} 100 (x_{i+1} - x_i^2)^2 + (1 - x_i)^2
//   2  steep quartic bowl with a ripple: the unit first trial step overshoots the minimum by far
//   3  function 0 where x_0 <= 0.5, NaN beyond
static const double EMU_C[6] = {0.7, -0.4, 0.25, 0.1, -0.2, 0.05};
static const double EMU_D[6] = {1.0, 6.309573444801933, 39.810717055349734, 251.18864315095823, 1584.893192461114, 1.0e4};

void emu_bfgs_test_function(const double* x, double* f, double* g, void* user) {
  const int which = *static_cast<const int*>(user);
  double s = 0;
  if (which == 0 || which == 3) {
    for (int i = 0; i < 6; i++) {
      const double d = x[i] - EMU_C[i];
      s += 0.5 * EMU_D[i] * d * d;
      g[i] = EMU_D[i] * d;
    }
    if (which == 3 && x[0] > 0.5) s = std::nan("");
  } else if (which == 1) {
    for (int i = 0; i < 6; i++) g[i] = 0;
    for (int i = 0; i < 5; i++) {
      const double a = x[i + 1] - x[i] * x[i], b = 1.0 - x[i];
      s += 100.0 * a * a + b * b;
      g[i] += -400.0 * a * x[i] - 2.0 * b;
      g[i + 1] += 200.0 * a;
    }
  } else {
    for (int i = 0; i < 6; i++) {
      const double d = x[i] - EMU_C[i], w = 3.0 + 2.0 * i;
      s += w * (d * d * d * d + 0.5 * d * d) + std::sin(3.0 * d) * std::sin(3.0 * d);
      g[i] = w * (4.0 * d * d * d + d) + 6.0 * std::sin(3.0 * d) * std::cos(3.0 * d);
    }
  }
  *f = s;
}

}  // extern "C"
