// TEST INFRASTRUCTURE.  Stand-alone replay of the analytic functions of harness.cpp through the automaton of csrc/gicp_bfgs.hpp,
// for a sanitizer build (tests/test_gicp_bfgs_cpu.py builds and runs it; nothing is loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all replay_main.cpp harness.cpp -o replay
// Exit status 0: every run ended for the expected reason at a finite point.
#include <cmath>
#include <cstdio>
#include <vector>

extern "C" {
typedef void (*emu_bfgs_fn)(const double* x6, double* f, double* g6, void* user);
int emu_bfgs_run(const double* x_start, int max_inner, emu_bfgs_fn fn, void* user, int capacity, double* xs, double* alphas, int* inner,
                 int* n_evals, int* n_inner, int* visited, double* x_final, double* f_final, double* g_final);
void emu_bfgs_test_function(const double* x, double* f, double* g, void* user);
}

namespace {
struct Run { int which; double x[6]; int max_inner; int capacity; int want_reason; };   // want_reason < 0: any
}

int main() {
  const double C6[6] = {0.7, -0.4, 0.25, 0.1, -0.2, 0.05};
  const Run runs[] = {
      {0, {0, 0, 0, 0, 0, 0}, 20, 256, 2},
      {0, {0, 0, 0, 0, 0, 0}, 0, 256, 0},                               // one step, the driver left still running
      {0, {C6[0], C6[1], C6[2], C6[3], C6[4], C6[5]}, 20, 256, 1},      // zero start gradient: no progress at once
      {1, {-1.2, 1.0, -1.2, 1.0, -1.2, 1.0}, 20, 256, 3},
      {1, {-1.2, 1.0, -1.2, 1.0, -1.2, 1.0}, 200, 8, -1},               // more evaluations than the trace holds
      {2, {1.0, -0.6, 0.5, 0.25, -0.5, 0.25}, 20, 256, 2},
      {3, {0, 0, 0, 0, 0, 0}, 20, 256, 4},
      {3, {0, 0, 0, 0, 0, 0}, 20, 0, 4},                                // no trace at all
  };
  int bad = 0;
  for (const Run& r : runs) {
    std::vector<double> xs((size_t)r.capacity * 6 + 1), al((size_t)r.capacity + 1);
    std::vector<int> inner((size_t)r.capacity + 1);
    int n_evals = 0, n_inner = 0, visited = 0, which = r.which;
    double xf[6], gf[6], ff = 0;
    const int reason = emu_bfgs_run(r.x, r.max_inner, emu_bfgs_test_function, &which, r.capacity, xs.data(), al.data(), inner.data(), &n_evals,
                                    &n_inner, &visited, xf, &ff, gf);
    bool ok = (r.want_reason < 0 || reason == r.want_reason) && n_inner >= 1 && n_evals >= 1;
    for (int k = 0; k < 6; k++) ok = ok && std::isfinite(xf[k]);
    std::printf("function %d max_inner %d: %d evaluations, %d steps, reason %d, visited 0x%x, f %.17g%s\n", r.which, r.max_inner, n_evals, n_inner,
                reason, visited, ff, ok ? "" : "  <-- unexpected");
    if (!ok) bad++;
  }
  return bad ? 1 : 0;
}
