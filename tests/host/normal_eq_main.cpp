// normal_eq_main.cpp -- the host solver of csrc/normal_eq.h on its own, for a sanitizer (tests/test_cpu_normal_eq_host.py builds it
// with csrc/normal_eq.cpp under AddressSanitizer + UBSan and expects exit status 0 and nothing on stderr).  The blocked factorisation
// pads its last columns and an odd last row by repeating indices; a slip there reads or writes past the matrix without changing any
// number a test sees, so only a sanitizer tells.  Sizes: both sides of the plain / blocked switch (64 / 65), of the block edge (47 /
// 48 / 49, 96 / 97) and three blocks and a row (145); arrow systems with the column map of Jacobian_indices.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "normal_eq.h"

namespace {

// fixed integer generator: the same systems on every machine
struct Lcg {
  uint64_t s;
  double next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(int64_t)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; }   // [-1, 1)
};

struct System { int nd, na, dim; std::vector<int32_t> jac; std::vector<double> JTJ, DTD, rhs1, rhs2; };

// J: 30 rows per dataset, non-zero in the columns of that dataset's active parameters (gadfit.F90:615-631: the first nl parameters
// local, the last ng global); JTJ = J^T J column-major, DTD its diagonal
System make_system(int nd, int nl, int ng, uint64_t seed) {
  System s; s.nd = nd; s.na = nl + ng; s.dim = ng + nl * nd;
  const int na = s.na, dim = s.dim, rows = 30;
  s.jac.resize((size_t)nd * na);
  int shift = 0;
  for (int d = 0; d < nd; d++) for (int j = 0; j < na; j++) {
    if (j >= nl) { s.jac[(size_t)d * na + j] = j; if (d > 0) shift++; }
    else s.jac[(size_t)d * na + j] = j + d * na - shift;
  }
  Lcg g{seed};
  std::vector<double> J((size_t)rows * nd * dim, 0.0);          // row-major
  for (int d = 0; d < nd; d++) for (int r = 0; r < rows; r++) for (int j = 0; j < na; j++)
    J[((size_t)d * rows + r) * dim + s.jac[(size_t)d * na + j]] = g.next();
  s.JTJ.assign((size_t)dim * dim, 0.0);
  for (int a = 0; a < dim; a++) for (int b = 0; b < dim; b++) {
    double t = 0.0;
    for (int r = 0; r < rows * nd; r++) t += J[(size_t)r * dim + a] * J[(size_t)r * dim + b];
    s.JTJ[(size_t)b * dim + a] = t;
  }
  s.DTD.resize(dim); s.rhs1.resize(dim); s.rhs2.resize(dim);
  for (int i = 0; i < dim; i++) { s.DTD[i] = s.JTJ[(size_t)i * dim + i]; s.rhs1[i] = g.next(); s.rhs2[i] = g.next(); }
  return s;
}

double max_abs(const std::vector<double>& v) { double m = 0; for (double x : v) m = std::fabs(x) > m ? std::fabs(x) : m; return m; }
double max_diff(const std::vector<double>& a, const std::vector<double>& b) {
  double m = 0; for (size_t i = 0; i < a.size(); i++) m = std::fabs(a[i] - b[i]) > m ? std::fabs(a[i] - b[i]) : m; return m;
}

int failures = 0;
void expect(bool ok, const char* what, int nd, int nl, int ng) {
  if (!ok) { failures++; printf("FAILED %s at (nd, nl, ng) = (%d, %d, %d)\n", what, nd, nl, ng); }
}

// factor + solve twice (the second factor is what a retried trial step does), each time with a second right-hand side against the
// same factor; returns the two solutions of the second round after checking that the rounds agree bit for bit
bool run_solver(const System& s, bool use_structure, double lambda, std::vector<double>* x1, std::vector<double>* x2) {
  gfh::DampedSolver solver;
  solver.setup(s.nd, s.na, s.jac.data(), s.dim, use_structure);
  std::vector<double> a1(s.dim), a2(s.dim);
  x1->assign(s.dim, 0.0); x2->assign(s.dim, 0.0);
  if (solver.factor(s.JTJ.data(), s.DTD.data(), lambda)) return false;
  solver.solve(s.rhs1.data(), a1.data()); solver.solve(s.rhs2.data(), a2.data());
  if (solver.factor(s.JTJ.data(), s.DTD.data(), lambda)) return false;
  solver.solve(s.rhs1.data(), x1->data()); solver.solve(s.rhs2.data(), x2->data());
  return a1 == *x1 && a2 == *x2;
}

void check(int nd, int nl, int ng) {
  const double lambda = 0.37, bound = 1e-12;      // tests/test_cpu_cabi.py::test_damped_solve_block_arrow_equals_dense: 1e-12 of the solution's scale
  const System s = make_system(nd, nl, ng, (uint64_t)(nd * 10000 + nl * 100 + ng));
  const int dim = s.dim;
  std::vector<double> xa1, xa2, xd1, xd2;
  expect(run_solver(s, true, lambda, &xa1, &xa2), "the solve with the structure (or its repeat)", nd, nl, ng);
  expect(run_solver(s, false, lambda, &xd1, &xd2), "the dense solve (or its repeat)", nd, nl, ng);
  expect(max_diff(xa1, xd1) <= bound * max_abs(xd1) && max_diff(xa2, xd2) <= bound * max_abs(xd2), "arrow against dense", nd, nl, ng);
  // ... and the dense arm against the plain factorisation (the same function up to dim 64, another order of additions above)
  std::vector<double> m(s.JTJ), p1(s.rhs1), p2(s.rhs2);
  for (int i = 0; i < dim; i++) m[(size_t)i * dim + i] += lambda * s.DTD[i];
  expect(gfh::potrf_upper_plain(dim, m.data()) == 0, "the plain factorisation", nd, nl, ng);
  gfh::potrs_upper(dim, m.data(), p1.data()); gfh::potrs_upper(dim, m.data(), p2.data());
  expect(max_diff(xd1, p1) <= bound * max_abs(p1) && max_diff(xd2, p2) <= bound * max_abs(p2), "dense against plain", nd, nl, ng);
  // a matrix that is not positive definite is a return value
  System bad = s; bad.JTJ[0] = -1.0;
  gfh::DampedSolver solver;
  for (int use = 0; use < 2; use++) {
    solver.setup(bad.nd, bad.na, bad.jac.data(), bad.dim, use != 0);
    expect(solver.factor(bad.JTJ.data(), bad.DTD.data(), 0.0) == 1, "refusal of an indefinite matrix", nd, nl, ng);
  }
}

}  // namespace

int main() {
  for (int dim : {1, 2, 47, 48, 49, 64, 65, 96, 97, 145}) check(1, 0, dim);
  check(2, 2, 1); check(3, 0, 4); check(5, 3, 0); check(2, 48, 1);
  if (!failures) printf("normal_eq: 14 systems solved\n");
  return failures ? 1 : 0;
}
