// normal_eq_invert_main.cpp -- the covariance algebra of csrc/normal_eq.h (DampedSolver::invert, cholesky_inverse) on its own, for a
// sanitizer (tests/test_cpu_plain_errors.py builds it with csrc/normal_eq.cpp under AddressSanitizer + UBSan and expects exit status 0
// and nothing on stderr).  The three steps work in place on one triangle and the arrow form walks per-dataset blocks of different
// sizes through offset tables; a slip there reads or writes past a block without necessarily changing a number a test sees.  Systems:
// dense at dim 1, 2, 4, 8, 32, 65; arrow systems with the column map of Jacobian_indices -- with local blocks, without global columns,
// without local columns, with a dataset that has a single local column; a failing pivot in a local block, in the global block and in
// the dense form.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "normal_eq.h"

namespace {

struct Lcg {
  uint64_t s;
  double next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(int64_t)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; }   // [-1, 1)
};

struct System { int nd, na, dim; std::vector<int32_t> jac; std::vector<double> JTJ; };

// J: 80 rows per dataset, non-zero in the columns of that dataset's active parameters (the first nl local, the last ng global)
System make_system(int nd, int nl, int ng, uint64_t seed) {
  System s; s.nd = nd; s.na = nl + ng; s.dim = ng + nl * nd;
  const int na = s.na, dim = s.dim, rows = 80;
  s.jac.resize((size_t)nd * na);
  int shift = 0;
  for (int d = 0; d < nd; d++) for (int j = 0; j < na; j++) {
    if (j >= nl) { s.jac[(size_t)d * na + j] = j; if (d > 0) shift++; }
    else s.jac[(size_t)d * na + j] = j + d * na - shift;
  }
  Lcg g{seed};
  std::vector<double> J((size_t)rows * nd * dim, 0.0);
  for (int d = 0; d < nd; d++) for (int r = 0; r < rows; r++) for (int j = 0; j < na; j++)
    J[((size_t)d * rows + r) * dim + s.jac[(size_t)d * na + j]] = g.next();
  s.JTJ.assign((size_t)dim * dim, 0.0);
  for (int a = 0; a < dim; a++) for (int b = 0; b < dim; b++) {
    double t = 0.0;
    for (int r = 0; r < rows * nd; r++) t += J[(size_t)r * dim + a] * J[(size_t)r * dim + b];
    s.JTJ[(size_t)b * dim + a] = t;
  }
  return s;
}

int failures = 0, systems = 0;
void expect(bool ok, const char* what, int nd, int nl, int ng) {
  if (!ok) { failures++; printf("FAILED %s at (nd, nl, ng) = (%d, %d, %d)\n", what, nd, nl, ng); }
}

// || C A - I ||_max
double residual(const System& s, const std::vector<double>& C) {
  double m = 0.0;
  for (int a = 0; a < s.dim; a++) for (int b = 0; b < s.dim; b++) {
    double t = 0.0;
    for (int k = 0; k < s.dim; k++) t += C[(size_t)k * s.dim + a] * s.JTJ[(size_t)b * s.dim + k];
    t -= a == b ? 1.0 : 0.0;
    m = std::fabs(t) > m ? std::fabs(t) : m;
  }
  return m;
}

void check(int nd, int nl, int ng, bool expect_arrow) {
  systems++;
  const System s = make_system(nd, nl, ng, (uint64_t)(nd * 10000 + nl * 100 + ng));
  const int dim = s.dim;
  std::vector<double> C[2], sig[2];
  for (int use = 0; use < 2; use++) {
    gfh::DampedSolver solver;
    solver.setup(s.nd, s.na, s.jac.data(), dim, use != 0);
    if (use) expect(solver.arrow() == expect_arrow, "the form taken", nd, nl, ng);
    C[use].assign((size_t)dim * dim, -7.0); sig[use].assign(dim, -7.0);
    expect(solver.invert(s.JTJ.data(), 1.0, C[use].data(), sig[use].data()) == 0, "the inverse", nd, nl, ng);
    bool sym = true, sd = true;
    for (int a = 0; a < dim; a++) {
      for (int b = 0; b < dim; b++) sym = sym && C[use][(size_t)b * dim + a] == C[use][(size_t)a * dim + b];
      sd = sd && sig[use][a] == std::sqrt(C[use][(size_t)a * dim + a]);
    }
    expect(sym, "symmetry bit for bit", nd, nl, ng);
    expect(sd, "sigma = sqrt(diag) bit for bit", nd, nl, ng);
    expect(residual(s, C[use]) <= 1e-10, "C A = I", nd, nl, ng);
    // every entry times a factor, bit for bit
    std::vector<double> Cf((size_t)dim * dim), sf(dim);
    solver.invert(s.JTJ.data(), 1.75, Cf.data(), sf.data());
    bool scaled = true;
    for (size_t k = 0; k < Cf.size(); k++) scaled = scaled && Cf[k] == C[use][k] * 1.75;
    expect(scaled, "the factor", nd, nl, ng);
    // a failing pivot: the last column zeroed (a local column of the last dataset, or the last global one), and a NaN in the first
    for (int what = 0; what < 2; what++) {
      System bad = s;
      const int col = what ? 0 : dim - 1;
      for (int k = 0; k < dim; k++) { bad.JTJ[(size_t)col * dim + k] = what ? NAN : 0.0; bad.JTJ[(size_t)k * dim + col] = what ? NAN : 0.0; }
      const int info = solver.invert(bad.JTJ.data(), 1.0, Cf.data(), sf.data());
      bool nan = info != 0;
      for (double v : Cf) nan = nan && std::isnan(v);
      for (double v : sf) nan = nan && std::isnan(v);
      expect(nan, "a failing pivot gives info and NaN throughout", nd, nl, ng);
      if (!what) expect(info == dim, "the zeroed column is the one reported", nd, nl, ng);
    }
  }
}

}  // namespace

int main() {
  for (int dim : {1, 2, 4, 8, 32, 65}) check(1, 0, dim, false);
  check(3, 4, 3, false);          // model_global7 over three datasets: dim 15, dense
  check(40, 4, 3, true);          // ... over forty: the arrow form
  check(9, 2, 0, true);           // no global columns
  check(20, 1, 2, true);          // a single local column per dataset
  check(3, 0, 20, false);         // no local columns
  if (!failures) printf("normal_eq invert: %d systems inverted\n", systems);
  return failures ? 1 : 0;
}
