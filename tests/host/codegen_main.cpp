// codegen_main.cpp -- the generator as a program of its own: three small tapes built by hand go through Model::load /
// load_variants and generate_source (default, finite differences, batch) and through two refusals.  Built with codegen.cpp,
// emit_*.cpp, ws_plan.cpp, model.cpp and device_text.cpp alone: no context, no HIP header.  tests/test_cpu_codegen_host.py
// compiles it under AddressSanitizer and UBSan; exit status 0 = every call returned what it should and every text is non-empty.
#include "codegen.h"
#include <cstdio>
#include <string>
#include <vector>

using namespace gfh;

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) { printf("FAILED: %s\n", what); failures++; }
}

struct TapeBuilder {
  std::vector<std::vector<gfh_node>> nodes;
  std::vector<int32_t> results;
  std::vector<gfh_integral> integrals;
  std::vector<int32_t> ipar_nodes;
  std::vector<gfh_subtape> subs;
  gfh_tape tape{};
  int add(int s, int op, int a = -1, int b = -1, int flags = 0, double c = 0.0) {
    if ((int)nodes.size() <= s) { nodes.resize((size_t)s + 1); results.resize((size_t)s + 1, 0); }
    nodes[(size_t)s].push_back({op, a, b, flags, c});
    return (int)nodes[(size_t)s].size() - 1;
  }
  const gfh_tape* finish(int n_pars) {
    subs.clear();
    for (size_t s = 0; s < nodes.size(); s++) subs.push_back({(int32_t)nodes[s].size(), results[s], nodes[s].data()});
    tape = gfh_tape{};
    tape.n_pars = n_pars; tape.n_subtapes = (int32_t)subs.size(); tape.sub = subs.data();
    tape.n_integrals = (int32_t)integrals.size(); tape.integrals = integrals.data(); tape.ipar_nodes = ipar_nodes.data();
    tape.rel_error_outer = 1e-10; tape.rel_error_inner = 1e-10;
    return &tape;
  }
};

// every arithmetic and unary operation over three parameters and x
void build_elementals(TapeBuilder& t) {
  const int p0 = t.add(0, GFH_PARAM, 0), p1 = t.add(0, GFH_PARAM, 1), p2 = t.add(0, GFH_PARAM, 2);
  const int x = t.add(0, GFH_X, -1, -1, GFH_F_REAL), two = t.add(0, GFH_CONST, -1, -1, GFH_F_REAL, 2.0);
  const int nx = t.add(0, GFH_NEG, x, -1, GFH_F_REAL), lx = t.add(0, GFH_LIFT, nx);
  const int val = t.add(0, GFH_VAL, p2, -1, GFH_F_REAL);
  int y = t.add(0, GFH_ADD, p0, p1);
  y = t.add(0, GFH_SUB, y, p2);
  y = t.add(0, GFH_MUL, y, x);
  y = t.add(0, GFH_DIV, y, p1);
  y = t.add(0, GFH_DIV, two, y);
  y = t.add(0, GFH_POW, y, p0);
  y = t.add(0, GFH_POW, y, two);
  y = t.add(0, GFH_ADD, y, lx);
  y = t.add(0, GFH_MUL, y, val);
  for (int n : {-2, 0, 1, 2, 3, 5}) { const int q = t.add(0, GFH_POWI, p1, n); y = t.add(0, GFH_ADD, y, q); }
  for (int op = GFH_ABS; op <= GFH_ERF; op++) { const int u = t.add(0, op, p0); y = t.add(0, GFH_ADD, y, u); }
  t.results[0] = y;
}

// p0 * int_{p1}^{inf} exp(-(q0 t)) t dt: a finite, active bound and an infinite one
void build_integral(TapeBuilder& t) {
  const int p0 = t.add(0, GFH_PARAM, 0), p1 = t.add(0, GFH_PARAM, 1);
  const int i = t.add(0, GFH_INTEGRATE, 0);
  t.results[0] = t.add(0, GFH_MUL, p0, i);
  const int tv = t.add(1, GFH_IVAR), q0 = t.add(1, GFH_IPARAM, 0);
  const int m = t.add(1, GFH_MUL, q0, tv), n = t.add(1, GFH_NEG, m), e = t.add(1, GFH_EXP, n);
  t.results[1] = t.add(1, GFH_MUL, e, tv);
  t.ipar_nodes = {p0};
  t.integrals.push_back({1, p1, -1, 0, +1, 1, 0, 1, -1.0, -1.0});
}

// x > p1 ? p0 * x : p0 + x, one recording per outcome
void build_branch(TapeBuilder& t, bool taken) {
  const int p0 = t.add(0, GFH_PARAM, 0), p1 = t.add(0, GFH_PARAM, 1), x = t.add(0, GFH_X, -1, -1, GFH_F_REAL);
  t.add(0, GFH_GUARD_GT, x, p1, taken ? GFH_F_TAKEN : 0);
  t.results[0] = t.add(0, taken ? GFH_MUL : GFH_ADD, p0, x);
}

// the default unit and the finite-difference unit of a model
void generate_both(const Model& m, const std::vector<int32_t>& active, const char* what) {
  for (int fd = 0; fd < 2; fd++) {
    GenConfig cfg; cfg.finite_diff = fd != 0;
    std::string src, err;
    expect(generate_source(m, active, cfg, &src, &err) && !src.empty() && src.find("gfh_point_grad") != std::string::npos, what);
    if (!err.empty()) printf("%s: %s\n", what, err.c_str());
  }
}

}  // namespace

int main() {
  std::string err, src;
  TapeBuilder elementals; build_elementals(elementals);
  Model m1;
  expect(m1.load(elementals.finish(3), &err), "load: elementals");
  generate_both(m1, {0, 2}, "elementals");
  {
    GenConfig cfg; cfg.batch = true; cfg.batch_lanes = 64;
    expect(generate_source(m1, {0, 2}, cfg, &src, &err) && src.find("gfh_k_fit_batch") != std::string::npos, "elementals: batch at 64 lanes");
    err.clear();
    expect(!generate_source(m1, {0, 3}, GenConfig(), &src, &err) && err == "active parameter out of range", "refusal: active parameter out of range");
  }
  TapeBuilder integral; build_integral(integral);
  Model m2;
  expect(m2.load(integral.finish(2), &err), "load: integral");
  generate_both(m2, {1}, "integral");
  expect(mesh_sites(m2) == 1 && unit_takes_mesh_args(m2, GenConfig()) && !unit_carries_omega_jt(m2, GenConfig(), 1), "integral: host contracts");
  {
    GenConfig cfg; cfg.batch = true;
    err.clear();
    expect(!generate_source(m2, {1}, cfg, &src, &err) && err.find("batch kernels") == 0, "refusal: batch with an integral");
  }
  TapeBuilder taken, not_taken; build_branch(taken, true); build_branch(not_taken, false);
  const gfh_tape* both[2] = {taken.finish(2), not_taken.finish(2)};
  Model m3;
  expect(m3.load_variants(2, both, -1, &err), "load: two variants");
  expect(m3.n_variants() == 2 && !m3.needs_hint(), "two variants: one guard, no fork");
  generate_both(m3, {0, 1}, "two variants");
  if (failures == 0) printf("ok\n");
  return failures == 0 ? 0 : 1;
}
