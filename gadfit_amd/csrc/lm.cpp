// lm.cpp -- the Levenberg-Marquardt driver gadf_fit (gadfit.F90:502-1035) on the host,
// requesting sweeps from the device.  By north_star the damped normal-equation solve and the
// lambda logic stay on the host; they are restated exactly because they decide which device
// passes are requested.  Host work per iteration is O(dim^3) on a
// dim x dim matrix; everything N-sized lives in HBM behind gfh_sweep/gfh_chi2/gfh_omega.
// This file is the driver only: the solve is normal_eq.cpp, the option defaults are lm_options.h.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "context.h"
#include "group.h"
#include "lm_options.h"
#include "normal_eq.h"

using namespace gfh;

namespace {

const char* const kNotPositiveDefinite = "Cholesky factorization failed (dpotrf).";

double ipow(double x, int n) {   // x**n with integer n, as the Fortran intrinsic
  if (n == 0) return 1.0;
  unsigned m = n < 0 ? (unsigned)(-(long)n) : (unsigned)n;
  double r = 1.0, b = x;
  while (m) { if (m & 1u) r *= b; m >>= 1; if (m) b *= b; }
  return n < 0 ? 1.0 / r : r;
}

// ---- the set-up gfh_fit and gfh_lm_iterate share ------------------------------------------------------------------------------------

// Device group: the whole LM loop runs on every member's thread, as on every coarray image of the reference (the sums are identical
// bits on all members, so the replicated host logic takes the same path), each member on its own copy of the parameter block;
// member 0 answers.
struct Members {
  int n = 0; size_t np = 0;
  std::vector<std::vector<double>> pars;
  int begin(gfh_ctx* c, const char* who, const double* p) {
    n = group_size(c);
    gfh_ctx* k0 = group_member(c, 0);
    if (!k0->has_model || !k0->nd) return fail(c, std::string(who) + ": model and data must be set first");
    np = (size_t)k0->nd * k0->model.n_pars;
    pars.assign((size_t)n, std::vector<double>(p, p + np));
    return 0;
  }
  template <class Call> int run(gfh_ctx* c, double* p, Call call) {      // call(member context, member index, its parameter block)
    const int rc = group_run(c, [&](gfh_ctx* k, int q) -> int { return call(k, q, pars[(size_t)q].data()); });
    memcpy(p, pars[0].data(), sizeof(double) * np);
    return rc;
  }
};

// The argument checks of one member's call, in the order both entry points make them; `own_refusal` words what the entry point
// itself refuses about its arguments (nullptr: nothing) and runs before active[] is read.
template <class Own> int check_call(gfh_ctx* c, const char* who, int na, const int32_t* active, Own own_refusal) {
  if (c->device < 0) return fail(c, "no GPU bound to this context (libgadfit_hip has no CPU fallback)");
  if (!c->has_model || !c->nd) return fail(c, std::string(who) + ": model and data must be set first");
  if (const char* refusal = own_refusal()) return fail(c, refusal);
  for (int j = 0; j < na; j++)          // active[] indexes is_global[] and the parameter block: checked before anything reads through it
    if (active[j] < 0 || active[j] >= c->model.n_pars) return fail(c, std::string(who) + ": active parameter index out of range");
  return 0;
}

// The state of a fit on the host: the parameter block and its column map, the images of the device passes, the steps.
struct Fit {
  double* pars; int na, np, nd, dim;
  const int32_t* active; std::vector<int32_t> jac;
  ZVec JTJ, nextJTJ;                          // dense dim x dim images (nextJTJ: the look-ahead sweep's at the trial point)
  std::vector<double> JTres, DTD, delta1, delta2, old_delta1, JTomega, old_pars;
  std::vector<double> nextJTres;
  DampedSolver solver;

  // what every loop needs: the column map (gadfit.F90:615-631), the solver for it, the first image and step, the saved parameters
  void init(const gfh_ctx* c, double* pars_, int na_, const int32_t* active_, const int32_t* is_global) {
    pars = pars_; na = na_; np = c->model.n_pars; nd = c->nd; active = active_;
    jac.resize((size_t)nd * na);
    dim = gfh_jacobian_indices(nd, na, active, is_global, jac.data());
    solver.setup(nd, na, jac.data(), dim);
    zero_image(JTJ, (size_t)dim * dim); JTres.assign(dim, 0); delta1.assign(dim, 0);
    old_pars.assign((size_t)na * nd, 0);
  }
  void lookahead_images() { zero_image(nextJTJ, (size_t)dim * dim); nextJTres.assign(dim, 0); }
  double dtd(const std::vector<double>& a, const std::vector<double>& b) const {
    double s = 0; for (int i = 0; i < dim; i++) s += a[i] * (DTD[i] * b[i]); return s;   // dot(a, matmul(DTD,b)), DTD diagonal
  }
  void restore() { for (int d = 0; d < nd; d++) for (int j = 0; j < na; j++) pars[d * np + active[j]] = old_pars[d * na + j]; }
  void save() { for (int d = 0; d < nd; d++) for (int j = 0; j < na; j++) old_pars[d * na + j] = pars[d * np + active[j]]; }
  void step(const std::vector<double>& delta) {                                                       // pars += delta, per dataset
    for (int d = 0; d < nd; d++) for (int j = 0; j < na; j++) pars[d * np + active[j]] += delta[jac[d * na + j]];
  }
};

// delta1 = (JTJ + lambda DTD)^-1 JTres (gadfit.F90:711-713); the factor stays in the solver for a second right-hand side
int solve_delta1(gfh_ctx* c, Fit& f, double lambda) {
  if (f.solver.factor(f.JTJ.data(), f.DTD.data(), lambda)) return fail(c, kNotPositiveDefinite);
  f.solver.solve(f.JTres.data(), f.delta1.data());
  return 0;
}

// Look-ahead (gadfit_hip.h, gfh_set_lookahead): the fused sweep already returns sum r^2, so the
// FIRST trial chi2() of an iteration (gadfit.F90:753) is taken from a sweep at the trial point;
// when the step is accepted that sweep IS the next iteration's STEP 1+2 (same parameters, same
// kernel, same numbers), so an accepted iteration costs one N-sized pass instead of two.
// Admitted only where the sweep's sum r^2 is bitwise what chi2() returns at the same parameters: the fused kernel (same
// partition and order of additions as gfh_k_chi2) with shared reciprocals (GADFIT_HIP_FAST_DIV=0 keeps the reference's
// two division forms, whose values differ by rounding between the active and the passive evaluation), and not under a robust loss
// (STEP 1 scales the residuals, chi2() does not).  Read after gfh_set_active: the answer depends on the kernels of the active set.
bool lookahead_admitted(const gfh_ctx* c) {
  return c->lookahead != 0 && c->gen.loss == 0 && sweep_chi2_is_bitwise(c) && c->gen.fast_div;
}

// WHEN to speculate is a prediction -- whichever kernel runs, the trial chi2 is the same bits -- and a wrong one costs a sweep
// thrown away (sweep - chi2(): 0.36 ms at the headline size, what four right ones save).  Round 6:
//   * the first iteration of a fit has no history: it speculates where the first step is substantially damped (lambda >= 0.1; the
//     reference's default is 1) and runs the reference's schedule where the caller asks for a near Gauss-Newton first step;
//   * later iterations speculate iff the previous iteration accepted its first trial (after a rejected first trial the next
//     iteration runs the reference's schedule, chi2 kernel first) ...
//   * ... and lambda is not at or below a level rejected within the last 4 iterations: the usual end state of the plain
//     lambda/10 - lambda*10 rule alternates "accepted at L, rejected at L/10, accepted at L", and that rejection is known ahead.
// bench.py's rejecting_fit leg (40 %-off start, lambda0 = 1e-6): no sweep thrown away, the reference's schedule pass for pass;
// the headline fits (all first trials accepted): one N-sized pass per iteration as before.
struct LookAheadPredictor {
  bool prev_first_accepted = true;
  double lam_rej = -1.0; int rej_age = 1 << 20;      // the largest lambda rejected by the last iteration that rejected any, and how long ago
  bool predicts_accept(int iterations, double lambda) const {
    return iterations == 0 ? lambda >= 0.1 : prev_first_accepted && !(rej_age <= 4 && lambda <= lam_rej * (1.0 + 1e-9));
  }
  // largest_lambda_rejected: of the trials this iteration rejected; negative where it rejected none
  void end_iteration(bool first_accepted, double largest_lambda_rejected) {
    prev_first_accepted = first_accepted;
    if (largest_lambda_rejected >= 0.0) { lam_rej = largest_lambda_rejected; rej_age = 0; } else if (rej_age < (1 << 20)) rej_age++;
  }
};

// ---- the lambda policies of STEP 4 --------------------------------------------------------------------------------------------------
// umnigh_a is the SAVEd local of gadfit.F90:515: the caller carries it from fit to fit (gfh_fit_options::umnigh_a).

double lambda_after_accept(const LmOptions& lo, const Fit& f, double lambda, double old_chi2, double new_chi2, double beta, double& umnigh_a) {
  const int dim = f.dim;
  const double umnigh_m = std::exp(-0.2);
  if (lo.policy & kLambdaNielsen) {                                                             // gadfit.F90:762-767
    double q = 0;
    for (int col = 0; col < dim; col++) {
      double s = 0;
      for (int k = 0; k < dim; k++) s += (f.JTJ[(size_t)k * dim + col] + (k == col ? lambda * f.DTD[col] : 0.0)) * f.delta1[k];
      q += f.delta1[col] * s;
    }
    const double rho = (old_chi2 - new_chi2) / 2 / q;
    const double t = 1 - ipow(2 * rho - 1, 3), lo_ = 1 / lo.lam_down;
    lambda = lambda * (lo_ > t ? lo_ : t);
  }
  if (lo.policy & kLambdaUmnigh) {                                                              // gadfit.F90:768-779
    if (new_chi2 < old_chi2 && beta >= 0.0) {
      umnigh_a = umnigh_a * umnigh_m + 1.0 - umnigh_m;
      double t = ipow(1.0 - std::fabs(2.0 * umnigh_a - 1.0), 2);
      t = t > 1e-2 ? t : 1e-2; t = t < 1.0 ? t : 1.0;
      lambda = lambda * t;
    } else {
      umnigh_a = umnigh_a * umnigh_m + (1.0 - umnigh_m) / 2.0;
      if (new_chi2 >= old_chi2) {
        double t = 1.0 - std::fabs(2.0 * umnigh_a - 1.0);
        t = t > 1.0 ? t : 1.0; t = t < 10.0 ? t : 10.0;
        lambda = lambda / t;
      }
    }
  }
  if (lo.policy == kLambdaPlain) lambda = lambda / lo.lam_down;                                 // gadfit.F90:780-782
  return lambda;
}

double lambda_after_reject(const LmOptions& lo, double lambda, double beta, double& umnigh_a) {   // gadfit.F90:785-808
  const double umnigh_m = std::exp(-0.2);
  if (lo.policy & kLambdaUmnigh) {
    umnigh_a = umnigh_a * umnigh_m;
    double t = 1.0 - std::fabs(2.0 * umnigh_a - 1.0);
    if (beta < 0.0) { t = t * t; t = t > 1e-2 ? t : 1e-2; } else { t = t > 0.1 ? t : 0.1; }
    t = t < 1.0 ? t : 1.0;
    return lambda * t;
  }
  return lo.lam_up * lambda;
}

// ---- STEP 5 (gadfit.F90:835-915): the exit tests in the reference's order.  *exit_reason stays as it is where the fit goes on;
// the return value is an error of gfh_aux.  The grad_chi2 test leaves the device's J^T res in f.JTres, as the reference does.
int exit_test(gfh_ctx* c, const gfh_fit_options* o, Fit& f, const int32_t* is_global, double dof, double old_chi2, double old_old_chi2,
              int iterations, int* exit_reason) {
  const int dim = f.dim, na = f.na;
  const double* pars = f.pars; const int32_t* active = f.active;
  if (o->has_chi2_abs && old_chi2 / dof < o->chi2_abs) { *exit_reason = 1; return 0; }
  if (o->has_chi2_rel && (old_old_chi2 - old_chi2) / old_chi2 < o->chi2_rel) { *exit_reason = 2; return 0; }
  if (o->has_grad_chi2) {                                                                         // gadfit.F90:848-860
    std::vector<double> g(dim);
    if (gfh_aux(c, 0, nullptr, g.data())) return 1;
    f.JTres = g;
    double s = 0; for (double v : g) s += v * v;
    if (2 * std::sqrt(s) < o->grad_chi2) { *exit_reason = 3; return 0; }
  }
  if (o->has_cos_phi) {                                                                           // gadfit.F90:861-884
    double s3[3];
    if (gfh_aux(c, 1, f.delta1.data(), s3)) return 1;
    if (std::fabs(s3[0]) / std::sqrt(s3[1]) / std::sqrt(s3[2]) < o->cos_phi) { *exit_reason = 4; return 0; }
  }
  if (o->has_rel_error) {                                                                         // gadfit.F90:885-898
    bool all = true;
    for (int d = 0; d < f.nd && all; d++) for (int j = 0; j < na; j++)
      if (std::fabs(f.delta1[f.jac[d * na + j]] / pars[d * f.np + active[j]]) > o->rel_error) { all = false; break; }
    if (all) { *exit_reason = 5; return 0; }
  }
  if (o->has_rel_error_global) {                                                                  // gadfit.F90:899-910
    bool any = false;
    for (int j = 0; j < na; j++)
      if (is_global[active[j]] && std::fabs(f.delta1[f.jac[j]] / pars[active[j]]) > o->rel_error_global) any = true;
    if (!any) { *exit_reason = 6; return 0; }
  }
  if (o->has_max_iter && iterations >= o->max_iter) { *exit_reason = 0; return 0; }               // gadfit.F90:911-915
  return 0;
}

// ---- the two debug outputs (the environment is read once per fit) -------------------------------------------------------------------

// GADFIT_HIP_DUMP_FIRST_PASS=<file>: J^T J, J^T r and chi2 of the FIRST pass of this fit (the start parameters: no solve and no
// accept / reject has touched them, so they compare with the oracle free of the fit's conditioning -- tests/test_gpu_fortran_fuzz.py),
// written by rank 0 with 17 digits; every later fit of the process appends.
void dump_first_pass(const char* path, const Fit& f, double chi2) {
  FILE* fh = fopen(path, "a");
  if (!fh) return;
  const int dim = f.dim;
  fprintf(fh, "first_pass dim %d chi2 %.17g\nJTres", dim, chi2);
  for (int j = 0; j < dim; j++) fprintf(fh, " %.17g", f.JTres[(size_t)j]);
  fprintf(fh, "\nJTJ");
  for (size_t j = 0; j < (size_t)dim * dim; j++) fprintf(fh, " %.17g", f.JTJ[j]);
  fprintf(fh, "\n");
  fclose(fh);
}
// GADFIT_HIP_TRACE_SUMS (debugging): what the iteration's pass returned, and every trial of it
void trace_pass(const Fit& f, int iteration, double chi2, double lambda) {
  const int dim = f.dim;
  fprintf(stderr, "iteration %d: chi2 %.17g  JTres", iteration, chi2);
  for (int j = 0; j < dim && j < 8; j++) fprintf(stderr, " %.10g", f.JTres[(size_t)j]);
  fprintf(stderr, "  JTJ");
  for (int j = 0; j < dim && j < 4; j++) for (int k = 0; k < dim && k < 4; k++) fprintf(stderr, " %.10g", f.JTJ[(size_t)j * dim + k]);
  fprintf(stderr, "  lambda %.6g\n", lambda);
}
void trace_trial(const Fit& f, int trial, bool from_sweep, double lambda, double chi2) {
  fprintf(stderr, "  trial %d (%s): lambda %.6g  chi2 %.17g  active parameters of dataset 1:", trial, from_sweep ? "sweep" : "chi2", lambda, chi2);
  for (int j = 0; j < f.na && j < 8; j++) fprintf(stderr, " %.17g", f.pars[f.active[j]]);
  fprintf(stderr, "\n");
}

// What a fit leaves behind on every way out, once armed: the context's per-fit switches back at rest, the result fields filled in.
struct FitScope {
  gfh_ctx* c; gfh_fit_result* r;
  const int& iterations; const double& lambda; const double& old_chi2;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  ~FitScope() {
    c->jtj_prezeroed = false; c->defer.fit = 0; c->defer.store_next = true;
    r->iterations = iterations; r->lambda = lambda; r->chi2 = old_chi2;
    r->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
};

}  // namespace

extern "C" int gfh_potr(int n, double* a, double* b) {
  if (potrf_upper(n, a)) { set_global_error(kNotPositiveDefinite); return 1; }
  potrs_upper(n, a, b);
  return 0;
}

// The damped solve exactly as gfh_fit performs it (host only; tests and callers with their own LM loop).
extern "C" int gfh_solve_damped(int n_datasets, int n_act, const int32_t* jac_idx, int dim, const double* JTJ,
                                const double* DTD, double lambda, const double* rhs, double* out, int use_structure) {
  if (n_datasets < 1 || n_act < 1 || dim < 1 || !jac_idx || !JTJ || !DTD || !rhs || !out) { set_global_error("gfh_solve_damped: bad arguments"); return 1; }
  for (size_t i = 0; i < (size_t)n_datasets * n_act; i++)
    if (jac_idx[i] < 0 || jac_idx[i] >= dim) { set_global_error("gfh_solve_damped: Jacobian index out of range"); return 1; }
  DampedSolver solver;
  solver.setup(n_datasets, n_act, jac_idx, dim, use_structure != 0);
  if (solver.factor(JTJ, DTD, lambda)) { set_global_error(kNotPositiveDefinite); return 1; }
  std::vector<double> x(dim);                     // (out may be rhs)
  solver.solve(rhs, x.data());
  memcpy(out, x.data(), sizeof(double) * dim);
  return 0;
}

extern "C" int gfh_fit(gfh_ctx* c, double* pars, int na, const int32_t* active, const int32_t* is_global,
                       gfh_fit_options* o, gfh_fit_result* r) {
  if (!c) return 1;
  if (c->grp) {
    Members m;
    if (m.begin(c, "gfh_fit", pars)) return 1;
    gfh_fit_options dflt; memset(&dflt, 0, sizeof dflt); dflt.umnigh_a = 0.5;
    std::vector<gfh_fit_options> O((size_t)m.n, o ? *o : dflt);
    std::vector<gfh_fit_result> R((size_t)m.n);
    for (int q = 1; q < m.n; q++) O[(size_t)q].verbosity = 0;                // one image prints (gadfit.F90:886)
    const int rc = m.run(c, pars, [&](gfh_ctx* k, int q, double* p) {
      return gfh_fit(k, p, na, active, is_global, &O[(size_t)q], &R[(size_t)q]); });
    if (o) o->umnigh_a = O[0].umnigh_a;
    if (r) *r = R[0];
    return rc;
  }
  if (check_call(c, "gfh_fit", na, active, [&]() -> const char* {
        if (na < 1) return "There are no active parameters.";                                        // gadfit.F90:602-603
        if (!pars || !active || !is_global) return "gfh_fit: null argument";
        if (na > c->model.n_pars) return "gfh_fit: more active parameters than the model has";
        return nullptr; })) return 1;
  gfh_fit_options defaults; memset(&defaults, 0, sizeof defaults); defaults.umnigh_a = 0.5;
  if (!o) o = &defaults;
  gfh::Range range("gadfit gfh_fit");
  LmOptions lo;                                                                                       // gadfit.F90:568-584
  if (const char* refusal = resolve_lm_options(*o, &lo)) return fail(c, refusal);
  double lambda = lo.lambda;
  const int lam_incs = lo.lam_incs;
  const char* const dump_path = c->rank == 0 ? getenv("GADFIT_HIP_DUMP_FIRST_PASS") : nullptr;
  const bool trace = getenv("GADFIT_HIP_TRACE_SUMS") != nullptr;

  Fit f; f.init(c, pars, na, active, is_global);
  const int dim = f.dim;
  f.DTD.assign(dim, 0); f.delta2.assign(dim, 0); f.old_delta1.assign(dim, 0); f.JTomega.assign(dim, 0);
  if (o->DTD_min) for (int i = 0; i < dim; i++) f.DTD[i] = o->DTD_min[i];                           // gadfit.F90:641-646
  long long dof_ll = (long long)c->n_total - dim;                                                    // gadfit.F90:648-657
  if (dof_ll < 0) return fail(c, "More independent fitting parameters than data points.");
  const double dof = dof_ll == 0 ? 1.0 : (double)dof_ll;
  f.save();
  gfh_fit_result local; if (!r) r = &local;
  memset(r, 0, sizeof *r); r->dim = dim; r->exit_reason = -1;
  r->dof = dof_ll == 0 ? 1 : (dof_ll > 2147483647LL ? 2147483647 : (int)dof_ll);      // (the fit itself uses the 64-bit count)
  int iterations = 0;
  double old_chi2 = 0, new_chi2 = 0, old_old_chi2 = 0, acc_ratio = 0, beta = 0, sweep_chi2 = 0;
  // f.JTJ / f.nextJTJ start as zeros and are only ever written by gfh_sweep with this fit's pattern: the
  // pattern-only transfer of global fits need not clear them again
  c->jtj_prezeroed = true;
  FitScope scope{c, r, iterations, lambda, old_chi2};        // from here on every return resets the context and fills the result
  // keep_jacobian = 2: J goes to HBM only if this fit reads it back (the grad_chi2 / cos_phi tests, and
  // STEP 3's J^T omega where gfh_k_omega_jt is not available: models with integrate(), robust losses); the fused kernel forms J^T J / J^T r from registers either way
  const bool reads_j = (lo.use_accth && omega_needs_jacobian(c, na)) || lo.reads_device_j;
  if (c->keep_jacobian == 2) {
    set_store_j(c, reads_j);
    set_store_res(c, lo.reads_device_j);
  }
  if (gfh_set_active(c, active, na, f.jac.data(), dim)) return 1;
  // adaptive parallelism (load_balancing, gadfit.F90:672-673): the ranges may be re-cut before an iteration, so no sweep is handed over
  const bool balancing = c->bal.on && c->nranks > 1;
  // keep_jacobian = 1 promises that J of the most recent sweep can be read once the fit has returned; until then every sweep
  // overwrites what the one before it wrote and -- with the fused kernel and options that do not read J -- nobody looks at it.  Such a
  // fit's sweeps skip the store (context.h, Deferred) unless max_iter guarantees that no later sweep of this fit can follow them:
  // the sweep handed to, or made by, the last permitted iteration, and the look-ahead sweep that would be handed to it.  A fit
  // that ends any other way owes J (materialise_jacobian).  (A parameter hook may upload columns that belong to the parameters of
  // a pass: a pass repeated later would not find them, so such fits store as before.)
  const bool defer = c->defer.on && c->keep_jacobian == 1 && c->gen.store_j && uses_fused_kernel(c) && !reads_j && !balancing && !c->pars_fn &&
                     sizeof(double) * (size_t)na * (size_t)std::max<int64_t>(1, c->ldj) >= c->defer.from;
  c->defer.fit = defer ? 2 : 1;
  auto last_permitted = [&](int iteration) { return o->has_max_iter && iteration >= o->max_iter; };   // (1-based; the loop runs once whatever max_iter says)
  // Look-ahead: off when the convergence tests read the device J/res pair the reference has at that point (old J, new res:
  // gadfit.F90:849-850, 865-873), and under adaptive parallelism (the ranges may be re-cut before an iteration, so no sweep is handed over)
  const bool la_ok = lookahead_admitted(c) && !lo.reads_device_j && !balancing;
  LookAheadPredictor predictor;
  bool have_next = false;                       // the look-ahead sweep of an accepted first trial waits in f.nextJTJ / f.nextJTres
  if (la_ok) f.lookahead_images();
  // old_chi2 = chi2() before the loop (gadfit.F90:670).  With look-ahead the first STEP 1+2 pass -- same
  // parameters -- returns that sum r^2 itself and is handed to the first iteration: one N-sized pass less per fit.
  if (la_ok) {
    c->defer.store_next = last_permitted(1);
    if (gfh_sweep(c, pars, active, na, f.jac.data(), dim, f.nextJTJ.data(), f.nextJTres.data(), &old_chi2)) return 1;
    have_next = true; r->n_lookahead++;
  } else if (gfh_chi2(c, pars, &old_chi2)) return 1;
  r->n_chi2++;
  for (;;) {
    if (balancing && iterations > 0 && gfh_rebalance(c, nullptr)) return 1;                         // re_initialize, gadfit.F90:672-673
    // STEP 1 + 2 (gadfit.F90:675-701): the sweep handed over by the iteration before, or a new one
    if (have_next) { f.JTJ.swap(f.nextJTJ); f.JTres.swap(f.nextJTres); have_next = false; }
    else {
      c->defer.store_next = last_permitted(iterations + 1);
      if (gfh_sweep(c, pars, active, na, f.jac.data(), dim, f.JTJ.data(), f.JTres.data(), &sweep_chi2)) return 1;
    }
    r->n_sweeps++;
    for (int i = 0; i < dim; i++) {                                                                 // gadfit.F90:702-710
      const double d = f.JTJ[(size_t)i * dim + i];
      if (lo.damp_plain) f.DTD[i] = d; else f.DTD[i] = f.DTD[i] > d ? f.DTD[i] : d;
    }
    if (dump_path && iterations == 0) dump_first_pass(dump_path, f, old_chi2);
    if (trace) trace_pass(f, iterations + 1, old_chi2, lambda);
    if (solve_delta1(c, f, lambda)) return 1;                                                       // gadfit.F90:711-713
    if (lo.use_accth) {                                                                             // STEP 3, gadfit.F90:715-743
      if (gfh_omega(c, pars, f.delta1.data(), f.JTomega.data())) return 1;
      r->n_omega++;
      f.solver.solve(f.JTomega.data(), f.delta2.data());                                              // gadfit.F90:736-738
      acc_ratio = std::sqrt(f.dtd(f.delta2, f.delta2) / f.dtd(f.delta1, f.delta1));
      if (acc_ratio > o->accth) std::fill(f.delta2.begin(), f.delta2.end(), 0.0);
    }
    for (int d = 0; d < f.nd; d++) for (int j = 0; j < na; j++) {                                   // gadfit.F90:745-750
      double& p = pars[d * f.np + active[j]];
      p = p + f.delta1[f.jac[d * na + j]] + 0.5 * f.delta2[f.jac[d * na + j]];
    }
    bool quit = false;
    bool first_accepted = false;
    double iter_lam_rej = -1.0;                   // (largest lambda whose trial this iteration rejected)
    for (int i = 1; i <= lam_incs + 1; i++) {                                                       // STEP 4, gadfit.F90:752-819
      // no look-ahead in the iteration that max_iter ends anyway (its Jacobian would not be used)
      const bool spec = la_ok && i == 1 && predictor.predicts_accept(iterations, lambda) && !(o->has_max_iter && iterations + 1 >= o->max_iter);
      const double lambda_of_trial = lambda;
      if (spec) {
        c->defer.store_next = last_permitted(iterations + 2);          // (handed to the next iteration if this trial is accepted)
        if (gfh_sweep(c, pars, active, na, f.jac.data(), dim, f.nextJTJ.data(), f.nextJTres.data(), &new_chi2)) return 1;
        r->n_lookahead++;
      } else if (gfh_chi2(c, pars, &new_chi2)) return 1;
      r->n_chi2++;
      if (trace) trace_trial(f, i, spec, lambda, new_chi2);
      if (iterations == 0) beta = 0.0;
      else beta = f.dtd(f.delta1, f.old_delta1) / std::sqrt(f.dtd(f.delta1, f.delta1)) / std::sqrt(f.dtd(f.old_delta1, f.old_delta1));
      if (ipow(1.0 - beta, lo.uphill) * new_chi2 < old_chi2) {                                      // accepted, gadfit.F90:761-783
        lambda = lambda_after_accept(lo, f, lambda, old_chi2, new_chi2, beta, o->umnigh_a);
        have_next = spec; first_accepted = i == 1;
        break;
      } else if (i <= lam_incs) {                                                                   // rejected, retried: gadfit.F90:785-808
        iter_lam_rej = iter_lam_rej > lambda_of_trial ? iter_lam_rej : lambda_of_trial;
        lambda = lambda_after_reject(lo, lambda, beta, o->umnigh_a);
        f.restore();
        if (solve_delta1(c, f, lambda)) return 1;
        f.step(f.delta1);
      } else {                                                                                      // rejected for the last time: gadfit.F90:809-816
        f.restore();
        if (o->verbosity) printf(" Lambda increased %d times in a row.\n", lam_incs + 1);
        r->exit_reason = 7; quit = true; break;
      }
    }
    if (quit) break;
    predictor.end_iteration(first_accepted, iter_lam_rej);
    f.save();                                                                                       // gadfit.F90:821-827
    f.old_delta1 = f.delta1;
    old_old_chi2 = old_chi2;
    old_chi2 = old_chi2 < new_chi2 ? old_chi2 : new_chi2;
    iterations++;
    if (o->verbosity) printf(" iteration %d  lambda %.6g  chi2/DOF %.15g\n", iterations, lambda, new_chi2 / dof);
    // STEP 5 (gadfit.F90:835-915)
    if (exit_test(c, o, f, is_global, dof, old_chi2, old_old_chi2, iterations, &r->exit_reason)) return 1;
    if (r->exit_reason >= 0) break;
  }
  return 0;
}


// n_iter iterations of the basic scheme with no convergence exits (see gadfit_hip.h).
extern "C" int gfh_lm_iterate(gfh_ctx* c, double* pars, int na, const int32_t* active, const int32_t* is_global,
                              int n_iter, double* state3, double* DTD) {
  if (!c) return 1;
  if (c->grp) {
    Members m;
    if (m.begin(c, "gfh_lm_iterate", pars)) return 1;
    gfh_ctx* k0 = group_member(c, 0);
    std::vector<int32_t> jtmp((size_t)k0->nd * na);
    const int gdim = gfh_jacobian_indices(k0->nd, na, active, is_global, jtmp.data());
    std::vector<std::vector<double>> S((size_t)m.n, std::vector<double>(state3, state3 + 3));
    std::vector<std::vector<double>> D((size_t)m.n, std::vector<double>(DTD, DTD + gdim));
    const int rc = m.run(c, pars, [&](gfh_ctx* k, int q, double* p) {
      return gfh_lm_iterate(k, p, na, active, is_global, n_iter, S[(size_t)q].data(), D[(size_t)q].data()); });
    memcpy(state3, S[0].data(), sizeof(double) * 3);
    memcpy(DTD, D[0].data(), sizeof(double) * gdim);
    return rc;
  }
  if (check_call(c, "gfh_lm_iterate", na, active, [&]() -> const char* {
        return na < 1 || na > c->model.n_pars || !pars || !active || !is_global || !state3 || !DTD ? "gfh_lm_iterate: bad arguments" : nullptr; })) return 1;
  Fit f; f.init(c, pars, na, active, is_global);
  const int dim = f.dim;
  f.DTD.assign(DTD, DTD + dim);
  f.lookahead_images();
  double lambda = state3[0], old_chi2 = state3[1], sweep_chi2 = 0, new_chi2 = 0;
  if (gfh_set_active(c, active, na, f.jac.data(), dim)) return 1;
  if (old_chi2 < 0 && gfh_chi2(c, pars, &old_chi2)) return 1;
  // look-ahead as in gfh_fit: the trial chi2 is the sum r^2 of a sweep at the trial point, which
  // an accepted step hands to the next iteration.  The hand-over does not cross calls: the first
  // iteration of every call sweeps, and a look-ahead of the last iteration is not started.
  const bool la_ok = lookahead_admitted(c);
  bool la_armed = la_ok, have_next = false;
  for (int it = 0; it < n_iter; it++) {
    f.save();
    if (have_next) { f.JTJ.swap(f.nextJTJ); f.JTres.swap(f.nextJTres); have_next = false; }
    else if (gfh_sweep(c, pars, active, na, f.jac.data(), dim, f.JTJ.data(), f.JTres.data(), &sweep_chi2)) return 1;
    for (int i = 0; i < dim; i++) { const double d = f.JTJ[(size_t)i * dim + i]; f.DTD[i] = f.DTD[i] > d ? f.DTD[i] : d; }
    if (solve_delta1(c, f, lambda)) return 1;
    f.step(f.delta1);
    const bool spec = la_armed && it + 1 < n_iter;
    if (spec) { if (gfh_sweep(c, pars, active, na, f.jac.data(), dim, f.nextJTJ.data(), f.nextJTres.data(), &new_chi2)) return 1; }
    else if (gfh_chi2(c, pars, &new_chi2)) return 1;
    if (new_chi2 < old_chi2) { old_chi2 = new_chi2; lambda /= 10.0; state3[2] += 1.0; have_next = spec; la_armed = la_ok; }
    else { f.restore(); lambda *= 10.0; la_armed = false; }
  }
  state3[0] = lambda; state3[1] = old_chi2;
  for (int i = 0; i < dim; i++) DTD[i] = f.DTD[i];
  return 0;
}
