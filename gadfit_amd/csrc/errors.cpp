// errors.cpp -- the errors of a plain fit: the parameter covariance (J^T J)^-1 and the standard errors of gfh_fit's path (one fit,
// possibly global over several datasets), LMsolver::getJTJ / getInvJTJ of the reference (lm_solver.cpp:551-585).  One STEP 1 + 2 pass
// through gfh_sweep -- whatever that call carries, this one carries: the pars hook, an unseen path, ranks and device groups, the
// robust loss, finite differences -- and the algebra of normal_eq.cpp on the host; gfh_invert_normal is that algebra without a context.
// Nothing here touches the device itself.
#include <cmath>
#include <cstring>
#include <exception>
#include <new>
#include <vector>
#include "context.h"
#include "group.h"
#include "normal_eq.h"

using namespace gfh;

namespace {

// the dense image a call cannot have is refused under the call's name, not thrown through the C ABI
std::string too_large(const char* who, long long dim) {
  return std::string(who) + ": the dense " + std::to_string(dim) + " x " + std::to_string(dim) + " image of the covariance cannot be allocated";
}

int invert_checked(const char* who, int dim, const double* JTJ, int nd, int na, const int32_t* jac, bool use_structure, double factor,
                   double* cov, double* sigma, int32_t* info, int32_t* form, std::string* err) {
  try {
    DampedSolver solver;
    solver.setup(nd, na, jac, dim, use_structure);
    if (form) *form = solver.arrow() ? 1 : 0;
    *info = solver.invert(JTJ, factor, cov, sigma);
    return 0;
  } catch (const std::bad_alloc&) { *err = too_large(who, dim); return 1; }
}

}  // namespace

extern "C" {

int gfh_invert_normal(int dim, const double* JTJ, int n_datasets, int n_act, const int32_t* jac_idx, int use_structure, double factor,
                      double* cov, double* sigma, int32_t* info, int32_t* form) {
  if (dim < 1 || n_datasets < 1 || n_act < 1 || !JTJ || !jac_idx || !cov || !sigma || !info) { set_global_error("gfh_invert_normal: bad arguments"); return 1; }
  for (size_t i = 0; i < (size_t)n_datasets * n_act; i++)
    if (jac_idx[i] < 0 || jac_idx[i] >= dim) { set_global_error("gfh_invert_normal: Jacobian index out of range"); return 1; }
  std::string err;
  if (invert_checked("gfh_invert_normal", dim, JTJ, n_datasets, n_act, jac_idx, use_structure != 0, factor, cov, sigma, info, form, &err)) {
    set_global_error(err);
    return 1;
  }
  return 0;
}

int gfh_covariance(gfh_ctx* c, const double* pars, int na, const int32_t* active, const int32_t* is_global, int scale, double* cov,
                   double* sigma, int32_t* info) try {
  if (!c) return 1;
  const gfh_ctx* k0 = c->grp ? group_member(c, 0) : c;          // (a device group: its members hold model and data, each its own range)
  if (!pars || !active || !is_global || !cov || !sigma || !info) return fail(c, "gfh_covariance: null argument");
  if (scale != 0 && scale != 1)
    return fail(c, "gfh_covariance: scale is 0 (the inverse of J^T J) or 1 (that times chi2 / dof), got " + std::to_string(scale));
  if (na < 1) return fail(c, "There are no active parameters.");                                       // gadfit.F90:602-603
  if (!k0->has_model) return fail(c, "gfh_covariance: no model set (gfh_set_model)");
  if (na > k0->model.n_pars) return fail(c, "gfh_covariance: more active parameters than the model has");
  for (int j = 0; j < na; j++) {
    if (active[j] < 0 || active[j] >= k0->model.n_pars) return fail(c, "gfh_covariance: active parameter index out of range");
    for (int k = 0; k < j; k++) if (active[k] == active[j]) return fail(c, "gfh_covariance: an active parameter is listed twice");
  }
  if (k0->device < 0) return fail(c, "no GPU bound to this context (libgadfit_hip has no CPU fallback)");
  if (!k0->nd) return fail(c, "gfh_covariance: no data set (gfh_set_data)");
  const int nd = k0->nd;
  std::vector<int32_t> jac((size_t)nd * na);
  const int dim = gfh_jacobian_indices(nd, na, active, is_global, jac.data());
  const long long dof_ll = (long long)k0->n_total - dim;                                              // gadfit.F90:648-657, as gfh_fit
  if (dof_ll < 0) return fail(c, "More independent fitting parameters than data points.");
  const double dof = dof_ll == 0 ? 1.0 : (double)dof_ll;
  ZVec JTJ;
  try { zero_image(JTJ, (size_t)dim * dim); } catch (const std::bad_alloc&) { return fail(c, too_large("gfh_covariance", dim)); }
  std::vector<double> JTres((size_t)dim);
  double chi2 = 0.0, sweep_chi2 = 0.0;
  // chi2 / dof under scale = 1: chi2 is what gfh_chi2 returns at pars.  Where the sweep's sum r^2 is bitwise that value it is taken
  // from the pass and nothing more is launched; elsewhere (a robust loss, whose sweep sums the scaled residuals; the two-kernel
  // paths; GADFIT_HIP_FAST_DIV=0) the chi2 pass runs FIRST, so that what the call leaves on the device is what its sweep left.
  if (scale) {
    if (gfh_set_active(c, active, na, jac.data(), dim)) return 1;
    if (!(k0->gen.loss == 0 && k0->gen.fast_div && sweep_chi2_is_bitwise(k0))) { if (gfh_chi2(c, pars, &chi2)) return 1; }
    else scale = 2;
  }
  if (gfh_sweep(c, pars, active, na, jac.data(), dim, JTJ.data(), JTres.data(), &sweep_chi2)) return 1;
  if (scale == 2) chi2 = sweep_chi2;
  std::string err;
  if (invert_checked("gfh_covariance", dim, JTJ.data(), nd, na, jac.data(), true, scale ? chi2 / dof : 1.0, cov, sigma, info, nullptr, &err))
    return fail(c, err);
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_covariance: ") + e.what()); }

int gfh_fit_errors(gfh_ctx* c, double* pars, int na, const int32_t* active, const int32_t* is_global, gfh_fit_options* o,
                   gfh_fit_result* r, int scale, double* cov, double* sigma, int32_t* info) {
  if (!c) return 1;
  if (!cov || !sigma || !info) return fail(c, "gfh_fit_errors: null argument");
  if (scale != 0 && scale != 1)
    return fail(c, "gfh_fit_errors: scale is 0 (the inverse of J^T J) or 1 (that times chi2 / dof), got " + std::to_string(scale));
  if (gfh_fit(c, pars, na, active, is_global, o, r)) return 1;
  return gfh_covariance(c, pars, na, active, is_global, scale, cov, sigma, info);
}

}  // extern "C"
