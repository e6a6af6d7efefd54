// lm_options.h -- the optional arguments of gadf_fit (gadfit.F90:502-510) resolved once into what a Levenberg-Marquardt loop reads:
// the host loop of gfh_fit (lm.cpp) and the device loop behind gfh_fit_batch (batch_calls.cpp, which refuses what its kernels do not carry
// before it comes here).  The exit tests, accth's value, max_iter and DTD_min are read from gfh_fit_options where they are used.
#pragma once
#include "../../include/gadfit_hip.h"

namespace gfh {

constexpr double kAccthTiny = 1.17549435e-38;   // tiny(1.0) of the reference's real32 accth: STEP 3 runs iff accth > tiny (gadfit.F90:715)

// nielsen and umnigh are independent flags in the reference (gadfit.F90:762-782: both branches run, in that order, where both are
// given), so the policy is a set of bits; 0 is the plain lambda / lam_down - lambda * lam_up rule
enum : unsigned { kLambdaPlain = 0u, kLambdaNielsen = 1u, kLambdaUmnigh = 2u };

struct LmOptions {
  double lambda = 1.0, lam_up = 10.0, lam_down = 10.0;    // gadfit.F90:568-573
  int lam_incs = 2, uphill = 0;                           // gadfit.F90:574-582
  unsigned policy = kLambdaPlain;
  bool use_accth = false;          // STEP 3 (geodesic acceleration) runs
  bool damp_plain = false;         // damp_max = .false.: DTD is the diagonal of this iteration's J^T J (gadfit.F90:702-710)
  bool reads_device_j = false;     // the grad_chi2 / cos_phi tests read J and res from the device (gadfit.F90:849-850, 865-873)
};

// nullptr, or the reference's refusal (gadfit.F90:575-578) for the caller to report
inline const char* resolve_lm_options(const gfh_fit_options& o, LmOptions* out) {
  LmOptions r;
  if (o.has_lambda) r.lambda = o.lambda;
  if (o.has_lam_up) r.lam_up = o.lam_up;
  if (o.has_lam_down) r.lam_down = o.lam_down;
  if (o.has_lam_incs) { if (o.lam_incs < 1) return "Input parameter lam_incs must be at least 1."; r.lam_incs = o.lam_incs; }
  if (o.has_uphill) r.uphill = o.uphill;
  if (o.has_nielsen && o.nielsen) r.policy |= kLambdaNielsen;
  if (o.has_umnigh && o.umnigh) r.policy |= kLambdaUmnigh;
  r.use_accth = o.has_accth && o.accth > kAccthTiny;
  r.damp_plain = o.has_damp_max && !o.damp_max;
  r.reads_device_j = o.has_grad_chi2 || o.has_cos_phi;
  *out = r;
  return nullptr;
}

}  // namespace gfh
