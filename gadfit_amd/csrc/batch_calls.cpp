// batch_calls.cpp -- what is done with the batch a context holds (batch_data.cpp): many Levenberg-Marquardt fits of ONE model in ONE
// kernel launch, each with its own data, start parameters, lambda history and exit (gfh_fit_batch, gfh_fit_batch_errors,
// gfh_fit_batch_bounded: the same loop inside one box per batch, device/batch_fit_bounded.hip, in a unit of its own), and their
// neighbours at given parameters (gfh_batch_pass, gfh_batch_covariance, gfh_batch_eval); gfh_batch_source, gfh_batch_prepare and
// gfh_set_batch_lanes.  The loop itself (gadfit.F90:670-915) is the generated kernel gfh_k_fit_batch (device/batch_fit.hip; codegen.cpp,
// emit_batch_kernels), a wave per fit or -- gfh_set_batch_lanes(16) -- a DPP row of 16 lanes per fit and four fits per wave, or --
// gfh_set_batch_lanes(256) -- a workgroup of four waves per fit.
//
// Every launching call is written in the same steps: check_batchable, its own argument checks, check_held -- everything the kernels
// do not carry is refused there with its own message, before anything touches the device -- then open_device, its blocks, and on the
// one stream: copy down, event, launch_batch (once; twice under gfh_fit_batch_errors), event, copy back, one synchronise.  The blocks
// (context.h, Batch) by call, each the size of the call at hand:
//   gfh_fit_batch         io = [pars n_fits x n_pars | records n_fits], down its head, back whole
//   gfh_fit_batch_errors  io = [pars | records | ErrorBlock], likewise
//   gfh_fit_batch_bounded io = [pars | records | at_bound n_fits], likewise
//   gfh_batch_covariance  io = [pars] down, img = ErrorBlock back
//   gfh_batch_pass        io = [pars] down, img = n_fits records [J^T J na x na | J^T r na | chi2] back
//   gfh_batch_eval        io = [pars | cov | x_eval] of the evaluated fits down, staged in batch.host; img = [model | residual | band],
//                         the requested ones, back
#include "batch_internal.h"
#include "lm_options.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <initializer_list>

using namespace gfh;

namespace {

// layouts shared with the generated source (batch_fit.hip: gfh_batch_opts, gfh_batch_rec)
struct BatchOpts {
  double lambda, lam_up, lam_down, accth, chi2_abs, chi2_rel, rel_error;
  double dtd_min[kValuGramMax];
  int lam_incs, max_iter, has_max_iter, use_accth, has_chi2_abs, has_chi2_rel, has_rel_error, damp_plain;
};
static_assert(sizeof(gfh_batch_result) == 40 && sizeof(BatchOpts) == 7 * 8 + 8 * kValuGramMax + 8 * 4, "layout shared with the generated kernels");

// The auto rule's two numbers: the largest measured spectrum length at which the row form was faster than the wave form, on the same
// card in the same run, by more than the two forms' own min-max spread (profiles/batch_rows.json; 0: nowhere).
// Measured at 4 and at 8 active parameters; 1 ... 4 take the first, 5 ... 8 the second.
constexpr int64_t kRowUpTo4 = 128, kRowUpTo8 = 256;

// The opening of a call, step one: can this context and this model with this active set be batched at all
int check_batchable(gfh_ctx* c, const char* who, int na, const int32_t* active) {
  if (check_context(c, who)) return 1;
  const std::string w(who);
  if (!c->has_model) return fail(c, w + ": no model set (gfh_set_model)");
  if (c->model.has_integrals()) return fail(c, w + ": models with integrate() are not carried by the batch kernels");
  if (c->model.branching()) return fail(c, w + ": models recorded as variant tapes (a branching eval()) are not carried by the batch kernels");
  if (c->model.n_aux > 0) return fail(c, w + ": models with auxiliary per-point columns are not carried by the batch kernels");
  if (c->pars_fn) return fail(c, w + ": a pars hook (gfh_set_pars_hook) cannot run inside a device-resident loop");
  if (c->gen.loss != 0) return fail(c, w + ": a robust loss (gfh_set_loss) is not carried by the batch kernels: a batch takes its loss and residual scale from gfh_set_batch_loss");
  if (c->gen.finite_diff) return fail(c, w + ": use_ad = 0 (finite differences) is not carried by the batch kernels");
  if (c->batch.estimator != 0 && c->batch.loss != 0)
    return fail(c, w + ": the poisson estimator (gfh_set_batch_estimator) together with a batch loss (gfh_set_batch_loss) is not carried: the robust costs are costs of a weighted residual, which the deviance has none of");
  if (na < 1) return fail(c, "There are no active parameters.");                                       // gadfit.F90:602-603
  if (na > kValuGramMax) return fail(c, w + ": more than " + std::to_string(kValuGramMax) + " active parameters per fit");
  if (!active) return fail(c, w + ": null argument");
  if (na > c->model.n_pars) return fail(c, w + ": more active parameters than the model has");
  for (int j = 0; j < na; j++) {
    if (active[j] < 0 || active[j] >= c->model.n_pars) return fail(c, w + ": active parameter index out of range");
    for (int k = 0; k < j; k++) if (active[k] == active[j]) return fail(c, w + ": an active parameter is listed twice");
  }
  return 0;
}
// ... step two, behind the call's own argument checks: is a batch held that na parameters can be fitted to -- every spectrum long
// enough, and of a cube begun by gfh_batch_frames_begin every frame put
int check_held(gfh_ctx* c, const char* who, int na) {
  const std::string w(who);
  if (c->batch.n_fits < 1) return fail(c, w + ": no batch data (gfh_set_batch_data, gfh_set_batch_cube)");
  if (c->batch.min_points < na) return fail(c, "More independent fitting parameters than data points (a fit of the batch has " +
                                              std::to_string((long long)c->batch.min_points) + " points).");      // gadfit.F90:648-657, per fit
  if (c->batch.frames && c->batch.frames_missing != 0)
    return fail(c, w + ": " + std::to_string((long long)c->batch.frames_missing) + " of " + std::to_string((long long)c->batch.max_points) +
                   " frames of the batch begun by gfh_batch_frames_begin have not been put (gfh_batch_frames_put)");
  return 0;
}

// the translation unit of an active set with the four batch kernels: generated, compiled and (load) loaded once per context, kept
// in the context's kernel cache under a key no plain active set has, so that a new model or gfh_destroy releases it with the rest
GenConfig batch_config(const gfh_ctx* c, int lanes, bool bounded) {
  GenConfig cfg;                    // the defaults, not the context's current switches: one form per (model, active set, lanes per fit)
  cfg.fast_div = c->gen.fast_div;
  cfg.batch = true;
  cfg.batch_lanes = lanes;
  cfg.batch_bounded = bounded;      // gfh_k_fit_batch_bounded in place of the four kernels: a unit of its own
  cfg.batch_loss = c->batch.loss;   // gfh_set_batch_loss: the batch's own setting (cfg.loss, the plain units' GFH_LOSS, stays 0); the scale is a kernel argument
  cfg.batch_cube = c->batch.cube;   // the data form held: a cube's sample type and weight rule are part of the text (batch_cube.hip)
  cfg.batch_estimator = c->batch.estimator;      // gfh_set_batch_estimator: likewise part of the text
  if (c->batch.cube) { cfg.batch_y_type = c->batch.y_type; cfg.batch_error_type = c->batch.error_type; }
  return cfg;
}
// the form a call uses: the context's setting, under auto what the rule gives for the geometry held (64 when the context holds none)
int batch_lanes(const gfh_ctx* c, int na) {
  if (c->batch.lanes != 0) return c->batch.lanes;
  return c->batch.n_fits < 1 ? 64 : gfh_batch_auto_lanes(na, c->batch.max_points);
}
int batch_kernels(gfh_ctx* c, const std::vector<int32_t>& active, int lanes, bool bounded, bool load, ModelKernels** out) {
  std::vector<int32_t> key = active;
  key.push_back(bounded ? -(1 << 30) - 2 : -(1 << 30));      // (no plain active set holds a negative entry; an eval unit holds -(1 << 30) - 1 here)
  key.push_back(lanes);             // both forms of one active set can be resident
  if (c->batch.cube) key.push_back(data_form(c));      // ... and so can its cube forms beside the ragged one (whose key stays what it was)
  if (c->batch.loss) key.push_back(-(1 << 29) - c->batch.loss);      // ... and its loss units beside the linear one (no lane count and no data form is negative)
  if (c->batch.estimator) key.push_back(-(1 << 28) - c->batch.estimator);      // ... and its Poisson units beside the least-squares ones
  auto it = c->kernel_cache.find(key);
  if (it != c->kernel_cache.end()) { if (out) *out = &it->second; return 0; }
  std::string src, err;
  if (!generate_source(c->model, active, batch_config(c, lanes, bounded), &src, &err)) return fail(c, err);
  ModelKernels mk;
  const uint64_t skey = load ? source_key(src) : 0;
  if (!(load && acquire_loaded(c->device, skey, &mk))) {
    std::vector<char> code; bool cached = false;
    if (!compile_to_code_object(src, &code, &err, &cached)) return fail(c, err);
    if (!load) return 0;
    if (!load_kernels(code, &mk, &err)) return fail(c, err);
    publish_loaded(c->device, skey, mk);
  }
  if (bounded ? !mk.fit_batch_bounded : !mk.fit_batch || !mk.batch_pass || !mk.batch_cov || !mk.batch_eval) { release_loaded(c->device, &mk); return fail(c, "the batch kernels are missing from their code object"); }
  mk.n_active = (int)active.size();
  ModelKernels* p = &c->kernel_cache.emplace(key, mk).first->second;
  if (out) *out = p;
  return 0;
}

// The device side of a call, opened under the caller's name: the GPU, the batch on it, the lane form and its loaded kernels
struct Opened { ModelKernels* mk = nullptr; int lanes = 0; };
int open_device(gfh_ctx* c, const char* who, int na, const int32_t* active, Opened* k, bool bounded = false) {
  NEED_GPU(c);
  if (!c->batch.on_device) return fail(c, std::string(who) + ": no batch data on the device (gfh_set_batch_data, gfh_set_batch_cube)");
  k->lanes = batch_lanes(c, na);
  return batch_kernels(c, std::vector<int32_t>(active, active + na), k->lanes, bounded, true, &k->mk);
}
// One launch of a batch kernel over n fits of the batch held, on the context's stream: workgroups of 256 threads, 256 / lanes fits
// each.  Every kernel's arguments are the data's four (GFH_BARGS: x, y, w and the offsets -- of a cube, n_points in their place),
// the call's own (`middle`: pointers to them, the kernel's fit count among them), under a loss (gfh_set_batch_loss) inv_c = 1 / scale
// for the kernels that sweep (`sweeps`: all but gfh_k_batch_eval, which the loss does not reach), and the status block.
int launch_batch(gfh_ctx* c, hipFunction_t kernel, int lanes, int64_t n, std::initializer_list<void*> middle, bool sweeps = true) {
  void* x = c->batch.x.p; void* y = c->batch.y.p; void* w = c->batch.w.p; void* off = c->batch.off_d.p;
  long long npts = c->batch.max_points; void* stp = c->status.p;
  double inv_c = 1.0 / c->batch.loss_scale;
  std::vector<void*> args = {&x, &y, &w, c->batch.cube ? (void*)&npts : (void*)&off};
  args.insert(args.end(), middle);
  if (sweeps && c->batch.loss != 0) args.push_back(&inv_c);
  args.push_back(&stp);
  const int per_wg = 256 / lanes;
  HIPCHK(c, hipModuleLaunchKernel(kernel, (unsigned)((n + per_wg - 1) / per_wg), 1, 1, 256, 1, 1, 0, c->stream, args.data(), nullptr));
  c->batch.last_lanes = lanes; c->batch.last_form = data_form(c);
  if (sweeps) { c->batch.last_loss = c->batch.loss; c->batch.last_loss_scale = c->batch.loss_scale; c->batch.last_estimator = c->batch.estimator; }
  return 0;
}

// The error outputs of a call (gfh_batch_covariance, gfh_fit_batch_errors) and their block, on the device as gfh_k_batch_cov
// (batch_cov.hip) writes it and on the host as it comes back: [cov n_fits x na x na | sigma n_fits x na | info n_fits], the ints
// last so that the doubles stay aligned
struct BatchErrors { int scale; double* cov; double* sigma; int32_t* info; };
struct ErrorBlock {
  size_t sigma, info, bytes;          // the offsets of sigma and info (cov is at 0) and the size of the block
  ErrorBlock(int64_t nf, int na) : sigma(sizeof(double) * (size_t)nf * na * na), info(sigma + sizeof(double) * (size_t)nf * na),
                                   bytes(info + sizeof(int32_t) * (size_t)nf) {}
};
int check_errors(gfh_ctx* c, const char* who, const BatchErrors& e) {
  const std::string w(who);
  if (!e.cov || !e.sigma || !e.info) return fail(c, w + ": null argument");
  if (e.scale != 0 && e.scale != 1)
    return fail(c, w + ": scale is 0 (the inverse of J^T J) or 1 (that times chi2 / dof), got " + std::to_string(e.scale));
  return 0;
}
// gfh_k_batch_cov over the batch held at the parameter block `pars` of the device, into the ErrorBlock at `out`
int launch_cov(gfh_ctx* c, const Opened& k, int na, int scale, void* pars, char* out) {
  const ErrorBlock at(c->batch.n_fits, na);
  void* cov = out; void* sigma = out + at.sigma; void* info = out + at.info; long long n = c->batch.n_fits;
  return launch_batch(c, k.mk->batch_cov, k.lanes, n, {&pars, &scale, &cov, &sigma, &info, &n});
}
void errors_out(const char* h, int64_t nf, int na, const BatchErrors& e) {
  const ErrorBlock at(nf, na);
  memcpy(e.cov, h, at.sigma); memcpy(e.sigma, h + at.sigma, at.info - at.sigma); memcpy(e.info, h + at.info, at.bytes - at.info);
}

// the options of gadf_fit as the device loop reads them; what it does not carry is refused
int batch_options(gfh_ctx* c, const std::string& who, const gfh_fit_options* o, int na, BatchOpts* out) {
  gfh_fit_options defaults; memset(&defaults, 0, sizeof defaults);
  if (!o) o = &defaults;
  if (o->has_uphill && o->uphill != 0) return fail(c, who + ": uphill != 0 is not carried by the batch kernel");
  if (o->has_nielsen && o->nielsen) return fail(c, who + ": the nielsen lambda strategy is not carried by the batch kernel");
  if (o->has_umnigh && o->umnigh) return fail(c, who + ": the umnigh lambda strategy is not carried by the batch kernel");
  if (o->has_grad_chi2) return fail(c, who + ": the grad_chi2 test is not carried by the batch kernel");
  if (o->has_cos_phi) return fail(c, who + ": the cos_phi test is not carried by the batch kernel");
  if (o->has_rel_error_global) return fail(c, who + ": rel_error_global has no meaning for independent fits");
  LmOptions lo;
  if (const char* refusal = resolve_lm_options(*o, &lo)) return fail(c, refusal);                        // gadfit.F90:575-578
  if (!o->has_max_iter || o->max_iter < 0) return fail(c, who + ": max_iter is required (a loop that runs on the device must be bounded)");
  if (c->batch.estimator != 0 && lo.use_accth)
    return fail(c, who + ": accth (geodesic acceleration) is not carried under the poisson estimator (gfh_set_batch_estimator): STEP 3's second derivative is that of the least-squares cost");
  BatchOpts bo; memset(&bo, 0, sizeof bo);
  bo.lambda = lo.lambda; bo.lam_up = lo.lam_up; bo.lam_down = lo.lam_down; bo.lam_incs = lo.lam_incs;      // gadfit.F90:568-584 (lm_options.h)
  bo.use_accth = lo.use_accth; bo.accth = o->accth;
  bo.has_chi2_abs = o->has_chi2_abs != 0; bo.chi2_abs = o->chi2_abs;
  bo.has_chi2_rel = o->has_chi2_rel != 0; bo.chi2_rel = o->chi2_rel;
  bo.has_rel_error = o->has_rel_error != 0; bo.rel_error = o->rel_error;
  bo.has_max_iter = 1; bo.max_iter = o->max_iter;
  bo.damp_plain = lo.damp_plain;
  if (o->DTD_min) for (int j = 0; j < na; j++) bo.dtd_min[j] = o->DTD_min[j];                            // gadfit.F90:641-646 (the same for every fit)
  *out = bo;
  return 0;
}
// The body of gfh_fit_batch and gfh_fit_batch_errors (errors: NULL, or where the second launch's outputs go), under the caller's name
int fit_batch(gfh_ctx* c, const char* who_, double* pars, int na, const int32_t* active, const gfh_fit_options* o, gfh_batch_result* results,
              double* seconds, const BatchErrors* errors) {
  const std::string who(who_);
  if (check_batchable(c, who_, na, active)) return 1;
  if (!pars || !results) return fail(c, who + ": null argument");
  if (errors && check_errors(c, who_, *errors)) return 1;
  BatchOpts bo;
  if (batch_options(c, who, o, na, &bo) || check_held(c, who_, na)) return 1;
  gfh::Range range("gadfit gfh_fit_batch");
  Opened k;
  if (open_device(c, who_, na, active, &k)) return 1;
  const int64_t nf = c->batch.n_fits;
  const size_t pb = sizeof(double) * (size_t)nf * (size_t)c->model.n_pars, rb = sizeof(gfh_batch_result) * (size_t)nf;
  const size_t eb = errors ? ErrorBlock(nf, na).bytes : 0;      // [pars | records | covariances, standard errors, info]: one block, one copy back
  if (dev_alloc(c, c->batch.io, pb + rb + eb)) return 1;
  c->batch.host.resize(pb + rb + eb);
  harvest_events(c);
  HIPCHK(c, hipMemcpyAsync(c->batch.io.p, pars, pb, hipMemcpyHostToDevice, c->stream));
  void* dp = c->batch.io.p; void* recs = c->batch.io.as<char>() + pb; long long n = nf;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (launch_batch(c, k.mk->fit_batch, k.lanes, nf, {&dp, &bo, &recs, &n})) return 1;
  if (errors && launch_cov(c, k, na, errors->scale, dp, c->batch.io.as<char>() + pb + rb)) return 1;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipMemcpyAsync(c->batch.host.data(), c->batch.io.p, pb + rb + eb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(pars, c->batch.host.data(), pb);
  memcpy(results, c->batch.host.data() + pb, rb);
  if (errors) errors_out(c->batch.host.data() + pb + rb, nf, na, *errors);
  if (seconds) *seconds = 1e-3 * ev_ms(c->ev[0], c->ev[1]);
  return 0;
}

// the text of a batch unit, the four kernels' or the bounded one, into the caller's buffer
int64_t batch_source(gfh_ctx* c, const char* who, int na, const int32_t* active, bool bounded, char* buf, int64_t cap) {
  if (check_batchable(c, who, na, active)) return -1;
  std::string src, err;
  if (!generate_source(c->model, std::vector<int32_t>(active, active + na), batch_config(c, batch_lanes(c, na), bounded), &src, &err)) { fail(c, err); return -1; }
  if (buf && cap > 0) { const size_t n = std::min<size_t>((size_t)cap - 1, src.size()); memcpy(buf, src.data(), n); buf[n] = 0; }
  return (int64_t)src.size() + 1;
}

// The box of gfh_fit_batch_bounded as the kernel takes it by value (batch_fit_bounded.hip: gfh_batch_box), and its refusals
struct BatchBox { double lo[kValuGramMax], hi[kValuGramMax]; };
static_assert(sizeof(BatchBox) == 2 * 8 * kValuGramMax && kValuGramMax <= 8, "layout shared with the generated kernel; at_bound holds 8 + 8 bits");
int batch_box(gfh_ctx* c, const std::string& who, int na, const double* lower, const double* upper, BatchBox* out) {
  BatchBox b;
  for (int j = 0; j < kValuGramMax; j++) { b.lo[j] = -HUGE_VAL; b.hi[j] = HUGE_VAL; }
  for (int j = 0; j < na; j++) {
    const std::string pj = "active parameter " + std::to_string(j);
    if (std::isnan(lower[j]) || std::isnan(upper[j])) return fail(c, who + ": a bound of " + pj + " is NaN (-inf / +inf: no bound on that side)");
    if (lower[j] == HUGE_VAL) return fail(c, who + ": the lower bound of " + pj + " is +inf (-inf: no lower bound)");
    if (upper[j] == -HUGE_VAL) return fail(c, who + ": the upper bound of " + pj + " is -inf (+inf: no upper bound)");
    if (lower[j] >= upper[j])
      return fail(c, who + ": the box of " + pj + " is empty or a single value (lower " + std::to_string(lower[j]) + " >= upper " +
                     std::to_string(upper[j]) + "); make that parameter passive instead");
    b.lo[j] = lower[j]; b.hi[j] = upper[j];
  }
  *out = b;
  return 0;
}

}  // namespace

extern "C" {

// gfh_fit_batch inside one box per batch: lower[na] <= p <= upper[na] in the order of active, -inf / +inf for no bound on that side,
// by the projected loop gfh_k_fit_batch_bounded (device/batch_fit_bounded.hip states the rule).  at_bound [n_fits]: bit j where the
// returned active parameter j == lower[j], bit 8 + j where it == upper[j].  One launch; at_bound rides in io behind the records.
int gfh_fit_batch_bounded(gfh_ctx* c, double* pars, int na, const int32_t* active, const double* lower, const double* upper,
                          const gfh_fit_options* o, gfh_batch_result* results, int32_t* at_bound, double* seconds) try {
  const char* who_ = "gfh_fit_batch_bounded";
  const std::string who(who_);
  if (check_batchable(c, who_, na, active)) return 1;
  if (!pars || !lower || !upper || !results || !at_bound) return fail(c, who + ": null argument");
  BatchBox box; BatchOpts bo;
  if (batch_box(c, who, na, lower, upper, &box) || batch_options(c, who, o, na, &bo) || check_held(c, who_, na)) return 1;
  const int64_t nf = c->batch.n_fits;
  const int np = c->model.n_pars;
  for (int64_t f = 0; f < nf; f++)
    for (int j = 0; j < na; j++) {
      const double p = pars[(size_t)f * np + active[j]];
      if (p < lower[j] || p > upper[j])
        return fail(c, who + ": the start of fit " + std::to_string((long long)f) + " lies outside the box at active parameter " + std::to_string(j) +
                       " (parameter " + std::to_string(active[j]) + ")");
    }
  gfh::Range range("gadfit gfh_fit_batch_bounded");
  Opened k;
  if (open_device(c, who_, na, active, &k, true)) return 1;
  const size_t pb = sizeof(double) * (size_t)nf * (size_t)np, rb = sizeof(gfh_batch_result) * (size_t)nf, ab = sizeof(int32_t) * (size_t)nf;
  if (dev_alloc(c, c->batch.io, pb + rb + ab)) return 1;
  c->batch.host.resize(pb + rb + ab);
  harvest_events(c);
  HIPCHK(c, hipMemcpyAsync(c->batch.io.p, pars, pb, hipMemcpyHostToDevice, c->stream));
  void* dp = c->batch.io.p; void* recs = c->batch.io.as<char>() + pb; void* at = c->batch.io.as<char>() + pb + rb; long long n = nf;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (launch_batch(c, k.mk->fit_batch_bounded, k.lanes, nf, {&dp, &bo, &box, &recs, &at, &n})) return 1;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipMemcpyAsync(c->batch.host.data(), c->batch.io.p, pb + rb + ab, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(pars, c->batch.host.data(), pb);
  memcpy(results, c->batch.host.data() + pb, rb);
  memcpy(at_bound, c->batch.host.data() + pb + rb, ab);
  if (seconds) *seconds = 1e-3 * ev_ms(c->ev[0], c->ev[1]);
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_fit_batch_bounded: ") + e.what()); }

// gadf_fit (gadfit.F90:502-1035) for every spectrum of the batch at once: STEP 1+2, the damped solve (potr_f08,
// gadfit_linalg.F90:36-57), STEP 3 under accth, STEP 4 with its retrials and STEP 5 run on the device, a wave or -- gfh_set_batch_lanes --
// a row of 16 lanes or a workgroup of 256 per fit.
int gfh_fit_batch(gfh_ctx* c, double* pars, int na, const int32_t* active, const gfh_fit_options* o, gfh_batch_result* results,
                  double* seconds) try {
  return fit_batch(c, "gfh_fit_batch", pars, na, active, o, results, seconds, nullptr);
} catch (const std::exception& e) { return fail(c, std::string("gfh_fit_batch: ") + e.what()); }

// gfh_fit_batch and, behind it on the same stream, gfh_k_batch_cov at the fitted parameters, which stay on the device between the two
// launches: parameters, records, covariances, standard errors and info come back in the one copy.  The fit's launch and its
// arguments are gfh_fit_batch's, so its outputs are that call's bits.  *seconds: the device time of both launches.
int gfh_fit_batch_errors(gfh_ctx* c, double* pars, int na, const int32_t* active, const gfh_fit_options* o, gfh_batch_result* results,
                         int scale, double* cov, double* sigma, int32_t* info, double* seconds) try {
  const BatchErrors e{scale, cov, sigma, info};
  return fit_batch(c, "gfh_fit_batch_errors", pars, na, active, o, results, seconds, &e);
} catch (const std::exception& e) { return fail(c, std::string("gfh_fit_batch_errors: ") + e.what()); }

// (J^T J)^-1 of every spectrum at given parameters (scale 0: the reference's LMsolver::getInvJTJ) or that times chi2 / dof (scale
// 1), and the standard errors sqrt of its diagonal: cov [n_fits][na * na] (symmetric, both triangles), sigma [n_fits][na], info
// [n_fits] (0, or j + 1: pivot j of the fit's Cholesky factor was not positive and finite -- its cov and sigma are NaN), in the
// caller's order of the active parameters.  On whichever batch data is held, as gfh_batch_pass; one launch, one copy back.
int gfh_batch_covariance(gfh_ctx* c, const double* pars, int na, const int32_t* active, int scale, double* cov, double* sigma,
                         int32_t* info) try {
  const char* who = "gfh_batch_covariance";
  if (check_batchable(c, who, na, active)) return 1;
  const BatchErrors e{scale, cov, sigma, info};
  if (!pars) return fail(c, "gfh_batch_covariance: null argument");
  if (check_errors(c, who, e) || check_held(c, who, na)) return 1;
  Opened k;
  if (open_device(c, who, na, active, &k)) return 1;
  const int64_t nf = c->batch.n_fits;
  const size_t pb = sizeof(double) * (size_t)nf * (size_t)c->model.n_pars, eb = ErrorBlock(nf, na).bytes;
  if (dev_alloc(c, c->batch.io, pb) || dev_alloc(c, c->batch.img, eb)) return 1;
  c->batch.host.resize(eb);
  HIPCHK(c, hipMemcpyAsync(c->batch.io.p, pars, pb, hipMemcpyHostToDevice, c->stream));
  if (launch_cov(c, k, na, scale, c->batch.io.p, c->batch.img.as<char>())) return 1;
  HIPCHK(c, hipMemcpyAsync(c->batch.host.data(), c->batch.img.p, eb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  errors_out(c->batch.host.data(), nf, na, e);
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_covariance: ") + e.what()); }

// STEP 1 + 2 (gadfit.F90:675-699) of every spectrum at given parameters: J^T J [n_fits][na * na] (symmetric, both triangles),
// J^T r [n_fits][na], chi2 [n_fits] -- for callers with their own loop.
int gfh_batch_pass(gfh_ctx* c, const double* pars, int na, const int32_t* active, double* JTJ, double* JTres, double* chi2) try {
  const char* who = "gfh_batch_pass";
  if (check_batchable(c, who, na, active)) return 1;
  if (!pars || !JTJ || !JTres || !chi2) return fail(c, "gfh_batch_pass: null argument");
  if (check_held(c, who, na)) return 1;
  Opened k;
  if (open_device(c, who, na, active, &k)) return 1;
  const int64_t nf = c->batch.n_fits;
  const size_t rec = (size_t)na * na + na + 1;
  const size_t pb = sizeof(double) * (size_t)nf * (size_t)c->model.n_pars, ib = sizeof(double) * (size_t)nf * rec;
  if (dev_alloc(c, c->batch.io, pb) || dev_alloc(c, c->batch.img, ib)) return 1;
  c->batch.host.resize(ib);
  HIPCHK(c, hipMemcpyAsync(c->batch.io.p, pars, pb, hipMemcpyHostToDevice, c->stream));
  void* dp = c->batch.io.p; void* img = c->batch.img.p; long long n = nf;
  harvest_events(c);
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (launch_batch(c, k.mk->batch_pass, k.lanes, nf, {&dp, &img, &n})) return 1;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipMemcpyAsync(c->batch.host.data(), c->batch.img.p, ib, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch.pass_ms = ev_ms(c->ev[0], c->ev[1]);
  const double* h = reinterpret_cast<const double*>(c->batch.host.data());
  for (int64_t f = 0; f < nf; f++) {
    const double* r = h + (size_t)f * rec;
    memcpy(JTJ + (size_t)f * na * na, r, sizeof(double) * (size_t)na * na);
    memcpy(JTres + (size_t)f * na, r + (size_t)na * na, sizeof(double) * (size_t)na);
    chi2[f] = r[(size_t)na * na + na];
  }
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_pass: ") + e.what()); }

// Curves of a batch (include/gadfit_hip.h): the model, the weighted residuals and the 1-sigma band of fits [first_fit, first_fit +
// n_fits_eval) of the batch held, on their own points or on the caller's grid, by gfh_k_batch_eval (batch_eval.hip).  Each requested
// output is `tot` doubles.
int gfh_batch_eval(gfh_ctx* c, const double* pars, int na, const int32_t* active, const double* cov, const double* x_eval, int64_t n_eval,
                   int64_t first_fit, int64_t n_fits_eval, double* model, double* residual, double* band, double* seconds) try {
  const char* who = "gfh_batch_eval";
  if (check_batchable(c, who, na, active)) return 1;
  if (!pars) return fail(c, "gfh_batch_eval: null argument (pars is required)");
  if (!model && !residual && !band) return fail(c, "gfh_batch_eval: no output requested (model, residual and band are all NULL)");
  if (band && !cov) return fail(c, "gfh_batch_eval: a band needs the fits' covariances (cov is NULL)");
  if (residual && c->batch.estimator != 0)
    return fail(c, "gfh_batch_eval: the weighted residual has no meaning under the poisson estimator (gfh_set_batch_estimator): the data form's weight is a mask there; model and band are given");
  if (residual && x_eval) return fail(c, "gfh_batch_eval: a residual on a caller's grid has no meaning (residual is given on the fits' own points alone)");
  if (x_eval && n_eval < 1) return fail(c, "gfh_batch_eval: a grid holds at least one point (x_eval given with n_eval = " + std::to_string((long long)n_eval) + ")");
  if (!x_eval && n_eval != 0) return fail(c, "gfh_batch_eval: n_eval = " + std::to_string((long long)n_eval) + " without x_eval (NULL, 0: the fits' own points)");
  if (check_held(c, who, na)) return 1;
  const int64_t nf = c->batch.n_fits;
  if (first_fit < 0 || n_fits_eval < 1 || first_fit > nf - n_fits_eval)
    return fail(c, "gfh_batch_eval: fits [" + std::to_string((long long)first_fit) + ", " + std::to_string((long long)first_fit) + " + " +
                   std::to_string((long long)n_fits_eval) + ") are empty or reach past the " + std::to_string((long long)nf) + " fits of the batch");
  // the points of one output: the data's own layout, or [n_fits_eval][n_eval]
  const int64_t per_fit = x_eval ? n_eval : c->batch.max_points;
  double* const outs[3] = {model, residual, band};
  const int n_out = (model ? 1 : 0) + (residual ? 1 : 0) + (band ? 1 : 0);
  if (per_fit > INT64_MAX / 8 / n_out / n_fits_eval) return fail(c, "gfh_batch_eval: the size of the outputs overflows");
  const int64_t tot = x_eval || c->batch.cube ? n_fits_eval * per_fit : c->batch.off[(size_t)(first_fit + n_fits_eval)] - c->batch.off[(size_t)first_fit];
  gfh::Range range("gadfit gfh_batch_eval");
  Opened k;
  if (open_device(c, who, na, active, &k)) return 1;
  const size_t pb = sizeof(double) * (size_t)n_fits_eval * (size_t)c->model.n_pars;
  const size_t cb = band ? sizeof(double) * (size_t)n_fits_eval * (size_t)na * na : 0, xb = x_eval ? sizeof(double) * (size_t)n_eval : 0;
  const size_t ob = sizeof(double) * (size_t)tot;
  if (dev_alloc(c, c->batch.io, pb + cb + xb) || dev_alloc(c, c->batch.img, std::max<size_t>(ob * n_out, 8))) return 1;
  c->batch.host.resize(std::max(pb + cb + xb, ob * n_out));
  char* h = c->batch.host.data();          // down from here, and -- behind the kernel in the stream's order -- back into it
  memcpy(h, pars, pb);
  if (cb) memcpy(h + pb, cov, cb);
  if (xb) memcpy(h + pb + cb, x_eval, xb);
  harvest_events(c);
  HIPCHK(c, hipMemcpyAsync(c->batch.io.p, h, pb + cb + xb, hipMemcpyHostToDevice, c->stream));
  char* in = c->batch.io.as<char>(); char* out = c->batch.img.as<char>();
  void* dp = in; void* dc = cb ? in + pb : nullptr; void* dx = xb ? in + pb + cb : nullptr;
  void* d[3] = {nullptr, nullptr, nullptr};          // the requested outputs back to back, in the order model, residual, band
  size_t at = 0;
  for (int j = 0; j < 3; j++) if (outs[j]) { d[j] = out + at; at += ob; }
  long long ne = n_eval, first = first_fit, n = n_fits_eval;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (launch_batch(c, k.mk->batch_eval, k.lanes, n_fits_eval, {&dp, &dc, &dx, &ne, &first, &n, &d[0], &d[1], &d[2]}, false)) return 1;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipMemcpyAsync(h, out, at, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < 3; j++) if (outs[j]) memcpy(outs[j], h + (static_cast<char*>(d[j]) - out), ob);
  if (seconds) *seconds = 1e-3 * ev_ms(c->ev[0], c->ev[1]);
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_eval: ") + e.what()); }

// The generated source of the batch translation unit for the current model and an active set, as gfh_model_source: in the form of
// the context's setting (under auto: what the rule gives for the geometry held, 64 without one); gfh_batch_prepare alike.
int64_t gfh_batch_source(gfh_ctx* c, int na, const int32_t* active, char* buf, int64_t cap) try {
  return batch_source(c, "gfh_batch_source", na, active, false, buf, cap);
} catch (const std::exception& e) { fail(c, std::string("gfh_batch_source: ") + e.what()); return -1; }
// ... and of the bounded unit (gfh_k_fit_batch_bounded behind the same point functions and passes)
int64_t gfh_batch_source_bounded(gfh_ctx* c, int na, const int32_t* active, char* buf, int64_t cap) try {
  return batch_source(c, "gfh_batch_source_bounded", na, active, true, buf, cap);
} catch (const std::exception& e) { fail(c, std::string("gfh_batch_source_bounded: ") + e.what()); return -1; }

// Compiles the batch translation unit (or finds it in the cache) without launching, as gfh_model_prepare; needs no GPU.
int gfh_batch_prepare(gfh_ctx* c, int na, const int32_t* active) try {
  if (check_batchable(c, "gfh_batch_prepare", na, active)) return 1;
  return batch_kernels(c, std::vector<int32_t>(active, active + na), batch_lanes(c, na), false, false, nullptr);
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_prepare: ") + e.what()); }
// ... and the bounded unit's
int gfh_batch_prepare_bounded(gfh_ctx* c, int na, const int32_t* active) try {
  if (check_batchable(c, "gfh_batch_prepare_bounded", na, active)) return 1;
  return batch_kernels(c, std::vector<int32_t>(active, active + na), batch_lanes(c, na), true, false, nullptr);
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_prepare_bounded: ") + e.what()); }

// Lanes per fit of the batch kernels from here on: 64 (the default) a wave per fit, 16 a DPP row per fit and four fits per wave, 256
// a workgroup per fit (few, long spectra), 0 auto -- gfh_batch_auto_lanes at every call, which chooses between 16 and 64 only.  A setting, not a launch: needs no GPU and no model.
int gfh_set_batch_lanes(gfh_ctx* c, int lanes) try {
  if (check_context(c, "gfh_set_batch_lanes")) return 1;
  if (lanes != 64 && lanes != 16 && lanes != 256 && lanes != 0)
    return fail(c, "gfh_set_batch_lanes: " + std::to_string(lanes) + " lanes per fit are not built (64: a wave per fit, 16: a row per fit, 256: a workgroup per fit, 0: auto)");
  c->batch.lanes = lanes;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_batch_lanes: ") + e.what()); }

// The loss of the batch kernels from here on (it stays set, as gfh_set_batch_lanes): 0 linear (the default), 1 Cauchy, 2 Huber -- the
// reference's costs (lm_solver.cpp:255-284), switching at |r| = scale in units of the weighted residual r = (y - f) w; scale 1 is the
// reference's own.  The loss is part of the batch unit's text, 1 / scale a kernel argument.  A setting, not a launch: needs no GPU and no model.
int gfh_set_batch_loss(gfh_ctx* c, int loss, double scale) try {
  if (check_context(c, "gfh_set_batch_loss")) return 1;
  if (loss < GFH_LOSS_LINEAR || loss > GFH_LOSS_HUBER)
    return fail(c, "gfh_set_batch_loss: unknown loss " + std::to_string(loss) + " (0: linear, 1: cauchy, 2: huber)");
  if (std::isnan(scale)) return fail(c, "gfh_set_batch_loss: the residual scale is NaN");
  if (std::isinf(scale)) return fail(c, "gfh_set_batch_loss: the residual scale is infinite (a loss that never switches is the linear one: loss 0)");
  if (!(scale > 0.0) || std::isinf(1.0 / scale))          // (the kernels take 1 / scale: a subnormal scale has no finite one)
    return fail(c, "gfh_set_batch_loss: the residual scale must be positive, with a finite reciprocal, got " + std::to_string(scale));
  c->batch.loss = loss; c->batch.loss_scale = scale;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_batch_loss: ") + e.what()); }
// The setting itself: the loss (return value; -1: no context) and *scale (may be NULL) that gfh_set_batch_loss left
int gfh_get_batch_loss(gfh_ctx* c, double* scale) {
  if (!c) return -1;
  if (scale) *scale = c->batch.loss_scale;
  return c->batch.loss;
}
// The loss and scale that the last sweeping batch launch of this context ran under (return -1: none yet; scale may be NULL)
int gfh_debug_batch_loss(gfh_ctx* c, double* scale) {
  if (!c) return -1;
  if (scale) *scale = c->batch.last_loss_scale;
  return c->batch.last_loss;
}

// What the batch kernels minimise from here on (it stays set, as gfh_set_batch_loss): 0 the weighted sum of squares (the default, and
// what a batch was before this setting), 1 the Poisson deviance 2 sum [f - y + y ln(y / f)] over the points of non-zero weight, by
// Fisher scoring (device/batch_fit.hip, GFH_BMLE).  Part of the batch unit's text.  A setting, not a launch: needs no GPU and no model.
int gfh_set_batch_estimator(gfh_ctx* c, int estimator) try {
  if (check_context(c, "gfh_set_batch_estimator")) return 1;
  if (estimator != GFH_ESTIMATOR_LSQ && estimator != GFH_ESTIMATOR_POISSON)
    return fail(c, "gfh_set_batch_estimator: unknown estimator " + std::to_string(estimator) + " (0: least squares, 1: poisson)");
  c->batch.estimator = estimator;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_batch_estimator: ") + e.what()); }
// The setting itself (-1: no context)
int gfh_get_batch_estimator(gfh_ctx* c) { return c ? c->batch.estimator : -1; }
// The estimator that the last sweeping batch launch of this context ran under (-1: none yet)
int gfh_debug_batch_estimator(gfh_ctx* c) { return c ? c->batch.last_estimator : -1; }

// The form of the last batch launch of this context (64, 16 or 256; 0: none yet), so that a test asserts the dispatch.
int gfh_debug_batch_lanes(gfh_ctx* c) { return c ? c->batch.last_lanes : 0; }
// device time of the kernel of the last gfh_batch_pass of this context in seconds (HIP events; 0: none yet)
double gfh_debug_batch_pass_seconds(gfh_ctx* c) { return c ? 1e-3 * c->batch.pass_ms : 0.0; }
// ... and its data form: -1 none yet, 0 ragged, else a cube, 1 + y_type + 3 * error_type
int gfh_debug_batch_form(gfh_ctx* c) { return c ? c->batch.last_form : -1; }

// The auto rule: a function of the active count and the longest spectrum of the batch, never of the data.  16 or 64: the workgroup
// form (256) is the caller's choice alone (it wins where the fits are fewer than the card's SIMDs, which the rule does not see;
// profiles/batch_workgroup.json).
int gfh_batch_auto_lanes(int n_act, int64_t longest) {
  if (n_act < 1 || n_act > kValuGramMax || longest < 1) return 64;
  return longest <= (n_act <= 4 ? kRowUpTo4 : kRowUpTo8) ? 16 : 64;
}

}  // extern "C"
