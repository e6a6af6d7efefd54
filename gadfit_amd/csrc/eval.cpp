// eval.cpp -- the curves of a plain fit: gfh_eval, gfh_eval_source, gfh_eval_prepare.  The fitted model, the weighted residuals and the
// 1-sigma band of gfh_fit's path (one fit, possibly global over several datasets) on the data's own points or on a caller's grid, by
// the generated kernels of device/eval.hip from the data the context holds and the model's own point functions.
//
// gfh_eval is written in the steps of the batch calls (batch_calls.cpp): its argument checks and everything the kernels do not carry,
// refused under the call's name before anything touches the device; then the device, its two blocks (context.h, Curves) and on the
// one stream: the parameters through the pass's own routine (upload_pars: the pars hook, the staging block), the covariance blocks
// and the grid down, event, one launch, event, the status word, the outputs back.  A data point that leaves the recorded paths of a
// branching eval() is handled as gfh_chi2 handles it: the handler extends the model and the pass is repeated.
#include "context_internal.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <exception>

using namespace gfh;

namespace {

// what no eval unit exists for: refused with or without a GPU
int check_evaluable(gfh_ctx* c, const char* who, int na, const int32_t* active) {
  const std::string w(who);
  if (!c) return 1;
  if (c->grp) return fail(c, w + " is not available on a device-group handle");
  if (c->nranks > 1) return fail(c, w + ": a context that is one of " + std::to_string(c->nranks) + " ranks is not carried (the curves of one rank's points alone)");
  if (!c->has_model) return fail(c, w + ": no model set (gfh_set_model)");
  if (c->model.has_integrals()) return fail(c, w + ": models with integrate() are not carried by the eval kernels");
  if (na < 1) return fail(c, "There are no active parameters.");                                       // gadfit.F90:602-603
  if (!active) return fail(c, w + ": null argument");
  if (na > c->model.n_pars) return fail(c, w + ": more active parameters than the model has");
  for (int j = 0; j < na; j++) {
    if (active[j] < 0 || active[j] >= c->model.n_pars) return fail(c, w + ": active parameter index out of range");
    for (int k = 0; k < j; k++) if (active[k] == active[j]) return fail(c, w + ": an active parameter is listed twice");
  }
  return 0;
}

// the parameter block by value while it fits the kernel-argument segment, as the kernels of a fit take it (active.cpp, get_kernels)
int kernarg_doubles(const gfh_ctx* c, int nd) {
  const int np = c->model.n_pars;
  return c->kernarg && np >= 1 && nd >= 1 && (int64_t)nd * np <= kMaxKernargPars ? nd * np : 0;
}
GenConfig eval_config(const gfh_ctx* c, int kernarg_pars) {
  GenConfig cfg = c->gen;           // the context's switches the point functions read: use_ad and its column sets, the divisions
  cfg.eval = true; cfg.batch = false;
  cfg.loss = 0; cfg.store_j = true; cfg.store_res = true;      // (no eval kernel reads them: one unit whatever they are)
  cfg.kernarg_pars = kernarg_pars;
  return cfg;
}
// the translation unit of an active set with the eval kernels: generated, compiled and (load) loaded once per context, kept in the
// context's kernel cache under a key no other unit has, so that a new model or gfh_destroy releases it with the rest
int eval_kernels(gfh_ctx* c, const std::vector<int32_t>& active, int kernarg_pars, bool load, ModelKernels** out) {
  std::vector<int32_t> key = active;
  key.push_back(-(1 << 30) - 1);    // (a batch unit holds -(1 << 30) here, a plain one a small negative number)
  key.push_back(kernarg_pars);
  key.push_back((c->gen.finite_diff ? 1 : 0) + (c->gen.finite_diff && c->gen.fd_col_sets ? 2 : 0));
  auto it = c->kernel_cache.find(key);
  if (it != c->kernel_cache.end()) { if (out) *out = &it->second; return 0; }
  std::string src, err;
  if (!generate_source(c->model, active, eval_config(c, kernarg_pars), &src, &err)) return fail(c, err);
  ModelKernels mk;
  const uint64_t skey = load ? source_key(src) : 0;
  if (!(load && acquire_loaded(c->device, skey, &mk))) {
    std::vector<char> code; bool cached = false;
    if (!compile_to_code_object(src, &code, &err, &cached)) return fail(c, err);
    if (!load) return 0;
    if (!load_eval_kernels(code, &mk, &err)) return fail(c, err);
    publish_loaded(c->device, skey, mk);
  }
  mk.kernarg_pars = kernarg_pars; mk.n_active = (int)active.size();
  ModelKernels* p = &c->kernel_cache.emplace(key, mk).first->second;
  if (out) *out = p;
  return 0;
}

struct EvalCall {
  const double* pars; int na; const int32_t* active; const int32_t* jac; int dim; const double* cov;
  const double* x_eval; int64_t n_eval; double* model; double* residual; double* band; double* seconds;
};

int eval_pass(gfh_ctx* c, const EvalCall& e) {
  gfh::Range range("gadfit gfh_eval");
  harvest_events(c);
  const int nd = c->nd, na = e.na;
  const bool grid = e.x_eval != nullptr;
  if (!grid && (check_aux(c) || ensure_tile_table(c))) return 1;
  ModelKernels* mk = nullptr;
  if (eval_kernels(c, std::vector<int32_t>(e.active, e.active + na), kernarg_doubles(c, nd), true, &mk)) return 1;
  hipFunction_t kernel = grid ? (e.band ? mk->eval_grid_band : mk->eval_grid) : (e.band ? mk->eval_band : mk->eval);
  if (!kernel) return fail(c, "gfh_eval: the kernel is missing from its code object");
  // down: the datasets' blocks of the covariance, gathered through Jacobian_indices, and the grid
  const size_t cb = e.band ? sizeof(double) * (size_t)nd * na * na : 0, xb = grid ? sizeof(double) * (size_t)e.n_eval : 0;
  std::vector<double> down((cb + xb) / sizeof(double));
  if (e.band)
    for (int d = 0; d < nd; d++) for (int a = 0; a < na; a++) for (int b = 0; b < na; b++)
      down[((size_t)d * na + a) * na + b] = e.cov[(size_t)e.jac[(size_t)d * na + a] * e.dim + e.jac[(size_t)d * na + b]];
  if (grid) memcpy(down.data() + cb / sizeof(double), e.x_eval, xb);
  double* const outs[3] = {e.model, e.residual, e.band};
  const int n_out = (e.model ? 1 : 0) + (e.residual ? 1 : 0) + (e.band ? 1 : 0);
  const size_t per_out = grid ? (size_t)nd * (size_t)e.n_eval : (size_t)c->n_slots, ob = sizeof(double) * per_out;
  if (dev_alloc(c, c->curves.io, std::max<size_t>(cb + xb, 8)) || dev_alloc(c, c->curves.out, std::max<size_t>(ob * n_out, 8))) return 1;
  if (upload_pars(c, e.pars)) return 1;
  // (upload_pars queues the copy of the block unless the kernels of the FIT take it by value; these take it as those do)
  if (!mk->kernarg_pars && c->cur && c->cur->kernarg_pars)
    HIPCHK(c, hipMemcpyAsync(c->pars.p, c->h_pars, sizeof(double) * (size_t)nd * c->model.n_pars, hipMemcpyHostToDevice, c->stream));
  if (cb + xb) HIPCHK(c, hipMemcpyAsync(c->curves.io.p, down.data(), cb + xb, hipMemcpyHostToDevice, c->stream));
  char* in = c->curves.io.as<char>(); char* out = c->curves.out.as<char>();
  void* dcov = cb ? in : nullptr; void* dx = xb ? in + cb : nullptr;
  void* d[3] = {nullptr, nullptr, nullptr};          // the requested outputs back to back, in the order model, residual, band
  size_t at = 0;
  for (int j = 0; j < 3; j++) if (outs[j]) { d[j] = out + at; at += ob; }
  void* pars = c->pars.p; void* parg = mk->kernarg_pars ? (void*)c->h_pars : (void*)&pars; void* stp = c->status.p;
  // (gfh_debug_eval_launches: the launch repeated back to back, each writing what the one before it wrote; the events bracket the last)
  for (int rep = std::max(1, c->curves.launches); rep > 0; rep--) {
    if (rep == 1) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    if (grid) {
      long long ne = e.n_eval; int tiles_per_ds = (int)((e.n_eval + c->gen.block - 1) / c->gen.block);
      void* args[] = {&dx, &ne, &tiles_per_ds, parg, &dcov, &d[0], &d[2], &stp};
      HIPCHK(c, hipModuleLaunchKernel(kernel, (unsigned)(nd * tiles_per_ds), 1, 1, c->gen.block, 1, 1, 0, c->stream, args, nullptr));
    } else if (c->n_tiles) {
      void* x = c->x.p; void* y = c->y.p; void* w = c->w.p; void* tds = c->tile_ds.p; int nt = c->n_tiles;
      void* ax = c->aux.p; long long lda = c->n_slots;
      void* args[] = {&x, &y, &w, parg, &tds, &nt, &dcov, &d[0], &d[1], &d[2], &stp, &ax, &lda};
      HIPCHK(c, hipModuleLaunchKernel(kernel, (unsigned)nt, 1, 1, c->gen.block, 1, 1, 0, c->stream, args, nullptr));
    }
  }
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int st = 0;
  HIPCHK(c, hipMemcpy(&st, c->status.p, sizeof(int), hipMemcpyDeviceToHost));
  PASS(status_check(c, st));
  for (int j = 0; j < 3; j++) {
    if (!outs[j]) continue;
    if (grid) HIPCHK(c, hipMemcpy(outs[j], d[j], ob, hipMemcpyDeviceToHost));
    else if (unpad(c, static_cast<const double*>(d[j]), outs[j])) return 1;          // the code gfh_get_residuals un-pads with
  }
  if (e.seconds) *e.seconds = 1e-3 * ev_ms(c->ev[0], c->ev[1]);
  return 0;
}

}  // namespace

extern "C" {

int gfh_eval(gfh_ctx* c, const double* pars, int na, const int32_t* active, const int32_t* jac, int dim, const double* cov,
             const double* x_eval, int64_t n_eval, double* model, double* residual, double* band, double* seconds) try {
  const char* who = "gfh_eval";
  if (check_evaluable(c, who, na, active)) return 1;
  if (!pars) return fail(c, "gfh_eval: null argument (pars is required)");
  if (!model && !residual && !band) return fail(c, "gfh_eval: no output requested (model, residual and band are all NULL)");
  if (band && !cov) return fail(c, "gfh_eval: a band needs the fit's covariance (cov is NULL)");
  if (band && (!jac || dim < 1)) return fail(c, "gfh_eval: a band needs the column map of the covariance (jac_idx and dim, gfh_jacobian_indices)");
  if (band && na > kEvalBandMax)
    return fail(c, "gfh_eval: a band is carried up to " + std::to_string(kEvalBandMax) + " active parameters per dataset, got " + std::to_string(na));
  if (residual && x_eval) return fail(c, "gfh_eval: a residual on a caller's grid has no meaning (residual is given on the data's own points alone)");
  if (x_eval && n_eval < 1) return fail(c, "gfh_eval: a grid holds at least one point (x_eval given with n_eval = " + std::to_string((long long)n_eval) + ")");
  if (!x_eval && n_eval != 0) return fail(c, "gfh_eval: n_eval = " + std::to_string((long long)n_eval) + " without x_eval (NULL, 0: the data's own points)");
  if (x_eval && c->model.branching()) return fail(c, "gfh_eval: on a grid, models recorded as variant tapes (a branching eval()) are not carried");
  if (x_eval && c->model.n_aux > 0) return fail(c, "gfh_eval: on a grid, models with auxiliary per-point columns are not carried (the columns belong to the data's points)");
  if (c->device < 0) return fail(c, "no GPU bound to this context (libgadfit_hip has no CPU fallback)");
  if (!c->nd) return fail(c, "gfh_eval: no data set (gfh_set_data)");
  const int nd = c->nd;
  if (band) for (size_t k = 0; k < (size_t)nd * na; k++) if (jac[k] < 0 || jac[k] >= dim) return fail(c, "gfh_eval: Jacobian index out of range");
  if (x_eval && (n_eval > INT_MAX / 2 - 1024 || (n_eval + 1023) / c->gen.block > (INT_MAX / 2) / nd))
    return fail(c, "gfh_eval: a grid of " + std::to_string((long long)n_eval) + " points for " + std::to_string(nd) + " datasets is more than one launch takes");
  if (band && c->gen.finite_diff) {
    if (c->gen.fd_col_sets && c->n_aux < c->model.n_aux * (1 + na))
      return fail(c, "gfh_eval: use_ad = 0 with column sets (gfh_set_fd_column_sets): gfh_set_aux must hold " + std::to_string(c->model.n_aux * (1 + na)) +
                     " columns; it holds " + std::to_string(c->n_aux));
    for (int d = 0; d < nd; d++) for (int j = 0; j < na; j++)          // grad_finite's own check (fitfunction.F90:164-167), as the sweep makes it
      if (!(std::fabs(0x1p-26 * pars[(size_t)d * c->model.n_pars + active[j]]) > 2.2250738585072014e-308))
        return fail(c, "Absolute value of parameter " + std::to_string(active[j] + 1) + " is too small.");
  }
  NEED_GPU(c);
  const EvalCall e{pars, na, active, jac, dim, cov, x_eval, n_eval, model, residual, band, seconds};
  for (;;) {
    // (a recovery replaces the model: what the sweep before this call left -- its active set, column map and Jacobian -- is kept, as
    // gfh_chi2 keeps it)
    const std::vector<int32_t> act = c->cur_active, cj = c->cur_jac; const int cdim = c->cur_dim;
    const bool had = c->have_sweep, jv = c->j_valid;
    const int rc = eval_pass(c, e);
    if (rc != kUnseen && rc != kGrowWs && rc != kIntegrandPath) return rc;
    if (repeat_pass(c, rc, pars)) return 1;
    if (!act.empty() && prepare_active(c, act.data(), (int)act.size(), cj.data(), cdim)) return 1;
    if (!act.empty()) { c->have_sweep = had; c->j_valid = jv; }
  }
} catch (const std::exception& e) { return fail(c, std::string("gfh_eval: ") + e.what()); }

// The generated source of the eval translation unit for the current model and an active set, as gfh_model_source: in the form a
// context with this one's datasets loads (one dataset where it holds none).
int64_t gfh_eval_source(gfh_ctx* c, int na, const int32_t* active, char* buf, int64_t cap) try {
  if (check_evaluable(c, "gfh_eval_source", na, active)) return -1;
  std::string src, err;
  if (!generate_source(c->model, std::vector<int32_t>(active, active + na), eval_config(c, kernarg_doubles(c, std::max(1, c->nd))), &src, &err)) { fail(c, err); return -1; }
  if (buf && cap > 0) { const size_t n = std::min<size_t>((size_t)cap - 1, src.size()); memcpy(buf, src.data(), n); buf[n] = 0; }
  return (int64_t)src.size() + 1;
} catch (const std::exception& e) { fail(c, std::string("gfh_eval_source: ") + e.what()); return -1; }

// Bench hook (tools/bench_eval.py): the kernel of every later gfh_eval on this context is launched n times back to back -- the same
// arguments, the same outputs -- and *seconds is the device time of the last of them, past the slow launches that follow an idle gap.
int gfh_debug_eval_launches(gfh_ctx* c, int n) {
  if (!c) return 1;
  if (c->grp) return fail(c, "gfh_debug_eval_launches is not available on a device-group handle");
  if (n < 1 || n > 1000) return fail(c, "gfh_debug_eval_launches: 1 to 1000 launches, got " + std::to_string(n));
  c->curves.launches = n;
  return 0;
}

// Compiles the eval translation unit (or finds it in the cache) without launching, as gfh_model_prepare; needs no GPU.  A context
// without data compiles the one-dataset form and the pointer form.
int gfh_eval_prepare(gfh_ctx* c, int na, const int32_t* active) try {
  if (check_evaluable(c, "gfh_eval_prepare", na, active)) return 1;
  const std::vector<int32_t> a(active, active + na);
  if (c->device < 0 && !c->nd) {
    const int kp = kernarg_doubles(c, 1);
    if (kp && eval_kernels(c, a, kp, false, nullptr)) return 1;
    return eval_kernels(c, a, 0, false, nullptr);
  }
  return eval_kernels(c, a, kernarg_doubles(c, c->nd), false, nullptr);
} catch (const std::exception& e) { return fail(c, std::string("gfh_eval_prepare: ") + e.what()); }

}  // extern "C"
