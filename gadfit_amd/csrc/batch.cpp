// batch.cpp -- batched independent fits: many Levenberg-Marquardt fits of ONE model in ONE kernel launch, each with its own data,
// start parameters, lambda history and exit (gfh_set_batch_data, gfh_fit_batch, gfh_batch_pass, gfh_batch_covariance, gfh_fit_batch_errors, gfh_batch_eval, gfh_batch_source, gfh_batch_prepare,
// gfh_set_batch_lanes; gfh_set_batch_cube: the same batch as a cube on one grid with narrow samples; gfh_batch_frames_begin,
// gfh_batch_frames_put, gfh_set_batch_frames: that cube from a frame-major stack, transposed on the device by frames.hip).  This file validates, uploads, compiles / loads and launches; the loop itself (gadfit.F90:670-915) is the
// generated kernel gfh_k_fit_batch (batch_fit.hip; codegen.cpp, emit_batch_kernels), a wave per fit or -- gfh_set_batch_lanes(16) -- a
// DPP row of 16 lanes per fit and four fits per wave, or -- gfh_set_batch_lanes(256) -- a workgroup of four waves per fit.  One stream, one launch and one device-to-host copy per call.
// Everything the kernels do not carry is refused here with its own message, before anything touches the device.
#include "context_internal.h"
#include "lm_options.h"
#include <algorithm>
#include <cstring>
#include <exception>

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

// what a batch cannot be: refused on any context, with or without a GPU
int check_context(gfh_ctx* c, const char* who) {
  if (!c) return 1;
  const std::string w(who);
  if (c->grp) return fail(c, w + " is not available on a device-group handle (the fits are independent: split the batch over the members' contexts)");
  if (c->nranks > 1) return fail(c, w + " is not available on a context with a communicator of more than one rank (the fits are independent: split the batch)");
  return 0;
}
int check_model(gfh_ctx* c, const char* who, int na, const int32_t* active) {
  const std::string w(who);
  if (!c->has_model) return fail(c, w + ": no model set (gfh_set_model)");
  if (c->model.has_integrals()) return fail(c, w + ": models with integrate() are not carried by the batch kernels");
  if (c->model.branching()) return fail(c, w + ": models recorded as variant tapes (a branching eval()) are not carried by the batch kernels");
  if (c->model.n_aux > 0) return fail(c, w + ": models with auxiliary per-point columns are not carried by the batch kernels");
  if (c->pars_fn) return fail(c, w + ": a pars hook (gfh_set_pars_hook) cannot run inside a device-resident loop");
  if (c->gen.loss != 0) return fail(c, w + ": a robust loss (gfh_set_loss) is not carried by the batch kernels");
  if (c->gen.finite_diff) return fail(c, w + ": use_ad = 0 (finite differences) is not carried by the batch kernels");
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
int check_geometry(gfh_ctx* c, const char* who, int na) {
  const std::string w(who);
  if (c->batch.n_fits < 1) return fail(c, w + ": no batch data (gfh_set_batch_data, gfh_set_batch_cube)");
  if (c->batch.min_points < na) return fail(c, "More independent fitting parameters than data points (a fit of the batch has " +
                                              std::to_string((long long)c->batch.min_points) + " points).");      // gadfit.F90:648-657, per fit
  return 0;
}
// a cube begun by gfh_batch_frames_begin is fitted once every frame has been put
int check_frames(gfh_ctx* c, const char* who) {
  if (!c->batch.frames || c->batch.frames_missing == 0) return 0;
  return fail(c, std::string(who) + ": " + std::to_string((long long)c->batch.frames_missing) + " of " + std::to_string((long long)c->batch.max_points) +
                 " frames of the batch begun by gfh_batch_frames_begin have not been put (gfh_batch_frames_put)");
}
// the batch held is no longer one that gfh_batch_frames_begin began
void frames_end(gfh_ctx* c) {
  c->batch.frames = false; c->batch.frame_put.clear(); c->batch.frames_missing = 0; c->batch.frames_kernel_ms = 0.0;
}
constexpr size_t elem_bytes(int y_type) { return y_type == 0 ? 8 : y_type == 1 ? 4 : 2; }
// The largest staging of gfh_set_batch_frames' default pieces (frames_per_put 0), samples and USER weights together.  Kept at the
// 256 MiB it was proposed with: every stack of the measured table (profiles/batch_frames.json; at most 262 MB)
// is ONE put under it, so the default there is the single put it was to be compared with, and the same stacks cut into eight puts
// took 0.15 ... 0.3 ms longer (about 30 us per further put) -- a stack above the bound pays that per 256 MiB, against 5 ms of upload.
// The measurement gave no reason for another value; it does not hold a smaller one to be worse by more than that.
constexpr int64_t kFramesStageBytes = (int64_t)256 << 20;

// what a cube can be, for the three calls that make one (gfh_set_batch_cube, gfh_batch_frames_begin, gfh_set_batch_frames): one
// order, one wording, each under its own name.  null_arg: a required pointer is NULL, `required` names them; has_w: -1 the call takes no w
int check_cube(gfh_ctx* c, const char* who, bool null_arg, const char* required, int64_t n_fits, int64_t n_points, int y_type, int error_type,
               int has_w) {
  const std::string w(who);
  if (null_arg) return fail(c, w + ": null argument (" + required + " required)");
  if (n_fits < 1) return fail(c, w + ": a batch holds at least one fit");
  if (n_points < 1) return fail(c, w + ": a spectrum holds at least one point");
  if (n_fits > ((int64_t)1 << 31) - 4) return fail(c, w + ": more fits than one launch takes (2^31 - 4)");
  if (y_type < 0 || y_type > 2) return fail(c, w + ": unknown y_type " + std::to_string(y_type) + " (0 double, 1 float, 2 uint16_t)");
  if (error_type < 0 || error_type > 4)
    return fail(c, w + ": unknown error_type " + std::to_string(error_type) + " (0 NONE, 1 SQRT_Y, 2 PROPTO_Y, 3 INVERSE_Y, 4 USER)");
  if (has_w >= 0 && error_type == 4 && !has_w) return fail(c, w + ": error_type USER needs the weights w");
  if (has_w >= 0 && error_type != 4 && has_w) return fail(c, w + ": w is taken under error_type USER alone (the other types form the weights from y on the device)");
  if (n_points > INT64_MAX / 8 / n_fits) return fail(c, w + ": n_fits x n_points overflows");
  return 0;
}

// the translation unit of an active set with the four batch kernels: generated, compiled and (load) loaded once per context, kept
// in the context's kernel cache under a key no plain active set has, so that a new model or gfh_destroy releases it with the rest
GenConfig batch_config(const gfh_ctx* c, int lanes) {
  GenConfig cfg;                    // the defaults, not the context's current switches: one form per (model, active set, lanes per fit)
  cfg.fast_div = c->gen.fast_div;
  cfg.batch = true;
  cfg.batch_lanes = lanes;
  cfg.batch_cube = c->batch.cube;   // the data form held: a cube's sample type and weight rule are part of the text (batch_cube.hip)
  if (c->batch.cube) { cfg.batch_y_type = c->batch.y_type; cfg.batch_error_type = c->batch.error_type; }
  return cfg;
}
// 0 ragged, 1 ... 15 a cube by sample type and weight rule: what gfh_debug_batch_form reports and the kernel cache keys on
int data_form(const gfh_ctx* c) { return c->batch.cube ? 1 + c->batch.y_type + 3 * c->batch.error_type : 0; }
// the form a call uses: the context's setting, under auto what the rule gives for the geometry held (64 when the context holds none)
int batch_lanes(const gfh_ctx* c, int na) {
  if (c->batch.lanes != 0) return c->batch.lanes;
  return c->batch.n_fits < 1 ? 64 : gfh_batch_auto_lanes(na, c->batch.max_points);
}
int batch_kernels(gfh_ctx* c, const std::vector<int32_t>& active, int lanes, bool load, ModelKernels** out) {
  std::vector<int32_t> key = active;
  key.push_back(-(1 << 30));        // (no plain active set holds a negative entry)
  key.push_back(lanes);             // both forms of one active set can be resident
  if (c->batch.cube) key.push_back(data_form(c));      // ... and so can its cube forms beside the ragged one (whose key stays what it was)
  auto it = c->kernel_cache.find(key);
  if (it != c->kernel_cache.end()) { if (out) *out = &it->second; return 0; }
  std::string src, err;
  if (!generate_source(c->model, active, batch_config(c, lanes), &src, &err)) return fail(c, err);
  ModelKernels mk;
  const uint64_t skey = load ? source_key(src) : 0;
  if (!(load && acquire_loaded(c->device, skey, &mk))) {
    std::vector<char> code; bool cached = false;
    if (!compile_to_code_object(src, &code, &err, &cached)) return fail(c, err);
    if (!load) return 0;
    if (!load_kernels(code, &mk, &err)) return fail(c, err);
    publish_loaded(c->device, skey, mk);
  }
  if (!mk.fit_batch || !mk.batch_pass || !mk.batch_cov || !mk.batch_eval) { release_loaded(c->device, &mk); return fail(c, "the batch kernels are missing from their code object"); }
  mk.n_active = (int)active.size();
  ModelKernels* p = &c->kernel_cache.emplace(key, mk).first->second;
  if (out) *out = p;
  return 0;
}

// The error outputs of a call (gfh_batch_covariance, gfh_fit_batch_errors) and their block on the device, written by gfh_k_batch_cov
// (batch_cov.hip): [cov n_fits x na x na | sigma n_fits x na | info n_fits], the ints last so that the doubles stay aligned
struct BatchErrors { int scale; double* cov; double* sigma; int32_t* info; };
int check_errors(gfh_ctx* c, const char* who, const BatchErrors& e) {
  const std::string w(who);
  if (!e.cov || !e.sigma || !e.info) return fail(c, w + ": null argument");
  if (e.scale != 0 && e.scale != 1)
    return fail(c, w + ": scale is 0 (the inverse of J^T J) or 1 (that times chi2 / dof), got " + std::to_string(e.scale));
  return 0;
}
size_t errors_bytes(int64_t nf, int na) { return sizeof(double) * (size_t)nf * ((size_t)na * na + na) + sizeof(int32_t) * (size_t)nf; }
void errors_out(const char* h, int64_t nf, int na, const BatchErrors& e) {
  const size_t cb = sizeof(double) * (size_t)nf * na * na, sb = sizeof(double) * (size_t)nf * na;
  memcpy(e.cov, h, cb); memcpy(e.sigma, h + cb, sb); memcpy(e.info, h + cb + sb, sizeof(int32_t) * (size_t)nf);
}
// gfh_k_batch_cov over the batch held at the parameter block `pars` of the device, into the block `out` (errors_bytes)
int launch_cov(gfh_ctx* c, ModelKernels* mk, int lanes, int na, int scale, void* pars, char* out) {
  const int64_t nf = c->batch.n_fits; const int per_wg = 256 / lanes;
  void* x = c->batch.x.p; void* y = c->batch.y.p; void* w = c->batch.w.p; void* off = c->batch.off_d.p;
  long long npts = c->batch.max_points;      // a cube's kernels take n_points where the ragged ones take the offsets (GFH_BARGS)
  void* cov = out; void* sigma = out + sizeof(double) * (size_t)nf * na * na; void* info = out + sizeof(double) * (size_t)nf * ((size_t)na * na + na);
  long long n = nf; void* stp = c->status.p;
  void* args[] = {&x, &y, &w, c->batch.cube ? (void*)&npts : (void*)&off, &pars, &scale, &cov, &sigma, &info, &n, &stp};
  HIPCHK(c, hipModuleLaunchKernel(mk->batch_cov, (unsigned)((nf + per_wg - 1) / per_wg), 1, 1, 256, 1, 1, 0, c->stream, args, nullptr));
  c->batch.last_lanes = lanes; c->batch.last_form = data_form(c);
  return 0;
}
// The body of gfh_fit_batch and gfh_fit_batch_errors (errors: NULL, or where the second launch's outputs go), under the caller's name
int fit_batch(gfh_ctx* c, const char* who_, double* pars, int na, const int32_t* active, const gfh_fit_options* o, gfh_batch_result* results,
              double* seconds, const BatchErrors* errors) {
  const std::string who(who_);
  if (check_context(c, who_) || check_model(c, who_, na, active)) return 1;
  if (!pars || !results) return fail(c, who + ": null argument");
  if (errors && check_errors(c, who_, *errors)) return 1;
  gfh_fit_options defaults; memset(&defaults, 0, sizeof defaults);
  if (!o) o = &defaults;
  // the options of gadf_fit a device-resident loop does not carry
  if (o->has_uphill && o->uphill != 0) return fail(c, who + ": uphill != 0 is not carried by the batch kernel");
  if (o->has_nielsen && o->nielsen) return fail(c, who + ": the nielsen lambda strategy is not carried by the batch kernel");
  if (o->has_umnigh && o->umnigh) return fail(c, who + ": the umnigh lambda strategy is not carried by the batch kernel");
  if (o->has_grad_chi2) return fail(c, who + ": the grad_chi2 test is not carried by the batch kernel");
  if (o->has_cos_phi) return fail(c, who + ": the cos_phi test is not carried by the batch kernel");
  if (o->has_rel_error_global) return fail(c, who + ": rel_error_global has no meaning for independent fits");
  LmOptions lo;
  if (const char* refusal = resolve_lm_options(*o, &lo)) return fail(c, refusal);                        // gadfit.F90:575-578
  if (!o->has_max_iter || o->max_iter < 0) return fail(c, who + ": max_iter is required (a loop that runs on the device must be bounded)");
  if (check_geometry(c, who_, na) || check_frames(c, who_)) return 1;
  BatchOpts bo; memset(&bo, 0, sizeof bo);
  bo.lambda = lo.lambda; bo.lam_up = lo.lam_up; bo.lam_down = lo.lam_down; bo.lam_incs = lo.lam_incs;      // gadfit.F90:568-584 (lm_options.h)
  bo.use_accth = lo.use_accth; bo.accth = o->accth;
  bo.has_chi2_abs = o->has_chi2_abs != 0; bo.chi2_abs = o->chi2_abs;
  bo.has_chi2_rel = o->has_chi2_rel != 0; bo.chi2_rel = o->chi2_rel;
  bo.has_rel_error = o->has_rel_error != 0; bo.rel_error = o->rel_error;
  bo.has_max_iter = 1; bo.max_iter = o->max_iter;
  bo.damp_plain = lo.damp_plain;
  if (o->DTD_min) for (int j = 0; j < na; j++) bo.dtd_min[j] = o->DTD_min[j];                            // gadfit.F90:641-646 (the same for every fit)
  NEED_GPU(c);
  if (!c->batch.on_device) return fail(c, who + ": no batch data on the device (gfh_set_batch_data, gfh_set_batch_cube)");
  gfh::Range range("gadfit gfh_fit_batch");
  ModelKernels* mk = nullptr;
  const int lanes = batch_lanes(c, na), per_wg = 256 / lanes;
  if (batch_kernels(c, std::vector<int32_t>(active, active + na), lanes, true, &mk)) return 1;
  const int64_t nf = c->batch.n_fits; const int np = c->model.n_pars;
  const size_t pb = sizeof(double) * (size_t)nf * (size_t)np, rb = sizeof(gfh_batch_result) * (size_t)nf;
  const size_t eb = errors ? errors_bytes(nf, na) : 0;          // [pars | records | covariances, standard errors, info]: one block, one copy back
  if (dev_alloc(c, c->batch.io, pb + rb + eb)) return 1;
  c->batch.host.resize(pb + rb + eb);
  harvest_events(c);
  HIPCHK(c, hipMemcpyAsync(c->batch.io.p, pars, pb, hipMemcpyHostToDevice, c->stream));
  void* x = c->batch.x.p; void* y = c->batch.y.p; void* w = c->batch.w.p; void* off = c->batch.off_d.p;
  long long npts = c->batch.max_points;      // a cube's kernels take n_points where the ragged ones take the offsets (GFH_BARGS)
  void* dp = c->batch.io.p; void* recs = c->batch.io.as<char>() + pb; long long n = nf; void* stp = c->status.p;
  void* args[] = {&x, &y, &w, c->batch.cube ? (void*)&npts : (void*)&off, &dp, &bo, &recs, &n, &stp};
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  HIPCHK(c, hipModuleLaunchKernel(mk->fit_batch, (unsigned)((nf + per_wg - 1) / per_wg), 1, 1, 256, 1, 1, 0, c->stream, args, nullptr));
  c->batch.last_lanes = lanes; c->batch.last_form = data_form(c);
  if (errors && launch_cov(c, mk, lanes, na, errors->scale, dp, c->batch.io.as<char>() + pb + rb)) return 1;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipMemcpyAsync(c->batch.host.data(), c->batch.io.p, pb + rb + eb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(pars, c->batch.host.data(), pb);
  memcpy(results, c->batch.host.data() + pb, rb);
  if (errors) errors_out(c->batch.host.data() + pb + rb, nf, na, *errors);
  if (seconds) *seconds = 1e-3 * ev_ms(c->ev[0], c->ev[1]);
  return 0;
}

}  // namespace

extern "C" {

// The spectra of a batch, back to back: fit f owns points [offsets[f], offsets[f + 1]) of x, y, w (w: the weights as used in
// (y - f) * w, gadfit.F90:682-683).  Replaces the batch the context held.  The geometry is checked and kept before the device is
// asked for, so a compile-only context ends in "no GPU" with the geometry known to the argument checks of the launches.
int gfh_set_batch_data(gfh_ctx* c, int64_t n_fits, const int64_t* offsets, const double* x, const double* y, const double* w) try {
  if (check_context(c, "gfh_set_batch_data")) return 1;
  if (n_fits < 1) return fail(c, "gfh_set_batch_data: a batch holds at least one fit");
  if (n_fits > ((int64_t)1 << 31) - 4) return fail(c, "gfh_set_batch_data: more fits than one launch takes (2^31 - 4)");
  if (!offsets || !x || !y || !w) return fail(c, "gfh_set_batch_data: null argument");
  if (offsets[0] != 0) return fail(c, "gfh_set_batch_data: offsets must begin at 0");
  int64_t shortest = offsets[1] - offsets[0], longest = shortest;
  for (int64_t f = 0; f < n_fits; f++) {
    if (offsets[f + 1] < offsets[f]) return fail(c, "gfh_set_batch_data: offsets must ascend (fit " + std::to_string((long long)f) + " ends before it begins)");
    shortest = std::min(shortest, offsets[f + 1] - offsets[f]); longest = std::max(longest, offsets[f + 1] - offsets[f]);
  }
  if (join_pending(c)) return 1;
  if (c->device >= 0 && c->batch.on_device) { hipSetDevice(c->device); if (c->stream) hipStreamSynchronize(c->stream); }
  batch_free(c); frames_end(c);
  c->batch.cube = false; c->batch.y_type = c->batch.error_type = 0;
  c->batch.n_fits = n_fits; c->batch.off.assign(offsets, offsets + n_fits + 1); c->batch.min_points = shortest; c->batch.max_points = longest;
  NEED_GPU(c);
  const size_t n = (size_t)offsets[n_fits], nb = sizeof(double) * std::max<size_t>(n, 1);
  if (dev_alloc(c, c->batch.x, nb) || dev_alloc(c, c->batch.y, nb) || dev_alloc(c, c->batch.w, nb) ||
      dev_alloc(c, c->batch.off_d, sizeof(int64_t) * (size_t)(n_fits + 1))) return 1;
  copy_path_ready();
  if (n) {
    HIPCHK(c, hipMemcpyAsync(c->batch.x.p, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->batch.y.p, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->batch.w.p, w, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(c->batch.off_d.p, offsets, sizeof(int64_t) * (size_t)(n_fits + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch.on_device = true;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_batch_data: ") + e.what()); }

// The same batch as a cube (include/gadfit_hip.h): one grid x [n_points] for every spectrum, the samples y [n_fits][n_points] in
// y_type (0 double, 1 float, 2 uint16_t), the weights formed in the kernels' load by error_type's rule -- no weight array anywhere --
// or, under USER (4), w [n_fits][n_points] as used.  Replaces the batch the context held; geometry AND form are kept before the device
// is asked for.  The launches below work on whichever data is held: a cube's kernels are translation units of their own.
int gfh_set_batch_cube(gfh_ctx* c, int64_t n_fits, int64_t n_points, const double* x, const void* y, int y_type, int error_type,
                       const double* w) try {
  if (check_context(c, "gfh_set_batch_cube")) return 1;
  if (check_cube(c, "gfh_set_batch_cube", !x || !y, "x and y are", n_fits, n_points, y_type, error_type, w != nullptr)) return 1;
  if (join_pending(c)) return 1;
  if (c->device >= 0 && c->batch.on_device) { hipSetDevice(c->device); if (c->stream) hipStreamSynchronize(c->stream); }
  batch_free(c); frames_end(c);
  c->batch.cube = true; c->batch.y_type = y_type; c->batch.error_type = error_type;
  c->batch.n_fits = n_fits; c->batch.off.clear(); c->batch.min_points = c->batch.max_points = n_points;
  NEED_GPU(c);
  const size_t n = (size_t)n_fits * (size_t)n_points, yb = n * (y_type == 0 ? 8 : y_type == 1 ? 4 : 2);
  if (dev_alloc(c, c->batch.x, sizeof(double) * (size_t)n_points) || dev_alloc(c, c->batch.y, yb)) return 1;
  if (w && dev_alloc(c, c->batch.w, sizeof(double) * n)) return 1;
  copy_path_ready();
  HIPCHK(c, hipMemcpyAsync(c->batch.x.p, x, sizeof(double) * (size_t)n_points, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->batch.y.p, y, yb, hipMemcpyHostToDevice, c->stream));
  if (w) HIPCHK(c, hipMemcpyAsync(c->batch.w.p, w, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch.on_device = true;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_batch_cube: ") + e.what()); }

// A cube that arrives frame by frame (include/gadfit_hip.h): instruments deliver F [n_points][n_fits], one image per abscissa with
// the pixel index fastest.  begin is gfh_set_batch_cube without the samples -- the same checks, the same state, the same blocks --
// and marks every frame as missing; gfh_batch_frames_put uploads a piece as it is stored and k_frames_to_cube (frames.hip)
// transposes it into the cube's columns.  Once no frame is missing nothing downstream knows where the cube came from.
int gfh_batch_frames_begin(gfh_ctx* c, int64_t n_fits, int64_t n_points, const double* x, int y_type, int error_type) try {
  if (check_context(c, "gfh_batch_frames_begin")) return 1;
  if (check_cube(c, "gfh_batch_frames_begin", !x, "x is", n_fits, n_points, y_type, error_type, -1)) return 1;
  std::vector<unsigned char> flags((size_t)n_points, 0);          // (before anything is replaced: this can fail)
  if (join_pending(c)) return 1;
  if (c->device >= 0 && c->batch.on_device) { hipSetDevice(c->device); if (c->stream) hipStreamSynchronize(c->stream); }
  batch_free(c); frames_end(c);
  c->batch.cube = true; c->batch.y_type = y_type; c->batch.error_type = error_type;
  c->batch.n_fits = n_fits; c->batch.off.clear(); c->batch.min_points = c->batch.max_points = n_points;
  c->batch.frames = true; c->batch.frame_put.swap(flags); c->batch.frames_missing = n_points;
  NEED_GPU(c);
  const size_t n = (size_t)n_fits * (size_t)n_points;
  if (dev_alloc(c, c->batch.x, sizeof(double) * (size_t)n_points) || dev_alloc(c, c->batch.y, n * elem_bytes(y_type))) return 1;
  if (error_type == 4 && dev_alloc(c, c->batch.w, sizeof(double) * n)) return 1;
  copy_path_ready();
  HIPCHK(c, hipMemcpyAsync(c->batch.x.p, x, sizeof(double) * (size_t)n_points, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch.on_device = true;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_frames_begin: ") + e.what()); }

// Frames [first_frame, first_frame + n_frames) of the begun batch: y [n_frames][n_fits] in the begun sample type, w alike as doubles
// under USER.  In any order and any piece sizes; a frame put again holds the later data.  The piece is staged in blocks of its own
// size, which go when no frame is missing; the call returns after the stream has drained, so the caller's buffers are free again.
int gfh_batch_frames_put(gfh_ctx* c, int64_t first_frame, int64_t n_frames, const void* y, const double* w) try {
  if (check_context(c, "gfh_batch_frames_put")) return 1;
  if (!c->batch.frames)
    return fail(c, "gfh_batch_frames_put: no batch has been begun (gfh_batch_frames_begin; gfh_set_batch_data and gfh_set_batch_cube replace a begun batch)");
  const int64_t n_fits = c->batch.n_fits, n_points = c->batch.max_points;
  if (first_frame < 0) return fail(c, "gfh_batch_frames_put: first_frame is negative (" + std::to_string((long long)first_frame) + ")");
  if (n_frames < 1) return fail(c, "gfh_batch_frames_put: a piece holds at least one frame");
  if (first_frame > n_points - n_frames)
    return fail(c, "gfh_batch_frames_put: frames [" + std::to_string((long long)first_frame) + ", " + std::to_string((long long)first_frame) + " + " +
                   std::to_string((long long)n_frames) + ") reach past the " + std::to_string((long long)n_points) + " frames of the batch");
  if (!y) return fail(c, "gfh_batch_frames_put: null argument (y is required)");
  if (c->batch.error_type == 4 && !w) return fail(c, "gfh_batch_frames_put: error_type USER needs the weights w");
  if (c->batch.error_type != 4 && w) return fail(c, "gfh_batch_frames_put: w is taken under error_type USER alone (the other types form the weights from y on the device)");
  NEED_GPU(c);
  if (!c->batch.on_device) return fail(c, "gfh_batch_frames_put: the begun batch is not on the device (gfh_batch_frames_begin failed)");
  const size_t eb = elem_bytes(c->batch.y_type), ne = (size_t)n_frames * (size_t)n_fits;
  if (dev_alloc(c, c->batch.stage_y, ne * eb)) return 1;
  if (w && dev_alloc(c, c->batch.stage_w, ne * sizeof(double))) return 1;
  copy_path_ready();
  harvest_events(c);
  HIPCHK(c, hipMemcpyAsync(c->batch.stage_y.p, y, ne * eb, hipMemcpyHostToDevice, c->stream));
  if (w) HIPCHK(c, hipMemcpyAsync(c->batch.stage_w.p, w, ne * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  HIPCHK(c, launch_frames_to_cube(c->stream, (int)eb, c->batch.stage_y.p, n_frames, n_fits, c->batch.y.p, n_points, first_frame));
  if (w) HIPCHK(c, launch_frames_to_cube(c->stream, 8, c->batch.stage_w.p, n_frames, n_fits, c->batch.w.p, n_points, first_frame));
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch.frames_kernel_ms += ev_ms(c->ev[0], c->ev[1]);
  for (int64_t p = first_frame; p < first_frame + n_frames; p++)
    if (!c->batch.frame_put[(size_t)p]) { c->batch.frame_put[(size_t)p] = 1; c->batch.frames_missing--; }
  if (c->batch.frames_missing == 0) { dev_free(c->batch.stage_y); dev_free(c->batch.stage_w); }
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_frames_put: ") + e.what()); }

// begin + puts of a whole stack y [n_points][n_fits] (w alike under USER), frames_per_put frames each; 0: the largest count whose
// staging -- samples and weights -- stays within kFramesStageBytes, but at least one frame
int gfh_set_batch_frames(gfh_ctx* c, int64_t n_fits, int64_t n_points, const double* x, const void* y, int y_type, int error_type,
                         const double* w, int64_t frames_per_put) try {
  if (check_context(c, "gfh_set_batch_frames")) return 1;
  if (check_cube(c, "gfh_set_batch_frames", !x || !y, "x and y are", n_fits, n_points, y_type, error_type, w != nullptr)) return 1;
  if (frames_per_put < 0) return fail(c, "gfh_set_batch_frames: frames_per_put is negative (0: pieces of at most " +
                                         std::to_string((long long)(kFramesStageBytes >> 20)) + " MiB of staging)");
  if (gfh_batch_frames_begin(c, n_fits, n_points, x, y_type, error_type)) return 1;
  const int64_t per_frame = n_fits * (int64_t)(elem_bytes(y_type) + (w ? sizeof(double) : 0));
  const int64_t step = frames_per_put ? frames_per_put : std::max<int64_t>(1, kFramesStageBytes / per_frame);
  for (int64_t p = 0, k; p < n_points; p += k) {
    k = std::min(step, n_points - p);
    if (gfh_batch_frames_put(c, p, k, static_cast<const char*>(y) + (size_t)p * (size_t)n_fits * elem_bytes(y_type),
                             w ? w + (size_t)p * (size_t)n_fits : nullptr)) return 1;
  }
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_batch_frames: ") + e.what()); }

// frames of the begun batch not yet put; -1: the batch held was not begun by gfh_batch_frames_begin
int64_t gfh_debug_batch_frames_missing(gfh_ctx* c) { return c && c->batch.frames ? c->batch.frames_missing : -1; }
// device time of the transposing kernels of every put since the last gfh_batch_frames_begin, in seconds (HIP events)
double gfh_debug_batch_frames_seconds(gfh_ctx* c) { return c && c->batch.frames ? 1e-3 * c->batch.frames_kernel_ms : 0.0; }

// Elements [first, first + count) of the cube held, as stored (row-major [n_fits][n_points]): which 0 the samples in their type, 1
// the USER weights as doubles.  For tests that hold the cube's bytes; frames not yet put read as whatever the block held.
int gfh_debug_batch_read(gfh_ctx* c, int which, int64_t first, int64_t count, void* dst) try {
  if (check_context(c, "gfh_debug_batch_read")) return 1;
  if (c->batch.n_fits < 1 || !c->batch.cube) return fail(c, "gfh_debug_batch_read: the context holds no cube (gfh_set_batch_cube, gfh_batch_frames_begin)");
  if (which != 0 && which != 1) return fail(c, "gfh_debug_batch_read: which is 0 (the samples) or 1 (the USER weights)");
  if (which == 1 && c->batch.error_type != 4) return fail(c, "gfh_debug_batch_read: the cube holds weights under error_type USER alone");
  if (first < 0 || count < 0 || first > c->batch.n_fits * c->batch.max_points - count)
    return fail(c, "gfh_debug_batch_read: elements [first, first + count) reach past the cube");
  if (!dst) return fail(c, "gfh_debug_batch_read: null argument");
  NEED_GPU(c);
  if (!c->batch.on_device) return fail(c, "gfh_debug_batch_read: no batch data on the device");
  const size_t eb = which ? sizeof(double) : elem_bytes(c->batch.y_type);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (count) HIPCHK(c, hipMemcpy(dst, (which ? c->batch.w : c->batch.y).as<char>() + (size_t)first * eb, (size_t)count * eb, hipMemcpyDeviceToHost));
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_debug_batch_read: ") + e.what()); }

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
  if (check_context(c, "gfh_batch_covariance") || check_model(c, "gfh_batch_covariance", na, active)) return 1;
  const BatchErrors e{scale, cov, sigma, info};
  if (!pars) return fail(c, "gfh_batch_covariance: null argument");
  if (check_errors(c, "gfh_batch_covariance", e)) return 1;
  if (check_geometry(c, "gfh_batch_covariance", na) || check_frames(c, "gfh_batch_covariance")) return 1;
  NEED_GPU(c);
  if (!c->batch.on_device) return fail(c, "gfh_batch_covariance: no batch data on the device (gfh_set_batch_data, gfh_set_batch_cube)");
  ModelKernels* mk = nullptr;
  const int lanes = batch_lanes(c, na);
  if (batch_kernels(c, std::vector<int32_t>(active, active + na), lanes, true, &mk)) return 1;
  const int64_t nf = c->batch.n_fits;
  const size_t pb = sizeof(double) * (size_t)nf * (size_t)c->model.n_pars, eb = errors_bytes(nf, na);
  if (dev_alloc(c, c->batch.io, pb) || dev_alloc(c, c->batch.img, eb)) return 1;
  c->batch.host.resize(eb);
  HIPCHK(c, hipMemcpyAsync(c->batch.io.p, pars, pb, hipMemcpyHostToDevice, c->stream));
  if (launch_cov(c, mk, lanes, na, scale, c->batch.io.p, c->batch.img.as<char>())) return 1;
  HIPCHK(c, hipMemcpyAsync(c->batch.host.data(), c->batch.img.p, eb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  errors_out(c->batch.host.data(), nf, na, e);
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_covariance: ") + e.what()); }

// STEP 1 + 2 (gadfit.F90:675-699) of every spectrum at given parameters: J^T J [n_fits][na * na] (symmetric, both triangles),
// J^T r [n_fits][na], chi2 [n_fits] -- for callers with their own loop.
int gfh_batch_pass(gfh_ctx* c, const double* pars, int na, const int32_t* active, double* JTJ, double* JTres, double* chi2) try {
  if (check_context(c, "gfh_batch_pass") || check_model(c, "gfh_batch_pass", na, active)) return 1;
  if (!pars || !JTJ || !JTres || !chi2) return fail(c, "gfh_batch_pass: null argument");
  if (check_geometry(c, "gfh_batch_pass", na) || check_frames(c, "gfh_batch_pass")) return 1;
  NEED_GPU(c);
  if (!c->batch.on_device) return fail(c, "gfh_batch_pass: no batch data on the device (gfh_set_batch_data, gfh_set_batch_cube)");
  ModelKernels* mk = nullptr;
  const int lanes = batch_lanes(c, na), per_wg = 256 / lanes;
  if (batch_kernels(c, std::vector<int32_t>(active, active + na), lanes, true, &mk)) return 1;
  const int64_t nf = c->batch.n_fits; const int np = c->model.n_pars;
  const size_t rec = (size_t)na * na + na + 1;
  const size_t pb = sizeof(double) * (size_t)nf * (size_t)np, ib = sizeof(double) * (size_t)nf * rec;
  if (dev_alloc(c, c->batch.io, pb) || dev_alloc(c, c->batch.img, ib)) return 1;
  c->batch.host.resize(ib);
  HIPCHK(c, hipMemcpyAsync(c->batch.io.p, pars, pb, hipMemcpyHostToDevice, c->stream));
  void* x = c->batch.x.p; void* y = c->batch.y.p; void* w = c->batch.w.p; void* off = c->batch.off_d.p;
  long long npts = c->batch.max_points;
  void* dp = c->batch.io.p; void* img = c->batch.img.p; long long n = nf; void* stp = c->status.p;
  void* args[] = {&x, &y, &w, c->batch.cube ? (void*)&npts : (void*)&off, &dp, &img, &n, &stp};
  harvest_events(c);
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  HIPCHK(c, hipModuleLaunchKernel(mk->batch_pass, (unsigned)((nf + per_wg - 1) / per_wg), 1, 1, 256, 1, 1, 0, c->stream, args, nullptr));
  c->batch.last_lanes = lanes; c->batch.last_form = data_form(c);
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
// n_fits_eval) of the batch held, on their own points or on the caller's grid, by gfh_k_batch_eval (batch_eval.hip).  Everything the
// batch kernels do not carry is refused by the shared checks under this call's name, its own refusals follow, all before the device
// is asked for.  io = [pars | cov | x_eval] goes down in one copy, img = [model | residual | band] (the requested ones, each `tot`
// doubles) comes back in one.
int gfh_batch_eval(gfh_ctx* c, const double* pars, int na, const int32_t* active, const double* cov, const double* x_eval, int64_t n_eval,
                   int64_t first_fit, int64_t n_fits_eval, double* model, double* residual, double* band, double* seconds) try {
  if (check_context(c, "gfh_batch_eval") || check_model(c, "gfh_batch_eval", na, active)) return 1;
  if (!pars) return fail(c, "gfh_batch_eval: null argument (pars is required)");
  if (!model && !residual && !band) return fail(c, "gfh_batch_eval: no output requested (model, residual and band are all NULL)");
  if (band && !cov) return fail(c, "gfh_batch_eval: a band needs the fits' covariances (cov is NULL)");
  if (residual && x_eval) return fail(c, "gfh_batch_eval: a residual on a caller's grid has no meaning (residual is given on the fits' own points alone)");
  if (x_eval && n_eval < 1) return fail(c, "gfh_batch_eval: a grid holds at least one point (x_eval given with n_eval = " + std::to_string((long long)n_eval) + ")");
  if (!x_eval && n_eval != 0) return fail(c, "gfh_batch_eval: n_eval = " + std::to_string((long long)n_eval) + " without x_eval (NULL, 0: the fits' own points)");
  if (check_geometry(c, "gfh_batch_eval", na) || check_frames(c, "gfh_batch_eval")) return 1;
  const int64_t nf = c->batch.n_fits;
  if (first_fit < 0 || n_fits_eval < 1 || first_fit > nf - n_fits_eval)
    return fail(c, "gfh_batch_eval: fits [" + std::to_string((long long)first_fit) + ", " + std::to_string((long long)first_fit) + " + " +
                   std::to_string((long long)n_fits_eval) + ") are empty or reach past the " + std::to_string((long long)nf) + " fits of the batch");
  // the points of one output: the data's own layout, or [n_fits_eval][n_eval]
  const int64_t per_fit = x_eval ? n_eval : c->batch.max_points;
  const int n_out = (model ? 1 : 0) + (residual ? 1 : 0) + (band ? 1 : 0);
  if (per_fit > INT64_MAX / 8 / n_out / n_fits_eval) return fail(c, "gfh_batch_eval: the size of the outputs overflows");
  const int64_t tot = x_eval || c->batch.cube ? n_fits_eval * per_fit : c->batch.off[(size_t)(first_fit + n_fits_eval)] - c->batch.off[(size_t)first_fit];
  NEED_GPU(c);
  if (!c->batch.on_device) return fail(c, "gfh_batch_eval: no batch data on the device (gfh_set_batch_data, gfh_set_batch_cube)");
  gfh::Range range("gadfit gfh_batch_eval");
  ModelKernels* mk = nullptr;
  const int lanes = batch_lanes(c, na), per_wg = 256 / lanes;
  if (batch_kernels(c, std::vector<int32_t>(active, active + na), lanes, true, &mk)) return 1;
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
  void* x = c->batch.x.p; void* y = c->batch.y.p; void* w = c->batch.w.p; void* off = c->batch.off_d.p;
  long long npts = c->batch.max_points;      // a cube's kernels take n_points where the ragged ones take the offsets (GFH_BARGS)
  char* in = c->batch.io.as<char>(); char* out = c->batch.img.as<char>();
  void* dp = in; void* dc = cb ? in + pb : nullptr; void* dx = xb ? in + pb + cb : nullptr;
  size_t at = 0;
  void* dm = nullptr; void* dr = nullptr; void* db = nullptr;
  if (model) { dm = out + at; at += ob; }
  if (residual) { dr = out + at; at += ob; }
  if (band) { db = out + at; at += ob; }
  long long ne = n_eval, first = first_fit, n = n_fits_eval; void* stp = c->status.p;
  void* args[] = {&x, &y, &w, c->batch.cube ? (void*)&npts : (void*)&off, &dp, &dc, &dx, &ne, &first, &n, &dm, &dr, &db, &stp};
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  HIPCHK(c, hipModuleLaunchKernel(mk->batch_eval, (unsigned)((n_fits_eval + per_wg - 1) / per_wg), 1, 1, 256, 1, 1, 0, c->stream, args, nullptr));
  c->batch.last_lanes = lanes; c->batch.last_form = data_form(c);
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipMemcpyAsync(h, out, at, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  at = 0;
  if (model) { memcpy(model, h + at, ob); at += ob; }
  if (residual) { memcpy(residual, h + at, ob); at += ob; }
  if (band) { memcpy(band, h + at, ob); at += ob; }
  if (seconds) *seconds = 1e-3 * ev_ms(c->ev[0], c->ev[1]);
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_eval: ") + e.what()); }

// The generated source of the batch translation unit for the current model and an active set, as gfh_model_source: in the form of
// the context's setting (under auto: what the rule gives for the geometry held, 64 without one); gfh_batch_prepare alike.
int64_t gfh_batch_source(gfh_ctx* c, int na, const int32_t* active, char* buf, int64_t cap) try {
  if (check_context(c, "gfh_batch_source") || check_model(c, "gfh_batch_source", na, active)) return -1;
  std::string src, err;
  if (!generate_source(c->model, std::vector<int32_t>(active, active + na), batch_config(c, batch_lanes(c, na)), &src, &err)) { fail(c, err); return -1; }
  if (buf && cap > 0) { const size_t n = std::min<size_t>((size_t)cap - 1, src.size()); memcpy(buf, src.data(), n); buf[n] = 0; }
  return (int64_t)src.size() + 1;
} catch (const std::exception& e) { fail(c, std::string("gfh_batch_source: ") + e.what()); return -1; }

// Compiles the batch translation unit (or finds it in the cache) without launching, as gfh_model_prepare; needs no GPU.
int gfh_batch_prepare(gfh_ctx* c, int na, const int32_t* active) try {
  if (check_context(c, "gfh_batch_prepare") || check_model(c, "gfh_batch_prepare", na, active)) return 1;
  return batch_kernels(c, std::vector<int32_t>(active, active + na), batch_lanes(c, na), false, nullptr);
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_prepare: ") + e.what()); }

// Lanes per fit of the batch kernels from here on: 64 (the default) a wave per fit, 16 a DPP row per fit and four fits per wave, 256
// a workgroup per fit (few, long spectra), 0 auto -- gfh_batch_auto_lanes at every call, which chooses between 16 and 64 only.  A setting, not a launch: needs no GPU and no model.
int gfh_set_batch_lanes(gfh_ctx* c, int lanes) try {
  if (check_context(c, "gfh_set_batch_lanes")) return 1;
  if (lanes != 64 && lanes != 16 && lanes != 256 && lanes != 0)
    return fail(c, "gfh_set_batch_lanes: " + std::to_string(lanes) + " lanes per fit are not built (64: a wave per fit, 16: a row per fit, 256: a workgroup per fit, 0: auto)");
  c->batch.lanes = lanes;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_batch_lanes: ") + e.what()); }

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
