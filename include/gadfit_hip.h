/* gadfit_hip.h -- C ABI of libgadfit_hip.so, the MI355X hot path of gadfit's LM fit.
 *
 * The reference (raullaasner/gadfit v2.0.1) has no FFI seam for this path: STEP 1 / STEP 2
 * and chi2() are inline code of gadf_fit (fortran/gadfit/gadfit.F90:674-701, 1015-1034).
 * This header IS the seam: each entry point names the reference code it replaces.  Plain
 * pointers and sizes only; all host arrays remain caller-owned; every call returns 0 on
 * success and non-zero on error (message via gfh_last_error) -- the Fortran wrapper turns
 * that into `call error(__FILE__, __LINE__, msg)` (messaging.f90:32-41 convention).
 *
 * Threading: one host thread per context (the reference is single-threaded per image).
 * One context drives one GPU; N processes (one per GPU) form a communicator over RCCL
 * (replaces the coarray images + co_sum of misc.F90:133-170).
 */
#ifndef GADFIT_HIP_H
#define GADFIT_HIP_H
#include <stdint.h>
#include "gadfit_tape.h"

#ifdef __cplusplus
extern "C" {
#endif
/* libgadfit_hip.so is built with -fvisibility=hidden: what this header declares is the library's whole dynamic symbol table
 * (tests/test_cpu_cabi.py compares `nm -D` with it). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct gfh_ctx gfh_ctx;

/* ---- lifetime: replaces ad_init_reverse (AD:272-313) / gadf_close (gadfit.F90:1399-1412).
 * A destroyed context leaves its stream, events, pinned buffers and small device blocks (up to 4 MB each, 64 MB per device) to the
 * next context created on the same device in this process (a batch of small fits, gadf_init ... gadf_close each: 3.6 ms of runtime
 * calls per cycle otherwise); everything larger goes back to the runtime at once.  GADFIT_HIP_POOL=0 switches that off. */
int  gfh_create(int device, gfh_ctx** ctx);
/* The same, returning at once: the device part of the creation -- the HIP runtime's own start-up, 80 ms per process and 240 ms for the
 * first process on a machine, then stream, events, mailbox -- runs on a thread of the context while the caller goes on with host work
 * (gadf_init ... gadf_set, then the recording of eval() in the first gadf_fit: ad_init_reverse, AD:272-313, costs the reference nothing
 * comparable).  The first call that needs the device waits for it and reports its failure, if any ("no HIP device available ...");
 * gfh_set_data_begin queues its upload behind it without waiting.  device < 0 and GADFIT_HIP_ASYNC_INIT=0: plain gfh_create. */
int  gfh_create_begin(int device, gfh_ctx** ctx);
void gfh_destroy(gfh_ctx* ctx);
const char* gfh_last_error(const gfh_ctx* ctx);          /* ctx may be NULL: last global error */

/* ---- single-process device group: num_images() images of the reference as one context per GPU,
 * each driven by its own host thread, behind ONE handle (a plain Fortran program on a multi-GPU node,
 * no launcher).  n_devices <= 0: every visible device; devices == NULL: 0 .. n_devices-1.  The
 * handle takes every call of this header; a call runs on all members at once: gfh_set_data splits the
 * concatenated point array by gfh_partition (gadfit.F90:977-983), passes and whole fits (gfh_fit: the
 * LM loop replicated per member, as per image) sum J^T J / J^T r / chi2 / J^T omega over the members
 * -- co_sum, misc.F90:133-170 -- with RCCL all-reduces over xGMI (ncclCommInitAll; the default wherever every member has a
 * card of its own), or under GADFIT_HIP_GROUP_REDUCE=host (and for members that share a card) on the host in rank order from
 * the members' pinned result mailboxes (identical bits on every member).
 * Outputs are member 0's; gfh_get_residuals / _jacobian / _omega return the whole arrays.  Not available
 * on a group handle: gfh_comm_init, gfh_debug_set_rank, gfh_set_data_local, gfh_set_aux_local. */
int  gfh_create_group(int n_devices, const int* devices, gfh_ctx** ctx);
int  gfh_group_size(const gfh_ctx* ctx);                  /* members of a group handle; 1 for a plain context */
/* Test hook (CPU tests of the group's host sum: a group whose devices are all -1 has compile-only members): member r
 * sums bufs[r][0..n) over the members in rank order, in place; status[r] becomes the maximum over the members;
 * member fail_member (>= 0) fails before the barrier and the others must return an error too. */
int  gfh_debug_group_allreduce(gfh_ctx* ctx, double* bufs, int n, int* status, int fail_member);
/* Host cost of the group's machinery, measured by the library itself (no Python between the calls): out2[0] = microseconds per
 * sum of n doubles over the members inside ONE task, as the passes of a gfh_fit on a group handle pay it (`rounds` sums back to
 * back); out2[1] = microseconds per fan-out of an empty call to the member threads (what every call on the handle pays once).
 * Works on groups of compile-only members too (tools/probes/group_latency.py, profiles/r04_scaling_model.md). */
int  gfh_debug_group_latency(gfh_ctx* ctx, int n, int rounds, double* out2);
/* What ONE cross-rank sum (co_sum, misc.F90:133-170; call sites gadfit.F90:700-701, 735, 1032) of n doubles + the status slot costs on
 * this context's own path, measured by the library: ncclAllReduce on its RCCL communicator (one process per GPU after gfh_comm_init, or
 * the members of a device group under ncclCommInitAll), else the group's ordered host sum.  COLLECTIVE: every rank (or the group handle)
 * calls it with the same n and rounds.  out6[0..3] = median, 95th percentile, shortest, longest microseconds of the sum alone -- between
 * two HIP events on the otherwise idle stream of the context (host sum: host clock) --, out6[4] = median microseconds on the host clock
 * from enqueueing the sum to its numbers lying in the host mailbox (all-reduce + publish + flag: what a pass adds to its kernel),
 * out6[5] = ranks the communicator (or the group) counts.  A context with neither fails.  (bench.py `allreduce_us`.) */
int  gfh_debug_allreduce_latency(gfh_ctx* ctx, int n, int rounds, double* out6);
int  gfh_version(void);

/* ---- communicator: replaces num_images()/this_image() + co_sum (misc.F90:133-170).
 * id is a 128-byte opaque RCCL unique id created by rank 0 and distributed by the caller
 * (torch.distributed store, a file, ...).  Without gfh_comm_init the context is 1 image. */
#define GFH_UNIQUE_ID_BYTES 128
int  gfh_comm_unique_id(void* id);
int  gfh_comm_init(gfh_ctx* ctx, int nranks, int rank, const void* id);
/* Launcher-free variant for plain (Fortran) programs started once per GPU by a shell loop:
 * reads GADFIT_HIP_NRANKS / GADFIT_HIP_RANK and exchanges the id through the file named by
 * GADFIT_HIP_IDFILE (rank 0 writes it atomically, the others poll).  No-op without the variables. */
int  gfh_comm_init_from_env(gfh_ctx* ctx);
/* How this context's cross-rank sums travel: *rccl_nranks = ranks of its RCCL communicator as RCCL reports them
 * (ncclCommCount; 0 = none: one image, or a device group summing on the host); *n_allreduce = all-reduces issued since
 * gfh_reset_timers.  Either pointer may be NULL. */
int  gfh_comm_info(gfh_ctx* ctx, int* rccl_nranks, int64_t* n_allreduce);
/* Test hook, needs no GPU: the share of the points and the layout of the all-reduced image [JTJ | JTres | chi2] (dense, or
 * pattern-only for global fits) as rank `rank` of `nranks` derives them from (n_total, data_positions, Jacobian_indices, dim).
 * out[0] length of the image, out[1] pattern-only (0/1), out[2] nnz, out[3] hash of the pattern and index tables -- the same
 * on every rank, which ncclAllReduce silently requires -- out[4] first point, out[5] point count, out[6] datasets held,
 * out[7] gram workgroups of this rank.  nz_row / nz_col (may be NULL; nz_cap entries): the (row <= col) pattern in the order
 * of the pattern-only image's leading nnz values. */
int  gfh_debug_packed_layout(int nranks, int rank, int64_t n_total, int n_datasets, const int64_t* data_positions, int n_act,
                             const int32_t* jac_idx, int dim, int sparse_ok, int64_t* out, int32_t* nz_row, int32_t* nz_col, int nz_cap);
/* Test hook: give the context the geometry of rank `rank` of `nranks` WITHOUT a communicator, so the
 * sharding (gfh_partition, per-dataset sub-ranges, local layout) can be exercised on one GPU; the
 * caller sums the per-rank results itself.  Must precede gfh_set_data. */
int  gfh_debug_set_rank(gfh_ctx* ctx, int nranks, int rank);

/* ---- partition: re_initialize STEP 2 (gadfit.F90:977-983) with equal image weights:
 * int(N/G) points each, remainder +1 to the first ranks; contiguous in the concatenated
 * [dataset 1 | dataset 2 | ...] order. */
void gfh_partition(int64_t n_total, int nranks, int rank, int64_t* begin, int64_t* count);

/* ---- the Gauss-Kronrod tables (gauss_kronrod_parameters.F90; numerical_integration.F90:139-171): roots[points], wk[points]
 * (Kronrod weights), wg[points / 2] (Gauss weights, for the even 1-based positions); points in {15, 21, 31, 41, 51, 61}, else 1.
 * Host data only -- what the generated kernels carry, handed to the Fortran layer's integrate() for evaluations of eval() outside
 * gadf_fit (gadf_print, gadfit.F90:1255-1397). */
int  gfh_gk_rule(int points, double* roots, double* wg, double* wk);

/* ---- data: replaces read_data (gadfit.F90:401-443) + re_initialize's img_bounds
 * (977-1002).  x, y, w: the GLOBAL concatenated arrays (w = weights as used in
 * (y-f)*w, i.e. after init_weights, gadfit.F90:445-470); data_positions: n_datasets+1
 * 0-based offsets.  The context uploads only its own rank's range. */
int  gfh_set_data(gfh_ctx* ctx, int64_t n_total, const double* x, const double* y,
                  const double* w, int n_datasets, const int64_t* data_positions);
/* The same, returning at once: geometry and small tables are set by the call, the N-sized copies run on a thread of the library
 * while the caller does host work of its own (the Fortran layer records eval() over the data meanwhile).  The arrays must stay
 * valid and unchanged until the NEXT call on this context, which waits for the upload and reports its failure, if any. */
int  gfh_set_data_begin(gfh_ctx* ctx, int64_t n_total, const double* x, const double* y,
                        const double* w, int n_datasets, const int64_t* data_positions);
/* A host-to-host copy of `bytes` bytes that the NEXT gfh_set_data_begin starts on a thread of its own, beside the upload (the
 * Fortran layer's private copy of the abscissas -- gadfit.F90:82-88 keeps x_data for later fits and gadf_print -- which is not needed
 * before this fit returns).  Nothing on the device waits for it; gfh_wait_host_copy does, and src / dst must stay valid until then. */
int  gfh_queue_host_copy(gfh_ctx* ctx, void* dst, const void* src, int64_t bytes);
int  gfh_wait_host_copy(gfh_ctx* ctx);
/* Same, but the caller passes only this rank's slice [begin, begin+count) as given by
 * gfh_partition (avoids materialising 1e8-point arrays on every rank). */
int  gfh_set_data_local(gfh_ctx* ctx, int64_t n_total, int n_datasets,
                        const int64_t* data_positions, int64_t begin, int64_t count,
                        const double* x_local, const double* y_local, const double* w_local);
/* Auxiliary per-point real inputs of the model (GFH_AUX nodes of the tape, gadfit_tape.h): n_aux columns,
 * column k = aux[k*n_total .. k*n_total + n_total) in the GLOBAL point order of gfh_set_data (the _local
 * variant takes this rank's slice, column stride = its count).  This is how real(kp) arithmetic on the
 * abscissa inside a Fortran eval() -- invisible to operator overloading, fitfunction.F90:59-63 -- reaches
 * the device: the recorder tabulates such values once per data point.  Call after gfh_set_data; new data
 * drops the columns.  A model with n_aux > 0 refuses to run until they are set. */
int  gfh_set_aux(gfh_ctx* ctx, int n_aux, const double* aux);
int  gfh_set_aux_local(gfh_ctx* ctx, int n_aux, const double* aux_local);
/* init_weights on the device from y (and sigma for USER), gadfit.F90:445-470.
 * error_type: 0 NONE, 1 SQRT_Y, 2 PROPTO_Y, 3 INVERSE_Y, 4 USER (w currently holds sigma). */
int  gfh_init_weights(gfh_ctx* ctx, int error_type);

/* ---- model: replaces the dynamic dispatch to fitfunc%eval (fitfunction.F90:47, 59-63).
 * The tape is copied.  Kernels are generated per (tape, active set) on first use, compiled
 * with hiprtc for gfx950 and cached on disk (GADFIT_HIP_CACHE or <libdir>/kcache). */
int  gfh_set_model(gfh_ctx* ctx, const gfh_tape* tape);
/* A model whose eval() BRANCHES.  The reference's `ad` module exports `>` and `<` on advar (automatic_differentiation.F90:
 * 315-395, values only) and gadf_fit evaluates eval() afresh at every point (gadfit.F90:679-690), so a piecewise model
 * (`if (x < pars(2)) ...`, max(p1, p2 x), a clipped term) simply takes its branch per point and per parameter set.  Here every
 * path through eval() that a recording has taken is one tape -- a VARIANT -- whose comparisons are guard nodes carrying the
 * outcome on that path (gadfit_tape.h, GFH_GUARD_*).  The device walks the variants' common decision tree per data point at the
 * CURRENT parameters and runs the body of the variant it arrives at; a breakpoint that is an active parameter moves points from
 * one variant to another between iterations without the host being involved.
 *   tapes[0 .. n_variants)  independent, complete tapes (same n_pars and quadrature settings); copied.  Tapes that take the same
 *                           path through eval() and differ only inside an INTEGRAND (an integrand comparing AD variables,
 *                           recorded with the integration variable at several places of its range) are pooled: one variant
 *                           whose integrand picks its recording per evaluation on the device (gfh_model_n_tapes counts them all).
 *   hint_aux                -1, or the auxiliary column (gfh_set_aux) holding, per data point, the index of the variant the point
 *                           took when the columns were tabulated.  Needed only when two variants part ways WITHOUT a guard
 *                           (a Fortran eval() branching on the plain real x, which no recorder sees): gfh_model_needs_hint.
 * gfh_set_model(ctx, t) == gfh_set_model_variants(ctx, 1, &t, -1). */
int  gfh_set_model_variants(gfh_ctx* ctx, int n_variants, const gfh_tape* const* tapes, int hint_aux);
/* One per-point variant column PER SET OF OUTCOMES (round 5), for the NEXT gfh_set_model_variants on this context (which must hand
 * over n_tapes tapes and a hint_aux >= 0; otherwise the call has no effect): cols[t] = the auxiliary column that holds, per data
 * point, the index of the tape the point follows when the comparisons of AD variables met on tape t's path come out as on tape t.
 * With the comparisons given, what is left to decide is plain-real control flow -- a function of the abscissa alone, whatever the
 * parameters: such a column is tabulated once, and a point whose comparison flips during a fit (a fitted breakpoint moving across it)
 * finds its leaf behind a fork without the host.  At a fork the walk reads the column of any recording that passes there, at a leaf
 * the column of the leaf's own outcomes, which must name the leaf (else the point is reported, as with the single column).  Tapes that
 * hold the same outcomes share a column. */
int  gfh_set_variant_hint_columns(gfh_ctx* ctx, int n_tapes, const int32_t* cols);
int  gfh_model_needs_hint(gfh_ctx* ctx);       /* 1: the current variants fork without a comparison; 0: they do not; -1: no model */
int  gfh_model_n_variants(gfh_ctx* ctx);
/* recordings the current model was made of (variants of eval() + further recordings of integrands that compare AD variables, which are
 * pooled into their call sites and do not count as variants) */
int  gfh_model_n_tapes(gfh_ctx* ctx);
/* A data point may take a turn through eval() that no recorded variant covers (a guard comes out the other way for the first time:
 * the parameters have moved, or the recordings sampled the data).  The kernels then raise status 3 and report the points (up to 120
 * per pass); the library calls `fn` -- on the calling thread (device groups: on the member's thread, one call at a time) --
 * with those points, expects it to extend the model (gfh_set_model_variants on `target`, and gfh_set_aux if columns change) and
 * repeats the pass.  Without a handler, or when the handler changes nothing, the call fails with a message naming the point.
 *   index[k]     global index of the point in the concatenated data (gadfit.F90:82)      dataset[k]  its dataset (0-based)
 *   x[k]         its abscissa
 *   path[k], n_guards[k]   outcomes of the comparisons the device evaluated before it left the recorded tree (bit j = outcome of
 *                the j-th comparison met): a recording of eval(x[k]) that FORCES these outcomes and decides the comparisons
 *                after them naturally yields the missing variant even where host and device values differ in the last bit
 *   pars         [n_datasets][n_pars] parameters of the pass.
 * n_points = 0 (all arrays NULL but pars): an INTEGRAND met a path through its comparisons of AD variables that no recording of it has
 * (status 2): the handler records eval() over a sample of the data again at these parameters -- the integration variable at several
 * places of its range -- and hands the extended model over; returning non-zero, or a model that gained nothing, ends in the error. */
typedef int (*gfh_unseen_handler)(void* user, gfh_ctx* target, int n_points, const int64_t* index, const int32_t* dataset,
                                  const double* x, const uint64_t* path, const int32_t* n_guards, const double* pars);
int  gfh_set_unseen_handler(gfh_ctx* ctx, gfh_unseen_handler fn, void* user);
/* A hook called before EVERY pass (gfh_sweep / gfh_chi2 / gfh_omega / gfh_aux, also those inside gfh_fit and gfh_lm_iterate) with the
 * [n_datasets][n_pars] parameter block the pass is about to use; it may rewrite PASSIVE entries in place.  This is how a real that a
 * Fortran eval() forms from the %val of a fitted parameter follows the parameters: the reference recomputes it whenever eval() runs
 * (gadfit.F90:679-690), the recorder cannot see inside plain real arithmetic, so the layer declares one passive pseudo-parameter per
 * such real (the tape reads it as GFH_VAL(GFH_PARAM(n)), gadfit_tape.h) and sets it here by calling eval() once per dataset at the
 * parameters of the pass.  Non-zero return: the pass fails.  Members of a device group call it one at a time. */
typedef int (*gfh_pars_hook)(void* user, gfh_ctx* target, double* pars);
int  gfh_set_pars_hook(gfh_ctx* ctx, gfh_pars_hook fn, void* user);
/* out4[0] = passes repeated because a point left the recorded decision tree, out4[1] = passes of quadrature models that replayed the
 * recorded meshes of the pass before them instead of bisecting again (same parameters: the sweep of an accepted step after the trial
 * chi2() there, STEP 3 after the sweep; bitwise the same results; GADFIT_HIP_MESH=0 switches the hand-over off), out4[2] = variants
 * of the model, out4[3] = the outer quadrature workspace the kernels currently carry (intervals) in the high 32 bits, the inner one in the low 32. */
int  gfh_get_counters(gfh_ctx* ctx, int64_t* out4);
/* Work count of the last recording pass of a model with integrate(), read back from the device's own mesh records: out4[0] = adaptive
 * integrals (data point x outermost call site) with a record, out4[1] = the bisections they made in all -- an integral that ends on n
 * intervals made n - 1 bisections: 2n - 1 Gauss-Kronrod panels on values, then n with the gradient in the reference
 * (numerical_integration.F90:236-284) --, out4[2] = integrals without a record (more than 63 bisections), out4[3] = call sites per point.
 * bench.py's algorithmic floor of BASELINE config 4 is formed from this.  Needs a GPU and a pass that recorded (gfh_sweep / gfh_chi2). */
int  gfh_debug_mesh_stats(gfh_ctx* ctx, int64_t* out4);
/* Device memory as this context sees it: out3[0] = free and out3[1] = total bytes of its card (hipMemGetInfo), out3[2] = bytes of the
 * context's pool of quadrature workspaces -- the user-sized interval workspaces of integrate() (numerical_integration.F90:40-51,
 * 128-134: heap arrays there) live in ONE allocation of the context, a slot per wave of a launch, once they exceed 8 KB of scratch per
 * lane; it is cut at the first pass that needs it, an error code if the card cannot provide it, and freed by gfh_destroy.  A group
 * handle reports member 0's card and the sum of the members' pools.  The blocks of a batch of independent fits (gfh_set_batch_data:
 * the spectra, their offsets, the parameter / result block and the images of gfh_batch_pass; after gfh_set_batch_cube the grid, the
 * samples in their narrow type and, under USER, the weights -- and nothing of the batch they replaced; while gfh_batch_frames_put
 * fills a cube, the staging blocks of a piece too) are counted in out3[2] as well. */
int  gfh_device_memory(gfh_ctx* ctx, int64_t* out3);
/* Generated HIP source for the current model and an active set (debug / AOT builds).
 * Returns bytes needed (including NUL); copies at most cap bytes. */
int64_t gfh_model_source(gfh_ctx* ctx, int n_act, const int32_t* active_pars, char* buf, int64_t cap);
/* Compile (or load from cache) without launching; usable without a GPU. */
int  gfh_model_prepare(gfh_ctx* ctx, int n_act, const int32_t* active_pars);
/* One translation unit into the kernel cache without loading it: the kernels a context that holds n_datasets datasets would load for
 * this active set (the parameter block by value while n_datasets * n_pars <= 480 doubles, else by pointer), with the Jacobian store
 * (store_jacobian != 0) or without it.  Usable without a GPU; not on a group handle. */
int  gfh_model_prepare_form(gfh_ctx* ctx, int n_act, const int32_t* active_pars, int n_datasets, int store_jacobian);

/* Selects the active set / column map ahead of the first sweep (gadfit.F90:586-631): loads
 * the kernels for it and sizes the device work arrays (re_initialize STEP 3, 1004-1011). */
int  gfh_set_active(gfh_ctx* ctx, const int32_t* active_pars, int n_act, const int32_t* jac_idx, int dim);

/* ---- STEP 1 + STEP 2 + co_sum (gadfit.F90:675-701): residuals, Jacobian, JTJ, JTres.
 * pars [n_datasets][n_pars]; active_pars: n_act 0-based parameter indices;
 * jac_idx [n_datasets][n_act] 0-based columns (Jacobian_indices, gadfit.F90:615-628);
 * JTJ dim*dim column-major (symmetric, both triangles filled), JTres dim, chi2 = sum res^2
 * at these parameters (free by-product).  Blocking; outputs are already summed over ranks.
 * J and res stay device-resident for gfh_omega / gfh_aux. */
int  gfh_sweep(gfh_ctx* ctx, const double* pars, const int32_t* active_pars, int n_act,
               const int32_t* jac_idx, int dim, double* JTJ, double* JTres, double* chi2);
/* ---- chi2() (gadfit.F90:1015-1034): all parameters passive; refreshes device res (except inside a gfh_fit under
 * keep_jacobian mode 2 whose options never read it, see gfh_set_keep_jacobian).  Same partition, thread-to-point map and
 * order of additions as the fused STEP 1+2 kernel: at the parameters of a sweep it returns bitwise that sweep's sum r^2. */
int  gfh_chi2(gfh_ctx* ctx, const double* pars, double* chi2);
/* ---- STEP 3 (gadfit.F90:715-735): omega_i = -f''_{delta1}(x_i) w_i in forward mode,
 * JTomega = J^T omega; delta1 length dim; pars = the parameters of the last gfh_sweep.  One kernel
 * (gfh_k_omega_jt) computes omega AND J^T omega, recomputing each point's Jacobian row in registers --
 * the stored J is not read (8*n_act B/point less traffic) and need not exist (gfh_set_keep_jacobian).
 * Models with integrate() and robust losses take the two-kernel path that reads the J of the last
 * gfh_sweep (env GADFIT_HIP_OMEGA_JT=0 forces it); both give bitwise the same J^T omega. */
int  gfh_omega(gfh_ctx* ctx, const double* pars, const double* delta1, double* JTomega);
/* ---- convergence reductions with the J of the last sweep and the res of the last
 * chi2/sweep: what=0: out[dim] = J^T res (gadfit.F90:849-850);
 * what=1: out[3] = {res.Jdelta, res.res, Jdelta.Jdelta} (gadfit.F90:865-874). */
int  gfh_aux(gfh_ctx* ctx, int what, const double* delta1, double* out);

/* ---- the LM driver gadf_fit (gadfit.F90:502-1035) on top of the calls above; the damped
 * solve (potr_f08, gadfit_linalg.F90:36-57) and the lambda logic run on the host. */
typedef struct gfh_fit_options {
  double lambda, lam_up, lam_down, accth, grad_chi2, cos_phi, rel_error, rel_error_global,
         chi2_rel, chi2_abs;
  int has_lambda, has_lam_up, has_lam_down, has_accth, has_grad_chi2, has_cos_phi,
      has_rel_error, has_rel_error_global, has_chi2_rel, has_chi2_abs;
  const double* DTD_min;   /* NULL = absent; length dim */
  int lam_incs, has_lam_incs;
  int uphill, has_uphill;
  int max_iter, has_max_iter;
  int damp_max, has_damp_max;
  int nielsen, has_nielsen;
  int umnigh, has_umnigh;
  int verbosity;           /* 0 silent, 1 one line per iteration on stdout */
  double umnigh_a;         /* in/out: the SAVEd local of gadfit.F90:515 */
} gfh_fit_options;

typedef struct gfh_fit_result {
  int iterations, dim, dof, exit_reason;
  double lambda, chi2;
  int n_sweeps, n_chi2, n_omega;   /* STEP 1+2 passes consumed, chi2 values requested, STEP 3 passes (the reference's counts) */
  int n_lookahead;                 /* how many of the n_chi2 trial values came from a look-ahead sweep */
  double seconds;          /* wall time of the main loop */
} gfh_fit_result;

/* Robust cost function of the C++ solver (c++/gadfit/lm_solver.h:76-83 `enum class Loss`,
 * lm_solver.cpp:255-284): STEP 1 scales the weighted residual and its Jacobian row by
 * sqrt(rho'(res^2)) (lm_solver.cpp:303-317); chi2() stays the plain sum (lm_solver.cpp:513-529).
 * The Fortran reference has no such option (= GFH_LOSS_LINEAR, the default). */
enum { GFH_LOSS_LINEAR = 0, GFH_LOSS_CAUCHY = 1, GFH_LOSS_HUBER = 2 };
int  gfh_set_loss(gfh_ctx* ctx, int loss);

/* Whether STEP 1 keeps the Jacobian in HBM.  The reference stores JacobianT because its STEP 2
 * is a separate matmul (gadfit.F90:689-698); the fused kernel forms J^T J / J^T r from registers,
 * so J is only read back by the grad_chi2 / cos_phi tests (849-850, 865-873), gfh_get_jacobian and --
 * for models with integrate() or a robust loss -- STEP 3 (J^T omega, gadfit.F90:734).  mode 1
 * (default): the Jacobian of the most recent sweep can always be read, bit for bit as if every sweep had written it.  gfh_sweep
 * and gfh_lm_iterate write it at every sweep.  Inside gfh_fit every sweep overwrites what the sweep before it wrote and nothing reads
 * it before the fit returns, so where the fused kernel serves the fit, the fit's options do not read J, load balancing is off, no
 * parameter hook is set and the buffer is large (Env GADFIT_HIP_DEFER_J_FROM, bytes; default 256 MB), only the sweeps that max_iter
 * guarantees to be the fit's last write it (the one handed to, or made by, the last permitted iteration, and the look-ahead sweep
 * that would be handed to it).  A fit that ends any other way owes the Jacobian: the first call that reads it (gfh_get_jacobian,
 * gfh_get_points, gfh_aux, a gfh_omega that reads J) launches the storing kernel at the parameters of the fit's most recent sweep, on
 * this rank alone (no collective), and repeats the chi2 pass that wrote the residual vector after that sweep, if one did, so that
 * gfh_get_residuals returns what it returned before.  Anything that invalidates a stored Jacobian (gfh_set_data, gfh_set_model,
 * another active set, this call with another mode) drops an owed one too.  Env GADFIT_HIP_DEFER_J=0: every sweep writes it.  mode 0: never (those calls then fail with a clear
 * message).  mode 2: gfh_fit writes it only when its options read it back, and likewise lets its chi2() passes skip the
 * residual store (res is read by the grad_chi2 / cos_phi tests and gfh_get_residuals only; a read-back of residuals that were
 * not kept fails with a clear message).  Without the store the sweep is bound by
 * the FP64 pipe instead of HBM writes and needs 8*n_act bytes per point less memory.
 * Env GADFIT_HIP_KEEP_J.  Results (J^T J, J^T r, chi2, res) are bitwise the same in all modes. */
int  gfh_set_keep_jacobian(gfh_ctx* ctx, int mode);
/* The deferred store of mode 1, counted since the context was created: out4[0] = sweeps inside fits that skipped the Jacobian store,
 * out4[1] = sweeps inside fits that wrote it, out4[2] = launches that materialised an owed Jacobian (not counted as sweeps by
 * gfh_get_timers), out4[3] = 1 while a Jacobian is owed.  A group handle reports member 0. */
int  gfh_debug_deferred(gfh_ctx* ctx, long long* out4);
/* Where the points lie and how the most recent gfh_sweep was dispatched (read-only; for tests that must know which path a case took):
 * out8[0] = padded slots on this rank, out8[1] = its gram workgroups, out8[2] = datasets that have at least one of them; of the most
 * recent sweep since the data were set (-1 each while there is none): out8[3] = 1 the fused sweep + Gram kernel, 0 the plain sweep and the
 * Gram launches, out8[4] = waves per workgroup of the fused kernel (0 when not fused), out8[5] = the tail mode it was handed (0: workgroup
 * partials and the reduce / assemble launches, 1: in-kernel tail into the packed image, 2: and into the host mailbox), out8[6] = 1 the
 * pattern-only image of a global fit, 0 the dense one, out8[7] = doubles of the parameter block passed by value as a kernel argument (0:
 * by pointer).  A group handle reports member 0. */
int  gfh_debug_layout(gfh_ctx* ctx, int64_t* out8);
/* Which kernels ran behind the model kernel, noted by the host at each launch (read-only; for tests that must know which instantiation
 * a case reached).  Of the most recent gfh_sweep: out[0] = the assembling step (0: none yet, 1: the fused kernel's own tail,
 * 2: k_gather_sum, 3: k_assemble_sparse, 4: k_assemble), out[2] = n, the number of Gram launches (0: the fused kernel formed the Gram
 * image), and from out[3] on six numbers per launch, as many launches as fit `cap` numbers: kind (0: k_gram_small<a>, 1: k_gram<a>,
 * 2: k_gram_block<a, b, sym>), a, b, sym, and the block's first row and column tile.  Of the most recent J^T v product (gfh_omega,
 * gfh_aux(0)): out[1] = its finish (0: none yet, 1: k_jtv_finish, 2: k_reduce_partials + k_assemble_vec and the copy).  cap >= 3.
 * A group handle reports member 0. */
int  gfh_debug_chain(gfh_ctx* ctx, int64_t* out, int cap);

/* load_balancing of gadf_fit -- "adaptive parallelism" (gadfit.F90:672-673, re_initialize 935-983): with more than
 * one rank (processes with a communicator, or the members of a device group) gfh_fit re-cuts the contiguous ranges
 * before every iteration from the device time each rank spent in the parallel parts (STEP 1+2, chi2, STEP 3) since the
 * last cut, by the reference's weight update; it pays when the cost per point varies along the array (adaptive
 * quadrature).  Every image of the reference holds all data, so there a new cut is free; here the library keeps a host
 * copy of the arrays given to gfh_set_data / gfh_set_aux (made by those calls while the option is on) and a cut that moves a share
 * by more than 1 % re-uploads the rank's points.  The look-ahead schedule is off while it is on.
 * gfh_repartition: the cut for given image weights [nranks] (same on every rank); gfh_rebalance: one measurement +
 * weight update + cut (collective; *moved = 1 when the ranges changed). */
int  gfh_set_load_balancing(gfh_ctx* ctx, int on);
int  gfh_repartition(gfh_ctx* ctx, const double* weights);
int  gfh_rebalance(gfh_ctx* ctx, int* moved);
/* current ranges [begin, begin+count) of the members of a group handle ([gfh_group_size] entries; one entry for a plain context) */
int  gfh_group_ranges(gfh_ctx* ctx, int64_t* begins, int64_t* counts);

/* use_ad of gadf_fit (gadfit.F90:501, 583-584; default 1).  0: every parameter stays passive; STEP 1 takes the
 * gradient by the reference's forward differences (grad_finite, fitfunction.F90:155-174: step = sqrt(epsilon)*p
 * as (p+step)-p, one extra value evaluation per active parameter; gadfit.F90:686-687) and STEP 3 the second
 * directional derivative by its central difference (dir_deriv_2nd_finite, fitfunction.F90:188-203, h =
 * epsilon**(1/4); gadfit.F90:725-728).  Same kernels otherwise (fused sweep + Gram, chi2, omega); a parameter
 * whose step underflows raises the reference's error. */
int  gfh_set_use_ad(gfh_ctx* ctx, int on);
/* use_ad = 0 for a model whose per-point columns (gfh_set_aux) follow the PARAMETERS -- reals a host eval() forms from parameter
 * values in plain arithmetic, up to a whole black-box function (what use_ad=.false. exists for, gadfit.F90:583-584): the reference's
 * forward differences call eval() at p + step e_j (fitfunction.F90:155-174), where those reals have moved.  on = 1: gfh_set_aux holds
 * 1 + n_active SETS of the model's n_aux columns, [set][column][point]; set 0 belongs to the parameters of the pass, set 1 + j to
 * p + step e_j for the j-th active parameter of gfh_sweep's list, step = sqrt(epsilon) p as (p + step) - p per dataset; evaluation j of
 * the differences reads set 1 + j.  The host fills the sets from a gfh_pars_hook.  gfh_chi2 reads set 0; gfh_omega is refused (its
 * central difference would need sets at p +- h delta).  Default 0. */
int  gfh_set_fd_column_sets(gfh_ctx* ctx, int on);

/* Look-ahead schedule of gfh_fit / gfh_lm_iterate (default 1; env GADFIT_HIP_LOOKAHEAD).
 * The reference evaluates chi2() at the trial parameters (gadfit.F90:753) and, after accepting,
 * sweeps the same parameters again for the Jacobian (675-701).  The fused sweep kernel returns
 * sum r^2 with J^T J / J^T r, so with look-ahead the first trial of an iteration runs the sweep
 * instead of chi2() and an accepted step hands J^T J / J^T r to the next iteration: one N-sized
 * pass per accepted iteration instead of two, same numbers; the chi2() before the loop (gadfit.F90:670)
 * likewise is the sum r^2 of the first iteration's sweep.  Armed from the start; a rejected first trial (its sweep
 * is thrown away) disarms it until 4 iterations in a row have accepted their first trial (8, 16, ... 64 after each further rejection
 * while armed: a fit that keeps rejecting runs the reference's schedule); retrials after a
 * rejection use chi2().  The sweep's sum r^2 is bitwise what chi2() returns at those parameters, so both schedules
 * see the same chi2 values, take the same decisions and return the same bits.  Not used together with the grad_chi2 /
 * cos_phi tests, which read the device's (old J, new res) pair, nor with a robust loss (the sweep's sum is then the
 * robust one), nor where that bitwise identity does not hold: the two-kernel STEP 1+2 path (models with integrate(), more
 * than 80 active parameters, GADFIT_HIP_FUSED=0) and GADFIT_HIP_FAST_DIV=0.  0 = the reference's schedule. */
int  gfh_set_lookahead(gfh_ctx* ctx, int on);

/* pars [n_datasets][n_pars] in/out; is_global [n_pars]. */
int  gfh_fit(gfh_ctx* ctx, double* pars, int n_act, const int32_t* active_pars,
             const int32_t* is_global, gfh_fit_options* opt, gfh_fit_result* res);

/* ---- Errors and curves of a plain fit: what gfh_batch_covariance and gfh_batch_eval give a fit of a batch, for gfh_fit's own path --
 * one fit, possibly global over several datasets.  Same definitions, same order of operations.
 *
 * gfh_covariance: the parameter covariance (J^T J)^-1 and the standard errors at pars [n_datasets][n_pars] (LMsolver::getJTJ /
 * getInvJTJ, lm_solver.cpp:551-585).  One STEP 1 + 2 pass through gfh_sweep's route -- the pars hook, a repeated pass after an unseen
 * path, the sum over ranks and device groups, the robust loss and finite differences as set -- then on the host (normal_eq.cpp) the
 * upper Cholesky factor of J^T J itself (no damping, no DTD; a pivot is accepted only if it is positive and finite), V = U^-1 and
 * C = V V^T with every entry formed once; for a global fit block by block through the arrow structure the damped solve uses
 * (gfh_solve_damped), where that applies.  cov [dim * dim], dense, both triangles, symmetric bit for bit, rows and columns in the
 * order of gfh_jacobian_indices; sigma [dim] = sqrt of its diagonal; *info 0, or j + 1 where the pivot of column j failed -- cov and
 * sigma are then NaN throughout (under the arrow form the local columns are eliminated first, so j may differ from the dense form's).
 * scale 0: the reference's getInvJTJ (under a robust loss the inverse of the scaled J^T J, as there); scale 1: every entry times
 * chi2 / dof, chi2 what gfh_chi2 returns at pars -- the sweep's own sum r^2 where that is bitwise the same (linear loss, fused
 * kernel: nothing more is launched), else a chi2 pass in front of the sweep -- and dof gfh_fit's (gadfit.F90:648-657; 1 where it
 * would be 0).  The context is left as gfh_sweep at pars leaves it.  A dim whose dense image cannot be allocated is refused.
 * gfh_fit_errors: gfh_fit, then gfh_covariance at the fitted parameters; pars and the result are gfh_fit's bits.
 * gfh_invert_normal: the algebra alone, without a context (host code, needs no GPU; errors through gfh_last_error(NULL)): JTJ
 * [dim * dim] symmetric, jac_idx [n_datasets][n_act]; use_structure as gfh_solve_damped; every entry times factor (1: as it is);
 * *form (may be NULL) 1 where the arrow form was taken, 0 the dense one. */
int  gfh_covariance(gfh_ctx* ctx, const double* pars, int n_act, const int32_t* active_pars, const int32_t* is_global, int scale,
                    double* cov, double* sigma, int32_t* info);
int  gfh_fit_errors(gfh_ctx* ctx, double* pars, int n_act, const int32_t* active_pars, const int32_t* is_global, gfh_fit_options* opt,
                    gfh_fit_result* res, int scale, double* cov, double* sigma, int32_t* info);
int  gfh_invert_normal(int dim, const double* JTJ, int n_datasets, int n_act, const int32_t* jac_idx, int use_structure, double factor,
                       double* cov, double* sigma, int32_t* info, int32_t* form);
/* gfh_eval: the fitted model, the weighted residuals and the 1-sigma band of the curve, computed on the device by generated kernels
 * of their own translation unit (gfh_k_eval, gfh_k_eval_band and on a grid gfh_k_eval_grid, gfh_k_eval_grid_band: device/eval.hip
 * behind the model's point functions) from the data the context holds.  pars [n_datasets][n_pars]; cov [dim * dim] as
 * gfh_covariance returns it with jac_idx [n_datasets][n_act] and dim of gfh_jacobian_indices (NULL without a band): dataset d's band
 * is formed with its n_act x n_act block cov[jac_idx[d][a]][jac_idx[d][b]], which holds its global and local columns and their coupling.
 *   x_eval NULL, n_eval 0: on the data's own points, this rank's gfh_local_count points in the order of gfh_get_residuals:
 *       model    = f(x_i; P_d)
 *       residual = (y_i - f) w_i, chi2()'s plain residual (gadfit.F90:682-683), also under a robust loss; without a band bit for bit
 *                  what gfh_get_residuals returns after gfh_chi2 at pars
 *       band     = sqrt(g^T C_d g), g[a] = df / dp_active_pars[a] (unweighted; under use_ad = 0 the sweep's forward difference):
 *                  t_a = sum_b C[a][b] g[b] with b ascending, s2 = sum_a g[a] t_a with a ascending, without contraction; a negative
 *                  s2 gives 0, NaN propagates -- a NaN cov gives NaN bands, model and residuals stay finite.
 *     Carried: plain and branching models (decided per point on the device; an unseen path is handled as gfh_chi2 handles it),
 *     auxiliary columns, the pars hook, automatic differentiation and use_ad = 0.
 *   x_eval [n_eval]: on a grid shared by all datasets, each with its own parameter row: model and band as [n_datasets][n_eval];
 *     residual must be NULL.  Carried: what the batch kernels carry -- one recorded path, no auxiliary columns.
 * model, residual, band: each may be NULL, at least one is not.  Without a band the value is computed without the gradient: the last
 * bits of model may differ between a call with a band and one without.  A band is carried up to 64 active parameters per dataset
 * and refused beyond, with the count.  Refused as well, each with its own message before the device is asked for: models with
 * integrate(), group handles and contexts that are one of several ranks.  The context's residuals, Jacobian and active set are left
 * as they were; the two blocks of the call (the covariance blocks and the grid; the outputs) are counted by gfh_device_memory.
 * *seconds (may be NULL) = device time of the kernel.
 * gfh_eval_source / gfh_eval_prepare: the generated source of that unit and its compilation without a launch, as gfh_model_source /
 * gfh_model_prepare (need no GPU).
 * Not built: a Fortran entry, outputs left on the device or in a narrow type, a prediction band that adds the noise term, curve
 * files as gadf_print writes them, gfh_eval over several ranks or a device group, models with integrate(). */
int  gfh_eval(gfh_ctx* ctx, const double* pars, int n_act, const int32_t* active_pars, const int32_t* jac_idx, int dim, const double* cov,
              const double* x_eval, int64_t n_eval, double* model, double* residual, double* band, double* seconds);
int64_t gfh_eval_source(gfh_ctx* ctx, int n_act, const int32_t* active_pars, char* buf, int64_t cap);
int  gfh_eval_prepare(gfh_ctx* ctx, int n_act, const int32_t* active_pars);
/* Bench hook: the kernel of every later gfh_eval of this context is launched n (1 ... 1000) times back to back, with the same arguments
 * and the same outputs, and *seconds is the device time of the last of them (tools/bench_eval.py: past the slow launches after an
 * idle gap).  1: as it was. */
int  gfh_debug_eval_launches(gfh_ctx* ctx, int n);

/* n_iter iterations of the basic LM scheme without convergence exits (bench / profiling):
 * each = gfh_sweep + damped solve + parameter update + chi2 at the trial parameters (gfh_chi2,
 * or with look-ahead the sweep at the trial point, which an accepted step hands to the next
 * iteration of the same call) + accept (lambda /= 10) or reject (restore, lambda *= 10),
 * damp_max DTD as gadfit.F90:702-710.
 * state3 in/out = {lambda, old_chi2 (<0: evaluate first), accepted count}; DTD in/out [dim]. */
int  gfh_lm_iterate(gfh_ctx* ctx, double* pars, int n_act, const int32_t* active_pars,
                    const int32_t* is_global, int n_iter, double* state3, double* DTD);

/* ---- Batched independent fits: MANY Levenberg-Marquardt fits of ONE model in ONE kernel launch -- a detector image, a
 * hyperspectral cube, a time series of decays.  Not a global fit with every parameter local: each fit has its own data, start
 * parameters, lambda history, accept / reject decisions and exit, so the loop of gadf_fit (gadfit.F90:670-915) runs on the device,
 * a wave per fit, and nothing returns to the host between iterations.
 * Carried: plain models (no integrate(), one recorded path, no auxiliary columns, no pars hook), automatic differentiation, the
 * linear loss, 1 to 8 active parameters, and the options lambda, lam_up, lam_down, lam_incs, accth, DTD_min (one vector for all
 * fits), damp_max, chi2_abs, chi2_rel, rel_error, max_iter (required: the loop must be bounded).  Everything else -- group handles,
 * communicators of several ranks, uphill, nielsen, umnigh, grad_chi2, cos_phi, rel_error_global -- is refused with a message of its
 * own before the device is asked for.
 *
 * gfh_set_batch_data: the spectra back to back; fit f owns points [offsets[f], offsets[f + 1]) of x, y, w, offsets[0] = 0 and
 * ascending; w are the weights as used in (y - f) * w (gadfit.F90:682-683).  Replaces the batch the context held; independent of
 * gfh_set_data. */
int  gfh_set_batch_data(gfh_ctx* ctx, int64_t n_fits, const int64_t* offsets, const double* x, const double* y, const double* w);
/* One record per fit.  exit_reason as gfh_fit_result (0 max_iter, 1 chi2_abs, 2 chi2_rel, 5 rel_error, 7 lambda raised lam_incs + 1
 * times in a row), and 8: the damped matrix of THIS fit was not positive definite (dpotrf's failure, gadfit_linalg.F90:36-57) -- it
 * ends with the parameters of its last accepted step while its neighbours go on.  n_sweeps, n_chi2, n_omega count STEP 1+2 passes,
 * chi2() values and STEP 3 passes by the reference's schedule. */
typedef struct gfh_batch_result { int iterations, exit_reason, n_sweeps, n_chi2, n_omega, dof; double lambda, chi2; } gfh_batch_result;
/* gadf_fit (gadfit.F90:502-1035) for every spectrum of the batch: pars [n_fits][n_pars] in/out (passive entries are read per fit),
 * results [n_fits]; *seconds (may be NULL) = device time of the launch.  The damped solve repeats gfh_fit's host solve operation for
 * operation, so a fit of the batch and gfh_fit on the same spectrum differ by the order of the point sums only. */
int  gfh_fit_batch(gfh_ctx* ctx, double* pars, int n_act, const int32_t* active_pars, const gfh_fit_options* opt,
                   gfh_batch_result* results, double* seconds);
/* STEP 1 + 2 (gadfit.F90:675-699) of every spectrum at given parameters, for callers with their own loop: JTJ [n_fits][n_act*n_act]
 * (symmetric, both triangles), JTres [n_fits][n_act], chi2 [n_fits]. */
int  gfh_batch_pass(gfh_ctx* ctx, const double* pars, int n_act, const int32_t* active_pars, double* JTJ, double* JTres, double* chi2);
/* Errors of a batch: each fit's parameter covariance and standard errors, computed on the device by a third kernel of the batch
 * translation units (gfh_k_batch_cov: STEP 1 + 2 at the parameters, the Cholesky factor of J^T J without damping, its inverse and
 * the product of the inverse with its transpose, in registers).  scale 0: cov = (J^T J)^-1, the reference's LMsolver::getInvJTJ;
 * scale 1: that times chi2 / dof with the chi2 and dof of the fit's record; any other value is refused.  cov [n_fits][n_act*n_act]
 * (symmetric bit for bit, both triangles), sigma [n_fits][n_act] = sqrt of cov's diagonal, info [n_fits]: 0, or j + 1 where pivot
 * j of the fit's factor was not positive and finite -- that fit's cov and sigma are NaN, its neighbours are unaffected.  Rows and
 * columns in the caller's order of active_pars.  NULL outputs are refused.
 * gfh_batch_covariance: at given parameters pars [n_fits][n_pars], on whichever batch data is held, with gfh_batch_pass's checks
 * and refusals under its own name; one launch, one copy back.
 * gfh_fit_batch_errors: gfh_fit_batch, then the covariance at the fitted parameters on the same stream -- the parameter block stays
 * on the device between the two launches and everything returns in one copy.  pars, results are the bits of gfh_fit_batch; *seconds
 * (may be NULL) = device time of both launches.
 * Not built: a Fortran entry, a covariance under a robust loss (a batch carries the linear loss alone).  The covariance of a plain
 * gfh_fit is gfh_covariance. */
int  gfh_batch_covariance(gfh_ctx* ctx, const double* pars, int n_act, const int32_t* active_pars, int scale, double* cov,
                          double* sigma, int32_t* info);
int  gfh_fit_batch_errors(gfh_ctx* ctx, double* pars, int n_act, const int32_t* active_pars, const gfh_fit_options* opt,
                          gfh_batch_result* results, int scale, double* cov, double* sigma, int32_t* info, double* seconds);
/* Bounds of a batch: gfh_fit_batch inside ONE box per batch, lower[n_act] <= p <= upper[n_act] in the order of active_pars, the same
 * for every fit; -inf / +inf: no bound on that side.  A projected Levenberg-Marquardt loop with an active set (the kernel
 * gfh_k_fit_batch_bounded, in a translation unit of its own): after STEP 1+2 an active parameter that sits on a wall (P_j == lower_j
 * or upper_j, exactly) while descent pushes through it (J^T r_j < 0 at the lower, > 0 at the upper wall) is pinned for that
 * iteration -- its row and column leave every damped solve, so its step is exactly 0 --, every trial point is clamped into the box
 * coordinate by coordinate, and a coordinate that sits on a bound does not hold the rel_error exit open.  Everything else is
 * gfh_fit_batch's loop: with no finite bound pars and results are that call's bits.  results as gfh_fit_batch; at_bound [n_fits]:
 * bit j set where the returned active parameter j == lower[j], bit 8 + j where it == upper[j].
 * Refused, each with its own message before the device is asked for, in this order: what gfh_fit_batch refuses of the context, the
 * model and the active set; NULL arguments; a box with a NaN bound, lower_j = +inf, upper_j = -inf or lower_j >= upper_j (make that
 * parameter passive instead); the options gfh_fit_batch refuses; no batch held or a spectrum too short; a start outside the box.
 * Not built: a box per fit, bounds on the plain gfh_fit, linear constraints, a covariance that knows the pinned set
 * (gfh_batch_covariance at the returned parameters is that of all active parameters), a Fortran entry. */
int  gfh_fit_batch_bounded(gfh_ctx* ctx, double* pars, int n_act, const int32_t* active_pars, const double* lower, const double* upper,
                           const gfh_fit_options* opt, gfh_batch_result* results, int32_t* at_bound, double* seconds);
/* Curves of a batch: the fitted model, the weighted residuals and the 1-sigma band of the curve, computed on the device by a fourth
 * kernel of the batch translation units (gfh_k_batch_eval) from the data held and the model's own point functions, for fits
 * [first_fit, first_fit + n_fits_eval) of the batch held.  pars [n_fits_eval][n_pars] and cov [n_fits_eval][n_act*n_act] (as
 * gfh_batch_covariance returns it; NULL without a band) hold the rows of the evaluated fits only: the caller slices.
 *   x_eval NULL, n_eval 0: on the fits' own points, in the data's own layout -- ragged (gfh_set_batch_data): flat arrays with fit f
 *     at offsets[f] - offsets[first_fit]; a cube: [n_fits_eval][n_points].
 *       model    = f(x_i; pars)
 *       residual = (y_i - f) w_i, with the weight as used (a cube's is formed from y by its error_type)
 *       band     = sqrt(g^T C g), g[a] = df / dp_active_pars[a] (unweighted), C the fit's cov: t_a = sum_b C[a][b] g[b] with b
 *                  ascending, s2 = sum_a g[a] t_a with a ascending, without contraction; a negative s2 gives 0, NaN propagates -- a
 *                  fit whose cov is NaN (info != 0 of gfh_batch_covariance) gets NaN bands, its model and residuals stay finite.
 *   x_eval [n_eval]: on a grid shared by all fits (finer than the data, or beyond its ends): model and band as
 *     [n_fits_eval][n_eval]; residual must be NULL.
 * model, residual, band: each may be NULL, at least one is not.  Without a band the value is computed without the gradient: the
 * last bits of model may differ between a call with a band and one without.  The three lane forms return the same bits.  With
 * gfh_batch_pass's checks and refusals under its own name; one upload, one launch (gfh_set_batch_lanes as elsewhere), one copy
 * back; *seconds (may be NULL) = device time of the kernel.
 * Not built: a Fortran entry, outputs in a narrow type or left on the device, a non-contiguous selection of fits, a prediction band
 * that adds the noise term.  The curves of a plain gfh_fit are gfh_eval. */
int  gfh_batch_eval(gfh_ctx* ctx, const double* pars, int n_act, const int32_t* active_pars, const double* cov,
                    const double* x_eval, int64_t n_eval, int64_t first_fit, int64_t n_fits_eval,
                    double* model, double* residual, double* band, double* seconds);
/* The generated source of the batch kernels (gfh_k_fit_batch, gfh_k_batch_pass, gfh_k_batch_cov, gfh_k_batch_eval: a translation unit of their own, behind the
 * model's point functions) as gfh_model_source, and its compilation without a launch as gfh_model_prepare (needs no GPU). */
int64_t gfh_batch_source(gfh_ctx* ctx, int n_act, const int32_t* active_pars, char* buf, int64_t cap);
int  gfh_batch_prepare(gfh_ctx* ctx, int n_act, const int32_t* active_pars);
/* ... and of the bounded unit (gfh_k_fit_batch_bounded behind the same point functions): the four kernels' unit does not hold it. */
int64_t gfh_batch_source_bounded(gfh_ctx* ctx, int n_act, const int32_t* active_pars, char* buf, int64_t cap);
int  gfh_batch_prepare_bounded(gfh_ctx* ctx, int n_act, const int32_t* active_pars);
/* Lanes per fit of the batch kernels, a setting of the context read by every later gfh_fit_batch, gfh_batch_pass, gfh_batch_source
 * and gfh_batch_prepare.  64 (the default): a wave per fit.  16: a DPP row of 16 lanes per fit, four fits per wave and sixteen per
 * workgroup -- for short spectra, where a wave per fit keeps most lanes on padding; the sums are reduced inside the row, fits of one
 * wave do not see each other, and every check and refusal is the same.  256: a workgroup of four waves per fit (grid = number of
 * fits) -- for few, long spectra, where a wave per fit walks each spectrum 64 points at a time and a batch of fewer fits than the card
 * has SIMDs leaves most of it idle; each wave sums its lanes, the four partial sums meet in LDS and are added in wave order, and every
 * check and refusal is again the same.  0: auto, gfh_batch_auto_lanes(n_act, longest spectrum of the
 * batch held; 64 where the context holds none).  Auto never chooses 256.  Any other value is refused.  All forms of an active set stay loaded side by side.
 * The forms add a fit's point sums in different orders: 16 and 64 return the same bits up to 16 points per spectrum, 64 and 256 up
 * to 64 points.  Measured against each other in profiles/batch_rows.json and profiles/batch_workgroup.json. */
int  gfh_set_batch_lanes(gfh_ctx* ctx, int lanes);
/* The auto rule: 16 or 64 from the active count and the longest spectrum alone, as measured (profiles/batch_rows.json). */
int  gfh_batch_auto_lanes(int n_act, int64_t longest_spectrum);
/* 64, 16 or 256: the form of the last batch launch of this context (0: none yet).  For tests that assert the dispatch. */
int  gfh_debug_batch_lanes(gfh_ctx* ctx);
/* The loss of every batch call from here on (it stays set, as gfh_set_batch_lanes; no GPU and no model needed): GFH_LOSS_LINEAR (the
 * default), GFH_LOSS_CAUCHY or GFH_LOSS_HUBER -- the reference's robust costs (lm_solver.cpp:255-284), as gfh_set_loss gives the plain
 * fit -- and a residual scale c > 0 (the f_scale of other least-squares libraries; 1: the reference's own).  With r = (y - f) w the
 * weighted residual and u = r / c, STEP 1+2 scale r and its Jacobian row by ls = sqrt(1 / (1 + u^2)) (Cauchy) or u^2 > 1 ?
 * sqrt(1 / |u|) : 1 (Huber); nothing is divided by c.  STEP 3's omega stays unscaled and its J^T omega takes the scaled rows.  chi2 stays
 * the plain sum r^2 everywhere: the trial chi2 of STEP 4, the acceptance test new < old (the reference's rule: a robust step is accepted
 * on the plain chi2), the record's chi2 and gfh_batch_pass's.  gfh_batch_covariance / gfh_fit_batch_errors invert J^T J of the scaled
 * Jacobian (the reference's getInvJTJ after a robust fit) and multiply, under scale 1, by the plain chi2 / dof as gfh_covariance does;
 * gfh_fit_batch_bounded pins on the sign of the scaled J^T r; gfh_batch_eval's residual stays the plain (y - f) w.  With c = 2^k every
 * sum equals 4^k times that of c = 1 with the weights times 2^-k: the same parameters, counts and lambda bit for bit.  A cube forms its
 * weights on the device, so c is the one way to move the threshold there.  Refused: an unknown loss; a scale that is NaN, infinite, or
 * not positive.  The context's gfh_set_loss != 0 stays refused by every batch call: a batch is built from its own settings.  One loss
 * and one scale per batch; the loss is part of the unit's text (units of all losses stay loaded side by side), 1 / c a kernel argument. */
int  gfh_set_batch_loss(gfh_ctx* ctx, int loss, double scale);
/* The setting as it stands: the loss (return value; -1: ctx is NULL) and *scale (may be NULL).  0 and 1.0 until it is set. */
int  gfh_get_batch_loss(gfh_ctx* ctx, double* scale);
/* The loss (return value; -1: none yet) and *scale (may be NULL) of the last batch launch of this context that sweeps. */
int  gfh_debug_batch_loss(gfh_ctx* ctx, double* scale);
/* What every batch call minimises from here on (it stays set, as gfh_set_batch_loss; no GPU and no model needed):
 * GFH_ESTIMATOR_LSQ (0, the default, and what a batch was before this setting) the weighted sum of squares chi2 = sum ((y - f) w)^2, or
 * GFH_ESTIMATOR_POISSON (1) the Poisson deviance D = 2 sum [f - y + y ln(y / f)] over the points whose weight is not 0 -- the
 * maximum-likelihood fit of counted data, where 1 / sqrt(y) weights bias the amplitudes low and a bin with y = 0 has no weight.  The
 * term of a point with y = 0 is 2 f; a term with f <= 0, y < 0 or an operand that is not finite is NaN.  The data form's weight is a mask
 * there and nothing more: give a cube error_type NONE (any rule works, but SQRT_Y then pays a sqrt and a division per point for nothing).
 * The loop runs by Fisher scoring: STEP 1+2 form J^T J = sum g g^T / f and J^T r = sum g (y - f) / f, the least-squares pass at the
 * weights 1 / sqrt(f(P)), so J^T J is positive semidefinite for every y >= 0, empty bins carry curvature, and its inverse, which
 * gfh_batch_covariance / gfh_fit_batch_errors return unchanged, is the Cramer-Rao covariance; under scale 1 it is multiplied by D / dof
 * (the quasi-Poisson factor).  D stands wherever chi2 stood: the first value, the acceptance test new < old (a NaN deviance is a
 * rejected trial), chi2_abs and chi2_rel, the record's chi2 and gfh_batch_pass's third output.  A fit that starts with a NaN deviance or
 * whose J^T J is not positive definite ends with exit reason 8; its neighbours go on.  gfh_fit_batch_bounded pins on the sign of
 * J^T r.  Refused by the launching calls, before the device is asked for: estimator 1 together with a batch loss != 0, with accth
 * (STEP 3's second derivative is that of the least-squares cost), and a residual from gfh_batch_eval (model and band are given).
 * Refused here: an unknown estimator.  One estimator per batch; it is part of the unit's text, and the text of a least-squares unit is
 * what it was.  Not built: other likelihoods, an estimator per fit, geodesic acceleration under it, a Fortran entry. */
enum { GFH_ESTIMATOR_LSQ = 0, GFH_ESTIMATOR_POISSON = 1 };
int  gfh_set_batch_estimator(gfh_ctx* ctx, int estimator);
/* The setting as it stands (-1: ctx is NULL); 0 until it is set. */
int  gfh_get_batch_estimator(gfh_ctx* ctx);
/* The estimator of the last batch launch of this context that sweeps (-1: none yet). */
int  gfh_debug_batch_estimator(gfh_ctx* ctx);
/* Device time of the kernel of this context's last gfh_batch_pass in seconds (HIP events around the launch; 0: none yet): the
 * yardstick tools/bench_batch.py --eval holds gfh_batch_eval's kernel against. */
double gfh_debug_batch_pass_seconds(gfh_ctx* ctx);
/* A batch as a data cube: n_fits spectra of n_points each on ONE abscissa grid x [n_points], the samples y [n_fits][n_points]
 * spectrum-major in the type y_type names -- 0 double, 1 float, 2 uint16_t, each of which converts to double exactly -- and the
 * weights formed from y on the device, inside the kernels' load, by error_type's rule (the numbers and expressions of
 * gfh_init_weights, gadfit.F90:445-470): 0 NONE 1, 1 SQRT_Y 1 / sqrt(y), 2 PROPTO_Y 1 / y (both 0 where |y| < 100 DBL_MIN),
 * 3 INVERSE_Y y, 4 USER.  Under 0 ... 3 no weight array exists anywhere and w must be NULL; under USER w [n_fits][n_points] is
 * required and holds the weights as used in (y - f) * w, the meaning of gfh_set_batch_data's w (NOT sigma).  The device holds
 * 8 n_points + (8, 4 or 2) n_fits n_points bytes (+ 8 per point under USER) against gfh_set_batch_data's 24 per point.
 * Replaces the batch the context held, ragged or cube, as gfh_set_batch_data replaces a cube.  gfh_fit_batch, gfh_batch_pass,
 * gfh_batch_source, gfh_batch_prepare and gfh_set_batch_lanes work on whichever data is held, with every check and refusal as it
 * is (the auto rule reads n_points as the longest spectrum); the cube forms are translation units of their own, one per (y_type,
 * error_type, lanes), with the LM loop's one text and another load, and return the bits of the ragged form fed x tiled, y widened
 * and gfh_init_weights' weights.  Refused, each with its own message, before the device is asked for: NULL x or y, n_fits < 1 or
 * n_points < 1, more fits than a launch takes, an unknown y_type or error_type, USER without w, w with another type, group handles
 * and communicators of several ranks.  A compile-only context keeps the geometry and the form, then ends in "no GPU". */
int  gfh_set_batch_cube(gfh_ctx* ctx, int64_t n_fits, int64_t n_points, const double* x, const void* y, int y_type,
                        int error_type, const double* w);
/* The data form of the last batch launch of this context: -1 none yet, 0 ragged (gfh_set_batch_data), else a cube:
 * 1 + y_type + 3 * error_type (1 ... 15).  For tests that assert the dispatch. */
int  gfh_debug_batch_form(gfh_ctx* ctx);
/* A cube from a stack of frames.  Instruments deliver a detector image followed over time, echoes per voxel or a hyperspectral cube
 * frame by frame, F [n_points][n_fits]: one image per abscissa with the pixel (fit) index fastest -- the transpose of what
 * gfh_set_batch_cube takes.  Here the frames are uploaded as they are stored and a small model-independent kernel (k_frames_to_cube,
 * gadfit_amd/csrc/frames.hip) transposes them through LDS into the cube's layout on the device; from there on the batch IS a cube:
 * its bytes, and from them the bits of gfh_fit_batch / gfh_batch_pass, are those of gfh_set_batch_cube on the transposed array, no
 * generated kernel differs, and gfh_debug_batch_form reports the same form.
 *
 * gfh_batch_frames_begin: geometry, grid, sample type and weight rule as gfh_set_batch_cube, with its checks in its order and
 * wording under this name (there is no y and no w to check yet).  Replaces the batch held; allocates x, the cube y and, under USER,
 * the cube w (counted by gfh_device_memory); marks all n_points frames as missing.  A compile-only context keeps geometry and form,
 * then ends in "no GPU".
 * gfh_batch_frames_put: frames [first_frame, first_frame + n_frames), y [n_frames][n_fits] in the begun sample type, w alike as
 * doubles under USER (else NULL).  Frames may come in any order and any piece sizes; a frame put again holds the later data.  The
 * piece is uploaded to staging blocks of its own size (counted by gfh_device_memory while they exist), transposed on the context's
 * stream, and the call returns after the stream has drained: the caller may reuse its buffers.  When a put leaves no frame missing
 * the staging blocks are freed and gfh_device_memory reports what gfh_set_batch_cube of the shape reports; a put into a complete
 * batch takes and frees its own staging.  Refused, each with its own message, before the device is asked for: no batch begun (or the
 * begun one replaced since by gfh_set_batch_data / gfh_set_batch_cube), first_frame < 0, n_frames < 1, a range past n_points, NULL
 * y, USER without w, w under another rule.
 * While frames are missing gfh_fit_batch and gfh_batch_pass are refused with a message that says how many of how many frames have not
 * been put; gfh_batch_source, gfh_batch_prepare and gfh_set_batch_lanes need no data and are unaffected.
 * gfh_set_batch_frames: begin + puts of a whole stack y [n_points][n_fits] (w alike under USER), frames_per_put frames each.
 * frames_per_put 0: the largest count whose staging, samples and weights together, stays within 256 MiB, but at least one frame;
 * negative values are refused, and so is everything gfh_set_batch_cube refuses.
 * Not built: a Fortran entry, pinned or overlapped uploads, frames with a row pitch, other sample types, cubes over several cards. */
int  gfh_batch_frames_begin(gfh_ctx* ctx, int64_t n_fits, int64_t n_points, const double* x, int y_type, int error_type);
int  gfh_batch_frames_put(gfh_ctx* ctx, int64_t first_frame, int64_t n_frames, const void* y, const double* w);
int  gfh_set_batch_frames(gfh_ctx* ctx, int64_t n_fits, int64_t n_points, const double* x, const void* y, int y_type, int error_type,
                          const double* w, int64_t frames_per_put);
/* Frames of the begun batch not yet put; -1: the batch held was not begun by gfh_batch_frames_begin. */
int64_t gfh_debug_batch_frames_missing(gfh_ctx* ctx);
/* Device time (HIP events) of the transposing kernels of every put since the last gfh_batch_frames_begin, in seconds. */
double gfh_debug_batch_frames_seconds(gfh_ctx* ctx);
/* Elements [first, first + count) of the cube held (row-major [n_fits][n_points]), as stored: which 0 the samples in their type,
 * 1 the USER weights as doubles.  For tests that hold the cube's bytes. */
int  gfh_debug_batch_read(gfh_ctx* ctx, int which, int64_t first, int64_t count, void* dst);

/* ---- Jacobian_indices / dim (gadfit.F90:615-631) as a helper for callers */
int  gfh_jacobian_indices(int n_datasets, int n_act, const int32_t* active_pars,
                          const int32_t* is_global, int32_t* jac_idx);
/* The damped normal-equation solve (JTJ + lambda DTD) out = rhs of gadfit.F90:711-713 as gfh_fit performs
 * it on the host.  jac_idx [n_datasets][n_act] as above; DTD is the diagonal [dim].  With
 * use_structure != 0 and several datasets the block-arrow structure of a global fit is used: the local
 * parameters of different datasets do not couple, so their blocks are factorised one by one and only
 * the Schur complement of the global parameters is dense (the reference factorises the whole matrix
 * densely, doc/user_guide.tex:222-235) -- the same solution up to rounding at a fraction of the host
 * time (dim 259: 0.55 ms -> 20 us).  use_structure = 0: dense Cholesky (blocked above dim 64). */
int  gfh_solve_damped(int n_datasets, int n_act, const int32_t* jac_idx, int dim, const double* JTJ,
                      const double* DTD, double lambda, const double* rhs, double* out, int use_structure);
/* potr_f08 (gadfit_linalg.F90:36-57): a n*n column-major (destroyed), b rhs -> solution */
int  gfh_potr(int n, double* a, double* b);

/* ---- timers (Jacobian_timer, linalg_timer, chi2_timer, omega_timer; gadfit.F90:109-110),
 * device time from HIP events, seconds accumulated since creation or gfh_reset_timers.
 * out[8] = {sweep kernel, gram kernel, reduce+assemble, allreduce, chi2 kernel,
 *           omega kernel, n_sweep_launches, n_chi2_launches}
 * An event record costs ~4 us of stream time (two per launch: 8 us of the 35 us a small fit's LM iteration takes), so the
 * level is selectable: 0 = none; 1 (default) = events around every 8th launch of each model kernel (sweep[+gram], chi2,
 * omega; every launch under adaptive load balancing), the reported sums scaled to the number of launches; 2 = every launch,
 * and also reduce+assemble and all-reduce (env GADFIT_HIP_TIMERS).  gfh_get_timer_spread counts the launches that were timed. */
int  gfh_get_timers(gfh_ctx* ctx, double* out8);
/* Placement of the Jacobian buffer (no reference counterpart: gadfit.F90:632-640 allocates JacobianT once per image).  The sweep is
 * bound by `n_act` concurrent column streams into this buffer, and how fast the part absorbs them depends on the physical pages
 * behind the allocation (0.41 ... 0.47 ms for the same 2.6 GB buffer over a row of fresh allocations).  Once `after` sweeps
 * (gfh_set_placement_after, default 48, 0 = at the first sweep) have written a (re)allocated buffer of 256 MB or more -- the
 * search costs 25-150 ms at the headline size, as much as 50-300 sweeps, and gains 5-10 % per sweep: a job that has run that long
 * is taken to run on; one ten-iteration fit never pays for it --
 * it is allocated up to `tries` times (default 16 = the most, 1 = take the first; all held at once, never beyond half of the card's
 * memory), each candidate timed with four launches of the kernel that is about to run, until one runs on the fast side -- judged
 * against this card's own device-to-device copy rate, measured inside the first candidate, and (round 6) never below 6.3 TB/s of
 * algorithmic traffic: slow pages under that copy would lower the bar for themselves; four candidates within 1.5 % of each other end
 * the search (a kernel bound by its arithmetic) --; the fastest is kept.  Round 6: while the kernel is still on the slow side the
 * four DATA arrays x, y, w, res are then re-placed as a set the same way (allocated anew, copied device to device, timed; up to
 * `tries` sets, four in a row without a gain end it): they are 32 of the kernel's 32 + 8 p bytes per point, and their pages decide
 * as much (GADFIT_HIP_PLACE_DATA=0: not).  Models with integrate() are not placed (their sweeps are bound by the quadrature).
 * gfh_get_placement: out8[0] = kernel time (ms) on the buffer in use, out8[1..6] = on the candidates that were freed (0 = none /
 * no placement ran), out8[7] = the measured copy rate in GB/s. */
int  gfh_set_placement_tries(gfh_ctx* ctx, int tries);
int  gfh_set_placement_after(gfh_ctx* ctx, int sweeps);
int  gfh_get_placement(gfh_ctx* ctx, double* out8);
int  gfh_set_timer_detail(gfh_ctx* ctx, int level);
/* Spread of the STEP 1(+2) kernel's launches since gfh_reset_timers: out[4] = {shortest, longest, last
 * duration in seconds, launches counted}.  Under sustained back-to-back launches an MI355X slows the
 * HBM-write-bound kernel by ~20 % against its first launches (power management): the shortest duration
 * is the kernel on a cool chip, the average (gfh_get_timers) is what a long fit sees. */
int  gfh_get_timer_spread(gfh_ctx* ctx, double* out4);
void gfh_reset_timers(gfh_ctx* ctx);

/* ---- bench / profiling hooks: launch kernels without the host round trip.
 * gfh_launch_sweep: the AD sweep kernel only (STEP 1) at the parameters already uploaded by
 * the last gfh_sweep; gfh_launch_gram: the JTJ/JTres kernel chain only (STEP 2).
 * Asynchronous on the context's stream; gfh_sync waits.  gfh_stream returns the hipStream_t. */
int  gfh_launch_sweep(gfh_ctx* ctx);
int  gfh_launch_gram(gfh_ctx* ctx);
int  gfh_launch_chi2(gfh_ctx* ctx);
int  gfh_sync(gfh_ctx* ctx);
void* gfh_stream(gfh_ctx* ctx);
/* event-timed repetition: runs `reps` launches of kernel `which` (0 sweep, 1 gram, 2 chi2,
 * 3 omega, 4 plain sweep, 5 fused sweep+gram, 6 omega + J^T omega, 7 J^T v from the stored Jacobian) on the context stream
 * between two HIP events; returns average ms per launch. */
int  gfh_time_kernel(gfh_ctx* ctx, int which, int reps, double* avg_ms);

/* ---- debug read-back (tests): local un-padded residuals (count) and Jacobian
 * [count][n_act] row-major (= JacobianT(dim,N) restricted to the active columns). */
int  gfh_get_residuals(gfh_ctx* ctx, double* res_out);
int  gfh_get_jacobian(gfh_ctx* ctx, double* jac_out);
/* The same for single points: index[k] = local index into this rank's range (gfh_local_begin / gfh_local_count); res_out[n] and/or
 * jac_out[n][n_act] (either may be NULL).  For checks at sizes where the whole Jacobian does not belong on the host. */
int  gfh_get_points(gfh_ctx* ctx, int n, const int64_t* index, double* res_out, double* jac_out);
/* Text data files of gadf_add_dataset(path) (gadfit.F90:212-215 counts the records that begin with a number with one list-directed read
 * each, gadfit.F90:422-437 then reads the first two or three numbers of every record; records that do not begin with a number are
 * skipped, blank ones are transparent).  gfh_read_columns parses the whole file once -- mapped, cut at line ends, a thread per piece;
 * Fortran's D/Q exponent letters, commas and r*c repeat counts understood -- and returns the number of data records; gfh_take_columns
 * copies the columns into the caller's arrays (w may be NULL; it is only written for n_columns = 3) and frees the handle.  A record
 * that begins with a number but holds fewer than n_columns values is an error (the reference would mis-align silently).  Host code:
 * needs no GPU and no context; errors through gfh_last_error(NULL).  GADFIT_HIP_READ_THREADS caps the threads. */
typedef struct gfh_columns gfh_columns;
int  gfh_read_columns(const char* path, int n_columns, gfh_columns** out, int64_t* n_points);
int  gfh_take_columns(gfh_columns* cols, double* x, double* y, double* w);
void gfh_free_columns(gfh_columns* cols);
/* The abscissas as uploaded, back into x_out[n_total] (the concatenated array of gfh_set_data): this rank's range; on a device-group
 * handle every member's, i.e. all of it.  (gadfit.F90:82-88 keeps x_data on the host; a host layer that prefers not to can read
 * the abscissas back from here.) */
int  gfh_get_abscissas(gfh_ctx* ctx, double* x_out);
int  gfh_get_omega(gfh_ctx* ctx, double* omega_out);
int  gfh_get_weights(gfh_ctx* ctx, double* w_out);                /* [local_count] the weights as the kernels use them (after gfh_init_weights, gadfit.F90:445-470) */
int64_t gfh_local_count(gfh_ctx* ctx);
int64_t gfh_local_begin(gfh_ctx* ctx);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
