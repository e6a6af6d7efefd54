// passes.cpp -- the three passes of an iteration and their recovery: STEP 1 + 2 (gfh_sweep), chi2 (gfh_chi2), STEP 3 (gfh_omega),
// the J^T v products behind gfh_aux, and what repeats a pass -- an unseen branch, an exhausted fast workspace, an unrecorded
// integrand path.  A pass sequences launch.cpp's launches and comm.cpp's sums; it allocates only through devmem.cpp.
#include "context_internal.h"
#include "group.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>

using namespace gfh;

// recorders (Fortran module state, the Python tracer) are not re-entrant: ONE callback into the host layer at a time, whichever it is --
// the parameter hook of one member of a device group must not run beside the unseen-branch handler of another
std::recursive_mutex gfh::g_handler_mutex;      // (recursive: a callback that makes a call which calls back stays on its own thread)

// kernels raise the status word (1: quadrature workspace exhausted, 2: an integrand met a path through its comparisons
// that no recording of it has, 3: a data point took a branch of eval() no recorded variant covers).  Queue its
// read-back; check after the stream synchronise.
static bool workspace_can_grow(const gfh_ctx* c) {
  return c->has_model && c->model.has_integrals() && (c->gen.ws_size < c->model.ws_size || c->gen.ws_size_inner < c->model.ws_size_inner);
}
int gfh::status_check(gfh_ctx* c, int st) {
  if (!st) { c->n_integrand_rounds = 0; return 0; }
  if (st == 3 && c->has_model && c->model.branching()) return kUnseen;       // (the status word and the report are read and cleared by recover_unseen)
  if (st == 1 && workspace_can_grow(c)) return kGrowWs;
  if (st == 2 && c->unseen_fn && c->n_integrand_rounds < 3) return kIntegrandPath;
  hipMemsetAsync(c->status.p, 0, sizeof(int), c->stream);
  hipStreamSynchronize(c->stream);
  if (st == 1) return fail(c, "Number of iterations was insufficient. Increase either workspace size or the error bound(s).");
  if (st == 2) return fail(c, "an integrand took a path through its comparisons of AD variables that no recording of it has (the recordings place the "
                               "integration variable at a few points of its range: record eval() at more abscissas or parameter values)");
  return fail(c, "device kernel reported status " + std::to_string(st));
}

// A point has left the recorded decision tree of a branching eval() (status 3; emit_branching.cpp, gfh_select): read the report, hand
// the points to the handler -- which records eval() there and extends the model -- and let the caller repeat the pass.  In a
// multi-rank run every rank comes here (the status word is part of the cross-rank sum); a rank whose own points were all covered
// has an empty report and simply repeats its pass, so the collectives stay in step.
static int recover_unseen(gfh_ctx* c, const double* pars) {
  gfh::Range range("gadfit unseen branch: record and extend the model");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned char> raw(kStatusBytes);
  HIPCHK(c, hipMemcpy(raw.data(), c->status.p, kStatusBytes, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemset(c->status.p, 0, sizeof(int)));
  HIPCHK(c, hipMemset(c->status.as<char>() + 64, 0, sizeof(unsigned)));
  if (++c->n_unseen_rounds > 4096) return fail(c, "a branching eval() keeps producing paths that were not recorded (4096 passes repeated)");
  unsigned cnt = 0; memcpy(&cnt, raw.data() + 64, sizeof cnt);
  const int n = (int)std::min<unsigned>(cnt, (unsigned)kUnseenCap);
  if (!n) return 0;
  const UnseenEntry* e = reinterpret_cast<const UnseenEntry*>(raw.data() + 128);
  std::vector<int64_t> index((size_t)n); std::vector<int32_t> ds((size_t)n), ng((size_t)n);
  std::vector<double> xs((size_t)n); std::vector<uint64_t> path((size_t)n);
  for (int k = 0; k < n; k++) {
    int64_t slot = e[k].slot;
    if (slot < 0 || slot >= c->n_slots) return fail(c, "corrupt report of an unseen branch");
    int d = 0;
    while (d + 1 < c->nd && slot >= c->ds_slot[(size_t)d + 1]) d++;
    const int64_t len = c->lb[(size_t)d + 1] - c->lb[(size_t)d];
    int64_t off = slot - c->ds_slot[(size_t)d];
    if (off >= len) off = len - 1;                          // a pad slot repeats its dataset's last point
    if (off < 0) off = 0;
    index[(size_t)k] = c->begin + c->lb[(size_t)d] + off; ds[(size_t)k] = d; ng[(size_t)k] = e[k].n_guards; path[(size_t)k] = e[k].path;
    HIPCHK(c, hipMemcpy(&xs[(size_t)k], c->x.as<double>() + slot, sizeof(double), hipMemcpyDeviceToHost));
  }
  char where[160];
  snprintf(where, sizeof where, " (first such point: x = %.17g, dataset %d, %u point(s) in this pass)", xs[0], ds[0] + 1, cnt);
  if (!c->unseen_fn)
    return fail(c, std::string("eval() takes a branch at a data point that none of the recorded variants covers, and no handler is "
                               "registered to record it (gfh_set_unseen_handler)") + where);
  const long ms = c->model_serial, as = c->aux_serial;
  int rc;
  { std::lock_guard<std::recursive_mutex> lk(g_handler_mutex);
    c->in_recovery = true;
    rc = c->unseen_fn(c->unseen_user, c, n, index.data(), ds.data(), xs.data(), path.data(), ng.data(), pars);
    c->in_recovery = false; }
  if (rc) return fail(c, std::string("the handler for unrecorded branches of eval() failed") + where + (c->err.empty() ? "" : ": " + c->err));
  if (ms == c->model_serial && as == c->aux_serial)
    return fail(c, std::string("eval() takes a branch that the recorder cannot reproduce on the host") + where);
  return 0;
}

// An adaptive integral ran out of the compiled-in workspace (status 1) while the user's workspace (the reference's default:
// 1000 intervals, NI:40) is larger: from now on this context's kernels carry the user's sizes; the caller repeats the pass.
// Only a pass that exhausts THOSE raises "Number of iterations was insufficient" (NI:282-283).
static int grow_workspace(gfh_ctx* c) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemset(c->status.p, 0, sizeof(int)));
  c->ws.grown = true;
  apply_ws_plan(c);
  c->cur = nullptr; c->prepared = false; c->disp.mesh_valid = false;
  return 0;
}
// An integrand met a path through its comparisons of AD variables that no recording of it has (status 2): the parameters have
// moved since the integrands were recorded (a kink has entered or left some point's range of integration).  The handler is
// called with NO points (n = 0): it records eval() over its sample of the data again, at the parameters of this pass, with the
// integration variable at its several places, and hands the extended model over; the pass is repeated.  Three such rounds in a
// row without a clean pass in between, or a handler that adds nothing, end in the error.
static int recover_integrand_path(gfh_ctx* c, const double* pars) {
  gfh::Range range("gadfit integrand path: record again and extend the model");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemset(c->status.p, 0, sizeof(int)));
  c->n_integrand_rounds++;
  const long ms = c->model_serial;
  int rc;
  { std::lock_guard<std::recursive_mutex> lk(g_handler_mutex);
    c->in_recovery = true;
    rc = c->unseen_fn(c->unseen_user, c, 0, nullptr, nullptr, nullptr, nullptr, nullptr, pars);
    c->in_recovery = false; }
  if (rc || ms == c->model_serial) { c->n_integrand_rounds = 3; return status_check(c, 2); }
  return 0;
}

int gfh::repeat_pass(gfh_ctx* c, int rc, const double* pars) {      // 0: repeat the pass; 1: failed
  if (rc == kUnseen) return recover_unseen(c, pars);
  if (rc == kGrowWs) return grow_workspace(c);
  if (rc == kIntegrandPath) return recover_integrand_path(c, pars);
  return 1;
}

static int sweep_pass(gfh_ctx* c, const double* pars, const int32_t* active, int na, const int32_t* jac, int dim,
                      double* JTJ, double* JTres, double* chi2) {
  gfh::Range range("gadfit sweep (STEP 1 + STEP 2)");
  harvest_events(c);
  if (!c->nd) return fail(c, "no data set (gfh_set_data)");
  if (prepare_active(c, active, na, jac, dim)) return 1;
  if (c->gen.finite_diff && c->gen.fd_col_sets && c->has_model && c->n_aux < c->model.n_aux * (1 + na))
    return fail(c, "use_ad = 0 with column sets (gfh_set_fd_column_sets): the model reads " + std::to_string(c->model.n_aux) + " column(s), " +
                std::to_string(na) + " parameter(s) are active, so gfh_set_aux must hold " + std::to_string(c->model.n_aux * (1 + na)) +
                " columns; it holds " + std::to_string(c->n_aux));
  if (c->gen.finite_diff)                              // grad_finite's own check (fitfunction.F90:164-167)
    for (int d = 0; d < c->nd; d++)
      for (int j = 0; j < na; j++) {
        const double step = 0x1p-26 * pars[(size_t)d * c->model.n_pars + active[j]];
        if (!(std::fabs(step) > 2.2250738585072014e-308))
          return fail(c, "Absolute value of parameter " + std::to_string(active[j] + 1) + " is too small.");
      }
  if (upload_pars(c, pars)) return 1;
  // an event record costs ~5 us of stream time: only the model kernel is bracketed by default
  const bool fused = use_fused(c);
  // a fit that defers the Jacobian store (context.h, Deferred): this sweep runs the kernels without it -- the same sums, bit for bit --
  // unless the fit has said that no later sweep of it can follow
  const ModelKernels* nostore = nullptr;
  if (c->defer.fit == 2 && !c->defer.store_next && fused && c->gen.store_j) {
    nostore = nostore_kernels(c);
    if (!nostore) return 1;
    if (!nostore->sweep_gram) nostore = nullptr;
  }
  const bool stores = c->gen.store_j && !nostore;
  // Small assemblies: the fused kernel's own tail reduces the workgroup partials, assembles the packed
  // normal equations and (single rank) writes the host mailbox -- no reduce/assemble/publish launches.
  const bool small = (int64_t)dim * dim * c->nd <= 65536;
  // (a single workgroup hands nothing over to anybody: the tail is always safe then -- the tiny fits)
  const bool tail = c->tail && fused && c->n_gb > 0 && small && (tail_one_workgroup_per_cu(c) || c->n_gb <= 256);
  // global fits beyond the tail's reach travel pattern-only: [nnz | JTres | chi2].  The layout of `packed` is what the
  // ranks all-reduce, so it may only depend on quantities every rank shares (not on whether THIS rank has points).
  const bool sparse = c->sparse && !small;
  const size_t packed_n = sparse ? (size_t)c->nnz + dim + 1 : (size_t)dim * dim + dim + 1;
  c->last_sweep = {fused ? 1 : 0, fused ? fused_waves_for(na) : 0, tail ? (c->comm ? 1 : 2) : 0, sparse ? 1 : 0};
  // (level 1 samples: every 8th launch since gfh_reset_timers is bracketed)
  const int tl_ = timed_launch(c, c->timers.n_sweep) ? c->timers.detail : 0;
  const int td = fused ? tl_ : (tl_ ? 2 : 0);
  unsigned long long seq = 0;
  if (tail) {
    if (pinned_reserve(c, sizeof(double) * std::max<size_t>(packed_n + 1, 4096)) || update_tail(c)) return 1;
    if (!c->comm) seq = ++c->mail_seq;
  }
  // (a sweep writes every column of J anew: moving the buffer between two sweeps loses nothing)
  if (c->place.pending && stores && c->J.p && c->place.sweeps_on_J >= c->place.after && place_jacobian_now(c, fused)) return 1;
  if (stores && c->J.p) c->place.sweeps_on_J++;
  if (td >= 1) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (fused ? launch_model_sweep_gram(c, tail ? (c->comm ? 1 : 2) : 0, seq, tail ? tail_lds_pad(c) : 0u, nostore) : launch_model_sweep(c, mesh_mode_for(c, pars, true))) return 1;
  if (td >= 1) HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  if (tail) {
    // reduction, assembly and (single rank) the mailbox write happened in the fused kernel's tail
    c->chain.gram.clear(); c->chain.assemble = 1;
    if (td >= 2) { HIPCHK(c, hipEventRecord(c->ev[2], c->stream)); HIPCHK(c, hipEventRecord(c->ev[3], c->stream)); }
    if (c->comm) {
      if (allreduce_sum(c, c->packed.as<double>(), packed_n, true)) return 1;
      if (td >= 2) HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
      PASS(fetch_result(c, c->packed.as<double>(), packed_n, true));
    } else {
      if (td >= 2) HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
      PASS(await_result(c, seq, packed_n));
    }
  } else {
    // single rank + pattern-only image: k_gather_sum posts the mailbox itself (no k_publish launch)
    const bool self_publish = c->gs_meta.p && c->gs_n && c->gs_sparse == sparse && !c->comm;
    unsigned long long pseq = 0;
    if (self_publish) {
      if (pinned_reserve(c, sizeof(double) * std::max<size_t>(packed_n + 1, 4096))) return 1;
      pseq = ++c->mail_seq;
    }
    if (launch_gram_chain(c, td >= 2, !fused, sparse, pseq)) return 1;
    if (td >= 2) HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    if (c->comm && allreduce_sum(c, c->packed.as<double>(), packed_n)) return 1;
    if (td >= 2) HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
    PASS(self_publish ? await_result(c, pseq, packed_n) : fetch_result(c, c->packed.as<double>(), packed_n, c->comm != nullptr));
  }
  // with the in-kernel tail the host holds the result before the kernel has formally completed:
  // the events are read when the next call (or gfh_get_timers) needs them
  c->timers.ev_pending = td;
  if (!(tail && !c->comm)) harvest_events(c);
  c->timers.n_sweep++;
  if (sparse) {
    if (JTJ) {
      if (!c->jtj_prezeroed) memset(JTJ, 0, sizeof(double) * (size_t)dim * dim);
      const int* nr = c->h_nz_row.data(); const int* nc = c->h_nz_col.data();
      for (int k = 0; k < c->nnz; k++) {
        const double v = c->h_pinned[k];
        JTJ[(size_t)nc[k] * dim + nr[k]] = v; JTJ[(size_t)nr[k] * dim + nc[k]] = v;      // both triangles, as the dense path
      }
    }
    if (JTres) memcpy(JTres, c->h_pinned + c->nnz, sizeof(double) * dim);
    if (chi2) *chi2 = c->h_pinned[(size_t)c->nnz + dim];
  } else {
    if (JTJ) memcpy(JTJ, c->h_pinned, sizeof(double) * (size_t)dim * dim);
    if (JTres) memcpy(JTres, c->h_pinned + (size_t)dim * dim, sizeof(double) * dim);
    if (chi2) *chi2 = c->h_pinned[(size_t)dim * dim + dim];
  }
  c->have_sweep = true; c->j_valid = stores; c->res_valid = true;
  // (J of THIS sweep is what a reader is owed from now on, or nothing is)
  c->defer.owed = nostore != nullptr; c->defer.chi2_after = false;
  if (nostore) { c->defer.pars.assign(pars, pars + (size_t)c->nd * c->model.n_pars); c->defer.n_deferred++; }
  else if (c->defer.fit && stores) c->defer.n_stored++;
  if (c->disp.order_measured && build_orders(c)) return 1;
  return 0;
}

static int chi2_pass(gfh_ctx* c, const double* pars, double* chi2) {
  gfh::Range range("gadfit chi2");
  harvest_events(c);
  if (!c->nd) return fail(c, "no data set (gfh_set_data)");
  if (check_aux(c) || ensure_gb_partition(c)) return 1;
  if (!c->cur) {   // chi2 before any sweep: kernels for "no active parameter" are the same TU
    std::vector<int32_t> none;
    if (get_kernels(c, none, true)) return 1;
  }
  // the partial buffer follows the data set (gfh_set_data may have changed it)
  if (dev_alloc(c, c->chi2_partial, sizeof(double) * (size_t)std::max(1, c->n_gb)) || dev_alloc(c, c->vec, sizeof(double) * 64) ||
      pinned_reserve(c, 4096) || ensure_mesh(c)) return 1;
  if (upload_pars(c, pars)) return 1;
  const bool timed = c->n_gb && timed_launch(c, c->timers.n_chi2);
  if (timed) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (!c->n_gb) {                                       // a rank without points contributes an exact zero
    HIPCHK(c, hipMemsetAsync(c->vec.p, 0, sizeof(double), c->stream));
    if (c->comm && allreduce_sum(c, c->vec.as<double>(), 1)) return 1;
    PASS(fetch_result(c, c->vec.as<double>(), 1, c->comm != nullptr));
  } else if (!c->comm) {                                // single rank (or member of a host-summed group): the kernel's last workgroup posts the mailbox
    const unsigned long long seq = ++c->mail_seq;
    if (launch_model_chi2(c, 2, seq, mesh_mode_for(c, pars, true))) return 1;
    if (timed) HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    PASS(await_result(c, seq, 1));
  } else {
    if (launch_model_chi2(c, 1, 0, mesh_mode_for(c, pars, true))) return 1;
    if (timed) HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    if (allreduce_sum(c, c->vec.as<double>(), 1, true)) return 1;
    PASS(fetch_result(c, c->vec.as<double>(), 1, true));
  }
  if (timed) { c->timers.t_chi2 += 1e-3 * ev_ms(c->ev[0], c->ev[1]); c->timers.n_chi2_timed++; }
  c->timers.n_chi2++;
  c->res_valid = c->gen.store_res;
  // (an owed Jacobian: materialising it rewrites res, so the pass that wrote res last is repeated behind it)
  if (c->defer.owed && c->gen.store_res) { c->defer.chi2_after = true; c->defer.chi2_pars.assign(pars, pars + (size_t)c->nd * c->model.n_pars); }
  *chi2 = c->h_pinned[0];
  return 0;
}

// scatter a dim-vector into per-dataset blocks through Jacobian_indices (gadfit.F90:719)
static void scatter_delta(gfh_ctx* c, const double* delta, std::vector<double>& by_par, std::vector<double>& by_act) {
  const int na = (int)c->cur_active.size(), np = c->model.n_pars;
  by_par.assign((size_t)c->nd * np, 0.0); by_act.assign((size_t)c->nd * na, 0.0);
  for (int d = 0; d < c->nd; d++)
    for (int k = 0; k < na; k++) {
      const double v = delta[c->cur_jac[(size_t)d * na + k]];
      by_par[(size_t)d * np + c->cur_active[k]] = v; by_act[(size_t)d * na + k] = v;
    }
}

// per-gram-block partials [b][a] of a J^T v product -> out[dim], summed over ranks
static int jtv_finish(gfh_ctx* c, double* out) {
  const int na = (int)c->cur_active.size(), dim = c->cur_dim;
  const int ps = gram_partial_stride(c->cur_T);
  if ((int64_t)c->nd * na <= 4096 && c->merge_small) {          // one single-workgroup launch instead of three
    if (pinned_reserve(c, sizeof(double) * std::max<size_t>((size_t)dim + 1, 4096))) return 1;
    if (c->comm) {
      HIPCHK(c, launch_jtv_finish(c->stream, c->partial.as<double>(), ps, na, c->ds_first_gb.as<int>(), c->nd, dim, c->inv.as<int>(),
                                  c->vec.as<double>(), c->status.as<int>(), nullptr, nullptr, 0));
      if (allreduce_sum(c, c->vec.as<double>(), (size_t)dim)) return 1;
      PASS(fetch_result(c, c->vec.as<double>(), dim, true));
    } else {
      const unsigned long long seq = ++c->mail_seq;
      HIPCHK(c, launch_jtv_finish(c->stream, c->partial.as<double>(), ps, na, c->ds_first_gb.as<int>(), c->nd, dim, c->inv.as<int>(),
                                  c->vec.as<double>(), c->status.as<int>(), c->h_pinned, c->h_flag, seq));
      PASS(await_result(c, seq, dim));
    }
    c->chain.jtv_finish = 1;
    memcpy(out, c->h_pinned, sizeof(double) * dim);
    return 0;
  }
  HIPCHK(c, launch_reduce_partials(c->stream, c->partial.as<double>(), ps, na, c->ds_first_gb.as<int>(), c->nd, c->G.as<double>()));
  HIPCHK(c, launch_assemble_vec(c->stream, c->G.as<double>(), na, c->nd, dim, c->inv.as<int>(), c->vec.as<double>()));
  c->chain.jtv_finish = 2;
  if (c->comm && allreduce_sum(c, c->vec.as<double>(), (size_t)dim)) return 1;
  PASS(fetch_result(c, c->vec.as<double>(), dim, c->comm != nullptr));
  memcpy(out, c->h_pinned, sizeof(double) * dim);
  return 0;
}

static int jtv_to_host(gfh_ctx* c, const double* v_dev, double* out) {
  const int na = (int)c->cur_active.size();
  const int ps = gram_partial_stride(c->cur_T);
  if (c->n_gb) HIPCHK(c, launch_jtv(c->stream, c->J.as<double>(), c->ldj, na, v_dev, c->gb_start.as<i64>(), c->gb_slots.as<int>(),
                                     c->n_gb, c->partial.as<double>(), ps));
  return jtv_finish(c, out);
}

// The Jacobian a fit owes (context.h, Deferred), written now: the storing kernel at the parameters of the fit's most recent sweep --
// workgroup partials only, no cross-rank sum, no mailbox, nothing of the host's sums changes: a read-back is not a collective --
// and, where a chi2 pass wrote the residual vector after that sweep, the chi2 kernel again at that pass's parameters, so that res
// holds the bits it held.  Called by every reader of the stored Jacobian before it looks at j_valid; a no-op when nothing is owed.
int gfh::materialise_jacobian(gfh_ctx* c) {
  if (!c->defer.owed || !c->have_sweep) return 0;
  if (!c->cur || !use_fused(c) || !c->gen.store_j || !c->J.p || c->defer.pars.size() != (size_t)c->nd * c->model.n_pars) {
    c->defer.owed = c->defer.chi2_after = false;          // (no state this can be true in: the reader then fails with its usual message)
    return 0;
  }
  gfh::Range range("gadfit materialise the deferred Jacobian");
  harvest_events(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (upload_pars(c, c->defer.pars.data()) || launch_model_sweep_gram(c, 0, 0, 0)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));              // (the staging block of the parameters is free again)
  if (c->defer.chi2_after) {
    if (dev_alloc(c, c->chi2_partial, sizeof(double) * (size_t)std::max(1, c->n_gb)) || upload_pars(c, c->defer.chi2_pars.data()) ||
        launch_model_chi2(c, 0, 0, 0)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  int st = 0;
  HIPCHK(c, hipMemcpy(&st, c->status.p, sizeof(int), hipMemcpyDeviceToHost));
  if (st) {
    HIPCHK(c, hipMemset(c->status.p, 0, sizeof(int)));
    return fail(c, "materialising the deferred Jacobian: device kernel reported status " + std::to_string(st));
  }
  c->defer.owed = c->defer.chi2_after = false;
  c->j_valid = true; c->defer.n_materialised++;
  return 0;
}

static int omega_pass(gfh_ctx* c, const double* pars, const double* delta1, double* JTomega) {
  gfh::Range range("gadfit omega (STEP 3)");
  harvest_events(c);
  if (!c->have_sweep) return fail(c, "gfh_omega needs a preceding gfh_sweep (active set, column map)");
  if (c->gen.finite_diff && c->gen.fd_col_sets)
    return fail(c, "gfh_omega: the central difference of use_ad = 0 (fitfunction.F90:188-203) has no column sets at p +- h*delta (gfh_set_fd_column_sets)");
  const bool recompute = c->cur && c->cur->omega_jt && !omega_needs_jacobian(c, (int)c->cur_active.size());
  if (!recompute && materialise_jacobian(c)) return 1;
  if (!recompute && !c->j_valid) return fail(c, "gfh_omega: the Jacobian was not kept (gfh_set_keep_jacobian)");
  if (ensure_tile_table(c)) return 1;
  std::vector<double> by_par, by_act;
  scatter_delta(c, delta1, by_par, by_act);
  if (upload_pars(c, pars)) return 1;
  // delta1 scattered per dataset: pinned staging; by value with the kernel arguments for single-dataset
  // fits (as the parameter block), else an asynchronous copy in front of the kernel
  if (pinned_stage(c, c->h_dpars, c->h_dpars_bytes, sizeof(double) * by_par.size())) return 1;
  memcpy(c->h_dpars, by_par.data(), sizeof(double) * by_par.size());
  if (dev_alloc(c, c->dpars, sizeof(double) * by_par.size())) return 1;
  if (!(c->cur && c->cur->kernarg_pars))
    HIPCHK(c, hipMemcpyAsync(c->dpars.p, c->h_dpars, sizeof(double) * by_par.size(), hipMemcpyHostToDevice, c->stream));
  const bool timed = timed_launch(c, c->timers.n_omega);
  if (timed) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (recompute ? launch_model_omega_jt(c) : launch_model_omega(c, mesh_mode_for(c, pars, false))) return 1;
  if (timed) HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  PASS(recompute ? jtv_finish(c, JTomega) : jtv_to_host(c, c->omega.as<double>(), JTomega));
  if (timed) { c->timers.t_omega += 1e-3 * ev_ms(c->ev[0], c->ev[1]); c->timers.n_omega_timed++; }
  c->timers.n_omega++;
  return 0;
}

extern "C" {

int gfh_sweep(gfh_ctx* c, const double* pars, const int32_t* active, int na, const int32_t* jac, int dim,
              double* JTJ, double* JTres, double* chi2) {
  // device group: every member holds the same sums afterwards; member 0 writes the caller's arrays
  GROUP(c, gfh_sweep(k, pars, active, na, jac, dim, r ? nullptr : JTJ, r ? nullptr : JTres, r ? nullptr : chi2));
  NEED_GPU(c);
  for (;;) {
    const int rc = sweep_pass(c, pars, active, na, jac, dim, JTJ, JTres, chi2);
    if (rc != kUnseen && rc != kGrowWs && rc != kIntegrandPath) return rc;
    if (repeat_pass(c, rc, pars)) return 1;
  }
}

int gfh_chi2(gfh_ctx* c, const double* pars, double* chi2) {
  if (c && c->grp) return gfh::group_run(c, [&](gfh_ctx* k, int r) -> int { double mine = 0.0; return gfh_chi2(k, pars, r ? &mine : chi2); });
  NEED_GPU(c);
  for (;;) {
    // (a recovery replaces the model: the pass then reloads the kernels of the active set the fit is using)
    const std::vector<int32_t> act = c->cur_active, jac = c->cur_jac; const int dim = c->cur_dim;
    const bool had = c->have_sweep, jv = c->j_valid;
    const int rc = chi2_pass(c, pars, chi2);
    if (rc != kUnseen && rc != kGrowWs && rc != kIntegrandPath) return rc;
    if (repeat_pass(c, rc, pars)) return 1;
    if (!act.empty() && prepare_active(c, act.data(), (int)act.size(), jac.data(), dim)) return 1;
    // the new model keeps what the sweep before this chi2() left: its active set, column map and Jacobian in HBM (gfh_omega,
    // gfh_get_points and gfh_time_kernel after a recovery inside chi2() build on them, as gfh_omega's own loop does)
    if (!act.empty()) { c->have_sweep = had; c->j_valid = jv; }
  }
}

int gfh_omega(gfh_ctx* c, const double* pars, const double* delta1, double* JTomega) {
  if (c && c->grp) return gfh::group_run(c, [&](gfh_ctx* k, int r) -> int {
    std::vector<double> mine(r ? (size_t)std::max(1, k->cur_dim) : 0);
    return gfh_omega(k, pars, delta1, r ? mine.data() : JTomega); });
  NEED_GPU(c);
  for (;;) {
    const std::vector<int32_t> act = c->cur_active, jac = c->cur_jac; const int dim = c->cur_dim;
    const bool jv = c->j_valid;
    const int rc = omega_pass(c, pars, delta1, JTomega);
    if (rc != kUnseen && rc != kGrowWs && rc != kIntegrandPath) return rc;
    if (repeat_pass(c, rc, pars)) return 1;
    // the new model keeps the state STEP 3 builds on: the active set and column map of the sweep before it (and its Jacobian in HBM)
    if (act.empty() || prepare_active(c, act.data(), (int)act.size(), jac.data(), dim)) return act.empty() ? fail(c, "gfh_omega needs a preceding gfh_sweep") : 1;
    c->have_sweep = true; c->j_valid = jv;
  }
}

int gfh_aux(gfh_ctx* c, int what, const double* delta1, double* out) {
  if (c && c->grp) return gfh::group_run(c, [&](gfh_ctx* k, int r) -> int {
    std::vector<double> mine(r ? (size_t)std::max(3, k->cur_dim) : 0);
    return gfh_aux(k, what, delta1, r ? mine.data() : out); });
  NEED_GPU(c);
  if (!c->have_sweep) return fail(c, "gfh_aux needs the Jacobian of a preceding gfh_sweep");
  if (materialise_jacobian(c)) return 1;
  if (!c->j_valid) return fail(c, "gfh_aux: the Jacobian was not kept (gfh_set_keep_jacobian)");
  if (!c->res_valid) return fail(c, "gfh_aux: the residual vector was not kept (gfh_set_keep_jacobian)");
  if (what == 0) return jtv_to_host(c, c->res.as<double>(), out);
  if (what != 1) return fail(c, "gfh_aux: unknown request");
  std::vector<double> by_par, by_act;
  scatter_delta(c, delta1, by_par, by_act);
  const int na = (int)c->cur_active.size(), ps = gram_partial_stride(c->cur_T);
  if (dev_alloc(c, c->dl, sizeof(double) * by_act.size())) return 1;
  HIPCHK(c, hipMemcpy(c->dl.p, by_act.data(), sizeof(double) * by_act.size(), hipMemcpyHostToDevice));
  if (c->n_gb) HIPCHK(c, launch_cosphi(c->stream, c->J.as<double>(), c->ldj, na, c->res.as<double>(), c->dl.as<double>(),
                                        c->gb_start.as<i64>(), c->gb_slots.as<int>(), c->gb_ds.as<int>(), c->n_gb, c->partial.as<double>(), ps));
  // sum over all workgroups regardless of dataset: reuse reduce with a 2-entry "dataset" table
  std::vector<int> all = {0, c->n_gb};
  DevBuf tmp; if (dev_alloc(c, tmp, sizeof(int) * 2)) return 1;
  HIPCHK(c, hipMemcpy(tmp.p, all.data(), sizeof(int) * 2, hipMemcpyHostToDevice));
  HIPCHK(c, launch_reduce_partials(c->stream, c->partial.as<double>(), ps, 3, tmp.as<int>(), 1, c->vec.as<double>()));
  if (c->comm && allreduce_sum(c, c->vec.as<double>(), 3)) { dev_free(tmp); return 1; }
  if (fetch_result(c, c->vec.as<double>(), 3, c->comm != nullptr)) { dev_free(tmp); return 1; }
  dev_free(tmp);
  memcpy(out, c->h_pinned, sizeof(double) * 3);
  return 0;
}

}  // extern "C"
