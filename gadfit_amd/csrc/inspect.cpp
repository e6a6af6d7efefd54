// inspect.cpp -- timers and read-backs: which launches are bracketed by events and how their times are scaled and reported, the
// bare launches and gfh_time_kernel of the benchmarks, and the debug read-backs of what lies on the device.  It changes no state
// a pass depends on.
#include "context_internal.h"
#include "group.h"
#include <algorithm>
#include <cstring>

using namespace gfh;

// (a result can reach the host mailbox a moment before its kernel has formally retired: wait for the closing event)
double gfh::ev_ms(hipEvent_t a, hipEvent_t b) { float ms = 0; hipEventSynchronize(b); hipEventElapsedTime(&ms, a, b); return ms; }

// timer level 1 brackets every 8th launch (every launch under adaptive load balancing, whose shares follow these times): the
// sum over the timed launches, scaled to all launches since gfh_reset_timers
bool gfh::timed_launch(const gfh_ctx* c, long n_so_far) {
  return c->timers.detail >= 2 || (c->timers.detail == 1 && (!(n_so_far & 7) || (c->bal.on && c->nranks > 1)));
}
double gfh::scaled_time(double t_timed, long n_all, long n_timed) { return n_timed > 0 ? t_timed * (double)n_all / (double)n_timed : 0.0; }

// sweep timers from the events of the last gfh_sweep (deferred while the kernel may still be finishing)
void gfh::harvest_events(gfh_ctx* c) {
  const int td = c->timers.ev_pending;
  c->timers.ev_pending = 0;
  if (td < 1) return;
  hipEventSynchronize(c->ev[td >= 2 ? 4 : 1]);
  const double ts = 1e-3 * ev_ms(c->ev[0], c->ev[1]);
  c->timers.t_sweep += ts; c->timers.t_sweep_last = ts;
  if (!c->timers.n_sweep_timed || ts < c->timers.t_sweep_min) c->timers.t_sweep_min = ts;
  if (!c->timers.n_sweep_timed || ts > c->timers.t_sweep_max) c->timers.t_sweep_max = ts;
  c->timers.n_sweep_timed++;
  if (td >= 2) {
    c->timers.t_gram += 1e-3 * ev_ms(c->ev[1], c->ev[2]);
    c->timers.t_reduce += 1e-3 * ev_ms(c->ev[2], c->ev[3]); c->timers.t_allreduce += 1e-3 * ev_ms(c->ev[3], c->ev[4]);
    c->timers.n_chain_timed++;
  }
}

// ------------------------------------------------------------------------- debug read-back
int gfh::unpad(gfh_ctx* c, const double* dev, double* out) {
  std::vector<double> h((size_t)c->n_slots);
  if (c->n_slots) HIPCHK(c, hipMemcpy(h.data(), dev, sizeof(double) * (size_t)c->n_slots, hipMemcpyDeviceToHost));
  for (int d = 0; d < c->nd; d++) {
    const int64_t len = c->lb[d + 1] - c->lb[d];
    if (len) memcpy(out + c->lb[d], &h[(size_t)c->ds_slot[d]], sizeof(double) * (size_t)len);
  }
  return 0;
}
extern "C" {

// ------------------------------------------------------------------------- timers / bench hooks
int gfh_get_timers(gfh_ctx* c, double* o) {
  if (!c) return 1;
  if (c->grp) {      // the slowest member of a device group (the counts are the same on all)
    for (int i = 0; i < 8; i++) o[i] = 0.0;
    for (int r = 0; r < gfh::group_size(c); r++) {
      double t[8];
      if (gfh_get_timers(gfh::group_member(c, r), t)) return 1;
      for (int i = 0; i < 8; i++) o[i] = std::max(o[i], t[i]);
    }
    return 0;
  }
  if (c->device >= 0) harvest_events(c);
  // (level 1 brackets every 8th sweep; the Gram / reduce / all-reduce stages are bracketed on those of the sampled sweeps that run
  // at level 2 -- every sampled one on the two-kernel path -- and scaled to all sweeps like the model kernels)
  o[0] = scaled_time(c->timers.t_sweep, c->timers.n_sweep, c->timers.n_sweep_timed); o[1] = scaled_time(c->timers.t_gram, c->timers.n_sweep, c->timers.n_chain_timed);
  o[2] = scaled_time(c->timers.t_reduce, c->timers.n_sweep, c->timers.n_chain_timed); o[3] = scaled_time(c->timers.t_allreduce, c->timers.n_sweep, c->timers.n_chain_timed);
  o[4] = scaled_time(c->timers.t_chi2, c->timers.n_chi2, c->timers.n_chi2_timed); o[5] = scaled_time(c->timers.t_omega, c->timers.n_omega, c->timers.n_omega_timed);
  o[6] = (double)c->timers.n_sweep; o[7] = (double)c->timers.n_chi2;
  return 0;
}
void gfh_reset_timers(gfh_ctx* c) {
  if (!c) return;
  if (c->grp) { for (int r = 0; r < gfh::group_size(c); r++) gfh_reset_timers(gfh::group_member(c, r)); return; }
  if (c->device >= 0) harvest_events(c);
  const int detail = c->timers.detail;        // (the level is an option, not a reading; no events are pending after the harvest)
  c->timers = {};
  c->timers.detail = detail;
}
int gfh_get_timer_spread(gfh_ctx* c, double* o) {
  if (!c) return 1;
  if (c->grp) return gfh_get_timer_spread(gfh::group_member(c, 0), o);
  if (c->device >= 0) harvest_events(c);
  o[0] = c->timers.t_sweep_min; o[1] = c->timers.t_sweep_max; o[2] = c->timers.t_sweep_last; o[3] = (double)c->timers.n_sweep_timed;
  return 0;
}

int gfh_launch_sweep(gfh_ctx* c) { GROUP(c, gfh_launch_sweep(k)); NEED_GPU(c); if (!c->have_sweep) return fail(c, "call gfh_sweep once first"); return launch_model_sweep(c); }
int gfh_launch_gram(gfh_ctx* c) { GROUP(c, gfh_launch_gram(k)); NEED_GPU(c); if (!c->have_sweep) return fail(c, "call gfh_sweep once first"); return launch_gram_chain(c, false); }
int gfh_launch_chi2(gfh_ctx* c) {
  GROUP(c, gfh_launch_chi2(k));
  NEED_GPU(c); if (!c->have_sweep) return fail(c, "call gfh_sweep once first");
  return launch_model_chi2(c, 1, 0);
}
int gfh_sync(gfh_ctx* c) { GROUP(c, gfh_sync(k)); NEED_GPU(c); HIPCHK(c, hipStreamSynchronize(c->stream)); return 0; }
void* gfh_stream(gfh_ctx* c) { if (c && c->grp) c = gfh::group_member(c, 0); return c ? (void*)c->stream : nullptr; }

int gfh_time_kernel(gfh_ctx* c, int which, int reps, double* avg_ms) {
  if (c && c->grp) {      // all members launch together; the slowest member's average
    std::vector<double> ms((size_t)gfh::group_size(c), 0.0);
    if (gfh::group_run(c, [&](gfh_ctx* k, int r) -> int { return gfh_time_kernel(k, which, reps, &ms[(size_t)r]); })) return 1;
    *avg_ms = *std::max_element(ms.begin(), ms.end());
    return 0;
  }
  NEED_GPU(c);
  harvest_events(c);
  if (!c->have_sweep) return fail(c, "call gfh_sweep once first");
  if (reps < 1) reps = 1;
  if ((which == 3 || which == 6 || which == 9) && !c->dpars.p) return fail(c, "call gfh_omega once first");
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  for (int r = 0; r < reps; r++) {
    int rc = 0;
    switch (which) {
      case 0: rc = use_fused(c) ? launch_model_sweep_gram(c) : launch_model_sweep(c); break;
      case 4: rc = launch_model_sweep(c); break;
      case 5: if (!use_fused(c)) return fail(c, "no fused kernel for this active set"); rc = launch_model_sweep_gram(c); break;
      case 1: if (c->n_gb) { hipError_t e = launch_gram(c->stream, c->cur_T, c->J.as<double>(), c->ldj, (int)c->cur_active.size(),
                                 c->res.as<double>(), c->gb_start.as<i64>(), c->gb_slots.as<int>(), c->n_gb, c->partial.as<double>());
                             if (e != hipSuccess) return fail(c, hipGetErrorString(e)); } break;
      case 2: rc = launch_model_chi2(c, 1, 0); break;
      case 3: rc = launch_model_omega(c); break;
      // (8, 9: STEP 1 / STEP 3 replaying the recorded quadrature meshes -- valid after a pass at the parameters still in the staging block)
      case 8: if (!c->disp.mesh_valid) return fail(c, "no recorded quadrature mesh to replay"); rc = launch_model_sweep(c, 2); break;
      case 9: if (!c->disp.mesh_valid) return fail(c, "no recorded quadrature mesh to replay"); rc = launch_model_omega(c, 2); break;
      case 6: if (!c->cur->omega_jt) return fail(c, "gfh_k_omega_jt is not available for this model"); rc = launch_model_omega_jt(c); break;
      case 7: if (materialise_jacobian(c)) return 1;
              if (!c->j_valid) return fail(c, "the Jacobian was not kept (gfh_set_keep_jacobian)");
              if (c->n_gb) { hipError_t e = launch_jtv(c->stream, c->J.as<double>(), c->ldj, (int)c->cur_active.size(), c->res.as<double>(),
                                 c->gb_start.as<i64>(), c->gb_slots.as<int>(), c->n_gb, c->partial.as<double>(), gram_partial_stride(c->cur_T));
                             if (e != hipSuccess) return fail(c, hipGetErrorString(e)); } break;
      default: return fail(c, "unknown kernel id");
    }
    if (rc) return rc;
  }
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *avg_ms = ev_ms(c->ev[0], c->ev[1]) / reps;
  return 0;
}

int gfh_get_residuals(gfh_ctx* c, double* out) {
  GROUP(c, gfh_get_residuals(k, out + k->begin));
  NEED_GPU(c);
  if (!c->res_valid) return fail(c, "the residual vector of the last chi2 pass was not kept (gfh_set_keep_jacobian mode 2)");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return unpad(c, c->res.as<double>(), out);
}
int gfh_get_weights(gfh_ctx* c, double* out) { GROUP(c, gfh_get_weights(k, out + k->begin)); NEED_GPU(c); HIPCHK(c, hipStreamSynchronize(c->stream)); return unpad(c, c->w.as<double>(), out); }
int gfh_get_omega(gfh_ctx* c, double* out) { GROUP(c, gfh_get_omega(k, out + k->begin)); NEED_GPU(c); HIPCHK(c, hipStreamSynchronize(c->stream)); return unpad(c, c->omega.as<double>(), out); }
int gfh_get_jacobian(gfh_ctx* c, double* out) {
  GROUP(c, gfh_get_jacobian(k, out + (size_t)k->begin * k->cur_active.size()));
  NEED_GPU(c);
  if (!c->have_sweep) return fail(c, "no Jacobian on the device yet");
  if (materialise_jacobian(c)) return 1;
  if (!c->j_valid) return fail(c, "the Jacobian was not kept (gfh_set_keep_jacobian)");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int na = (int)c->cur_active.size();
  std::vector<double> col((size_t)c->count);
  for (int a = 0; a < na; a++) {
    if (unpad(c, c->J.as<double>() + (size_t)a * c->ldj, col.data())) return 1;
    for (int64_t i = 0; i < c->count; i++) out[(size_t)i * na + a] = col[(size_t)i];
  }
  return 0;
}

// Read-back of single points (local indices into this rank's range): the residual and the Jacobian row [n][n_act] of each -- for
// checks at sizes where the whole Jacobian (28.8 GB at 1e8 points x 32 parameters) does not belong on the host.
int gfh_get_points(gfh_ctx* c, int n, const int64_t* index, double* res_out, double* jac_out) {
  NOT_FOR_GROUP(c, "gfh_get_points");
  NEED_GPU(c);
  if (!c->have_sweep) return fail(c, "no sweep on the device yet");
  if (jac_out && materialise_jacobian(c)) return 1;
  if (jac_out && !c->j_valid) return fail(c, "the Jacobian was not kept (gfh_set_keep_jacobian)");
  if (res_out && !c->res_valid) return fail(c, "the residual vector of the last pass was not kept");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int na = (int)c->cur_active.size();
  for (int k = 0; k < n; k++) {
    const int64_t i = index[k];
    if (i < 0 || i >= c->count) return fail(c, "gfh_get_points: index outside this rank's range");
    int d = 0;
    while (d + 1 < c->nd && i >= c->lb[(size_t)d + 1]) d++;
    const int64_t slot = c->ds_slot[(size_t)d] + (i - c->lb[(size_t)d]);
    if (res_out) HIPCHK(c, hipMemcpy(res_out + k, c->res.as<double>() + slot, sizeof(double), hipMemcpyDeviceToHost));
    if (jac_out) HIPCHK(c, hipMemcpy2D(jac_out + (size_t)k * na, sizeof(double), c->J.as<double>() + slot, sizeof(double) * (size_t)c->ldj,
                                       sizeof(double), (size_t)na, hipMemcpyDeviceToHost));
  }
  return 0;
}

// The abscissas as they lie on the device, back into the caller's concatenated array: this rank's range [begin, begin + count) of
// x_out[n_total] (a device group: every member's range, so the whole array).
int gfh_get_abscissas(gfh_ctx* c, double* x_out) {
  GROUP(c, gfh_get_abscissas(k, x_out));
  NEED_GPU(c);
  if (!x_out) return fail(c, "gfh_get_abscissas: null argument");
  if (!c->nd) return fail(c, "no data set (gfh_set_data)");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int d = 0; d < c->nd; d++) {
    const int64_t len = c->lb[(size_t)d + 1] - c->lb[(size_t)d];
    if (len > 0) HIPCHK(c, hipMemcpy(x_out + c->begin + c->lb[(size_t)d], c->x.as<double>() + c->ds_slot[(size_t)d], sizeof(double) * (size_t)len,
                                     hipMemcpyDeviceToHost));
  }
  return 0;
}

int gfh_get_counters(gfh_ctx* c, int64_t* out4) {
  if (!c || !out4) return 1;
  gfh_ctx* k = c->grp ? gfh::group_member(c, 0) : c;
  out4[0] = k->n_unseen_rounds; out4[1] = k->disp.n_mesh_replays; out4[2] = k->has_model ? k->model.n_variants() : 0;
  out4[3] = k->has_model ? ((int64_t)k->gen.ws_size << 32) + k->gen.ws_size_inner : 0;
  return 0;
}
// What the last recording pass of a quadrature model did, from the device's own mesh records (one per slot and outermost integrate()
// call site: byte 0 = bisections of that adaptive integral, 255 = none recorded): the work count behind the algorithmic roofline of
// BASELINE config 4 (numerical_integration.F90:236-284: n intervals = (2n - 1) panels of the bisection + n of the final pass).
int gfh_debug_mesh_stats(gfh_ctx* c, int64_t* out4) {
  if (!c || !out4) return 1;
  NOT_FOR_GROUP(c, "gfh_debug_mesh_stats");
  gfh_ctx* k = c;
  NEED_GPU(k);
  out4[0] = out4[1] = out4[2] = out4[3] = 0;
  if (!k->disp.mesh.p || !k->disp.mesh_stride || !k->disp.mesh_valid) return fail(c, "gfh_debug_mesh_stats: no recorded quadrature mesh (a pass of a model with integrate() must have run)");
  HIPCHK(k, hipStreamSynchronize(k->stream));
  const size_t bytes = (size_t)k->disp.mesh_stride * (size_t)k->n_slots;
  std::vector<unsigned char> h(bytes);
  HIPCHK(k, hipMemcpy(h.data(), k->disp.mesh.p, bytes, hipMemcpyDeviceToHost));
  const int sites = k->disp.mesh_stride / kMeshRecord;
  // (data slots only: the pads between datasets carry w = 0 and are evaluated like any other slot, but are not data)
  for (int d = 0; d < k->nd; d++)
    for (int64_t sl = k->ds_slot[d], e = k->ds_slot[d] + (k->lb[d + 1] - k->lb[d]); sl < e; sl++)
      for (int q = 0; q < sites; q++) {
        const unsigned char v = h[(size_t)sl * k->disp.mesh_stride + (size_t)q * kMeshRecord];
        if (v == 255) out4[2]++; else { out4[0]++; out4[1] += v; }
      }
  out4[3] = (int64_t)sites;
  return 0;
}
int gfh_debug_deferred(gfh_ctx* c, long long* out4) {
  if (!c || !out4) return 1;
  const gfh_ctx* k = c->grp ? gfh::group_member(c, 0) : c;
  out4[0] = k->defer.n_deferred; out4[1] = k->defer.n_stored; out4[2] = k->defer.n_materialised;
  out4[3] = k->defer.owed && k->have_sweep ? 1 : 0;
  return 0;
}
int gfh_debug_layout(gfh_ctx* c, int64_t* out8) {
  if (!c || !out8) return 1;
  const gfh_ctx* k = c->grp ? gfh::group_member(c, 0) : c;
  int held = 0;
  for (int d = 0; d < k->nd && (size_t)d + 1 < k->h_ds_first_gb.size(); d++) if (k->h_ds_first_gb[(size_t)d + 1] > k->h_ds_first_gb[(size_t)d]) held++;
  out8[0] = k->n_slots; out8[1] = k->n_gb; out8[2] = held;
  const bool swept = k->have_sweep && k->cur;
  out8[3] = swept ? k->last_sweep.fused : -1; out8[4] = swept ? k->last_sweep.waves : -1; out8[5] = swept ? k->last_sweep.tail_mode : -1;
  out8[6] = swept ? k->last_sweep.sparse : -1; out8[7] = swept ? k->cur->kernarg_pars : -1;
  return 0;
}
// What ran behind the model kernel of the most recent sweep and of the most recent J^T v product, as the host noted it at each launch
// (context.h, Chain): a report, not a rule -- the rules are launch_gram, launch_gram_chain, sweep_pass and jtv_finish.
int gfh_debug_chain(gfh_ctx* c, int64_t* out, int cap) {
  if (!c || !out || cap < 3) return 1;
  const gfh_ctx* k = c->grp ? gfh::group_member(c, 0) : c;
  out[0] = k->chain.assemble; out[1] = k->chain.jtv_finish; out[2] = (int64_t)k->chain.gram.size();
  for (size_t i = 0; i < k->chain.gram.size() && 3 + 6 * (i + 1) <= (size_t)cap; i++) {
    const GramLaunch& g = k->chain.gram[i];
    int64_t* o = out + 3 + 6 * i;
    o[0] = g.kind; o[1] = g.a; o[2] = g.b; o[3] = g.sym; o[4] = g.r0; o[5] = g.c0;
  }
  return 0;
}
int gfh_device_memory(gfh_ctx* c, int64_t* out3) {
  if (!c || !out3) return 1;
  gfh_ctx* k = c->grp ? gfh::group_member(c, 0) : c;
  if (k->device < 0) return fail(c, "no GPU bound to this context");
  if (hipSetDevice(k->device) != hipSuccess) return fail(c, "hipSetDevice failed");
  size_t free_b = 0, total_b = 0;
  HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
  out3[0] = (int64_t)free_b; out3[1] = (int64_t)total_b; out3[2] = 0;
  const int n = c->grp ? gfh_group_size(c) : 1;
  for (int r = 0; r < n; r++) out3[2] += (int64_t)(c->grp ? gfh::group_member(c, r) : c)->ws.wsg.bytes;
  out3[2] += (int64_t)batch_bytes(c) + (int64_t)curves_bytes(c);
  return 0;
}

}  // extern "C"
