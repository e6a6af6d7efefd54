// data.cpp -- partition and residency of the points: which range of the caller's arrays a rank holds (gfh_partition), the padded
// slot layout and the gram-block tables built from it, the upload of points and auxiliary columns, and the re-cut of the ranges
// under adaptive load balancing.  It knows nothing of models or kernels beyond the model kind that sizes the gram blocks.
#include "context_internal.h"
#include "group.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <memory>

using namespace gfh;

// gadfit.F90:977-983 with arbitrary image weights (re_initialize STEP 2): sizes = int(w*N), remainder +1 to the first images
static void partition_weighted(int64_t n_total, const std::vector<double>& w, int rank, int64_t* begin, int64_t* count) {
  const int n = (int)w.size();
  std::vector<int64_t> sizes(n);
  int64_t tmp = 0;
  for (int i = 0; i < n; i++) { sizes[i] = (int64_t)(w[i] * (double)n_total); if (sizes[i] < 0) sizes[i] = 0; tmp += sizes[i]; }
  for (int i = 0; i < n; i++) if (i + 1 <= n_total - tmp) sizes[i]++;
  int64_t b = 0;
  for (int i = 0; i < rank; i++) b += sizes[i];
  *begin = b; *count = sizes[rank];
}

// ------------------------------------------------------------------------- data
constexpr int kGramTarget = 512;       // aimed number of gram workgroups (about two per CU)
constexpr int kGramTargetFine = 8192;  // models with integrate(): the cost of a point varies along x (number of bisections), so
                                       // the contiguous blocks are kept small and the hardware deals them out as workgroups retire
constexpr int kPassGranule = 512;      // slots one pass of an 8-wave workgroup covers; divides kPadGranule
// Number of gram workgroups to aim for: about two 8-wave workgroups per CU; many small ones for quadrature models.
// (4-wave workgroups on 768 blocks for the VALU form of the fused kernel were measured: cfg 2 0.174 against 0.166 ms, and
// gfh_k_chi2 on the same partition 0.077 against 0.064 ms.)
static int gb_target_for(const gfh_ctx* c) {
  return c->has_model && c->model.has_integrals() ? kGramTargetFine : kGramTarget;
}

static int build_layout(gfh_ctx* c) {
  // local per-dataset ranges = intersection of [begin, begin+count) with each dataset
  // (equivalent to img_bounds, gadfit.F90:984-1002)
  const int nd = c->nd;
  c->lb.assign(nd + 1, 0);
  c->ds_slot.assign(nd + 1, 0);
  const int64_t lo = c->begin, hi = c->begin + c->count;
  for (int d = 0; d < nd; d++) {
    int64_t a = std::max(lo, c->dp[d]), b = std::min(hi, c->dp[d + 1]);
    int64_t len = b > a ? b - a : 0;
    c->lb[d + 1] = c->lb[d] + len;
    int64_t padded = (len + kPadGranule - 1) / kPadGranule * kPadGranule;
    c->ds_slot[d + 1] = c->ds_slot[d] + padded;
  }
  c->n_slots = c->ds_slot[nd];
  c->ldj = c->n_slots;
  // gram workgroups: whole 256-slot tiles of one dataset each
  c->gb_target = gb_target_for(c);
  const int target = c->gb_target;
  int64_t per = (c->n_slots + target - 1) / target;
  per = std::max<int64_t>(kPassGranule, (per + kPassGranule - 1) / kPassGranule * kPassGranule);   // whole passes of the widest workgroup (8 waves)
  // a few passes in all (the fits of a few hundred points most of gadfit's use consists of): one workgroup per dataset -- a pass
  // costs ~2 us, a hand-off between workgroups ~5, and a single workgroup takes the fused kernel's short tail
  if (c->n_slots <= 4 * kPassGranule) per = std::max<int64_t>(per, c->n_slots);
  c->h_gb_start.clear(); c->h_gb_slots.clear(); c->h_gb_ds.clear(); c->h_ds_first_gb.assign(nd + 1, 0);
  for (int d = 0; d < nd; d++) {
    c->h_ds_first_gb[d] = (int)c->h_gb_start.size();
    for (int64_t s = c->ds_slot[d]; s < c->ds_slot[d + 1]; s += per) {
      c->h_gb_start.push_back(s);
      c->h_gb_slots.push_back((int)std::min<int64_t>(per, c->ds_slot[d + 1] - s));
      c->h_gb_ds.push_back(d);
    }
  }
  c->h_ds_first_gb[nd] = (int)c->h_gb_start.size();
  c->n_gb = (int)c->h_gb_start.size();
  return 0;
}

static int upload_tables(gfh_ctx* c) {
  const int ngb = std::max(1, c->n_gb);
  if (dev_alloc(c, c->gb_start, sizeof(int64_t) * ngb) || dev_alloc(c, c->gb_slots, sizeof(int) * ngb) ||
      dev_alloc(c, c->gb_ds, sizeof(int) * ngb) || dev_alloc(c, c->ds_first_gb, sizeof(int) * (c->nd + 1))) return 1;
  if (c->n_gb) {
    HIPCHK(c, hipMemcpy(c->gb_start.p, c->h_gb_start.data(), sizeof(int64_t) * c->n_gb, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->gb_slots.p, c->h_gb_slots.data(), sizeof(int) * c->n_gb, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->gb_ds.p, c->h_gb_ds.data(), sizeof(int) * c->n_gb, hipMemcpyHostToDevice));
  }
  HIPCHK(c, hipMemcpy(c->ds_first_gb.p, c->h_ds_first_gb.data(), sizeof(int) * (c->nd + 1), hipMemcpyHostToDevice));
  c->tile = 0;   // tile_ds is rebuilt lazily for the kernel's tile size
  return 0;
}

// the gram-block partition follows the model kind (build_layout): rebuilt when a model set AFTER the data changes it
int gfh::ensure_gb_partition(gfh_ctx* c) {
  if (!c->nd || c->gb_target == gb_target_for(c)) return 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (build_layout(c)) return 1;
  c->prepared = false; c->have_sweep = false; c->tail_host.clear();
  return upload_tables(c);
}

int gfh::ensure_tile_table(gfh_ctx* c) {
  const int tile = c->gen.block;
  if (c->tile == tile) return 0;
  if (kPadGranule % tile) return fail(c, "tile size must divide the pad granule");
  c->n_tiles = (int)(c->n_slots / tile);
  std::vector<int> t(std::max(1, c->n_tiles));
  for (int d = 0; d < c->nd; d++)
    for (int64_t s = c->ds_slot[d] / tile; s < c->ds_slot[d + 1] / tile; s++) t[s] = d;
  if (dev_alloc(c, c->tile_ds, sizeof(int) * t.size())) return 1;
  HIPCHK(c, hipMemcpy(c->tile_ds.p, t.data(), sizeof(int) * t.size(), hipMemcpyHostToDevice));
  c->tile = tile;
  return 0;
}

// xs/ys/ws point at the element with global index `begin` (local slice)
static int upload_points_impl(gfh_ctx* c, const double* xs, const double* ys, const double* ws) {
  gfh::Range range("gadfit upload of the data points");
  copy_path_ready();
  const size_t nb = sizeof(double) * (size_t)std::max<int64_t>(1, c->n_slots);
  if (dev_alloc(c, c->x, nb) || dev_alloc(c, c->y, nb) || dev_alloc(c, c->w, nb) || dev_alloc(c, c->res, nb) ||
      dev_alloc(c, c->omega, nb) || dev_alloc(c, c->is_pad, (size_t)std::max<int64_t>(1, c->n_slots))) return 1;
  const double* src[3] = {xs, ys, ws};
  DevBuf* dst[3] = {&c->x, &c->y, &c->w};
  if (c->nd <= 256 && c->n_slots) {
    // Few, long datasets (the large-N case): every dataset's points go down straight from the caller's arrays, one copy per
    // array and dataset, and a small kernel writes the pad slots -- no host-side staging pass over N-sized arrays (that pass and the
    // staged copies were 35 ms of a 50 ms hand-over at N = 1e7; a ten-iteration fit is 5-6 ms).
    std::vector<int64_t> seg((size_t)3 * c->nd);
    for (int d = 0; d < c->nd; d++) { seg[3 * d] = c->ds_slot[d]; seg[3 * d + 1] = c->lb[d + 1] - c->lb[d]; seg[3 * d + 2] = c->ds_slot[d + 1]; }
    DevBuf dseg;
    if (dev_alloc(c, dseg, sizeof(int64_t) * seg.size())) return 1;
    hipError_t e = hipMemcpy(dseg.p, seg.data(), sizeof(int64_t) * seg.size(), hipMemcpyHostToDevice);
    // (the FIRST upload of a process takes ~16 ms for 3 x 80 MB, every later one ~5 ms -- fresh arrays, a second context alike,
    // tools/probes/upload_cost.py: a one-time cost of the runtime's copy path, not of these arrays; three threads, one per array,
    // change nothing.  warm_copy_path pays it beside the caller's own work after gfh_create, where there is any.)
    for (int k = 0; k < 3 && e == hipSuccess; k++)
      for (int d = 0; d < c->nd && e == hipSuccess; d++) {
        const int64_t len = c->lb[d + 1] - c->lb[d];
        if (len) e = hipMemcpy(dst[k]->as<double>() + c->ds_slot[d], src[k] + c->lb[d], sizeof(double) * (size_t)len, hipMemcpyHostToDevice);
      }
    if (e == hipSuccess) e = hipMemsetAsync(c->is_pad.p, 0, (size_t)c->n_slots, c->stream);
    if (e == hipSuccess) e = launch_fill_pads(c->stream, c->nd, dseg.as<i64>(), c->x.as<double>(), c->y.as<double>(), c->w.as<double>(), c->is_pad.as<unsigned char>());
    if (e == hipSuccess) e = hipMemsetAsync(c->res.p, 0, sizeof(double) * (size_t)c->n_slots, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->omega.p, 0, sizeof(double) * (size_t)c->n_slots, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(dseg);
    if (e != hipSuccess) return fail(c, std::string("gfh_set_data: ") + hipGetErrorString(e));
    c->have_sweep = false;
    return 0;
  }
  std::vector<double> stage((size_t)c->n_slots);
  std::vector<unsigned char> pad((size_t)c->n_slots, 1);
  for (int k = 0; k < 3; k++) {
    for (int d = 0; d < c->nd; d++) {
      const int64_t len = c->lb[d + 1] - c->lb[d];
      const int64_t s0 = c->ds_slot[d], s1 = c->ds_slot[d + 1];
      if (len) memcpy(&stage[(size_t)s0], src[k] + c->lb[d], sizeof(double) * (size_t)len);
      // pad slots: a real abscissa of the same dataset (so f stays finite), y = 0, w = 0
      const double fill = (k == 0 && len) ? src[0][c->lb[d] + len - 1] : 0.0;
      for (int64_t s = s0 + len; s < s1; s++) stage[(size_t)s] = fill;
      if (k == 0) for (int64_t s = s0; s < s0 + len; s++) pad[(size_t)s] = 0;
    }
    if (c->n_slots) HIPCHK(c, hipMemcpy(dst[k]->p, stage.data(), sizeof(double) * (size_t)c->n_slots, hipMemcpyHostToDevice));
  }
  if (c->n_slots) {
    HIPCHK(c, hipMemcpy(c->is_pad.p, pad.data(), (size_t)c->n_slots, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->res.p, 0, sizeof(double) * (size_t)c->n_slots));
    HIPCHK(c, hipMemset(c->omega.p, 0, sizeof(double) * (size_t)c->n_slots));
  }
  c->have_sweep = false;
  return 0;
}
static int upload_points(gfh_ctx* c, const double* xs, const double* ys, const double* ws) {
  // no C++ exception may cross the C ABI: host staging of N-sized arrays can run out of memory
  try { return upload_points_impl(c, xs, ys, ws); }
  catch (const std::exception& e) { return fail(c, std::string("gfh_set_data: ") + e.what()); }
}

int gfh::set_geometry(gfh_ctx* c, int64_t n_total, int nd, const int64_t* dp) {
  if (nd < 1 || !dp || dp[0] != 0 || dp[nd] != n_total) return fail(c, "data_positions must start at 0 and end at n_total");
  for (int d = 0; d < nd; d++) if (dp[d + 1] < dp[d]) return fail(c, "data_positions must be non-decreasing");
  c->n_total = n_total; c->nd = nd; c->dp.assign(dp, dp + nd + 1);
  // new data: the Jacobian/residuals on the device are stale, and the kernel form follows n_datasets
  c->cur = nullptr; c->cur_active.clear(); c->have_sweep = false; c->j_valid = false; c->defer.owed = c->defer.chi2_after = false; c->prepared = false;
  c->n_aux = 0;                     // auxiliary columns belong to the data they were tabulated for
  c->disp.mesh_valid = false;
  c->disp.order_ready = false; c->disp.order_want = true;
  if ((int)c->bal.part_w.size() == c->nranks) partition_weighted(n_total, c->bal.part_w, c->rank, &c->begin, &c->count);
  else gfh_partition(n_total, c->nranks, c->rank, &c->begin, &c->count);
  return build_layout(c);
}

extern "C" {

void gfh_partition(int64_t n_total, int nranks, int rank, int64_t* begin, int64_t* count) {
  // gadfit.F90:978-983 with img_weights = 1/num_images: sizes = int(w*N), remainder +1 to
  // the first images.
  std::vector<int64_t> sizes(nranks);
  int64_t tmp = 0;
  for (int i = 0; i < nranks; i++) { sizes[i] = (int64_t)((1.0 / nranks) * (double)n_total); tmp += sizes[i]; }
  for (int i = 0; i < nranks; i++) if (i + 1 <= n_total - tmp) sizes[i]++;
  int64_t b = 0;
  for (int i = 0; i < rank; i++) b += sizes[i];
  *begin = b; *count = sizes[rank];
}

int gfh_set_data(gfh_ctx* c, int64_t n_total, const double* x, const double* y, const double* w, int nd, const int64_t* dp) {
  GROUP(c, gfh_set_data(k, n_total, x, y, w, nd, dp));      // every member uploads its own contiguous range (gadfit.F90:977-983)
  NEED_GPU(c);
  if (!x || !y || !w) return fail(c, "null data array");
  c->bal.part_w.clear(); c->bal.t_prev = 0.0; c->bal.weights_type = -1; c->bal.haux.clear(); c->bal.h_n_aux = 0;
  if (set_geometry(c, n_total, nd, dp)) return 1;
  if (c->bal.on) {
    try { c->bal.hx.assign(x, x + n_total); c->bal.hy.assign(y, y + n_total); c->bal.hw.assign(w, w + n_total); }
    catch (const std::exception& e) { return fail(c, std::string("gfh_set_data (host copy for load balancing): ") + e.what()); }
  } else { c->bal.hx.clear(); c->bal.hy.clear(); c->bal.hw.clear(); }
  if (upload_tables(c)) return 1;
  return upload_points(c, x + c->begin, y + c->begin, w + c->begin);
}

}  // extern "C"

// gfh_set_data that returns at once: geometry and tables are set here, the N-sized copies run on a thread of the library and are
// waited for by the next call on this context (whose return code then carries a failure of the upload).  For callers that have
// host work of their own to do meanwhile -- the Fortran layer records eval() over the data (gadfit.F90, discover).
// The copy queued by gfh_queue_host_copy is made whatever becomes of the call it was queued for (an early return through
// gfh_set_data under load balancing, an error): on a thread of its own, or at once if none can be started; nothing stays queued.
static void start_host_copy(gfh_ctx* c) {
  if (c->up.host_copy.joinable()) c->up.host_copy.join();
  void* dst = c->up.hc_dst; const void* src = c->up.hc_src; const size_t bytes = c->up.hc_bytes;
  c->up.hc_dst = nullptr; c->up.hc_src = nullptr; c->up.hc_bytes = 0;
  if (!dst || !src || !bytes) return;
  try { c->up.host_copy = std::thread([dst, src, bytes]() { memcpy(dst, src, bytes); }); }
  catch (const std::exception&) { memcpy(dst, src, bytes); }
}

extern "C" {

int gfh_set_data_begin(gfh_ctx* c, int64_t n_total, const double* x, const double* y, const double* w, int nd, const int64_t* dp) {
  GROUP(c, gfh_set_data_begin(k, n_total, x, y, w, nd, dp));
  // the caller's own copy of its abscissas (gfh_queue_host_copy): beside the upload, on a thread of its own -- 80 MB into fresh
  // pages take longer than the upload of 240 MB, and nothing on the device waits for them (gfh_wait_host_copy)
  if (c) start_host_copy(c);
  // (a context whose device part is still being set up, gfh_create_begin: the upload is queued behind it instead of waiting here)
  std::thread creation;
  if (c && c->device >= 0 && c->up.creating && c->up.pending.joinable() && !c->bal.on) { creation = std::move(c->up.pending); c->up.creating = false; }
  else NEED_GPU(c);
  auto bail = [&](int rc) { if (creation.joinable()) { creation.join(); if (c->up.pending_rc) rc = 1; c->up.pending_rc = 0; } return rc; };
  if (!x || !y || !w) return bail(fail(c, "null data array"));
  if (c->bal.on) return gfh_set_data(c, n_total, x, y, w, nd, dp);      // (keeps a host copy: nothing to overlap)
  c->bal.part_w.clear(); c->bal.t_prev = 0.0; c->bal.weights_type = -1; c->bal.haux.clear(); c->bal.h_n_aux = 0;
  if (set_geometry(c, n_total, nd, dp)) return bail(1);
  c->bal.hx.clear(); c->bal.hy.clear(); c->bal.hw.clear();
  const int64_t b = c->begin;
  if (!creation.joinable()) c->up.pending_rc = 0;
  // (the creation thread, still running, travels into the upload thread inside `prev`.  Should that thread not start -- std::thread
  // throws on EAGAIN -- `prev` must be joined HERE: unwinding would destroy a joinable std::thread, which is std::terminate
  // before any handler runs, and bail() only knows `creation`, moved from by then: round-5 advisor)
  std::shared_ptr<std::thread> prev;
  try {
    prev = std::make_shared<std::thread>(std::move(creation));
    c->up.pending = std::thread([c, x, y, w, b, prev]() {
      int rc = 0;
      if (prev->joinable()) { prev->join(); rc = c->up.pending_rc; }      // (its failure is this upload's: create_failed holds the message)
      if (!rc) rc = hipSetDevice(c->device) == hipSuccess ? 0 : fail(c, "hipSetDevice failed");
      if (!rc) rc = upload_tables(c);
      if (!rc) rc = upload_points(c, x + b, y + b, w + b);
      c->up.pending_rc = rc;
    });
  } catch (const std::exception& e) {
    int rc = fail(c, std::string("gfh_set_data_begin: ") + e.what());
    if (prev && prev->joinable()) { prev->join(); if (c->up.pending_rc) rc = 1; c->up.pending_rc = 0; }
    return bail(rc);
  }
  return 0;
}

// A host-to-host copy for the thread of the next gfh_set_data_begin to make once its upload is done (handle of a device group: member 0's thread).
int gfh_queue_host_copy(gfh_ctx* c, void* dst, const void* src, int64_t bytes) {
  if (!c) return 1;
  gfh_ctx* k = c->grp ? gfh::group_member(c, 0) : c;
  if (k->up.pending.joinable() && !k->up.creating) return fail(c, "gfh_queue_host_copy: an upload is in flight already");
  if (k->up.host_copy.joinable()) k->up.host_copy.join();
  k->up.hc_dst = dst; k->up.hc_src = src; k->up.hc_bytes = bytes > 0 ? (size_t)bytes : 0;
  return 0;
}
int gfh_wait_host_copy(gfh_ctx* c) {
  if (!c) return 1;
  gfh_ctx* k = c->grp ? gfh::group_member(c, 0) : c;
  if (k->up.host_copy.joinable()) k->up.host_copy.join();
  return 0;
}

int gfh_set_data_local(gfh_ctx* c, int64_t n_total, int nd, const int64_t* dp, int64_t begin, int64_t count,
                       const double* x, const double* y, const double* w) {
  NOT_FOR_GROUP(c, "gfh_set_data_local");
  NEED_GPU(c);
  if (c->bal.on) return fail(c, "load balancing needs the whole arrays: use gfh_set_data");
  c->bal.part_w.clear();
  if (set_geometry(c, n_total, nd, dp)) return 1;
  if (begin != c->begin || count != c->count) return fail(c, "local slice does not match gfh_partition for this rank");
  if (upload_tables(c)) return 1;
  return upload_points(c, x, y, w);
}

}  // extern "C"

// Auxiliary per-point columns (GFH_AUX nodes): column k of the caller's [n_aux][ld] array, laid out on
// the device like x (per-dataset padding; pad slots repeat the dataset's last real point, their w is 0).
static int upload_aux(gfh_ctx* c, int n_aux, const double* aux_local, int64_t ld) try {
  if (!c->nd) return fail(c, "gfh_set_aux: set the data first (gfh_set_data)");
  if (n_aux < 0 || (n_aux > 0 && !aux_local)) return fail(c, "gfh_set_aux: bad arguments");
  c->n_aux = n_aux; c->aux_serial++; c->disp.mesh_valid = false;
  if (!n_aux) return 0;
  if (dev_alloc(c, c->aux, sizeof(double) * (size_t)n_aux * (size_t)std::max<int64_t>(1, c->n_slots))) return 1;
  // From inside the parameter hook (columns that follow the parameters, refreshed before a pass) the copies below overwrite what the
  // kernels of the PREVIOUS pass read, and they are synchronous copies on the null stream while c->stream is non-blocking: nothing
  // but this wait orders them behind those kernels (the host has seen the previous pass's mailbox, but a result can arrive before
  // its kernel has retired: round-5 advisor).  A few microseconds before a tabulation of milliseconds.
  if (c->in_pars_hook) HIPCHK(c, hipStreamSynchronize(c->stream));
  // each dataset's segment straight from the caller's column (no staging copy of the whole column: at 1e7 points that copy and
  // its fresh pages cost more than the transfer), then its pad slots (fewer than 512 per dataset)
  std::vector<double> pads;
  for (int k = 0; k < n_aux; k++) {
    const double* src = aux_local + (size_t)k * (size_t)ld;
    double* dst = c->aux.as<double>() + (size_t)k * (size_t)c->n_slots;
    for (int d = 0; d < c->nd; d++) {
      const int64_t len = c->lb[d + 1] - c->lb[d];
      const int64_t s0 = c->ds_slot[d], s1 = c->ds_slot[d + 1];
      if (len) HIPCHK(c, hipMemcpy(dst + s0, src + c->lb[d], sizeof(double) * (size_t)len, hipMemcpyHostToDevice));
      if (s1 > s0 + len) {
        pads.assign((size_t)(s1 - s0 - len), len ? src[c->lb[d] + len - 1] : 0.0);
        HIPCHK(c, hipMemcpy(dst + s0 + len, pads.data(), sizeof(double) * pads.size(), hipMemcpyHostToDevice));
      }
    }
  }
  if (!c->in_pars_hook) c->have_sweep = false;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_aux: ") + e.what()); }

extern "C" {

int gfh_set_aux(gfh_ctx* c, int n_aux, const double* aux) {
  GROUP(c, gfh_set_aux(k, n_aux, aux));
  NEED_GPU(c);
  if (c->bal.on && n_aux > 0 && aux) {
    try { c->bal.haux.assign(aux, aux + (size_t)n_aux * (size_t)c->n_total); c->bal.h_n_aux = n_aux; }
    catch (const std::exception& e) { return fail(c, std::string("gfh_set_aux (host copy for load balancing): ") + e.what()); }
  } else { c->bal.haux.clear(); c->bal.h_n_aux = 0; }
  return upload_aux(c, n_aux, aux ? aux + c->begin : nullptr, c->n_total);
}
int gfh_set_aux_local(gfh_ctx* c, int n_aux, const double* aux_local) {
  NOT_FOR_GROUP(c, "gfh_set_aux_local");
  NEED_GPU(c);
  return upload_aux(c, n_aux, aux_local, c->count);
}

int gfh_set_load_balancing(gfh_ctx* c, int on) {
  if (!c) return 1;
  GROUP(c, gfh_set_load_balancing(k, on));
  c->bal.on = on != 0;      // takes effect for data set from now on (the host copy is made by gfh_set_data)
  if (!on) { c->bal.hx.clear(); c->bal.hy.clear(); c->bal.hw.clear(); c->bal.haux.clear(); c->bal.hx.shrink_to_fit(); c->bal.hy.shrink_to_fit(); c->bal.hw.shrink_to_fit(); c->bal.haux.shrink_to_fit(); }
  return 0;
}

// New ranges for every rank from image weights (all ranks pass the same): layout, tables and this rank's points are
// rebuilt from the host copy; weights (gfh_init_weights) and auxiliary columns are re-applied.
int gfh_repartition(gfh_ctx* c, const double* weights) {
  GROUP(c, gfh_repartition(k, weights));
  NEED_GPU(c);
  if (!c->bal.on || c->bal.hx.empty()) return fail(c, "gfh_repartition needs gfh_set_load_balancing(1) before gfh_set_data");
  double sum = 0.0;
  for (int i = 0; i < c->nranks; i++) { if (!(weights[i] >= 0.0)) return fail(c, "gfh_repartition: negative weight"); sum += weights[i]; }
  if (!(sum > 0.0)) return fail(c, "gfh_repartition: weights sum to zero");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->bal.part_w.assign(weights, weights + c->nranks);
  for (double& v : c->bal.part_w) v /= sum;                  // the sizes int(w*N) + remainder only add up to N for weights that sum to one
  const std::vector<int64_t> dp = c->dp;                 // set_geometry assigns c->dp from its argument
  const int n_aux = c->bal.h_n_aux;
  if (set_geometry(c, c->n_total, c->nd, dp.data())) return 1;
  if (upload_tables(c)) return 1;
  if (upload_points(c, c->bal.hx.data() + c->begin, c->bal.hy.data() + c->begin, c->bal.hw.data() + c->begin)) return 1;
  if (c->bal.weights_type >= 0 && gfh_init_weights(c, c->bal.weights_type)) return 1;
  if (n_aux && upload_aux(c, n_aux, c->bal.haux.data() + c->begin, c->n_total)) return 1;
  c->bal.moves++;
  return 0;
}

int gfh_init_weights(gfh_ctx* c, int type) {
  GROUP(c, gfh_init_weights(k, type));
  NEED_GPU(c);
  if (type < 0 || type > 4) return fail(c, "Unknown weight specifier. Allowed values are NONE, SQRT_Y, PROPTO_Y, INVERSE_Y, and USER.");
  c->bal.weights_type = type;
  if (!c->n_slots) return 0;
  HIPCHK(c, launch_init_weights(c->stream, type, c->n_slots, c->y.as<double>(), c->w.as<double>(), c->is_pad.as<unsigned char>()));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int64_t gfh_local_count(gfh_ctx* c) {
  if (c && c->grp) { int64_t n = 0; for (int r = 0; r < gfh::group_size(c); r++) n += gfh::group_member(c, r)->count; return n; }   // the whole array
  return c ? c->count : 0;
}
int64_t gfh_local_begin(gfh_ctx* c) { return c && !c->grp ? c->begin : 0; }
int gfh_group_ranges(gfh_ctx* c, int64_t* begins, int64_t* counts) {
  if (!c) return 1;
  if (!c->grp) { begins[0] = c->begin; counts[0] = c->count; return 0; }
  for (int r = 0; r < gfh::group_size(c); r++) { begins[r] = gfh::group_member(c, r)->begin; counts[r] = gfh::group_member(c, r)->count; }
  return 0;
}

// Adaptive parallelism, re_initialize STEP 1 (gadfit.F90:940-975): every rank's device time in the parallel parts
// (STEP 1+2, chi2, STEP 3) since the last call gives new image weights w = old - (1/n - (1/t)/sum(1/t)); the ranges are
// re-cut when that moves some rank's share by more than 1 % of an even share (the reference re-cuts every iteration at
// no cost because every image holds all data; here a move re-uploads the rank's points).  Collective.
int gfh_rebalance(gfh_ctx* c, int* moved) {
  GROUP(c, gfh_rebalance(k, r ? nullptr : moved));
  NEED_GPU(c);
  if (moved) *moved = 0;
  if (!c->bal.on || c->nranks < 2 || c->bal.hx.empty()) return 0;      // (switched on after gfh_set_data: nothing to cut from)
  harvest_events(c);
  const int n = c->nranks;
  const double total = scaled_time(c->timers.t_sweep, c->timers.n_sweep, c->timers.n_sweep_timed) + scaled_time(c->timers.t_gram, c->timers.n_sweep, c->timers.n_chain_timed) + scaled_time(c->timers.t_chi2, c->timers.n_chi2, c->timers.n_chi2_timed) +
                       scaled_time(c->timers.t_omega, c->timers.n_omega, c->timers.n_omega_timed);
  std::vector<double> t((size_t)n, 0.0);
  t[(size_t)c->rank] = total - c->bal.t_prev;
  c->bal.t_prev = total;
  if (c->comm) {
    if (dev_alloc(c, c->vec, sizeof(double) * (size_t)std::max(64, n + 1))) return 1;
    HIPCHK(c, hipMemcpyAsync(c->vec.p, t.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if (allreduce_sum(c, c->vec.as<double>(), (size_t)n)) return 1;
    if (fetch_result(c, c->vec.as<double>(), n, true)) return 1;
    for (int i = 0; i < n; i++) t[(size_t)i] = c->h_pinned[i];
  } else if (c->member_of) {
    int st = 0;
    if (gfh::group_allreduce(c, t.data(), (size_t)n, &st)) return 1;
  } else return 0;                                          // pseudo-ranks (gfh_debug_set_rank): nobody to exchange with
  std::vector<double> old_w = c->bal.part_w;
  if ((int)old_w.size() != n) old_w.assign((size_t)n, 1.0 / n);
  double tmin = t[0];
  for (double v : t) tmin = std::min(tmin, v);
  if (!(tmin > 2.220446049250313e-16)) {                    // "too fast for load balancing to be effective" (gadfit.F90:964-970)
    c->bal.on = false;
    return 0;
  }
  std::vector<double> w((size_t)n);
  double sum = 0.0;
  for (int i = 0; i < n; i++) { w[(size_t)i] = 1.0 / t[(size_t)i]; sum += w[(size_t)i]; }
  for (int i = 0; i < n; i++) {
    w[(size_t)i] = old_w[(size_t)i] - (1.0 / n - w[(size_t)i] / sum);     // gadfit.F90:974-975
    if (w[(size_t)i] < 0.0) w[(size_t)i] = 0.0;
  }
  double shift = 0.0;
  for (int i = 0; i < n; i++) shift = std::max(shift, std::fabs(w[(size_t)i] - old_w[(size_t)i]));
  if (shift * n < 0.01) return 0;
  if (gfh_repartition(c, w.data())) return 1;
  if (moved) *moved = 1;
  return 0;
}

}  // extern "C"
