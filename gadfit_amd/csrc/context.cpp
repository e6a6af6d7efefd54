// context.cpp -- the life cycle of a context (include/gadfit_hip.h): error state, creation on the caller's or the context's own
// thread, destruction, and the plain option setters.  Everything N-sized stays in HBM; per call only the parameter block goes
// down (<= n_datasets*n_pars doubles) and the packed [JTJ | JTres | chi2] comes back.  Memory is devmem.cpp's: this file creates
// and destroys streams and events, never a device or pinned block.
#include "context_internal.h"
#include <dlfcn.h>
#include "group.h"
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>

using namespace gfh;

namespace gfh {
static std::string g_err;
static std::mutex g_err_mutex;     // the members of a device group fail on their own threads
void set_global_error(const std::string& m) { std::lock_guard<std::mutex> lk(g_err_mutex); g_err = m; }
int fail(gfh_ctx* c, const std::string& msg) { if (c) c->err = msg; set_global_error(msg); return 1; }
}  // namespace gfh

namespace gfh {
namespace {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* e = getenv("GADFIT_HIP_ROCTX");
    if (!e || atoi(e) == 0) return;
    void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!push || !pop) { push = nullptr; pop = nullptr; }
  }
};
const Roctx& roctx() { static Roctx r; return r; }
}  // namespace
Range::Range(const char* name) : on_(roctx().push != nullptr) { if (on_) roctx().push(name); }
Range::~Range() { if (on_) roctx().pop(); }

int join_pending(gfh_ctx* c) {
  if (!c->up.pending.joinable()) return 0;
  c->up.pending.join();
  c->up.creating = false;
  const int rc = c->up.pending_rc;
  c->up.pending_rc = 0;
  return rc;
}
// choose whether the next sweeps write the Jacobian (only the fused kernel can do without it)
// does STEP 3 (J^T omega) read the Jacobian back from HBM for the current model and options?
bool omega_needs_jacobian(const gfh_ctx* c, int n_active) {
  return !(c->has_model && unit_carries_omega_jt(c->model, c->gen, n_active));
}

void set_store_j(gfh_ctx* c, bool on) {
  if (!c->fused || (c->has_model && c->model.has_integrals())) on = true;   // the two-kernel path re-reads J
  if (on != c->gen.store_j) { c->gen.store_j = on; c->cur = nullptr; c->have_sweep = false; c->j_valid = false; c->defer.owed = c->defer.chi2_after = false; }
}
// chi2() overwrites the residual vector in the reference (gadfit.F90:1024-1026); only the grad_chi2 / cos_phi tests
// and read-backs ever look at it, so gfh_fit under keep_jacobian mode 2 lets the chi2 kernel skip the 8 B/point store
void set_store_res(gfh_ctx* c, bool on) {
  if (on != c->gen.store_res) { c->gen.store_res = on; c->cur = nullptr; c->prepared = false; c->have_sweep = false; }
}
}  // namespace gfh

// The first host-to-device copy of more than a few KB in a process costs ~10 ms on top of its transfer (the runtime sets its copy
// path up: tools/probes/upload_warm.py -- a first upload of 3 x 80 MB takes 15 ms, after ANY earlier copy of 0.8 MB it takes 5.8).
// The first context of a process makes that copy on a thread of its own, beside whatever the caller does between creating the
// context and handing its data over; an upload waits for it (copy_path_ready), since two first copies at once pay twice.
namespace {
std::once_flag g_copy_warm_once;
std::thread g_copy_warm;
std::mutex g_copy_warm_mutex;
void warm_copy_path(int device) {
  if (const char* e = getenv("GADFIT_HIP_WARM_COPY")) if (atoi(e) == 0) return;
  std::call_once(g_copy_warm_once, [device]() {
    try {
      std::lock_guard<std::mutex> lk(g_copy_warm_mutex);
      g_copy_warm = std::thread([device]() {
        if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return; }
        const size_t bytes = (size_t)1 << 20;
        std::vector<char> host(bytes, 1);
        DevBuf dev;
        if (!dev_alloc_fresh(dev, bytes)) return;
        if (hipMemcpy(dev.p, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) (void)hipGetLastError();
        dev_free(dev);
      });
      std::atexit(copy_path_ready);       // a process that ends without gfh_destroy: the thread is joined before the statics go
    } catch (const std::exception&) {}
  });
}
}  // namespace
void gfh::copy_path_ready() {
  std::lock_guard<std::mutex> lk(g_copy_warm_mutex);
  if (g_copy_warm.joinable()) g_copy_warm.join();
}

// the device part of gfh_create: runtime initialisation (hipGetDeviceCount is where a process pays for it: 80 ms, 240 ms for the first
// process on a box), stream, events, status word, result mailbox -- on the caller's thread (gfh_create) or on the context's own
// (gfh_create_begin); failure leaves the message in the context and in the global slot
static int init_device(gfh_ctx* c) {
  const int device = c->device;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(c, "no HIP device available (libgadfit_hip has no CPU fallback)");
  if (device >= n) return fail(c, "device index out of range");
  if (hipSetDevice(device) != hipSuccess) return fail(c, "cannot initialise HIP device");
  // what the last context destroyed on this device left behind, if anything
  const bool adopted = base_adopt(c);
  if (!adopted && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    return fail(c, "cannot initialise HIP device");
  }
  // the status word (+ the report area of unseen branches, kStatusBytes), the result mailbox's flag and the timing events: every
  // later call dereferences them, so a context without them is not handed out
  bool ok = true;
  if (!adopted) {
    for (auto& ev : c->ev) ok = ok && hipEventCreate(&ev) == hipSuccess;
    ok = ok && base_alloc(c);
  }
  if (ok) ok = hipMemset(c->status.p, 0, gfh::kStatusBytes) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    for (auto& ev : c->ev) { if (ev) hipEventDestroy(ev); ev = nullptr; }
    base_free(c);
    hipStreamDestroy(c->stream);
    c->stream = nullptr;
    return fail(c, "cannot allocate the status word, the result mailbox or the timing events of a context");
  }
  memset(c->h_status, 0, 64); c->h_flag = reinterpret_cast<unsigned long long*>(c->h_status + 2);
  warm_copy_path(device);
  return 0;
}

extern "C" {

int gfh_version(void) { return 100; }

// (the process-wide message is copied under its mutex into a per-thread snapshot: device-group members fail on their own threads)
const char* gfh_last_error(const gfh_ctx* ctx) {
  if (ctx) return ctx->err.c_str();
  static thread_local std::string snap;
  { std::lock_guard<std::mutex> lk(g_err_mutex); snap = g_err; }
  return snap.c_str();
}

int gfh_create(int device, gfh_ctx** out) {
  if (!out) return 1;
  *out = nullptr;
  gfh_ctx* c = new gfh_ctx();
  c->device = device;
  if (const char* e = getenv("GADFIT_HIP_OMEGA_JT")) c->gen.omega_jt = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_KERNARG")) c->kernarg = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_TAIL")) c->tail = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_SPARSE")) c->sparse_ok = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_MERGE_SMALL")) c->merge_small = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_FAST_DIV")) c->gen.fast_div = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_FUSED")) c->fused = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_LOOKAHEAD")) c->lookahead = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_KEEP_J")) { int v = atoi(e); if (v >= 0 && v <= 2) { c->keep_jacobian = v; c->gen.store_j = v != 0; } }
  if (const char* e = getenv("GADFIT_HIP_DEFER_J")) c->defer.on = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_DEFER_J_FROM")) { const long long v = atoll(e); if (v >= 0) c->defer.from = (size_t)v; }
  if (const char* e = getenv("GADFIT_HIP_MESH")) c->disp.mesh_on = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_ORDER")) c->disp.order_on = atoi(e) != 0;
  if (const char* e = getenv("GADFIT_HIP_PLACEMENT_AFTER")) { int v = atoi(e); if (v >= 0) c->place.after = v; }
  if (const char* e = getenv("GADFIT_HIP_WS_FAST")) { int v = atoi(e); if (v >= 0) c->ws.fast = v; }
  if (const char* e = getenv("GADFIT_HIP_TIMERS")) { int v = atoi(e); if (v >= 0 && v <= 2) c->timers.detail = v; }
  if (device >= 0 && init_device(c)) { delete c; return 1; }
  *out = c;
  return 0;
}

// gfh_create that returns at once: the device part runs on a thread of the context, beside whatever the caller does next on the
// host; the first call that needs the device waits for it (NEED_GPU), and gfh_set_data_begin queues its upload behind it.
int gfh_create_begin(int device, gfh_ctx** out) {
  if (device < 0) return gfh_create(device, out);
  if (const char* e = getenv("GADFIT_HIP_ASYNC_INIT")) if (atoi(e) == 0) return gfh_create(device, out);
  if (!out) return 1;
  *out = nullptr;
  gfh_ctx* c = nullptr;
  if (gfh_create(-1, &c)) return 1;          // (the host part: configuration from the environment)
  c->device = device;
  c->up.pending_rc = 0; c->up.creating = true;
  try {
    c->up.pending = std::thread([c]() {
      const int rc = init_device(c);
      if (rc) { c->up.create_failed = true; c->up.create_err = c->err; }
      c->up.pending_rc = rc;
    });
  } catch (const std::exception&) {
    c->up.creating = false;
    if (init_device(c)) { c->device = -1; gfh_destroy(c); return 1; }
  }
  *out = c;
  return 0;
}

int gfh_create_group(int n_devices, const int* devices, gfh_ctx** out) { return gfh::group_create(n_devices, devices, out); }
int gfh_group_size(const gfh_ctx* c) { return c ? (c->grp ? gfh::group_size(c) : 1) : 0; }

void gfh_destroy(gfh_ctx* c) {
  if (!c) return;
  (void)gfh::join_pending(c);          // (stops the upload thread's keep-warm loop instead of waiting it out)
  if (c->up.host_copy.joinable()) c->up.host_copy.join();
  copy_path_ready();
  if (c->grp) gfh::group_destroy(c);
  if (c->device >= 0) {
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->comm) ncclCommDestroy(c->comm);
    for (auto& kv : c->kernel_cache) release_loaded(c->device, &kv.second);
    DevBuf* bufs[] = {&c->x, &c->y, &c->w, &c->res, &c->omega, &c->is_pad, &c->J, &c->tile_ds, &c->gb_start, &c->gb_slots,
                      &c->gb_ds, &c->ds_first_gb, &c->partial, &c->G, &c->chi2_partial, &c->packed, &c->pars, &c->dpars,
                      &c->inv, &c->dl, &c->vec, &c->slice, &c->counters, &c->tail_dev, &c->aux, &c->disp.mesh, &c->disp.tile_cost, &c->disp.tile_order, &c->disp.gb_order, &c->owner, &c->nz_row, &c->nz_col, &c->gs_meta, &c->gs_list, &c->ws.wsg,
                      &c->batch.x, &c->batch.y, &c->batch.w, &c->batch.off_d, &c->batch.io, &c->batch.img,
                      &c->batch.stage_y, &c->batch.stage_w, &c->curves.io, &c->curves.out};
    for (DevBuf* b : bufs) dev_release(c->device, *b);
    // stream, events, status word and pinned buffers: parked for the next context of this device (one set), else given back
    if (!base_park(c)) {
      base_free(c);
      for (auto& ev : c->ev) if (ev) hipEventDestroy(ev);
      if (c->stream) hipStreamDestroy(c->stream);
    }
  }
  delete c;
}

int gfh_set_loss(gfh_ctx* c, int loss) {
  if (!c) return 1;
  GROUP(c, gfh_set_loss(k, loss));
  if (loss < GFH_LOSS_LINEAR || loss > GFH_LOSS_HUBER) return fail(c, "gfh_set_loss: unknown loss function");
  if (loss != c->gen.loss) { c->gen.loss = loss; c->cur = nullptr; c->have_sweep = false; }
  return 0;
}

int gfh_set_use_ad(gfh_ctx* c, int on) {
  if (!c) return 1;
  GROUP(c, gfh_set_use_ad(k, on));
  const bool fd = on == 0;
  if (fd != c->gen.finite_diff) { c->gen.finite_diff = fd; c->cur = nullptr; c->have_sweep = false; c->prepared = false; c->disp.mesh_valid = false; }
  return 0;
}

int gfh_set_fd_column_sets(gfh_ctx* c, int on) {
  if (!c) return 1;
  GROUP(c, gfh_set_fd_column_sets(k, on));
  const bool v = on != 0;
  if (v != c->gen.fd_col_sets) { c->gen.fd_col_sets = v; c->cur = nullptr; c->have_sweep = false; c->prepared = false; }
  return 0;
}

int gfh_set_keep_jacobian(gfh_ctx* c, int mode) {
  if (!c) return 1;
  GROUP(c, gfh_set_keep_jacobian(k, mode));
  if (mode < 0 || mode > 2) return fail(c, "gfh_set_keep_jacobian: mode must be 0, 1 or 2");
  c->keep_jacobian = mode;
  gfh::set_store_j(c, mode != 0);
  if (mode != 2) gfh::set_store_res(c, true);
  return 0;
}

int gfh_set_timer_detail(gfh_ctx* c, int level) {
  if (!c) return 1;
  GROUP(c, gfh_set_timer_detail(k, level));
  if (level < 0 || level > 2) return fail(c, "gfh_set_timer_detail: level must be 0, 1 or 2");
  c->timers.detail = level;
  return 0;
}

int gfh_set_lookahead(gfh_ctx* c, int on) {
  if (!c) return 1;
  GROUP(c, gfh_set_lookahead(k, on));
  c->lookahead = on != 0;
  return 0;
}

int gfh_set_pars_hook(gfh_ctx* c, gfh_pars_hook fn, void* user) {
  if (!c) return 1;
  GROUP(c, gfh_set_pars_hook(k, fn, user));
  c->pars_fn = fn; c->pars_user = user;
  return 0;
}
int gfh_set_unseen_handler(gfh_ctx* c, gfh_unseen_handler fn, void* user) {
  if (!c) return 1;
  GROUP(c, gfh_set_unseen_handler(k, fn, user));
  c->unseen_fn = fn; c->unseen_user = user;
  return 0;
}

}  // extern "C"
