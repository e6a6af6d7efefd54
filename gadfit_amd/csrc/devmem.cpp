// devmem.cpp -- all device and pinned memory of the library: the blocks of a context (DevBuf), the per-device pool that keeps small
// ones between contexts, the parked base resources of a destroyed context, and the pinned mailbox and staging blocks.  No other file
// calls the runtime's allocation or free functions; this one launches nothing and knows nothing of what the blocks hold.
#include "context_internal.h"
#include <cstdlib>
#include <map>
#include <mutex>

using namespace gfh;

// A batch of small fits -- gadf_init ... gadf_close per spectrum -- creates and destroys a context per fit, and what that costs is
// the runtime's own calls: ~25 hipFree (each waits for the device) and as many hipMalloc, a stream, six events, three pinned
// allocations: 3.6 ms around a fit of 0.9 ms (tools/probes/context_cycle.py).  So what a destroyed context held is kept for the
// next one of the same device: its small device blocks (up to 4 MB each, 64 MB per device in all, in power-of-two classes) and
// its stream, events, status word and pinned buffers (BaseRes, one parked set per device).  GADFIT_HIP_POOL=0: everything is
// returned to the runtime as before.  Blocks enter the pool only from gfh_destroy, after the context's stream has drained.
namespace {
constexpr size_t kPoolBlockMax = (size_t)4 << 20, kPoolCap = (size_t)64 << 20;
struct BaseRes {
  hipStream_t stream = nullptr; hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  DevBuf status; int* h_status = nullptr;
  double* h_pinned = nullptr; size_t h_pinned_bytes = 0;
  double* h_pars = nullptr; size_t h_pars_bytes = 0;
  double* h_dpars = nullptr; size_t h_dpars_bytes = 0;
};
struct DevicePool { std::vector<void*> blocks[32]; size_t cached = 0; bool has_base = false; BaseRes base; };
std::mutex g_pool_mutex;
std::map<int, DevicePool> g_pool;
bool pool_on() { static const bool on = [] { const char* e = getenv("GADFIT_HIP_POOL"); return !e || atoi(e) != 0; }(); return on; }
int pool_class(size_t bytes) { int c = 8; while (((size_t)1 << c) < bytes) c++; return c; }       // 256 B ... 4 MB
}  // namespace

// (every block records in `cap` what was really allocated: a request of up to 4 MB gets the size of its pool class, so that
// dev_release can file it there; `bytes` is what was asked for)
int gfh::dev_alloc(gfh_ctx* c, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return 0;
  dev_free(b);
  if (bytes == 0) bytes = 8;
  if (bytes <= kPoolBlockMax && pool_on()) {
    const int cls = pool_class(bytes);
    {
      std::lock_guard<std::mutex> lk(g_pool_mutex);
      auto it = g_pool.find(c->device);
      if (it != g_pool.end() && !it->second.blocks[cls].empty()) {
        b.p = it->second.blocks[cls].back(); it->second.blocks[cls].pop_back();
        it->second.cached -= (size_t)1 << cls;
      }
    }
    if (!b.p) HIPCHK(c, hipMalloc(&b.p, (size_t)1 << cls));
    b.bytes = bytes; b.cap = (size_t)1 << cls;
    return 0;
  }
  HIPCHK(c, hipMalloc(&b.p, bytes));
  b.bytes = bytes; b.cap = bytes;
  return 0;
}
// A NEW block of the current device by dev_alloc's size rule, never one the pool hands back: what a placement search times is the
// pages behind a fresh allocation.  Failure is a value (false, b left empty, the runtime's error cleared): every caller takes it as
// "stop searching".
bool gfh::dev_alloc_fresh(DevBuf& b, size_t bytes) {
  dev_free(b);
  if (bytes == 0) bytes = 8;
  const size_t cap = bytes <= kPoolBlockMax && pool_on() ? (size_t)1 << pool_class(bytes) : bytes;
  if (hipMalloc(&b.p, cap) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return false; }
  b.bytes = bytes; b.cap = cap;
  return true;
}
void gfh::dev_free(DevBuf& b) { if (b.p) hipFree(b.p); b.p = nullptr; b.bytes = 0; b.cap = 0; }
// gfh_destroy's form (the stream has drained): a small block goes to the pool of its device -- if it really is as long as the
// blocks of the class it would be filed in (checked here, where blocks enter the pool, not assumed from how they were made)
void gfh::dev_release(int device, DevBuf& b) {
  if (b.p && b.cap <= kPoolBlockMax && b.cap == (size_t)1 << pool_class(b.cap) && pool_on()) {
    const int cls = pool_class(b.cap);
    std::lock_guard<std::mutex> lk(g_pool_mutex);
    DevicePool& dp = g_pool[device];
    if (dp.cached + ((size_t)1 << cls) <= kPoolCap) {
      dp.blocks[cls].push_back(b.p); dp.cached += (size_t)1 << cls;
      b.p = nullptr; b.bytes = 0; b.cap = 0;
      return;
    }
  }
  dev_free(b);
}

// the blocks of a batch of independent fits (context.h, Batch; batch_data.cpp and batch_calls.cpp fill them): dropped together by the next
// gfh_set_batch_data or gfh_set_batch_cube, and what gfh_device_memory reports of them (a cube holds its grid in x, its narrow
// samples in y, w under USER alone and no offsets; while gfh_batch_frames_put fills it, the staging blocks of a piece as well)
void gfh::batch_free(gfh_ctx* c) {
  DevBuf* bufs[] = {&c->batch.x, &c->batch.y, &c->batch.w, &c->batch.off_d, &c->batch.io, &c->batch.img, &c->batch.stage_y, &c->batch.stage_w};
  for (DevBuf* b : bufs) dev_free(*b);
  c->batch.on_device = false;
}
size_t gfh::batch_bytes(const gfh_ctx* c) {
  return c->batch.x.bytes + c->batch.y.bytes + c->batch.w.bytes + c->batch.off_d.bytes + c->batch.io.bytes + c->batch.img.bytes +
         c->batch.stage_y.bytes + c->batch.stage_w.bytes;
}
// the blocks of gfh_eval (context.h, Curves), as gfh_device_memory counts them
size_t gfh::curves_bytes(const gfh_ctx* c) { return c->curves.io.bytes + c->curves.out.bytes; }

int gfh::pinned_reserve(gfh_ctx* c, size_t bytes) {
  if (c->h_pinned_bytes >= bytes) return 0;
  if (c->h_pinned) hipHostFree(c->h_pinned);
  c->h_pinned = nullptr; c->h_pinned_bytes = 0;
  // host-coherent and mapped: k_publish writes results into it from the device (result mailbox)
  HIPCHK(c, hipHostMalloc((void**)&c->h_pinned, bytes, hipHostMallocCoherent | hipHostMallocMapped));
  c->h_pinned_bytes = bytes;
  return 0;
}
// the pinned staging blocks of the parameter block and of delta1 (c->h_pars, c->h_dpars): grown when a call needs more, never shrunk
int gfh::pinned_stage(gfh_ctx* c, double*& p, size_t& have, size_t bytes) {
  if (have >= bytes) return 0;
  if (p) hipHostFree(p);
  p = nullptr; have = 0;
  HIPCHK(c, hipHostMalloc((void**)&p, bytes, hipHostMallocDefault));
  have = bytes;
  return 0;
}

// what the last context destroyed on this device left behind (BaseRes), if anything
bool gfh::base_adopt(gfh_ctx* c) {
  if (!pool_on()) return false;
  std::lock_guard<std::mutex> lk(g_pool_mutex);
  auto it = g_pool.find(c->device);
  if (it == g_pool.end() || !it->second.has_base) return false;
  BaseRes& r = it->second.base;
  c->stream = r.stream; for (int k = 0; k < 6; k++) c->ev[k] = r.ev[k];
  c->status = r.status; c->h_status = r.h_status;
  c->h_pinned = r.h_pinned; c->h_pinned_bytes = r.h_pinned_bytes;
  c->h_pars = r.h_pars; c->h_pars_bytes = r.h_pars_bytes; c->h_dpars = r.h_dpars; c->h_dpars_bytes = r.h_dpars_bytes;
  it->second.has_base = false; r = BaseRes();
  return true;
}
// the status word (+ the report area of unseen branches, kStatusBytes) and the 64 pinned bytes the result mailbox's flag lives in
bool gfh::base_alloc(gfh_ctx* c) {
  return dev_alloc_fresh(c->status, kStatusBytes) &&
         hipHostMalloc((void**)&c->h_status, 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess && c->h_status;
}
// stream, events, status word and pinned buffers: parked for the next context of this device (one set), else given back
bool gfh::base_park(gfh_ctx* c) {
  if (!(pool_on() && c->stream && c->status.p && c->h_status)) return false;
  std::lock_guard<std::mutex> lk(g_pool_mutex);
  DevicePool& dp = g_pool[c->device];
  if (dp.has_base) return false;
  BaseRes& r = dp.base;
  r.stream = c->stream; for (int k = 0; k < 6; k++) r.ev[k] = c->ev[k];
  r.status = c->status; r.h_status = c->h_status;
  r.h_pinned = c->h_pinned; r.h_pinned_bytes = c->h_pinned_bytes;
  r.h_pars = c->h_pars; r.h_pars_bytes = c->h_pars_bytes; r.h_dpars = c->h_dpars; r.h_dpars_bytes = c->h_dpars_bytes;
  dp.has_base = true;
  return true;
}
void gfh::base_free(gfh_ctx* c) {
  dev_free(c->status);
  if (c->h_pinned) hipHostFree(c->h_pinned);
  if (c->h_pars) hipHostFree(c->h_pars);
  if (c->h_dpars) hipHostFree(c->h_dpars);
  if (c->h_status) hipHostFree(c->h_status);
  c->h_pinned = c->h_pars = c->h_dpars = nullptr; c->h_status = nullptr;
  c->h_pinned_bytes = c->h_pars_bytes = c->h_dpars_bytes = 0;
}
