// context_internal.h -- what the translation units behind the C ABI share besides the context itself (context.h): the error macros,
// the internal return codes of a pass, and the functions that cross a file boundary, grouped by the file that defines them.  A
// function that is not declared here is static in its file.  Default arguments live on these declarations only.
#pragma once
#include "context.h"
#include <mutex>

#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
  return fail(c, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
// (a pass may end with kUnseen instead of 0 / 1: passed up unchanged to the loop that recovers and repeats it)
#define PASS(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)
#define NCCLCHK(c, call) do { ncclResult_t r_ = (call); if (r_ != ncclSuccess) \
  return fail(c, std::string(#call) + ": " + ncclGetErrorString(r_)); } while (0)
#define NEED_GPU(c) do { if (!(c)) return 1; if ((c)->device < 0) \
  return fail(c, "no GPU bound to this context (libgadfit_hip has no CPU fallback)"); \
  if (gfh::join_pending(c)) return 1; \
  if ((c)->up.create_failed) return fail(c, (c)->up.create_err); \
  hipError_t e_ = hipSetDevice((c)->device); if (e_ != hipSuccess) return fail(c, "hipSetDevice failed"); } while (0)
// a device-group handle: the same call on every member, each on its own thread (k = member, r = its rank)
#define GROUP(c, expr) do { if ((c) && (c)->grp) return gfh::group_run((c), [&](gfh_ctx* k, int r) -> int { (void)k; (void)r; return (expr); }); } while (0)
#define NOT_FOR_GROUP(c, what) do { if ((c) && (c)->grp) return fail(c, what " is not available on a device-group handle"); } while (0)

namespace gfh {

constexpr int kUnseen = 77;      // internal return code: a point left the recorded decision tree (status 3); the caller recovers and repeats the pass
constexpr int kGrowWs = 78;      // internal return code: the compiled-in quadrature workspace was exhausted but the user's is larger
constexpr int kIntegrandPath = 79;   // internal return code: an integrand met a path through its comparisons that no recording has (status 2)

// devmem.cpp
int dev_alloc(gfh_ctx* c, DevBuf& b, size_t bytes);
bool dev_alloc_fresh(DevBuf& b, size_t bytes);
void dev_free(DevBuf& b);
void dev_release(int device, DevBuf& b);
void batch_free(gfh_ctx* c);
size_t batch_bytes(const gfh_ctx* c);
size_t curves_bytes(const gfh_ctx* c);
int pinned_reserve(gfh_ctx* c, size_t bytes);
int pinned_stage(gfh_ctx* c, double*& p, size_t& have, size_t bytes);
bool base_adopt(gfh_ctx* c);
bool base_alloc(gfh_ctx* c);
bool base_park(gfh_ctx* c);
void base_free(gfh_ctx* c);

// context.cpp
void copy_path_ready();

// comm.cpp
int await_result(gfh_ctx* c, unsigned long long seq, size_t n, bool summed = false);
int fetch_result(gfh_ctx* c, const double* src, size_t n, bool summed = false);
int allreduce_sum(gfh_ctx* c, double* buf, size_t n, bool slot_written = false);

// data.cpp
int ensure_gb_partition(gfh_ctx* c);
int ensure_tile_table(gfh_ctx* c);
int set_geometry(gfh_ctx* c, int64_t n_total, int nd, const int64_t* dp);

// active.cpp
constexpr int kMaxKernargPars = 480;   // doubles of a parameter block passed by value; the kernel-argument segment holds 4 KiB
void apply_ws_plan(gfh_ctx* c);
int get_kernels(gfh_ctx* c, const std::vector<int32_t>& active, bool load);
ModelKernels* nostore_kernels(gfh_ctx* c);
int check_aux(gfh_ctx* c);
int ensure_mesh(gfh_ctx* c);
int prepare_active(gfh_ctx* c, const int32_t* active, int na, const int32_t* jac, int dim);

// launch.cpp
int upload_pars(gfh_ctx* c, const double* pars);
bool use_fused(const gfh_ctx* c);
int mesh_mode_for(gfh_ctx* c, const double* pars, bool recording_pass);
int launch_model_sweep(gfh_ctx* c, int mesh_mode = 0);
int build_orders(gfh_ctx* c);
int launch_model_sweep_gram(gfh_ctx* c, int tail_mode = 0, unsigned long long seq = 0, unsigned lds_pad = 0, const ModelKernels* mk = nullptr);
bool tail_one_workgroup_per_cu(const gfh_ctx* c);
unsigned tail_lds_pad(const gfh_ctx* c);
int update_tail(gfh_ctx* c);
int launch_model_chi2(gfh_ctx* c, int tail_mode, unsigned long long seq, int mesh_mode = 0);
int launch_model_omega(gfh_ctx* c, int mesh_mode = 0);
int launch_gram_chain(gfh_ctx* c, bool time_it, bool with_gram = true, bool sparse = false, unsigned long long publish_seq = 0);
int launch_model_omega_jt(gfh_ctx* c);

// placement.cpp
int place_jacobian(gfh_ctx* c, int na);
int place_jacobian_now(gfh_ctx* c, bool fused);

// passes.cpp
extern std::recursive_mutex g_handler_mutex;
int status_check(gfh_ctx* c, int st);
int repeat_pass(gfh_ctx* c, int rc, const double* pars);      // after kUnseen / kGrowWs / kIntegrandPath: 0 repeat the pass, 1 failed

// batch_data.cpp, batch_calls.cpp: what the two share is in batch_internal.h; nothing of theirs is used outside them

// inspect.cpp
double ev_ms(hipEvent_t a, hipEvent_t b);
bool timed_launch(const gfh_ctx* c, long n_so_far);
double scaled_time(double t_timed, long n_all, long n_timed);
void harvest_events(gfh_ctx* c);
int unpad(gfh_ctx* c, const double* dev, double* out);        // a padded device array [n_slots] into this rank's `count` points, in the caller's order

}  // namespace gfh
