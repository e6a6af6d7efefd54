// context.h -- per-GPU state of the hot path (one context = one "image" of the reference).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <map>
#include <thread>
#include <string>
#include <vector>
#include "../../include/gadfit_hip.h"
#include "kernels.h"
#include "codegen.h"
#include "unseen_report.h"
#include "rtc.h"

namespace gfh {

constexpr int kPadGranule = 512;    // dataset segments are padded to this many slots (= one pass of the widest workgroup, 8 waves)

// The status buffer of a context: [0] the kernels' status word (0 ok, 1 quadrature workspace exhausted, 2 not lowered, 3 a data point
// took a branch of eval() no recorded variant covers), [16] and [24] arrival counters of k_publish / gfh_k_chi2, and from byte 64 the
// report of unseen branches: an arrival counter, then from byte 128 up to kUnseenCap entries {slot, guard outcomes so far (bit k = guard k
// taken), their number} -- layout shared with the generated source (unseen_report.h; device/unseen.hip, gfh_report_unseen).
constexpr size_t kPlacedJacobianBytes = (size_t)256 << 20;   // a Jacobian buffer from this size on is placed (placement.cpp) and its store deferred inside fits
constexpr size_t kStatusBytes = 128 + (size_t)kUnseenCap * sizeof(UnseenEntry);

struct Group;                       // group.h: single-process device group

// a device block (devmem.cpp allocates and frees them, nobody else): `bytes` as asked for, `cap` as really allocated
struct DevBuf {
  void* p = nullptr; size_t bytes = 0, cap = 0;
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

}  // namespace gfh

struct gfh_ctx {
  int device = -1;                 // -1: compile-only context (no GPU bound)
  hipStream_t stream = nullptr;
  std::string err;

  // communicator (replaces coarray images)
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  gfh::Group* grp = nullptr;        // this context is the handle of a device group (gfh_create_group): calls fan out to the members
  gfh::Group* member_of = nullptr;  // this context is member `rank` of that group: results are summed over the members on the host

  // adaptive parallelism (load_balancing of gadf_fit, gadfit.F90:672-673, 935-983): image weights of the current
  // partition, and a host copy of the whole point array (every image of the reference holds it) to cut new ranges from (data.cpp)
  struct LoadBalance {
    bool on = false;
    std::vector<double> part_w;     // empty = 1/nranks each
    std::vector<double> hx, hy, hw, haux; int h_n_aux = 0; int weights_type = -1;
    double t_prev = 0.0; long moves = 0;
  } bal;
  // data partition
  int64_t n_total = 0, begin = 0, count = 0;
  int nd = 0;
  std::vector<int64_t> dp;          // global data_positions (nd+1)
  std::vector<int64_t> lb;          // local img_bounds relative to `begin` (nd+1)
  std::vector<int64_t> ds_slot;     // first slot of each dataset (nd+1)
  int64_t n_slots = 0;
  int64_t ldj = 0;                  // column stride of J in doubles (= n_slots)
  int n_gb = 0;
  int gb_target = 0;                // number of gram workgroups the partition was built for (follows the model kind)
  std::vector<int64_t> h_gb_start; std::vector<int> h_gb_slots, h_gb_ds, h_ds_first_gb;
  gfh::DevBuf x, y, w, res, omega, is_pad, J, tile_ds, gb_start, gb_slots, gb_ds, ds_first_gb;
  // pattern-only assembly/transfer of global fits: upper-triangle entries (row <= col) some dataset touches
  bool sparse_ok = true, sparse = false; int nnz = 0;   // GADFIT_HIP_SPARSE
  gfh::DevBuf nz_row, nz_col; std::vector<int> h_nz_row, h_nz_col;
  gfh::DevBuf gs_meta, gs_list; int gs_n = 0; bool gs_sparse = false;   // source lists of the packed (pattern) image for k_gather_sum
  bool jtj_prezeroed = false;       // gfh_fit: the caller's JTJ buffer holds zeros off the pattern already
  gfh::DevBuf owner;                // [dim] the one dataset using a column, or -1 (k_assemble)
  gfh::DevBuf aux; int n_aux = 0;   // auxiliary per-point columns [n_aux][n_slots] (gfh_set_aux)
  // Mesh hand-over of quadrature models (emit_quadrature.cpp, mesh_build): per slot and outermost integrate() call site the record of the
  // bisections the last recording pass made, and the parameter block it made them at.  A pass at exactly those parameters replays
  // them instead of bisecting again: the sweep of an accepted step after the trial chi2() there, STEP 3 after the sweep.  (launch.cpp)
  struct Dispatch {
    gfh::DevBuf tile_cost, tile_order, gb_order;   // models with integrate(): measured cost per tile, tiles / gram blocks expensive first (build_orders)
    bool order_on = true, order_ready = false, order_want = false, order_measured = false; int order_age = 0;
    gfh::DevBuf mesh; int mesh_stride = 0;
    std::vector<double> mesh_pars; bool mesh_valid = false, mesh_on = true;   // GADFIT_HIP_MESH (0: every pass bisects)
    long n_mesh_replays = 0;
  } disp;
  int n_integrand_rounds = 0;          // passes repeated in a row because an integrand met an unrecorded path (recover_integrand_path)
  gfh::DevBuf partial, G, chi2_partial, packed, pars, dpars, inv, dl, vec, status;
  int* h_status = nullptr;          // pinned, host-coherent 64 B: the result mailbox's flag lives at byte 8
  unsigned long long* h_flag = nullptr;   // sequence number of the last published result (k_publish)
  unsigned long long mail_seq = 0;
  int tile = 0, n_tiles = 0;        // tile of the loaded kernels (tile_ds is built for it)
  double* h_pinned = nullptr; size_t h_pinned_bytes = 0;   // results (D2H)
  double* h_pars = nullptr; size_t h_pars_bytes = 0;       // parameter block (H2D)
  double* h_dpars = nullptr; size_t h_dpars_bytes = 0;     // delta1 per dataset for STEP 3 (H2D / kernel argument)

  // model + kernels
  gfh::Model model; bool has_model = false;
  long model_serial = 0, aux_serial = 0;   // bumped by gfh_set_model* / gfh_set_aux*: did an unseen-branch handler change anything?
  gfh_unseen_handler unseen_fn = nullptr; void* unseen_user = nullptr;
  gfh_pars_hook pars_fn = nullptr; void* pars_user = nullptr;      // gfh_set_pars_hook: passive entries refreshed before every pass
  bool in_pars_hook = false;                                         // ... the hook is running (on this context's own thread)
  // Quadrature workspaces beyond the scratch budget (GenConfig::ws_global): the context's pool in global memory, one slot of
  // wsg_wave_doubles per wave of a launch; the launchers cap their grids at the slots there are.  Allocated at the first launch that
  // needs it (hipMalloc: a failure is an error code, not the runtime's abort), freed by gfh_destroy / when the model changes its sizes.
  // (cut by launch.cpp, wsg_grid; sized by active.cpp, apply_ws_plan)
  struct WsPool {
    gfh::DevBuf wsg; int64_t waves = 0, wave_doubles = 0;
    int64_t tried = 0;              // the largest number of slots the pool was last ASKED for (the card may have granted fewer: waves): not asked again until more are wanted
    bool grown = false;             // a pass has exhausted the fast workspaces: the kernels carry the user's sizes (kept through a recovery's new model)
    int fast = 100;                 // quadrature workspace the kernels carry first (GADFIT_HIP_WS_FAST; 0: the user's size from the start)
  } ws;
  bool in_recovery = false;         // the unseen-branch handler is running (gfh_set_model_variants then keeps ws.grown)
  // what is in flight beside the caller: the device part of a creation, an upload, a host-side copy (context.cpp, data.cpp)
  struct Upload {
    std::thread pending;            // gfh_set_data_begin: the upload in flight (joined by the next call on this context)
    std::vector<int32_t> pending_hint_cols;   // gfh_set_variant_hint_columns: consumed by the next gfh_set_model_variants
    bool creating = false;    // `pending` is the device part of gfh_create_begin (not an upload): gfh_set_data_begin chains its upload behind it
    bool create_failed = false; std::string create_err;      // ... and it failed: every call that needs the device fails with its message
    int pending_rc = 0;
    void* hc_dst = nullptr; const void* hc_src = nullptr; size_t hc_bytes = 0;   // gfh_queue_host_copy: a host-side copy made beside the next upload
    std::thread host_copy;             // ... on a thread of its own (gfh_wait_host_copy joins it)
  } up;
  long n_unseen_rounds = 0;         // passes repeated because a point left the recorded decision tree (since the model was set)
  gfh::GenConfig gen;
  std::map<std::vector<int32_t>, gfh::ModelKernels> kernel_cache;
  gfh::ModelKernels* cur = nullptr;
  std::vector<int32_t> cur_active, cur_jac;
  int cur_dim = 0, cur_T = 0;
  const gfh::ModelKernels* prepared_cur = nullptr;
  bool prepared = false, prepared_store_j = true;   // prepare_active's work is valid for (cur, cur_active, cur_jac, cur_dim)
  bool have_sweep = false;          // a sweep ran with the current active set (res valid on device)
  bool j_valid = false;             // the Jacobian of that sweep is in HBM
  bool res_valid = false;           // the residual vector of the last pass is in HBM
  int keep_jacobian = 1;            // 0 never, 1 always (reference behaviour), 2 gfh_fit decides (GADFIT_HIP_KEEP_J)
  // Deferred Jacobian store (gfh_fit, lm.cpp; materialise_jacobian, passes.cpp).  Inside a fit nobody reads the stored J: the fused
  // kernel forms its sums from registers and every sweep overwrites what the one before it wrote.  Under keep_jacobian mode 1 the
  // sweeps of such a fit run the no-store kernel, except those no later sweep of the fit can follow (max_iter).  A fit that ends any
  // other way leaves J OWED: the parameter block of its most recent sweep is kept -- and that of a chi2 pass that wrote res after
  // it -- and the first call that reads J launches the storing kernel there (and the chi2 kernel again), on this rank alone.
  struct Deferred {
    bool on = true;                 // GADFIT_HIP_DEFER_J
    size_t from = gfh::kPlacedJacobianBytes;   // smallest Jacobian (bytes) whose store is deferred (GADFIT_HIP_DEFER_J_FROM)
    int fit = 0;                    // 0: no gfh_fit is running, 1: one that stores at every sweep, 2: one that defers
    bool store_next = true;         // fit == 2: no later sweep of the fit can follow the one about to be requested
    bool owed = false;              // the most recent sweep (have_sweep) skipped the store: J at `pars` is owed
    bool chi2_after = false;        // ... and a chi2 pass at `chi2_pars` has written res since
    std::vector<double> pars, chi2_pars;
    long long n_deferred = 0, n_stored = 0, n_materialised = 0;   // sweeps inside fits without / with the store; materialising launches
  } defer;
  int lookahead = 1;                // gfh_fit / gfh_lm_iterate: first trial chi2 from a sweep at the trial point (GADFIT_HIP_LOOKAHEAD)
  bool kernarg = true;              // one dataset: parameters as a by-value kernel argument instead of an H2D copy per pass (GADFIT_HIP_KERNARG)
  bool merge_small = true;          // J^T v: reduce + assemble + publish as one single-workgroup launch when small (GADFIT_HIP_MERGE_SMALL)
  bool tail = true;                 // fused kernel reduces/assembles/publishes in its own tail for small dim^2*n_datasets (GADFIT_HIP_TAIL)
  gfh::DevBuf slice, counters, tail_dev; std::vector<char> tail_host;
  bool fused = true;                // STEP 1+2 in one kernel (GADFIT_HIP_FUSED=0: separate sweep and Gram kernels)
  // how the most recent sweep was dispatched (sweep_pass notes it, gfh_debug_layout reports it): the fused kernel or the plain sweep,
  // its waves per workgroup, the tail mode it was handed (0: the launch chain), the pattern-only image
  struct LastSweep { int fused = 0, waves = 0, tail_mode = 0, sparse = 0; } last_sweep;
  // which kernels the most recent sweep and the most recent J^T v product launched behind the model kernel, each noted at its launch
  // (gfh_debug_chain reports them; nothing reads them to decide anything): the Gram launches of launch_gram (none: the fused kernel),
  // the assembling step (0 none yet, 1 the fused kernel's tail, 2 k_gather_sum, 3 k_assemble_sparse, 4 k_assemble) and the J^T v
  // finish (0 none yet, 1 k_jtv_finish, 2 k_reduce_partials + k_assemble_vec + the fetch)
  struct Chain { std::vector<gfh::GramLaunch> gram; int assemble = 0, jtv_finish = 0; } chain;

  // timers (seconds) + counters (inspect.cpp; the passes count and bracket their launches)
  struct Timers {
    double t_sweep = 0, t_gram = 0, t_reduce = 0, t_allreduce = 0, t_chi2 = 0, t_omega = 0;
    long n_sweep = 0, n_chi2 = 0, n_allreduce = 0;
    double t_sweep_min = 0, t_sweep_max = 0, t_sweep_last = 0; long n_sweep_timed = 0, n_chi2_timed = 0, n_omega = 0, n_omega_timed = 0, n_chain_timed = 0;
    // 0: no events; 1: events around every 8th launch of each model kernel (an event record costs ~4 us of stream time: two per
    // launch were 8 us of a 35 us small-fit iteration), the sums scaled to all launches; 2: every launch, also reduce/all-reduce
    int detail = 1;
    int ev_pending = 0;             // timer level of a sweep whose events have not been read yet
  } timers;
  // the placement search (placement.cpp)
  struct Placement {
    int tries = 16;                 // candidate allocations of a large Jacobian buffer that are timed (gfh_set_placement_tries; 1: take the first)
    double ms[8] = {0};             // the candidates' store-stream times of the last placement, [0] = the one kept
    int n = 0;
    int data_n = 0; double data_ms = 0.0;   // round 6: re-placements of {x, y, w, res} tried behind the Jacobian's, the kernel's time on the set kept
    int after = 48;                 // sweeps that must have written the buffer before candidates are timed (gfh_set_placement_after)
    int64_t sweeps_on_J = 0;        // ... counted since the buffer was (re)allocated
    double copy_rate = 0;           // B/s of a device-to-device copy inside the first candidate (the measure the placement's thresholds scale with)
    bool pending = false;           // the Jacobian buffer was (re)allocated and is large: the next sweep that writes it times candidates first
  } place;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // batched independent fits: the geometry and form of the batch held (batch_data.cpp records them on the host: the argument checks
  // of the calls read them before the device is asked for), its data on the device, and two blocks that the five launching calls
  // share, each call sizing them for itself -- io what goes down (under gfh_fit_batch also what comes back), img what the other
  // calls bring back; their layouts by call are at the head of batch_calls.cpp
  struct Batch {
    int64_t n_fits = 0;
    std::vector<int64_t> off;       // [n_fits + 1]
    int64_t min_points = 0;         // of the shortest spectrum
    int64_t max_points = 0;         // of the longest: with the active count, all the auto rule of gfh_set_batch_lanes reads
    int lanes = 64;                 // gfh_set_batch_lanes: 64 a wave per fit, 16 a DPP row per fit, 256 a workgroup per fit, 0 auto (gfh_batch_auto_lanes: 16 or 64)
    int last_lanes = 0;             // the form of the last batch launch (gfh_debug_batch_lanes); 0: none yet
    int loss = 0;                   // gfh_set_batch_loss: 0 linear, 1 cauchy, 2 huber -- the batch's own, part of its unit's text; the plain fit's gfh_set_loss is refused in a batch
    double loss_scale = 1.0;        // ... and the residual scale c of it (the loss switches at |r| = c); the kernels take 1 / c as an argument
    int last_loss = -1;             // the loss and scale of the last batch launch that carries one (gfh_debug_batch_loss); -1: none yet
    double last_loss_scale = 0.0;
    int estimator = 0;              // gfh_set_batch_estimator: 0 least squares, 1 the Poisson deviance by Fisher scoring -- part of the unit's text, as the loss
    int last_estimator = -1;        // ... of the last batch launch that sweeps (gfh_debug_batch_estimator); -1: none yet
    // gfh_set_batch_cube: every spectrum on one grid.  x holds the grid [n_points], y the samples [n_fits][n_points] in y_type
    // (0 double, 1 float, 2 uint16_t), w the weights under error_type 4 (USER) alone, off stays empty (min_points = max_points = n_points)
    bool cube = false;
    int y_type = 0, error_type = 0;
    int last_form = -1;             // the data form of the last batch launch (gfh_debug_batch_form); -1: none yet
    double pass_ms = 0.0;           // device time of the last gfh_batch_pass's kernel (gfh_debug_batch_pass_seconds): a yardstick for its neighbours
    bool on_device = false;
    gfh::DevBuf x, y, w, off_d, io, img;
    // gfh_batch_frames_begin: the cube above, filled frame by frame.  One flag per frame (1: put), the count of those still 0, the
    // staging blocks of the piece in flight (stage_y, and stage_w under USER: freed when no frame is missing) and the device time of
    // the transposing kernels since begin.  frames goes back to false with the next gfh_set_batch_data / gfh_set_batch_cube.
    bool frames = false;
    std::vector<unsigned char> frame_put;
    int64_t frames_missing = 0;
    double frames_kernel_ms = 0.0;
    gfh::DevBuf stage_y, stage_w;
    std::vector<char> host;         // where the one device-to-host copy of a call lands
  } batch;
  // the curves of a plain fit (gfh_eval, eval.cpp): io what goes down with the parameters -- the datasets' blocks of the covariance
  // [n_datasets][n_act * n_act], then the caller's grid --, out the requested outputs back to back -- padded [n_slots] each on the
  // data's own points, [n_datasets][n_eval] each on a grid.  Sized by the call at hand, kept for the next, counted by gfh_device_memory.
  struct Curves { gfh::DevBuf io, out; int launches = 1; } curves;      // (launches: gfh_debug_eval_launches)
};

namespace gfh {
int fail(gfh_ctx* c, const std::string& msg);
void set_global_error(const std::string& msg);
void set_store_j(gfh_ctx* c, bool on);
void set_store_res(gfh_ctx* c, bool on);
bool uses_fused_kernel(const gfh_ctx* c);
bool sweep_chi2_is_bitwise(const gfh_ctx* c);
bool omega_needs_jacobian(const gfh_ctx* c, int n_active);
int materialise_jacobian(gfh_ctx* c);   // passes.cpp: every reader of the stored Jacobian calls it before it looks at j_valid
int join_pending(gfh_ctx* c);     // waits for an upload started by gfh_set_data_begin; its result
// Named ranges for `rocprofv3 --marker-trace` (ROCTX): every pass, a fit and its iterations, an upload, the recovery from an unseen
// branch.  Off unless GADFIT_HIP_ROCTX=1 (the library is looked up at run time: no link dependency, no cost when off).
struct Range {
  explicit Range(const char* name);
  ~Range();
  Range(const Range&) = delete; Range& operator=(const Range&) = delete;
 private:
  bool on_;
};
}  // namespace gfh
