// launch.cpp -- one function per kernel launch and what sizes its grid: the parameter block of a pass (upload_pars), the generated
// kernels' argument lists, the pool of global quadrature workspaces that caps their grids (wsg_grid), the fused kernel's tail
// descriptor and the order of dispatch of quadrature models.  It decides nothing about a pass (passes.cpp) and waits for no result.
#include "context_internal.h"
#include <algorithm>
#include <cstring>
#include <mutex>

using namespace gfh;

int gfh::upload_pars(gfh_ctx* c, const double* pars) {
  const size_t n = (size_t)c->nd * c->model.n_pars;
  if (pinned_reserve(c, 4096)) return 1;
  if (pinned_stage(c, c->h_pars, c->h_pars_bytes, sizeof(double) * n)) return 1;
  if (dev_alloc(c, c->pars, sizeof(double) * n)) return 1;
  // every public call ends with a stream synchronise, so the staging buffer is free here
  memcpy(c->h_pars, pars, sizeof(double) * n);
  if (c->pars_fn) {            // (gfh_set_pars_hook: the host's reals that follow the parameters, refreshed in the staging copy)
    int rc;
    // (in_pars_hook: columns the hook uploads belong to the parameters of THIS pass -- a real that follows the parameters and the
    // abscissa, tabulated anew; what the device holds of the last sweep -- active set, Jacobian, residuals -- stays what it was)
    { std::lock_guard<std::recursive_mutex> lk(g_handler_mutex); c->in_pars_hook = true; rc = c->pars_fn(c->pars_user, c, c->h_pars); c->in_pars_hook = false; }
    if (rc) return fail(c, "the parameter hook failed (gfh_set_pars_hook)" + (c->err.empty() ? std::string() : ": " + c->err));
  }
  // kernels that take the block by value read it from c->h_pars at launch (the runtime copies kernel
  // arguments during the launch call); nothing is queued on the stream
  if (c->cur && c->cur->kernarg_pars) return 0;
  HIPCHK(c, hipMemcpyAsync(c->pars.p, c->h_pars, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  return 0;
}

// STEP 1 + STEP 2 in one kernel?  Up to 64 active parameters (4 tiles of 16); beyond that the plain sweep
// writes J and k_gram_block forms the Gram image from it.
// Models with integrate() also take the two-kernel path: the adaptive quadrature makes the per-point work
// long and uneven, and the fused kernel's one 8-wave workgroup per CU with its LDS stage loses to the plain
// sweep's small workgroups (cfg 4: 2.39 ms fused against 1.77 + 0.02 ms).
static bool fusable_model(const gfh_ctx* c) { return !(c->has_model && c->model.has_integrals()); }
bool gfh::use_fused(const gfh_ctx* c) {
  return c->fused && fusable_model(c) && (int)c->cur_active.size() <= kFusedMaxActive && c->cur && c->cur->sweep_gram;
}

namespace gfh {
bool uses_fused_kernel(const gfh_ctx* c) { return use_fused(c); }
// Is the sum r^2 a sweep returns bitwise what chi2() returns at the same parameters (what the look-ahead schedule needs)?  The fused
// kernel: by construction (same partition and order of additions as gfh_k_chi2).  The two-kernel path with up to 8 active parameters
// (quadrature models; GADFIT_HIP_FUSED=0): k_gram_small sums r^2 per lane over the lane's points in ascending order, wave tree, waves
// in order -- gfh_k_chi2's map and order at its 8 waves per workgroup -- and k_reduce_partials / k_gather_sum are the order gfh_k_chi2's
// tail restates; the residuals themselves agree bit for bit (same value expressions; the quadrature's final pass rounds its panel
// sums like the value-only pass).  Pinned by test_chi2_is_bitwise_the_sweeps_sum_of_squares*.
// (k_gram_block adds r^2 in gfh_k_chi2's order as well, at the waves that kernel runs with for the active count: 8 beyond 128 active
// parameters -- tests/test_gpu_gram_layouts.py holds it --, 4 at 65 ... 128 on the two-kernel path -- tests/test_gpu_gram_chain.py --;
// the look-ahead schedule is not extended to them here.)
bool sweep_chi2_is_bitwise(const gfh_ctx* c) {
  if (use_fused(c)) return true;
  return c->cur && c->cur_active.size() <= 8 && fused_waves_for((int)c->cur_active.size()) == 8 && !c->gen.finite_diff;
}
}  // namespace gfh

// The mode a pass at `pars` runs its quadrature in (generated kernels, mesh_build): 2 = replay the recorded bisections (they were made
// at exactly these parameters), 1 = bisect and record (recording pass: from now on the record belongs to these parameters), 0 = bisect.
int gfh::mesh_mode_for(gfh_ctx* c, const double* pars, bool recording_pass) {
  if (!c->disp.mesh.p || !c->disp.mesh_stride || !pars) return 0;
  const size_t n = (size_t)c->nd * c->model.n_pars;
  if (c->disp.mesh_valid && c->disp.mesh_pars.size() == n && !memcmp(c->disp.mesh_pars.data(), pars, sizeof(double) * n)) { c->disp.n_mesh_replays++; return 2; }
  if (!recording_pass) return 0;
  c->disp.mesh_pars.assign(pars, pars + n); c->disp.mesh_valid = true;
  return 1;
}

// Workgroups of `threads` threads that are resident on the chip at once for this kernel: the occupancy the runtime reports,
// capped at 6 per CU for 256 threads -- with more than 96 SGPRs (a by-value parameter block) the hardware admits
// fewer than the API says (MI355X_MICROARCH.md, residency).  Kernels whose workgroups each own a fixed share of the
// points are launched with at most this many, so no workgroup waits for a second round behind the first.
static int resident_grid(gfh_ctx* c, hipFunction_t f, int threads) {
  int per_cu = 0, cus = 0;
  if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, threads, 0) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 1; }
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus < 1) { (void)hipGetLastError(); cus = 256; }
  const int cap = std::max(1, 6 * 256 / threads);
  return cus * std::min(per_cu, cap);
}

// Kernels whose quadrature workspaces are the global pool (GenConfig::ws_global): the pool holds one slot per wave of a launch, so the
// grid is capped at the slots there are -- as many workgroups as are resident at once where the memory allows (more would only wait
// for a second round) -- and the kernels stride over their tiles / gram blocks.  The pool is an ordinary allocation of the context:
// cut at the first launch that needs it, halved until the card can provide it (never more than half of what is free), an error code
// if not even one workgroup's slots fit, freed by gfh_destroy.  *grid: the workgroups to launch for `blocks` units of work.
static int wsg_grid(gfh_ctx* c, hipFunction_t f, int threads, int64_t blocks, int* grid) {
  *grid = (int)blocks;
  if (!c->gen.ws_global || !c->ws.wave_doubles) return 0;
  const int wpb = threads / 64;
  const int64_t want = std::min<int64_t>(blocks, resident_grid(c, f, threads)) * wpb;
  // (a pool the card cut short stays as it is until a launch wants MORE slots than the cut was made for -- kernels of different
  // workgroup sizes then alternate on the same pool instead of each freeing and cutting it again at every pass)
  // (... and once more, whatever was asked before, when the pool at hand cannot serve even ONE workgroup of this kernel: memory may
  // have come free since the card cut it short -- the Jacobian dropped, another context destroyed: round-5 advisor)
  for (int attempt = 0; attempt < 2 && (attempt == 0 || c->ws.waves < wpb); attempt++)
  if (c->ws.waves < want && (want > c->ws.tried || attempt == 1)) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    dev_free(c->ws.wsg); c->ws.waves = 0; c->ws.tried = want;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)1 << 40; }
    int64_t n = want;
    for (;;) {
      const size_t bytes = (size_t)n * (size_t)c->ws.wave_doubles * sizeof(double);
      if (bytes <= free_b / 2) {
        if (dev_alloc_fresh(c->ws.wsg, bytes)) break;
      }
      if (n <= wpb) return fail(c, "the device cannot provide the quadrature workspaces of one workgroup (" + std::to_string(bytes >> 20) +
                                   " MB at ws_size " + std::to_string(c->gen.ws_size) + " / " + std::to_string(c->gen.ws_size_inner) + "): lower ws_size");
      n = std::max<int64_t>(wpb, (n / 2 + wpb - 1) / wpb * wpb);
    }
    c->ws.waves = n;
  }
  if (c->ws.waves < wpb) return fail(c, "the pool of quadrature workspaces holds fewer slots than one workgroup of this kernel needs: lower ws_size");
  *grid = (int)std::min<int64_t>(blocks, c->ws.waves / wpb);
  return 0;
}
// (the generated kernels take the mesh / order arguments and the pool's address only where the model has them: codegen.cpp,
// GFH_MESH_KPARAMS, GFH_ORDER_KPARAMS, GFH_WSG_KPARAMS)
static bool takes_mesh_args(const gfh_ctx* c) { return unit_takes_mesh_args(c->model, c->gen); }

int gfh::launch_model_sweep(gfh_ctx* c, int mesh_mode) {
  if (!c->n_tiles) return 0;
  void* x = c->x.p; void* y = c->y.p; void* w = c->w.p; void* pars = c->pars.p; void* parg = c->cur->kernarg_pars ? (void*)c->h_pars : (void*)&pars; void* tds = c->tile_ds.p;
  void* res = c->res.p; void* J = c->J.p; long long ldj = c->ldj; int nt = c->n_tiles; void* stp = c->status.p;
  void* ax = c->aux.p; long long lda = c->n_slots; void* mesh = c->disp.mesh.p;
  // (mesh ... cost: kernels of models with integrate() only.  The sweep that bisects measures the cost of its tiles when an order
  // of dispatch is wanted: build_orders)
  const bool ordered = c->disp.order_on && takes_mesh_args(c);      // (kernels that take the arguments: codegen.cpp, GFH_ORDER_KPARAMS)
  void* ord = ordered && c->disp.order_ready ? c->disp.tile_order.p : nullptr;
  void* cst = nullptr;
  if (ordered && c->disp.order_ready && ++c->disp.order_age >= 64) c->disp.order_want = true;      // (the profile moves with the parameters: measured again now and then)
  if (ordered && c->disp.order_want) {       // (a sweep that replays meshes ranks its tiles like one that bisects: by the number of intervals)
    if (c->disp.tile_cost.bytes < sizeof(int) * (size_t)c->n_tiles && dev_alloc(c, c->disp.tile_cost, sizeof(int) * (size_t)c->n_tiles)) return 1;
    cst = c->disp.tile_cost.p; c->disp.order_measured = true;
  }
  int grid; if (wsg_grid(c, c->cur->sweep, c->gen.block, c->n_tiles, &grid)) return 1;
  void* pool = c->ws.wsg.p;
  std::vector<void*> args{&x, &y, &w, parg, &tds, &nt, &res, &J, &ldj, &stp, &ax, &lda};
  if (takes_mesh_args(c)) { args.push_back(&mesh); args.push_back(&mesh_mode); args.push_back(&ord); args.push_back(&cst); }
  if (c->gen.ws_global) args.push_back(&pool);
  HIPCHK(c, hipModuleLaunchKernel(c->cur->sweep, grid, 1, 1, c->gen.block, 1, 1, 0, c->stream, args.data(), nullptr));
  return 0;
}

// Tiles and gram blocks in the order of their measured cost, expensive first (codegen.cpp, GFH_ORD): called once the sweep that
// measured has completed.  16 KB down, two sorts of a few thousand keys, 24 KB up: a few tenths of a millisecond, once per data set /
// model and again after every 64 sweeps (the profile moves with the parameters).
int gfh::build_orders(gfh_ctx* c) {
  gfh::Range range("gadfit order of dispatch");
  c->disp.order_measured = false; c->disp.order_want = false; c->disp.order_age = 0;
  const size_t nt = (size_t)c->n_tiles, ngb = (size_t)c->n_gb;
  if (!nt || !ngb) return 0;
  std::vector<int> cost(nt);
  HIPCHK(c, hipMemcpyAsync(cost.data(), c->disp.tile_cost.p, sizeof(int) * nt, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<int> to(nt), go(ngb);
  for (size_t t = 0; t < nt; t++) to[t] = (int)t;
  std::stable_sort(to.begin(), to.end(), [&](int a, int b) { return cost[(size_t)a] > cost[(size_t)b]; });
  std::vector<long long> gc(ngb, 0);
  const int64_t tile = c->gen.block;
  for (size_t b = 0; b < ngb; b++) {
    const int64_t t0 = c->h_gb_start[b] / tile, t1 = (c->h_gb_start[b] + c->h_gb_slots[b] + tile - 1) / tile;
    for (int64_t t = t0; t < t1 && t < (int64_t)nt; t++) gc[b] += cost[(size_t)t];
    go[b] = (int)b;
  }
  std::stable_sort(go.begin(), go.end(), [&](int a, int b) { return gc[(size_t)a] > gc[(size_t)b]; });
  if (dev_alloc(c, c->disp.tile_order, sizeof(int) * nt) || dev_alloc(c, c->disp.gb_order, sizeof(int) * ngb)) return 1;
  HIPCHK(c, hipMemcpyAsync(c->disp.tile_order.p, to.data(), sizeof(int) * nt, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->disp.gb_order.p, go.data(), sizeof(int) * ngb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));          // (the vectors go out of scope)
  c->disp.order_ready = true;
  return 0;
}

// tail_mode 0: workgroup partials only; 1: + in-kernel reduction and assembly into c->packed;
// 2: + the result mailbox (sequence number seq).  Modes 1/2 need update_tail().  mk: the kernels of the same active set
// without the Jacobian store (nostore_kernels) instead of c->cur -- same arguments, same grid.
int gfh::launch_model_sweep_gram(gfh_ctx* c, int tail_mode, unsigned long long seq, unsigned lds_pad, const ModelKernels* mk) {
  if (!c->n_gb) return 0;
  if (!mk) mk = c->cur;
  void* x = c->x.p; void* y = c->y.p; void* w = c->w.p; void* pars = c->pars.p; void* parg = c->cur->kernarg_pars ? (void*)c->h_pars : (void*)&pars;
  void* gs = c->gb_start.p; void* gn = c->gb_slots.p; void* gd = c->gb_ds.p;
  void* res = c->res.p; void* J = c->J.p; long long ldj = c->ldj; void* part = c->partial.p;
  int ps = gram_partial_stride(c->cur_T); void* stp = c->status.p; void* tl = c->tail_dev.p;
  void* ax = c->aux.p; long long lda = c->n_slots;
  void* args[] = {&x, &y, &w, parg, &gs, &gn, &gd, &res, &J, &ldj, &part, &ps, &stp, &ax, &lda, &tl, &seq, &tail_mode};
  const int fw = fused_waves_for((int)c->cur_active.size());
  HIPCHK(c, hipModuleLaunchKernel(mk->sweep_gram, c->n_gb, 1, 1, 64 * fw, 1, 1, lds_pad, c->stream, args, nullptr));
  return 0;
}

// The tail's fence-free hand-off is the form measured with ONE workgroup per CU (MI355X_MICROARCH.md, inter-workgroup
// visibility, table).  Up to 16 active parameters two workgroups of the fused kernel fit a CU's LDS (and the kernel wants
// them: padding it down to one costs 15 % at cfg 2); those models keep the three-launch chain.
static long fused_lds_bytes(const gfh_ctx* c) {
  const int na = (int)c->cur_active.size(), fw = fused_waves_for(na);
  if (na <= kValuGramMax) return (fw + 1) * (na * (na + 1) / 2 + na + 1) * 8 + 273 * 8 + 64;      // the VALU path: the cross-wave reduction and the image
  return fused_lds_bytes_for(na, fw);
}
bool gfh::tail_one_workgroup_per_cu(const gfh_ctx* c) { return fused_lds_bytes(c) > 80 * 1024; }
// Grids of at most 256 workgroups (one per CU at most) may take the tail with <= 16 parameters too: a dynamic LDS pad makes
// a second workgroup on a CU impossible, and with so few workgroups the occupancy it costs is not there to lose.
unsigned gfh::tail_lds_pad(const gfh_ctx* c) {
  return (!tail_one_workgroup_per_cu(c) && c->n_gb > 1 && c->n_gb <= 256) ? (unsigned)(81 * 1024 - fused_lds_bytes(c)) : 0u;
}

// Device-side descriptor of the fused kernel's tail (layout = struct gfh_tail of the generated source).
struct TailDesc {
  const int* ds_first_gb; const int* inv; double* slice; double* G; double* packed; double* host_out;
  unsigned long long* host_flag; unsigned* counters; int nd, dim, n_slices, pad;
};

int gfh::update_tail(gfh_ctx* c) {
  const int ps = gram_partial_stride(c->cur_T);
  if (dev_alloc(c, c->slice, sizeof(double) * (size_t)c->nd * 32 * ps)) return 1;
  const size_t cb = sizeof(unsigned) * (size_t)(1 + c->nd * 32);
  if (c->counters.bytes < cb) {
    if (dev_alloc(c, c->counters, cb)) return 1;
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, c->counters.bytes, c->stream));
  }
  if (dev_alloc(c, c->tail_dev, sizeof(TailDesc))) return 1;
  TailDesc t;
  memset(&t, 0, sizeof t);
  t.ds_first_gb = c->ds_first_gb.as<int>(); t.inv = c->inv.as<int>(); t.slice = c->slice.as<double>(); t.G = c->G.as<double>();
  t.packed = c->packed.as<double>(); t.host_out = c->h_pinned; t.host_flag = c->h_flag; t.counters = c->counters.as<unsigned>();
  t.nd = c->nd; t.dim = c->cur_dim; t.n_slices = 0;
  for (int d = 0; d < c->nd; d++) t.n_slices += std::min(32, c->h_ds_first_gb[d + 1] - c->h_ds_first_gb[d]);
  if (c->tail_host.size() == sizeof t && !memcmp(c->tail_host.data(), &t, sizeof t)) return 0;
  c->tail_host.assign(reinterpret_cast<const char*>(&t), reinterpret_cast<const char*>(&t) + sizeof t);
  HIPCHK(c, hipMemcpyAsync(c->tail_dev.p, c->tail_host.data(), sizeof t, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// tail_mode 0: workgroup sums only; 1: total in c->vec[0]; 2: and in the host mailbox under sequence number seq
int gfh::launch_model_chi2(gfh_ctx* c, int tail_mode, unsigned long long seq, int mesh_mode) {
  if (!c->n_gb) return 0;
  void* x = c->x.p; void* y = c->y.p; void* w = c->w.p; void* pars = c->pars.p; void* parg = c->cur->kernarg_pars ? (void*)c->h_pars : (void*)&pars;
  void* gs = c->gb_start.p; void* gn = c->gb_slots.p; void* gd = c->gb_ds.p;
  void* res = c->res.p; void* part = c->chi2_partial.p; void* stp = c->status.p;
  void* ax = c->aux.p; long long lda = c->n_slots; void* dfg = c->ds_first_gb.p; int nd = c->nd;
  void* out = c->vec.p; void* hout = c->h_pinned; void* hflag = c->h_flag; void* cnt = c->status.as<char>() + 24;
  void* mesh = c->disp.mesh.p;
  void* ord = c->disp.order_on && c->disp.order_ready && takes_mesh_args(c) ? c->disp.gb_order.p : nullptr; void* cst = nullptr;
  const int cw = chi2_waves_for(c->cur->n_active);
  int grid; if (wsg_grid(c, c->cur->chi2, 64 * cw, c->n_gb, &grid)) return 1;
  void* pool = c->ws.wsg.p;
  std::vector<void*> args{&x, &y, &w, parg, &gs, &gn, &gd, &res, &part, &stp, &ax, &lda, &dfg, &nd, &out, &hout, &hflag, &cnt, &seq, &tail_mode};
  if (takes_mesh_args(c)) { args.push_back(&mesh); args.push_back(&mesh_mode); args.push_back(&ord); args.push_back(&cst); }
  if (c->gen.ws_global) args.push_back(&pool);
  HIPCHK(c, hipModuleLaunchKernel(c->cur->chi2, grid, 1, 1, 64 * cw, 1, 1, 0, c->stream, args.data(), nullptr));
  return 0;
}

int gfh::launch_model_omega(gfh_ctx* c, int mesh_mode) {
  if (!c->n_tiles) return 0;
  void* x = c->x.p; void* w = c->w.p; void* pars = c->pars.p; void* parg = c->cur->kernarg_pars ? (void*)c->h_pars : (void*)&pars; void* dpp = c->dpars.p; void* dp = c->cur->kernarg_pars ? (void*)c->h_dpars : (void*)&dpp; void* tds = c->tile_ds.p; void* om = c->omega.p;
  int nt = c->n_tiles; void* stp = c->status.p;
  void* ax = c->aux.p; long long lda = c->n_slots;
  void* mesh = c->disp.mesh.p;
  void* ord = c->disp.order_on && c->disp.order_ready && takes_mesh_args(c) ? c->disp.tile_order.p : nullptr; void* cst = nullptr;
  // (quadrature models: uneven cost per point -- one tile per workgroup, dealt out as workgroups retire)
  if (!c->cur->omega_grid) c->cur->omega_grid = c->model.has_integrals() ? (1 << 30) : resident_grid(c, c->cur->omega, c->gen.block);
  int grid; if (wsg_grid(c, c->cur->omega, c->gen.block, std::min(c->n_tiles, c->cur->omega_grid), &grid)) return 1;
  void* pool = c->ws.wsg.p;
  std::vector<void*> args{&x, &w, parg, dp, &tds, &nt, &om, &stp, &ax, &lda};
  if (takes_mesh_args(c)) { args.push_back(&mesh); args.push_back(&mesh_mode); args.push_back(&ord); args.push_back(&cst); }
  if (c->gen.ws_global) args.push_back(&pool);
  HIPCHK(c, hipModuleLaunchKernel(c->cur->omega, grid, 1, 1, c->gen.block, 1, 1, 0, c->stream, args.data(), nullptr));
  return 0;
}

// publish_seq != 0 (single rank, pattern-only image through k_gather_sum): the assembling kernel writes the result mailbox itself
int gfh::launch_gram_chain(gfh_ctx* c, bool time_it, bool with_gram, bool sparse, unsigned long long publish_seq) {
  const int na = (int)c->cur_active.size(), T = c->cur_T, ps = gram_partial_stride(T);
  const int gw = ps;
  c->chain.gram.clear();
  if (c->n_gb && with_gram) HIPCHK(c, launch_gram(c->stream, T, c->J.as<double>(), c->ldj, na, c->res.as<double>(), c->gb_start.as<i64>(),
                                      c->gb_slots.as<int>(), c->n_gb, c->partial.as<double>(), &c->chain.gram));
  if (time_it) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  HIPCHK(c, launch_reduce_partials(c->stream, c->partial.as<double>(), ps, gw, c->ds_first_gb.as<int>(), c->nd, c->G.as<double>()));
  if (c->gs_meta.p && c->gs_n && c->gs_sparse == sparse) {
    HIPCHK(c, launch_gather_sum(c->stream, c->G.as<double>(), c->gs_meta.as<int>(), c->gs_list.as<int>(), c->gs_n, c->packed.as<double>(),
                                c->status.as<int>(), publish_seq ? c->h_pinned : nullptr, reinterpret_cast<unsigned*>(c->status.as<char>() + 16),
                                c->h_flag, publish_seq));
    c->chain.assemble = 2;
  } else if (sparse) {
    HIPCHK(c, launch_assemble_sparse(c->stream, c->G.as<double>(), gw, T, c->nd, c->cur_dim, c->inv.as<int>(), c->owner.as<int>(),
                                     c->nz_row.as<int>(), c->nz_col.as<int>(), c->nnz, c->packed.as<double>()));
    c->chain.assemble = 3;
  } else {
    HIPCHK(c, launch_assemble(c->stream, c->G.as<double>(), gw, T, c->nd, c->cur_dim, c->inv.as<int>(), c->owner.as<int>(), c->packed.as<double>()));
    c->chain.assemble = 4;
  }
  return 0;
}

// STEP 3 without the stored Jacobian: gfh_k_omega_jt (generated) recomputes each point's Jacobian row
int gfh::launch_model_omega_jt(gfh_ctx* c) {
  if (!c->n_gb) return 0;
  void* x = c->x.p; void* w = c->w.p; void* pars = c->pars.p; void* parg = c->cur->kernarg_pars ? (void*)c->h_pars : (void*)&pars;
  void* dpp = c->dpars.p; void* dp = c->cur->kernarg_pars ? (void*)c->h_dpars : (void*)&dpp;
  void* gs = c->gb_start.p; void* gn = c->gb_slots.p; void* gd = c->gb_ds.p; void* om = c->omega.p;
  void* part = c->partial.p; int ps = gram_partial_stride(c->cur_T); void* stp = c->status.p;
  void* ax = c->aux.p; long long lda = c->n_slots;
  void* args[] = {&x, &w, parg, dp, &gs, &gn, &gd, &om, &part, &ps, &stp, &ax, &lda};
  HIPCHK(c, hipModuleLaunchKernel(c->cur->omega_jt, c->n_gb, 1, 1, 256, 1, 1, 0, c->stream, args, nullptr));
  return 0;
}
