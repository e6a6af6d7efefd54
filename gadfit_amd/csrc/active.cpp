// active.cpp -- model, kernels and active set: the model a context fits (gfh_set_model*), the generated kernels of an active set
// (get_kernels: generate, compile, load, cache), and prepare_active, which sizes every buffer a pass of that active set needs and
// uploads the layout of the packed image the ranks sum (packed_layout.cpp).  It launches nothing and owns no timing; buffers come from devmem.cpp.
#include "context_internal.h"
#include "group.h"
#include "packed_layout.h"
#include <algorithm>
#include <cstring>
#include <exception>

using namespace gfh;

// ------------------------------------------------------------------------- model
// The quadrature workspaces the next kernels carry (model.h, plan_workspaces): the fast form in scratch, or the user's sizes -- in
// scratch while they fit the budget, else in the context's global pool.
void gfh::apply_ws_plan(gfh_ctx* c) {
  const gfh::WsPlan p = gfh::plan_workspaces(c->model, c->ws.fast, c->ws.grown);
  c->gen.ws_size = p.ws_size; c->gen.ws_size_inner = p.ws_size_inner; c->gen.ws_global = p.global;
  const int64_t wave = p.global ? gfh::wsg_wave_doubles(c->model, p.ws_size, p.ws_size_inner) : 0;
  if (wave != c->ws.wave_doubles) {          // (another slot size: the pool is cut anew at the next launch that needs it)
    if (c->ws.wsg.p && c->device >= 0) { hipSetDevice(c->device); if (c->stream) hipStreamSynchronize(c->stream); dev_free(c->ws.wsg); }
    c->ws.waves = 0; c->ws.tried = 0; c->ws.wave_doubles = wave;
  }
}

static int get_kernels_variant(gfh_ctx* c, const std::vector<int32_t>& active, bool load, int kernarg_pars) {
  // loaded kernels are keyed by the active set and the generator options that can change per context
  std::vector<int32_t> key = active;
  key.push_back(-1 - c->gen.loss - 4 * (c->gen.finite_diff ? 1 : 0) - 8 * (c->gen.store_j ? 0 : 1) - 16 * (c->gen.store_res ? 0 : 1) - 32 * kernarg_pars);
  key.push_back(-1 - c->gen.ws_size); key.push_back(-1 - c->gen.ws_size_inner); key.push_back(c->gen.ws_global ? -2 : -1);
  key.push_back(c->gen.finite_diff && c->gen.fd_col_sets ? -2 : -1);
  auto it = c->kernel_cache.find(key);
  if (it != c->kernel_cache.end()) { c->cur = &it->second; return 0; }
  std::string src, err;
  GenConfig cfg = c->gen; cfg.kernarg_pars = kernarg_pars;
  if (!generate_source(c->model, active, cfg, &src, &err)) return fail(c, err);
  ModelKernels mk;
  const uint64_t skey = load ? source_key(src) : 0;
  if (!(load && acquire_loaded(c->device, skey, &mk))) {       // (a code object this process already has loaded on this card: rtc.h)
    std::vector<char> code; bool cached = false;
    if (!compile_to_code_object(src, &code, &err, &cached)) return fail(c, err);
    if (!load) return 0;
    if (!load_kernels(code, &mk, &err)) return fail(c, err);
    publish_loaded(c->device, skey, mk);
  }
  mk.kernarg_pars = kernarg_pars; mk.n_active = (int)active.size();
  c->cur = &c->kernel_cache.emplace(key, mk).first->second;
  return 0;
}

int gfh::get_kernels(gfh_ctx* c, const std::vector<int32_t>& active, bool load) {
  if (!c->has_model) return fail(c, "no model set (gfh_set_model)");
  const int np = c->model.n_pars;
  const bool can = c->kernarg && np >= 1 && np <= kMaxKernargPars;
  if (c->device < 0 && !c->nd) {          // compile-only context without data: the one-dataset and the pointer form go to the cache
    if (can && get_kernels_variant(c, active, load, np)) return 1;
    return get_kernels_variant(c, active, load, 0);
  }
  // the whole [n_datasets][n_pars] block by value while it fits the kernel-argument segment
  const bool fits = can && c->nd >= 1 && (int64_t)c->nd * np <= kMaxKernargPars;
  return get_kernels_variant(c, active, load, fits ? c->nd * np : 0);
}

// The kernels of the current active set without the Jacobian store, beside c->cur (which stays what it is): what a sweep of a fit
// that defers the store launches.  A lookup in the cache; the first call for an active set loads (or compiles) them.
ModelKernels* gfh::nostore_kernels(gfh_ctx* c) {
  if (!c->cur || !c->gen.store_j) return c->cur;
  ModelKernels* const keep = c->cur;
  c->gen.store_j = false;
  const int rc = get_kernels(c, c->cur_active, true);
  ModelKernels* const mk = rc ? nullptr : c->cur;
  c->gen.store_j = true; c->cur = keep;
  return mk;
}

int gfh::check_aux(gfh_ctx* c) {
  if (c->has_model && c->model.n_aux > c->n_aux)
    return fail(c, "the model reads " + std::to_string(c->model.n_aux) + " auxiliary per-point column(s); call gfh_set_aux after gfh_set_data");
  return 0;
}

// the buffer of the quadrature meshes (context.h): one record per slot and outermost integrate() call site of the model
int gfh::ensure_mesh(gfh_ctx* c) {
  const int sites = (c->has_model && c->disp.mesh_on && c->gen.fast_div && unit_takes_mesh_args(c->model, c->gen)) ? mesh_sites(c->model) : 0;
  const int stride = sites * kMeshRecord;
  if (stride != c->disp.mesh_stride) { c->disp.mesh_stride = stride; c->disp.mesh_valid = false; }
  if (stride) {
    const size_t need = (size_t)stride * (size_t)std::max<int64_t>(1, c->n_slots);
    if (c->disp.mesh.bytes < need) { c->disp.mesh_valid = false; if (dev_alloc(c, c->disp.mesh, need)) return 1; }
  } else dev_free(c->disp.mesh);
  return 0;
}

int gfh::prepare_active(gfh_ctx* c, const int32_t* active, int na, const int32_t* jac, int dim) {
  if (na < 1) return fail(c, "There are no active parameters.");
  if (check_aux(c) || ensure_gb_partition(c)) return 1;
  if ((na > kFusedMaxActive || (c->has_model && c->model.has_integrals())) && !c->gen.store_j)
    set_store_j(c, true);   // beyond 4 tiles, and for quadrature models, STEP 2 is a separate pass over the stored Jacobian
  // fast path of the LM loop: the same active set, column map and kernels as in the previous call
  if (c->cur && c->prepared && c->cur == c->prepared_cur && dim == c->cur_dim && (int)c->cur_active.size() == na && c->prepared_store_j == c->gen.store_j &&
      std::equal(active, active + na, c->cur_active.begin()) && c->cur_jac.size() == (size_t)c->nd * na &&
      std::equal(jac, jac + (size_t)c->nd * na, c->cur_jac.begin()))
    return 0;
  c->prepared = false;
  std::vector<int32_t> a(active, active + na);
  if (get_kernels(c, a, true)) return 1;
  if (ensure_tile_table(c)) return 1;
  std::vector<int32_t> j(jac, jac + (size_t)c->nd * na);
  const bool same = (a == c->cur_active) && (j == c->cur_jac) && dim == c->cur_dim;
  c->cur_T = (na + 15) / 16;
  if (!same) {
    PackedLayout L; std::string lerr;
    if (!compute_layout(c->nd, na, jac, dim, c->sparse_ok, &L, &lerr)) return fail(c, lerr);
    const std::vector<int>& inv = L.inv;
    if (dev_alloc(c, c->inv, sizeof(int) * inv.size())) return 1;
    HIPCHK(c, hipMemcpy(c->inv.p, inv.data(), sizeof(int) * inv.size(), hipMemcpyHostToDevice));
    if (dev_alloc(c, c->owner, sizeof(int) * (size_t)dim)) return 1;
    HIPCHK(c, hipMemcpy(c->owner.p, L.owner.data(), sizeof(int) * (size_t)dim, hipMemcpyHostToDevice));
    c->sparse = L.sparse; c->nnz = L.nnz; c->h_nz_row = L.nz_row; c->h_nz_col = L.nz_col;
    if (c->sparse) {
      if (dev_alloc(c, c->nz_row, sizeof(int) * (size_t)c->nnz) || dev_alloc(c, c->nz_col, sizeof(int) * (size_t)c->nnz)) return 1;
      HIPCHK(c, hipMemcpy(c->nz_row.p, c->h_nz_row.data(), sizeof(int) * (size_t)c->nnz, hipMemcpyHostToDevice));
      HIPCHK(c, hipMemcpy(c->nz_col.p, c->h_nz_col.data(), sizeof(int) * (size_t)c->nnz, hipMemcpyHostToDevice));
    }
    // source lists for k_gather_sum, for the layout the launch chain will use (none: the chain assembles through owner / inv)
    {
      std::vector<int> meta, list;
      dev_free(c->gs_meta); c->gs_n = 0; c->gs_sparse = L.transfer_sparse();
      if (build_gather_lists(L, c->nd, dim, c->cur_T, &meta, &list)) {
        if (dev_alloc(c, c->gs_meta, sizeof(int) * meta.size()) || dev_alloc(c, c->gs_list, sizeof(int) * list.size())) return 1;
        HIPCHK(c, hipMemcpy(c->gs_meta.p, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->gs_list.p, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
        c->gs_n = (int)meta.size();
      }
    }
    c->cur_active = a; c->cur_jac = j; c->cur_dim = dim; c->have_sweep = false;
  }
  if (ensure_mesh(c)) return 1;
  const int ps = gram_partial_stride(c->cur_T);
  const size_t packed_n = (size_t)dim * dim + dim + 2;       // (+ the status slot that travels with a cross-rank sum)
  if ((c->gen.store_j && place_jacobian(c, na)) ||
      dev_alloc(c, c->partial, sizeof(double) * (size_t)std::max(1, c->n_gb) * ps) ||
      dev_alloc(c, c->G, sizeof(double) * (size_t)c->nd * ps) ||
      dev_alloc(c, c->packed, sizeof(double) * packed_n) ||
      dev_alloc(c, c->chi2_partial, sizeof(double) * (size_t)std::max(1, c->n_gb)) ||
      dev_alloc(c, c->vec, sizeof(double) * (size_t)(dim + 8)) ||
      pinned_reserve(c, sizeof(double) * std::max<size_t>(packed_n + 1, 4096))) return 1;
  c->prepared = true; c->prepared_store_j = c->gen.store_j; c->prepared_cur = c->cur;
  return 0;
}

extern "C" {

int gfh_set_model_variants(gfh_ctx* c, int n, const gfh_tape* const* t, int hint_aux) try {
  if (!c) return 1;
  GROUP(c, gfh_set_model_variants(k, n, t, hint_aux));
  std::string err;
  Model m;
  // (per-tape hint columns left by gfh_set_variant_hint_columns for exactly this hand-over)
  const std::vector<int32_t> cols = std::move(c->up.pending_hint_cols);
  c->up.pending_hint_cols.clear();
  if (!m.load_variants(n, t, hint_aux, &err, (int)cols.size() == n ? &cols : nullptr)) return fail(c, "gfh_set_model: " + err);
  if (gfh::join_pending(c)) return 1;
  if (c->device >= 0) { hipSetDevice(c->device); if (c->stream) hipStreamSynchronize(c->stream); for (auto& kv : c->kernel_cache) release_loaded(c->device, &kv.second); }
  c->kernel_cache.clear(); c->cur = nullptr; c->cur_active.clear(); c->have_sweep = false; c->prepared = false;
  c->model = std::move(m); c->has_model = true; c->model_serial++; c->disp.mesh_valid = false;
  c->disp.order_ready = false; c->disp.order_want = true;
  // the kernels first carry small quadrature workspaces (fast: 3.2 KB of scratch per lane and level); a pass that exhausts them is
  // repeated with the user's sizes (grow_workspace)
  // (a model handed over by a recovery's handler keeps the grown state: the pass that is about to be repeated has needed it)
  c->ws.grown = c->ws.grown && c->in_recovery;
  apply_ws_plan(c);
  // Models with integrate(): the plain kernels are bound by VALU issue and their bodies take 135-150 VGPRs as the compiler
  // allocates them (3 waves per SIMD; gfh_k_chi2's 8-wave workgroups then fit once per CU = 2 waves per SIMD).  Capped at 128
  // registers (4 waves) a handful of values spill and chi2 runs 20 % faster, the sweep 4 %; at 96 (5 waves) the spills cost
  // more than the waves bring (profiles/r03_cfg4.md).
  c->gen.waves_per_eu = c->model.has_integrals() ? 4 : 0;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_model: ") + e.what()); }

int gfh_set_model(gfh_ctx* c, const gfh_tape* t) { return gfh_set_model_variants(c, 1, &t, -1); }

int gfh_set_variant_hint_columns(gfh_ctx* c, int n_tapes, const int32_t* cols) {
  if (!c) return 1;
  GROUP(c, gfh_set_variant_hint_columns(k, n_tapes, cols));
  if (n_tapes < 0 || (n_tapes > 0 && !cols)) return fail(c, "gfh_set_variant_hint_columns: bad arguments");
  c->up.pending_hint_cols.assign(cols, cols + n_tapes);
  return 0;
}

int gfh_model_needs_hint(gfh_ctx* c) {
  if (!c) return -1;
  if (c->grp) return gfh_model_needs_hint(gfh::group_member(c, 0));
  if (!c->has_model) return -1;
  try { return c->model.needs_hint() ? 1 : 0; } catch (const std::exception&) { return -1; }
}
int gfh_model_n_variants(gfh_ctx* c) {
  if (!c) return 0;
  if (c->grp) return gfh_model_n_variants(gfh::group_member(c, 0));
  return c->has_model ? c->model.n_variants() : 0;
}
int gfh_model_n_tapes(gfh_ctx* c) {
  if (!c) return 0;
  if (c->grp) return gfh_model_n_tapes(gfh::group_member(c, 0));
  return c->has_model ? c->model.n_tapes : 0;
}
int64_t gfh_model_source(gfh_ctx* c, int n_act, const int32_t* active, char* buf, int64_t cap) {
  if (c && c->grp) {
    gfh_ctx* k0 = gfh::group_member(c, 0);
    const int64_t n = gfh_model_source(k0, n_act, active, buf, cap);
    if (n < 0) fail(c, k0->err);
    return n;
  }
  if (!c || !c->has_model) { fail(c, "no model set"); return -1; }
  std::string src, err;
  std::vector<int32_t> a(active, active + n_act);
  GenConfig cfg = c->gen;
  const int np = c->model.n_pars;
  if (c->kernarg && np >= 1 && (int64_t)std::max(1, c->nd) * np <= kMaxKernargPars) cfg.kernarg_pars = std::max(1, c->nd) * np;
  if (!generate_source(c->model, a, cfg, &src, &err)) { fail(c, err); return -1; }
  if (buf && cap > 0) { size_t n = std::min<size_t>((size_t)cap - 1, src.size()); memcpy(buf, src.data(), n); buf[n] = 0; }
  return (int64_t)src.size() + 1;
}

int gfh_model_prepare(gfh_ctx* c, int n_act, const int32_t* active) {
  if (!c) return 1;
  GROUP(c, gfh_model_prepare(k, n_act, active));      // compiled once: rtc.cpp serialises, the other members load the cached code object
  std::vector<int32_t> a(active, active + n_act);
  if (c->device >= 0) return get_kernels(c, a, false);
  // compile-only context (build time): also the forms gfh_fit switches to under keep_jacobian mode 2 -- without the Jacobian
  // store (plain fits) and without the residual store -- and the one its sweeps run under mode 1 while the store is deferred (no
  // Jacobian store, residuals kept), so that a GPU box finds them in the cache
  const bool sj = c->gen.store_j, sr = c->gen.store_res;
  int rc = get_kernels(c, a, false);
  const bool combos[3][2] = {{false, false}, {true, false}, {false, true}};
  for (int k = 0; k < 3 && !rc; k++) {
    c->gen.store_j = combos[k][0] || !c->fused || c->model.has_integrals() || n_act > kFusedMaxActive; c->gen.store_res = combos[k][1];
    rc = get_kernels(c, a, false);
  }
  c->gen.store_j = sj; c->gen.store_res = sr;
  return rc;
}

// ONE translation unit into the cache, not loaded: the kernels a context that holds n_datasets datasets loads for this active set --
// the parameter block by value while n_datasets * n_pars doubles fit the kernel-argument segment, else by pointer -- with the Jacobian
// store or without it.  (gfh_model_prepare on a compile-only context builds the one-dataset and the pointer form in all four
// combinations of the stores; this is for callers that know which units they will ask for.)  Needs no GPU.
int gfh_model_prepare_form(gfh_ctx* c, int n_act, const int32_t* active, int n_datasets, int store_jacobian) {
  if (!c) return 1;
  NOT_FOR_GROUP(c, "gfh_model_prepare_form");
  if (!c->has_model) return fail(c, "no model set (gfh_set_model)");
  if (n_act < 1 || !active || n_datasets < 1) return fail(c, "gfh_model_prepare_form: bad arguments");
  const std::vector<int32_t> a(active, active + n_act);
  const int np = c->model.n_pars;
  const bool by_value = c->kernarg && np >= 1 && (int64_t)n_datasets * np <= kMaxKernargPars;
  const bool sj = c->gen.store_j;
  ModelKernels* const keep = c->cur;
  c->gen.store_j = store_jacobian != 0 || !c->fused || c->model.has_integrals() || n_act > kFusedMaxActive;
  const int rc = get_kernels_variant(c, a, false, by_value ? n_datasets * np : 0);
  c->gen.store_j = sj; c->cur = keep;
  return rc;
}

// Test hook (no GPU needed): the geometry and the layout of the all-reduced image as rank `rank` of `nranks` derives them.
// out[0] = length of the packed image, out[1] = pattern-only transfer (0/1), out[2] = nnz, out[3] = FNV-1a hash of the
// pattern lists and of inv/owner, out[4] = first global point of this rank, out[5] = its point count, out[6] = number
// of datasets it holds points of, out[7] = its number of gram workgroups.  Every rank must report the same out[0..3].
int gfh_debug_packed_layout(int nranks, int rank, int64_t n_total, int nd, const int64_t* dp, int na, const int32_t* jac, int dim,
                            int sparse_ok, int64_t* out, int32_t* nz_row, int32_t* nz_col, int nz_cap) {
  if (nranks < 1 || rank < 0 || rank >= nranks || !dp || !jac || !out || na < 1 || nd < 1) { set_global_error("gfh_debug_packed_layout: bad arguments"); return 1; }
  gfh_ctx c;
  c.nranks = nranks; c.rank = rank;
  if (set_geometry(&c, n_total, nd, dp)) { set_global_error(c.err); return 1; }
  PackedLayout L; std::string lerr;
  if (!compute_layout(nd, na, jac, dim, sparse_ok != 0, &L, &lerr)) { set_global_error(lerr); return 1; }
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const std::vector<int>& v) { for (int x : v) { h ^= (uint32_t)x; h *= 1099511628211ull; } h ^= 0xffu; h *= 1099511628211ull; };
  mix(L.nz_row); mix(L.nz_col); mix(L.inv); mix(L.owner);
  int held = 0;
  for (int d = 0; d < nd; d++) if (c.lb[d + 1] > c.lb[d]) held++;
  out[0] = (int64_t)L.packed_n(dim); out[1] = L.transfer_sparse() ? 1 : 0; out[2] = L.nnz; out[3] = (int64_t)(h >> 1);
  out[4] = c.begin; out[5] = c.count; out[6] = held; out[7] = c.n_gb;
  for (int k = 0; k < L.nnz && k < nz_cap; k++) { if (nz_row) nz_row[k] = L.nz_row[k]; if (nz_col) nz_col[k] = L.nz_col[k]; }
  return 0;
}

int gfh_set_active(gfh_ctx* c, const int32_t* active, int na, const int32_t* jac, int dim) {
  GROUP(c, gfh_set_active(k, active, na, jac, dim));
  NEED_GPU(c);
  if (!c->nd) return fail(c, "no data set (gfh_set_data)");
  return prepare_active(c, active, na, jac, dim);
}

int gfh_jacobian_indices(int nd, int na, const int32_t* active, const int32_t* is_global, int32_t* jac) {
  int shift = 0;   // gadfit.F90:618-628
  for (int i = 0; i < nd; i++)
    for (int j = 0; j < na; j++) {
      if (is_global[active[j]]) { jac[i * na + j] = j; if (i > 0) shift++; }
      else jac[i * na + j] = j + i * na - shift;
    }
  return nd * na - shift;
}

}  // extern "C"
