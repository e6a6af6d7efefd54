// codegen.cpp -- lowers a model tape to HIP source for gfx950: generate_source, the layout of one translation unit.
//
// Three kernels per (model, active set):
//   gfh_k_sweep  STEP 1 (gadfit.F90:675-693): res_i = (y_i-f)*w_i, J[a][i] = df/dp_a * w_i
//   gfh_k_chi2   chi2() (gadfit.F90:1015-1034): all parameters passive, res_i and sum res^2
//   gfh_k_omega  STEP 3 (gadfit.F90:715-731): omega_i = -f''_delta(x_i) * w_i, forward mode
//
// Only what depends on the tape is generated here: the point functions, the quadrature call sites, the selector and the
// #defines in front of them (emit_ad.cpp unrolls a tape, emit_quadrature.cpp and emit_branching.cpp write what integrate() and a
// branching eval() add).  The kernels themselves are hand-written HIP that no tape changes; they are plain files under
// device/ (sweep.hip, fused_sweep_gram.hip, chi2.hip, omega.hip, omega_jt.hip, batch_fit.hip, batch_cov.hip, batch_eval.hip, batch_wg_sum.hip, batch_cube.hip, eval.hip, ...), embedded by
// device_text.cpp and streamed into the translation unit by generate_source as they are.  Loading and validating a tape is
// model.cpp.
#include "codegen_internal.h"
#include "device_text.h"
#include <algorithm>
#include <cstring>

namespace gfh {

namespace {

// The cooperative form of the fused kernel (GFH_COOP, 5 ... 8 tiles): its switch and, per wave W of the workgroup, the straight-line
// code of its share of the tile pairs -- a contiguous run of the row-major upper triangle:
//   GFH_CLOAD_W(B, U)  fragment reads of k-step U into buffer B: one per DISTINCT tile of the run + the residual row
//   GFH_CMMA_W(B)      one v_mfma_f64_16x16x4_f64 per pair; J^T r of tile t with the owner of pair (t, t)
//   GFH_CPUT_W         the wave's accumulators into the workgroup's image
static std::string coop_defines(int NA) {
  std::ostringstream o;
  const bool on = fused_coop(NA);
  o << "\n#define GFH_COOP " << (on ? 1 : 0);
  if (!on) return o.str();
  const int T = (NA + 15) / 16, npair = T * (T + 1) / 2, fw = fused_waves_for(NA);
  std::vector<std::pair<int, int>> pairs;
  for (int ti = 0; ti < T; ti++) for (int tj = ti; tj < T; tj++) pairs.push_back({ti, tj});
  int cnd = 0;
  std::ostringstream body;
  for (int w = 0, p0 = 0; w < fw; w++) {
    const int nk = npair / fw + (w < npair % fw ? 1 : 0);
    std::vector<int> tiles;                                   // distinct tiles of this wave's run, in order of first use
    auto slot = [&](int t) { for (size_t d = 0; d < tiles.size(); d++) if (tiles[d] == t) return (int)d; tiles.push_back(t); return (int)tiles.size() - 1; };
    std::ostringstream mma0, mma, put;
    for (int k = 0; k < nk; k++) {
      const int ti = pairs[(size_t)(p0 + k)].first, tj = pairs[(size_t)(p0 + k)].second;
      const int ia = slot(ti), ib = slot(tj);
      (k == 0 ? mma0 : mma) << " GFH_MFMA(f[B_][" << ia << "], f[B_][" << ib << "], acc[" << k << "]);";
      if (ti == tj) mma << " accr[" << k << "] += f[B_][" << ia << "] * fr[B_];";
      put << " GFH_CPUT(" << k << ", " << (p0 + k) << ")";
      if (ti == tj) put << " GFH_CPUTR(" << k << ", " << ti << ")";
    }
    body << "\n#define GFH_CLOAD_" << w << "(B_, U_) fr[B_] = sb[16 * GFH_T * GFH_S + 4 * (U_) + q];";
    for (size_t d = 0; d < tiles.size(); d++) body << " f[B_][" << d << "] = sb[(16 * " << tiles[d] << " + r) * GFH_S + 4 * (U_) + q];";
    body << "\n#define GFH_CMMA0_" << w << "(B_)" << mma0.str();
    body << "\n#define GFH_CMMA_" << w << "(B_)" << mma.str();
    body << "\n#define GFH_CPUT_" << w << put.str();
    cnd = std::max(cnd, (int)tiles.size());
    p0 += nk;
  }
  o << "\n#define GFH_CK " << (npair + fw - 1) / fw << "\n#define GFH_CND " << std::max(1, cnd) << body.str();
  return o.str();
}

// GenConfig::batch: the four kernels of batched independent fits, behind the point functions of the translation unit (batch.cpp is
// their host side and refuses what they do not carry before it comes here; the checks below keep the generator honest on its own).
// A file of the batch text with its `#if GFH_BLOSS` / `#else  // GFH_BLOSS` / `#endif  // GFH_BLOSS` lines resolved HERE, not by the
// preprocessor: the three directives (whole lines, exactly these) and the arm not taken are left out, so a linear unit is the text it
// was before a batch had a loss and a loss unit reads as straight as that one.  The regions do not nest; any other directive passes through.
// The estimator's regions (`macro` GFH_BMLE, GenConfig::batch_estimator) are resolved by a second walk over the result of the first: they
// stand outside the loss's regions or inside their linear arms, which a loss unit has dropped by then, directives and all.
static std::string resolve_batch_loss(const char* text, bool loss, const char* macro = "GFH_BLOSS") {
  std::string out; out.reserve(strlen(text));
  const std::string m_if = std::string("#if ") + macro + "\n", m_else = std::string("#else  // ") + macro + "\n", m_endif = std::string("#endif  // ") + macro + "\n";
  int arm = 0;                      // 0 outside a region, 1 in its loss arm, 2 in its linear arm
  for (const char* p = text; *p;) {
    const char* e = strchr(p, '\n');
    const size_t n = e ? (size_t)(e - p) + 1 : strlen(p);
    const std::string line(p, n);
    p += n;
    if (line == m_if) { arm = 1; continue; }
    if (arm && line == m_else) { arm = 2; continue; }
    if (arm && line == m_endif) { arm = 0; continue; }
    if (arm == 0 || (arm == 1) == loss) out += line;
  }
  return out;
}

static bool emit_batch_kernels(const Model& m, const std::vector<int32_t>& active, const GenConfig& cfg, std::ostringstream& s, std::string* err) {
  const int NA = (int)active.size();
  if (NA < 1 || NA > kValuGramMax) { *err = "batch kernels: 1 to " + std::to_string(kValuGramMax) + " active parameters"; return false; }
  if (m.has_integrals() || m.branching() || m.n_aux > 0) { *err = "batch kernels: models with integrate(), variant tapes or auxiliary columns are not carried"; return false; }
  if (cfg.finite_diff || cfg.loss != 0 || !cfg.omega_jt) { *err = "batch kernels: use_ad = 0, robust losses and GADFIT_HIP_OMEGA_JT=0 are not carried"; return false; }
  if (cfg.batch_lanes != 64 && cfg.batch_lanes != 16 && cfg.batch_lanes != 256) { *err = "batch kernels: 64, 16 or 256 lanes per fit"; return false; }
  s << "\n#define GFH_BATCH 1\n#define GFH_BACT {";
  for (int j = 0; j < NA; j++) s << (j ? ", " : "") << active[j];
  s << "}\n#define GFH_BLANES " << cfg.batch_lanes << "\n";
  if (cfg.batch_loss < 0 || cfg.batch_loss > 2) { *err = "batch kernels: batch_loss is 0 (linear), 1 (cauchy) or 2 (huber)"; return false; }
  const bool loss = cfg.batch_loss != 0;
  if (loss) s << "#define GFH_BLOSS " << cfg.batch_loss << "\n";      // in the text of the loss units alone
  if (cfg.batch_estimator < 0 || cfg.batch_estimator > 1) { *err = "batch kernels: batch_estimator is 0 (least squares) or 1 (poisson)"; return false; }
  const bool mle = cfg.batch_estimator != 0;
  if (mle && loss) { *err = "batch kernels: the poisson estimator is not carried under a loss"; return false; }
  if (mle) s << "#define GFH_BMLE " << cfg.batch_estimator << "\n";   // in the text of the Poisson units alone
  const auto resolve = [&](const char* text) { return resolve_batch_loss(resolve_batch_loss(text, loss).c_str(), mle, "GFH_BMLE"); };
  if (cfg.batch_cube) {             // batch_cube.hip: the data form and the load of a cube, in the text of the cube forms alone
    if (cfg.batch_y_type < 0 || cfg.batch_y_type > 2 || cfg.batch_error_type < 0 || cfg.batch_error_type > 4) { *err = "batch kernels: a cube's y_type is 0 ... 2, its error_type 0 ... 4"; return false; }
    s << "#define GFH_BCUBE 1\n#define GFH_BYTYPE " << cfg.batch_y_type << "\n#define GFH_BERR " << cfg.batch_error_type << "\n" << kBatchCube;
  }
  if (cfg.batch_lanes == 256) s << kBatchWgSum;          // batch_wg_sum.hip: LDS and a barrier, in the text of the workgroup form alone
  s << resolve(kBatchFit);                               // batch_fit.hip: the passes and the solve of a fit, written once against GFH_BLANES
  if (cfg.batch_bounded) {          // the bounded unit: gfh_k_fit_batch_bounded alone behind them (batch_fit_bounded.hip)
    s << resolve(kBatchFitBounded);
    return true;
  }
  s << resolve(kBatchFitKernels);                 // batch_fit_kernels.hip: gfh_k_fit_batch, gfh_k_batch_pass
  s << resolve(kBatchCov);                               // batch_cov.hip: gfh_k_batch_cov, behind them in every form
  s << kBatchEval;                  // batch_eval.hip: gfh_k_batch_eval, behind that
  return true;
}

}  // namespace

// ---- the four functions of a data point (codegen_internal.h, PointFn)
#define GFH_PAD54 "                                                      "

const PointFn kPointValue{"value", "double", "// One data point, every parameter passive (chi2 path): value only.\n",
                          " int* STATUS,\n", GFH_PAD54 "   ", "X, P, STATUS",
                          " gfh_report_unseen(STATUS, SLOT, path, ng); return 0.0;", 0, false};
const PointFn kPointGrad{"grad", "void", "// One data point, reverse mode: value F and gradient G[a] = dF/dp_active(a).\n",
                         "\n" GFH_PAD54 "double& F, double (&G)[GFH_NA], int* STATUS,\n", GFH_PAD54, "X, P, F, G, STATUS",
                         "\n      F = 0.0;\n#pragma unroll\n      for (int a = 0; a < GFH_NA; a++) G[a] = 0.0;\n      gfh_report_unseen(STATUS, SLOT, path, ng);", 1, true};
const PointFn kPointDd{"dd", "double", "// One data point, forward mode: second directional derivative along DP (per-parameter d seeds).\n",
                       "\n" GFH_PAD54 "const double* __restrict__ DP, int* STATUS,\n", GFH_PAD54, "X, P, DP, STATUS",
                       " gfh_report_unseen(STATUS, SLOT, path, ng); return 0.0;", 2, false};
// One data point, forward mode AND reverse mode over ONE evaluation of the forward values: the second directional
// derivative along DP and the gradient.  The forward values are the expressions of gfh_point_grad / gfh_point_dd (the same
// emit_value_node), the reverse sweep is gfh_point_grad's, so G is bitwise the Jacobian row the sweep kernel stores.
const PointFn kPointDdGrad{"dd_grad", "double", "",
                           "\n" GFH_PAD54 "     const double* __restrict__ DP, double (&G)[GFH_NA], int* STATUS,\n", GFH_PAD54 "     ", "X, P, DP, G, STATUS",
                           "\n#pragma unroll\n      for (int a = 0; a < GFH_NA; a++) G[a] = 0.0;\n      gfh_report_unseen(STATUS, SLOT, path, ng); return 0.0;", 2, true};
#undef GFH_PAD54

std::string point_head(const PointFn& f, const std::string& sfx, const std::string& slot) {
  return std::string("static __device__ __forceinline__ ") + f.ret + " gfh_point_" + f.name + sfx + "(const double X, const double* __restrict__ P," + f.params +
         f.pad + "const double* __restrict__ AXP, const i64 LDA GFH_MESH_DECL" + slot + ") {\n";
}

namespace {

// What the steps of generate_source share: the inputs, the text so far, and the activity of the parameters.
struct Unit {
  const Model& m;
  const std::vector<int32_t>& active;
  const GenConfig& cfg;
  const int NA;
  std::vector<char> pa, none;      // per parameter: active in this unit / all passive
  const bool mesh_on;              // the kernels take the mesh and order arguments
  std::ostringstream s;
  Unit(const Model& mm, const std::vector<int32_t>& a, const GenConfig& c)
      : m(mm), active(a), cfg(c), NA((int)a.size()), pa((size_t)mm.n_pars, 0), none((size_t)mm.n_pars, 0), mesh_on(unit_takes_mesh_args(mm, c)) {
    for (int p : a) pa[(size_t)p] = 1;
  }
};

bool check_arguments(const Model& m, const std::vector<int32_t>& active, std::string* err) {
  for (int v = 0; v < m.n_variants(); v++)
    for (const Node& nd : m.eval(v).nodes)
      if (nd.op == GFH_IVAR || nd.op == GFH_IPARAM) { *err = "integrand node in eval() tape"; return false; }
  for (int a : active) if (a < 0 || a >= m.n_pars) { *err = "active parameter out of range"; return false; }
  return true;
}

// the first line and the #defines of the unit's options and of the fused kernel's geometry
void emit_option_defines(Unit& u) {
  const GenConfig& cfg = u.cfg; const int NA = u.NA, NP = u.m.n_pars;
  u.s << "// generated by libgadfit_hip codegen -- model with " << u.m.sub[0].nodes.size() << " tape nodes, "
      << NP << " parameters, " << NA << " active\n";
  u.s << "#define GFH_OMEGA_JT " << (cfg.omega_jt ? 1 : 0) << "\n#define GFH_FW " << fused_waves_for(NA) << "\n#define GFH_HALF " << (fused_half_stage(NA) ? 1 : 0) << "\n#define GFH_RED1 " << (fused_single_image(NA) ? 1 : 0) << "\n#define GFH_FUSED_MAX " << kFusedMaxActive << coop_defines(NA) << "\n#define GFH_FAST_DIV " << (cfg.fast_div ? 1 : 0)
      << "\n#define GFH_STORE_J " << (cfg.store_j ? 1 : 0) << "\n#define GFH_STORE_RES " << (cfg.store_res ? 1 : 0) << "\n#define GFH_LOSS " << cfg.loss << "\n#define GFH_BLOCK " << cfg.block << "\n#define GFH_NP " << NP
      << "\n#define GFH_NA " << (NA > 0 ? NA : 1) << "\n#define GFH_VALU_GRAM_MAX " << kValuGramMax << "\n#define GFH_AD_PRIO " << (cfg.store_j ? 0 : 1) << "\n";
  u.s << "#define GFH_PARG " << cfg.kernarg_pars << "\n";
}

// what every body leans on: gfh_exp, gfh_pow_ln where a tape raises an AD variable to one, i64, the status word, the lane stash
// of integrands that read the data point, the parameter block
void emit_prelude(Unit& u) {
  const Model& m = u.m; std::ostringstream& s = u.s;
  s << kExp;                        // exp.hip: gfh_exp
  bool has_pow = false;
  for (const std::vector<SubTape>* tapes : {&m.sub, &m.more_evals})
    for (const SubTape& t_ : *tapes) for (const Node& nd : t_.nodes) if (nd.op == GFH_POW && !(nd.flags & GFH_F_REAL)) has_pow = true;
  if (has_pow && u.cfg.fast_div) s << kPowLn;      // pow_ln.hip: gfh_pow_ln
  bool lane_stash = false;          // some integrand reads the data point's abscissa or auxiliary columns (Gen::in_integrand)
  for (size_t k = 1; k < m.sub.size(); k++) for (const Node& nd : m.sub[k].nodes) if (nd.op == GFH_X || nd.op == GFH_AUX) lane_stash = true;
  s << "\ntypedef long long i64;\n// kernels raise the status word with an agent-scope atomic: visible to whichever workgroup posts it to the host\n#define GFH_RAISE(p, v) __hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)\n"
       "#define GFH_STATUS_SLOT(st) ((st) == 0 ? 0.0 : (st) == 1 ? 1.0 : (st) == 2 ? 4096.0 : 16777216.0)\n";
  if (lane_stash)
    s << "// what an integrand takes from the enclosing eval() without passing it through pars(:): the lane's abscissa and its auxiliary\n"
         "// columns, left here by the point functions (same thread writes and reads: program order)\n"
         "__shared__ double gfh_lane_x[512];\n__shared__ const double* gfh_lane_axp[512];\n__shared__ i64 gfh_lane_lda;\n"
         "#define GFH_LANE_STASH gfh_lane_x[threadIdx.x] = X; gfh_lane_axp[threadIdx.x] = AXP; gfh_lane_lda = LDA;\n";
  else s << "#define GFH_LANE_STASH\n";
  s << kParsBlock;                  // pars_block.hip: GFH_PARS_DECL / GFH_PARS_AT
}

// The macro groups the signatures of the point functions and of the kernels are written against: GFH_OCC, GFH_SLOT_*, GFH_MESH_*,
// GFH_ORDER_* / GFH_ORD, GFH_WSG_*.  The host builds its argument lists from the same facts (codegen.h, unit_takes_mesh_args).
void emit_signature_macros(Unit& u) {
  const Model& m = u.m; const GenConfig& cfg = u.cfg; std::ostringstream& s = u.s;
  // register cap of the plain kernels (GenConfig::waves_per_eu): models with integrate() are bound by VALU issue and want waves, not registers
  if (cfg.waves_per_eu > 0) s << "#define GFH_OCC __attribute__((amdgpu_waves_per_eu(" << cfg.waves_per_eu << ")))\n";
  else s << "#define GFH_OCC\n";
  // (the dispatchers of a branching model take the lane's slot as one more argument, for the report of an unseen turn)
  s << (m.branching() ? "#define GFH_SLOT_DECL , const i64 SLOT\n#define GFH_SLOT(i) , (i64)(i)\n#define GFH_SLOT_PASS , SLOT\n"
                      : "#define GFH_SLOT_DECL\n#define GFH_SLOT(i)\n#define GFH_SLOT_PASS\n");
  // Mesh hand-over (emit_integral_site, mesh_build): models with integrate() carry a per-lane record pointer and a mode
  // (0 none, 1 this pass records its bisections, 2 it replays recorded ones) from the kernels down to the call sites.
  if (u.mesh_on)
    s << "#define GFH_MESH_STRIDE " << kMeshRecord * mesh_sites(m) << "\n#define GFH_MESH_DECL , unsigned char* __restrict__ MESH, const int MESH_MODE\n"
         "#define GFH_MESH_PASS , MESH, MESH_MODE\n#define GFH_MESH_AT(i) , (mesh ? mesh + (i64)(i) * GFH_MESH_STRIDE : (unsigned char*)nullptr), mesh_mode\n"
         "#define GFH_MESH_NONE , (unsigned char*)nullptr, 0\n#define GFH_MESH_KPARAMS , unsigned char* __restrict__ mesh, const int mesh_mode\n";
  else
    s << "#define GFH_MESH_DECL\n#define GFH_MESH_PASS\n#define GFH_MESH_AT(i)\n#define GFH_MESH_NONE\n#define GFH_MESH_KPARAMS\n";
  // Order of dispatch (launch.cpp, build_orders): the cost of a point of a model with integrate() is the number of its bisections,
  // workgroups are dispatched in index order, and x-sorted data put the expensive tiles last -- they would run alone at the end.  The
  // plain kernels of such models take the tile / block a workgroup works on from a table sorted by measured cost, expensive first;
  // the sweep measures (shader clock per tile).  Which workgroup does a tile changes no result: every sum is defined on the fixed
  // partition.
  if (u.mesh_on)         // (the same kernels that take the mesh arguments: the host passes both groups or neither)
    s << "#define GFH_HAS_ORDER 1\n#define GFH_ORDER_KPARAMS , const int* __restrict__ order, int* __restrict__ cost\n#define GFH_ORD(b) (order ? order[b] : (int)(b))\n";
  else
    s << "#define GFH_HAS_ORDER 0\n#define GFH_ORDER_KPARAMS\n#define GFH_ORD(b) ((int)(b))\n";
  // (kernels whose quadrature workspaces are the global pool take its address as their last argument and post it in LDS)
  if (m.has_integrals() && cfg.ws_global)
    s << "#define GFH_WSG_KPARAMS , double* __restrict__ wsg\n#define GFH_WSG_INIT if (threadIdx.x == 0) gfh_wsg_base = wsg; __syncthreads();\n";
  else
    s << "#define GFH_WSG 0\n#define GFH_WSG_KPARAMS\n#define GFH_WSG_INIT\n";
}

// One point function with a body of its own: tape t unrolled in the function's mode.
void emit_point_fn(Unit& u, const PointFn& f, const SubTape& t, const std::string& sfx, const std::string& slot) {
  std::ostringstream& s = u.s;
  s << "\n" << f.comment << point_head(f, sfx, slot) << "  GFH_LANE_STASH\n";
  Gen g(u.m, t, u.cfg.fast_div); g.mode = f.mode; g.mesh_top = u.mesh_on; g.analyse(f.mode == 0 ? u.none : u.pa);
  if (f.mode == 2) g.emit_forward_all(); else g.emit_values();
  if (f.reverse) g.emit_reverse();
  s << g.o.str();
  if (f.mode == 1) s << "  F = " << g.v(t.result) << ";\n";
  // adjoint source per active parameter: every PARAM node of that parameter
  for (int j = 0; f.reverse && j < u.NA; j++) {
    std::string e;
    for (int k = 0; k < (int)t.nodes.size(); k++)
      if (t.nodes[k].op == GFH_PARAM && t.nodes[k].a == u.active[j] && g.act[k]) e += (e.empty() ? "" : " + ") + g.b(k);
    s << "  G[" << j << "] = " << (e.empty() ? std::string("0.0") : e) << ";\n";
  }
  if (f.mode == 0) s << "  return " << g.v(t.result) << ";\n";
  if (f.mode == 2) s << "  return " << (g.act[t.result] ? g.dd(t.result) : std::string("0.0")) << ";\n";
  s << "}\n";
}

// A point function under its plain name.  A model with ONE recorded path and no comparison gets the body itself; a branching model
// (Model::branching) gets it once per variant (suffix _v<k>) and a dispatcher that takes the lane's slot as one more argument.
void emit_variant_bodies(Unit& u, std::initializer_list<const PointFn*> fns) {
  for (int v = 0; v < u.m.n_variants(); v++) for (const PointFn* f : fns) emit_point_fn(u, *f, u.m.eval(v), "_v" + std::to_string(v), "");
  for (const PointFn* f : fns) emit_dispatcher(*f, u.m.n_variants(), u.s);
}

// gfh_point_grad and gfh_point_dd of use_ad = .false. (gadfit.F90:684-687, 721-726): every parameter passive, the gradient by forward
// differences (fitfunction.F90:155-174) and the second directional derivative by a central difference (188-203); the
// value body is inlined once per evaluation the reference makes (it re-evaluates f(p); the value is the same).
// (A branching model takes its branch afresh in each of those evaluations, as the reference's eval() does.)
void emit_finite_difference_fns(Unit& u) {
  const Model& m = u.m; const GenConfig& cfg = u.cfg; const std::vector<int32_t>& active = u.active; const int NA = u.NA; std::ostringstream& s = u.s;
  s << R"(
// One data point, finite differences (grad_finite, fitfunction.F90:155-174): step = sqrt(epsilon)*p, taken as
// (p + step) - p; G[a] = (f(p + step e_a) - f(p)) / step.
)" << point_head(kPointGrad, "", " GFH_SLOT_DECL") << R"(  double Q[GFH_NP];
#pragma unroll
  for (int k = 0; k < GFH_NP; k++) Q[k] = P[k];
  F = gfh_point_value(X, Q, STATUS, AXP, LDA GFH_MESH_PASS GFH_SLOT_PASS);
)";
  for (int j = 0; j < NA; j++) {
    const int pj = active[j];
    // (fd_col_sets: the per-point columns of this evaluation are those the host tabulated at p + step e_j -- set 1 + j)
    const std::string axp = cfg.fd_col_sets && m.n_aux > 0 ? "AXP + (i64)" + std::to_string((j + 1) * m.n_aux) + " * LDA" : "AXP";
    s << "  { const double saved = Q[" << pj << "]; double step = 0x1p-26 * saved; Q[" << pj << "] = saved + step; step = Q[" << pj
      << "] - saved;\n    const double fp = gfh_point_value(X, Q, STATUS, " << axp << ", LDA GFH_MESH_PASS GFH_SLOT_PASS); Q[" << pj << "] = saved; G[" << j
      << "] = (fp - F) / step; }\n";
  }
  s << R"(}

// One data point, second directional derivative along DP by finite differences (dir_deriv_2nd_finite,
// fitfunction.F90:188-203): h = epsilon**(1/4); (f(p + h d) + f(p - h d) - 2 f(p)) / sqrt(epsilon).
)" << point_head(kPointDd, "", " GFH_SLOT_DECL") << R"(  double Q[GFH_NP];
#pragma unroll
  for (int k = 0; k < GFH_NP; k++) Q[k] = P[k];
)";
  for (int j = 0; j < NA; j++) s << "  Q[" << active[j] << "] = P[" << active[j] << "] + 0x1p-13 * DP[" << active[j] << "];\n";
  s << "  double y = gfh_point_value(X, Q, STATUS, AXP, LDA GFH_MESH_PASS GFH_SLOT_PASS);\n";
  for (int j = 0; j < NA; j++) s << "  Q[" << active[j] << "] = P[" << active[j] << "] - 0x1p-13 * DP[" << active[j] << "];\n";
  s << "  y = y + gfh_point_value(X, Q, STATUS, AXP, LDA GFH_MESH_PASS GFH_SLOT_PASS);\n";
  for (int j = 0; j < NA; j++) s << "  Q[" << active[j] << "] = P[" << active[j] << "];\n";
  s << "  y = y - 2.0 * gfh_point_value(X, Q, STATUS, AXP, LDA GFH_MESH_PASS GFH_SLOT_PASS);\n  return y / 0x1p-26;\n}\n";
}

// gfh_point_value, gfh_point_grad and gfh_point_dd: what gfh_k_sweep, gfh_k_chi2 and gfh_k_omega call per data point
void emit_point_functions(Unit& u) {
  const SubTape& st = u.m.sub[0];
  const char* slot = " GFH_SLOT_DECL";
  if (u.cfg.finite_diff) {
    if (u.m.branching()) emit_variant_bodies(u, {&kPointValue}); else emit_point_fn(u, kPointValue, st, "", slot);
    emit_finite_difference_fns(u);
  } else if (u.m.branching()) emit_variant_bodies(u, {&kPointValue, &kPointGrad, &kPointDd});
  else { emit_point_fn(u, kPointGrad, st, "", slot); emit_point_fn(u, kPointValue, st, "", slot); emit_point_fn(u, kPointDd, st, "", slot); }
}

// gfh_point_dd_grad, what gfh_k_omega_jt calls per data point
void emit_dd_grad_function(Unit& u) {
  if (u.m.branching()) emit_variant_bodies(u, {&kPointDdGrad}); else emit_point_fn(u, kPointDdGrad, u.m.sub[0], "", " GFH_SLOT_DECL");
}

}  // namespace

// The translation unit, top to bottom.
bool generate_source(const Model& m, const std::vector<int32_t>& active, const GenConfig& cfg,
                     std::string* src, std::string* err) {
  if (!check_arguments(m, active, err)) return false;
  Unit u(m, active, cfg);
  emit_option_defines(u);
  emit_prelude(u);
  if (m.has_integrals() && !emit_quadrature(m, cfg, u.s, err)) return false;
  emit_signature_macros(u);
  if (m.branching() && !emit_selector(m, u.s, err)) return false;
  emit_point_functions(u);
  if (cfg.eval) {                   // eval.hip: the curves of a plain fit stand alone behind the point functions
    if (m.has_integrals()) { *err = "eval kernels: models with integrate() are not carried"; return false; }
    if (u.NA < 1) { *err = "eval kernels: at least one active parameter"; return false; }
    u.s << "\n#define GFH_EVAL 1\n#define GFH_EVAL_GRID " << (!m.branching() && m.n_aux == 0 ? 1 : 0) << "\n" << kEval;
    *src = u.s.str();
    return true;
  }
  // ---- the hand-written kernels, in this order (the model body above is the only generated part)
  u.s << kSweep << kWaveSum << kFusedSweepGram << kChi2 << kOmega;
  if (unit_carries_omega_jt(m, cfg, u.NA)) {
    emit_dd_grad_function(u);
    u.s << kOmegaJt;                // omega_jt.hip: gfh_k_omega_jt
  }
  if (cfg.batch && !emit_batch_kernels(m, active, cfg, u.s, err)) return false;
  *src = u.s.str();
  return true;
}

}  // namespace gfh
