// codegen.h -- the generator's interface: its options, where the quadrature workspaces live, the fused kernel's geometry, and the
// facts about a translation unit that the host must know to launch its kernels.
#pragma once
#include "model.h"

namespace gfh {

// Options of the generated kernels (kept in the source text so the cache key sees them).
struct GenConfig {
  int block = 256;        // threads per workgroup of the plain sweep / chi2 / omega kernels = slots per tile
  bool fd_col_sets = false; // ... with the auxiliary columns in 1 + n_active sets (gfh_set_fd_column_sets): evaluation j of the forward differences reads set 1 + j
  bool finite_diff = false; // use_ad = .false.: gradient / second directional derivative by the reference's finite differences (fitfunction.F90:155-203)
  bool omega_jt = true;   // STEP 3 kernel that recomputes the Jacobian row instead of reading J (gfh_k_omega_jt)
  int kernarg_pars = 0;   // > 0: the parameter block (this many doubles) is a by-value kernel argument
  int ws_size = 100;      // per-lane quadrature workspace (intervals) per nesting level that is compiled in: the fast form carries 100; a
                          // pass that exhausts it is repeated with the user's size (Model::ws_size, reference default 1000) before the reference's error is raised
  int ws_size_inner = 100;
  bool ws_global = false; // the interval workspaces live in a pool in GLOBAL memory, [wave slot][level][interval][lo|hi|err|sum][64 lanes] (a
                          // wave's access to one field of one interval is one coalesced 512 B row), handed to the kernels as an argument, instead
                          // of per-lane scratch: every workspace too large for kScratchBudget bytes of scratch per lane (plan_workspaces)
  bool store_j = true;    // fused kernel writes the Jacobian to HBM (gfh_set_keep_jacobian).  Without the store a wave runs its AD phase at
                          // s_setprio 3 and its matrix phase at 0 (GFH_AD_PRIO).  The two waves of a SIMD share one FP64 pipe; the wave in its AD phase issues short
                          // instructions between the other wave's 64- and 17-cycle matrix instructions when it goes first: 0.327 -> 0.314 ms at the headline
                          // size (profiles/r04_nostore.md); the stored form (waves of a workgroup in phase, store-bound) does not move and is left alone
  bool store_res = true;  // chi2 kernel writes the residual vector (the reference's chi2() side effect, gadfit.F90:1024-1026)
  int loss = 0;           // robust cost (gfh_set_loss): 0 linear, 1 cauchy, 2 huber
  bool fast_div = true;   // share one reciprocal per denominator (<= 1 ulp from the reference's r/v)
  int waves_per_eu = 0;   // > 0: the plain sweep / chi2 / omega kernels are compiled for at least this many waves per SIMD (register cap)
  bool batch = false;     // four more kernels behind the point functions: gfh_k_fit_batch (a whole LM fit per wave), gfh_k_batch_pass, gfh_k_batch_cov, gfh_k_batch_eval
                          // (batch.cpp).  A translation unit of its own: the default one does not change by a byte
  int batch_lanes = 64;   // ... lanes per fit of those two (GFH_BLANES): 64, a wave per fit, 16, a DPP row per fit and four fits per wave,
                          // or 256, a workgroup per fit
  bool batch_cube = false; // ... their data is a cube (gfh_set_batch_cube): one shared grid, the samples in batch_y_type, the weight formed
                          // in the load by batch_error_type's rule (GFH_BCUBE, GFH_BYTYPE, GFH_BERR; batch_cube.hip).  Again translation
                          // units of their own: the ragged ones carry none of the three macros
  int batch_y_type = 0;   // 0 double, 1 float, 2 uint16_t
  int batch_error_type = 0; // gfh_init_weights' numbers: 0 NONE, 1 SQRT_Y, 2 PROPTO_Y, 3 INVERSE_Y, 4 USER (a plain load of w)
  bool batch_bounded = false; // ... the unit holds gfh_k_fit_batch_bounded (batch_fit_bounded.hip: the loop inside a box) INSTEAD of the four kernels:
                          // a translation unit of its own once more, so that the text of the four kernels' unit does not change by a byte
  int batch_loss = 0;     // ... the loss of a batch (gfh_set_batch_loss): 0 linear, 1 cauchy, 2 huber.  Non-zero: `#define GFH_BLOSS <n>` in front of the
                          // batch text, whose kernels then take inv_c = 1 / scale as one more argument; the scale is no part of the text.  The
                          // text of a linear unit does not change by a byte.  `loss` above (GFH_LOSS of the plain units) stays 0 in a batch unit
  int batch_estimator = 0; // ... what a batch minimises (gfh_set_batch_estimator): 0 the weighted sum of squares, 1 the Poisson deviance by Fisher
                          // scoring.  Non-zero: `#define GFH_BMLE 1` in front of the batch text and the GFH_BMLE arms of batch_fit.hip, chosen by the
                          // generator as the loss's are; refused together with batch_loss.  The text of a least-squares unit does not change by a byte
  bool eval = false;      // the curves of a plain fit (eval.cpp): behind the point functions stand gfh_k_eval / gfh_k_eval_band and, for models a
                          // grid carries, gfh_k_eval_grid / gfh_k_eval_grid_band (eval.hip) INSTEAD of the kernels of a fit.  A translation
                          // unit of its own once more: the default one does not change by a byte
};
// The band of gfh_eval is carried up to this many active parameters per dataset (the block of the covariance is n^2 doubles per
// dataset, read through the scalar cache, and the band's 2 (n^2 + n) operations are unrolled); beyond it a band is refused.
constexpr int kEvalBandMax = 64;

// Where the quadrature workspaces of a translation unit live (numerical_integration.F90:40-51, 128-134: the reference's are heap arrays
// of the user's size).  Up to kScratchBudget bytes per lane they are private scratch (the fast form: the user's sizes capped at `fast`
// intervals and at what the budget holds once the per-interval gradients the bisection carries are counted); anything larger is the
// global pool (GenConfig::ws_global), which the context allocates with hipMalloc and frees with itself -- private scratch of tens of
// KB per lane is reserved by the runtime for the whole device until the process ends, and two queues asking for it at once can end
// the process (HSA_STATUS_ERROR_OUT_OF_RESOURCES).  grown: a pass has exhausted the fast form, carry the user's sizes.
constexpr int kScratchBudget = 7936;      // 8 KB per lane less 256 B for the register spills of the bodies
struct WsPlan { int ws_size, ws_size_inner; bool global; };
WsPlan plan_workspaces(const Model& m, int fast, bool grown);
bool carries_gradients(int n_ipars, int ws, bool global);      // does the bisection of a call site keep its panels' gradients per interval?
// The global pool's row of one interval at nesting level 1 or 2: [lo|hi|err|sum] and, where the level's call sites carry their panels'
// gradients (round 5: the pool form as well -- up to kWsgCarryMax integrand parameters), one more field per parameter; x 64 lanes.
constexpr int kWsgCarryMax = 8;
int wsg_row_fields(const Model& m, int level);
inline long wsg_wave_doubles(const Model& m, int ws1, int ws2) {
  bool nested = false; for (const Integral& in : m.integrals) if (in.depth >= 2) nested = true;
  return 64L * wsg_row_fields(m, 1) * ws1 + (nested ? 64L * wsg_row_fields(m, 2) * ws2 : 0L);
}
inline bool nested_integrals(const Model& m) { for (const Integral& in : m.integrals) if (in.depth >= 2) return true; return false; }

// Mesh hand-over between passes at the same parameters (emit_quadrature.cpp, emit_integral_site): per data point and outermost
// integrate() call site one record of kMeshRecord bytes -- [0] the number of bisections (255: not recorded), [1..] which interval
// each bisection split.  mesh_sites: records per point the model's kernels use (0: none).
constexpr int kMeshRecord = 64, kMeshSitesMax = 4;
int mesh_sites(const Model& m);

// Up to this many active parameters the fused kernel forms J^T J / J^T r in per-lane VALU accumulators
// (n (n + 1) / 2 + n + 1 of them) instead of on the matrix cores (fused_sweep_gram.hip, GFH_K_SWEEP_GRAM).  Measured at N = 1e7: 8 parameters
// 0.166 ms against 0.179 ms with one matrix tile; 12 parameters 0.258 ms (252 VGPRs) against 0.188 ms: the boundary stays at 8.
constexpr int kValuGramMax = 8;
// ... and how many passes ahead that form loads its inputs: ONE.  Two (three rotating register sets) were built
// and measured in round 6 on the theory that two waves per SIMD leave too few bytes in flight: in-process A/B over six fresh contexts
// each, configs 2 and 3 -- 0.1496 / 0.0925 ms against 0.1498 / 0.0896 (profiles/r06_valu_form_ab.txt): nothing at 8 parameters, a
// loss at 7 (126 -> 136 VGPRs costs the fourth wave per SIMD).  What the short kernels had been losing was their epilogue.

// The fused STEP 1 + STEP 2 kernel exists for up to this many active parameters (8 tiles of 16); beyond it gfh_k_sweep writes J and
// k_gram_block forms the Gram image from it.  Up to 4 tiles every wave keeps all tile pairs of its own points; round 5 took 5 tiles
// that way on a half stage (21 accumulator tiles at 6 spilled 150-200 registers and lost to the two-kernel path: profiles/r05_fused_tiles.md);
// round 6: from 6 tiles on (81 ... 128 parameters) the waves of a workgroup share the tile pairs out and read each other's stages
// (GFH_COOP, codegen.cpp).
// gfh_k_omega_jt (STEP 3 without the stored Jacobian) stops at kOmegaJtMaxActive.
constexpr int kFusedMaxActive = 128, kFusedMaxActiveNoCoop = 80, kOmegaJtMaxActive = 64;
// Does the fused kernel's matrix path stage 32 points per wave (two half-passes) instead of 64?  Measured at 32 parameters
// (profiles/r05_halfstage.md): the half-passes themselves cost 18 % at equal occupancy (twice the stage-write instructions, a
// bubble at the half boundary) and the gradient that waits in registers keeps three waves per SIMD out of reach (55 spills at 168
// registers), so up to 4 tiles the full stage stays.  With 5 and 6 tiles four full stages do not fit the 160 KB of a CU: there
// the half stage is what makes the fused kernel possible at all (against a Jacobian written and read back: 4.6 x the traffic).
// (5 tiles stay with round 5's per-wave form: 0.76 against 0.89 ms at p = 80, N = 4e6 -- there the 15 accumulator tiles still fit and
// its diagonal tiles run as 4x4x4 blocks: profiles/r06_coop.md)
inline bool fused_coop(int n_active) { return n_active > kFusedMaxActiveNoCoop; }
inline bool fused_half_stage(int n_active) { return n_active > 64; }
// 5 tiles: ONE cross-wave reduction image per workgroup that the waves add into in order (the same order of additions as one
// image per wave, a quarter of the LDS), laid over the stages once they are dead.
inline bool fused_single_image(int n_active) { return !fused_coop(n_active) && n_active > 64; }
inline int fused_stage_stride(int n_active) { return fused_half_stage(n_active) ? 34 : 66; }
// LDS of one workgroup of the fused kernel's matrix path with fw waves (the generated source declares exactly this: GFH_LDS_DOUBLES)
inline long fused_lds_bytes_for(int n_active, int fw) {
  const long T = (n_active + 15) / 16, npair = T * (T + 1) / 2;
  const long stage = (16 * T + 1) * fused_stage_stride(n_active);
  const long img = npair * 256 + 16 * T + 1;                          // the workgroup's own sums, kept for the single-workgroup tail
  if (fused_coop(n_active)) return std::max(fw * stage, T * 64 + 8 + img) * 8;      // (the epilogue lies over the stages)
  if (fused_single_image(n_active)) return std::max(fw * stage, npair * 256 + fw * (T * 64 + 4) + img) * 8;
  const long red = npair * 256 + T * 64 + 4;                          // cross-wave reduction image, one per wave, shares the stages' buffer
  return fw * std::max(stage, red) * 8 + img * 8 + 64;
}
// Waves per workgroup of the fused kernel: 8 (one workgroup per CU at 32 parameters), fewer where 8 stages of
// [(16T+1) rows][stride] fp64 do not fit the 160 KB LDS.
inline int fused_waves_for(int n_active) {
  int fw = fused_coop(n_active) ? 4 : 8;      // (cooperative form: one wave per SIMD -- the gradient alone is 2 NA registers)
  while (fw > 1 && fused_lds_bytes_for(n_active, fw) > 160L * 1024) fw /= 2;
  return fw;
}
// Waves per workgroup of gfh_k_chi2 (GFH_CW of the generated source): the fused kernel's while that exists, 8 beyond it.  Its launch
// needs it, and so does k_gram_block, which adds sum r^2 in gfh_k_chi2's order.
inline int chi2_waves_for(int n_active) { return n_active <= kFusedMaxActive ? fused_waves_for(n_active) : 8; }

// ---- What the host must know about a translation unit to launch its kernels: each stated here once, used by the generator where it
// writes the text and by the host where it builds the argument list.
// Does the unit carry gfh_k_omega_jt (STEP 3 from a recomputed Jacobian row: no integrate(), no robust loss, AD)?
inline bool unit_carries_omega_jt(const Model& m, const GenConfig& cfg, int n_active) {
  return cfg.omega_jt && !cfg.finite_diff && !m.has_integrals() && cfg.loss == 0 && n_active <= kOmegaJtMaxActive;
}
// Do the unit's kernels take the mesh arguments and, with them, the order arguments (GFH_MESH_KPARAMS, GFH_ORDER_KPARAMS)?
inline bool unit_takes_mesh_args(const Model& m, const GenConfig& cfg) { return !cfg.finite_diff && mesh_sites(m) > 0; }

// Generates one HIP translation unit with three kernels for (model, active set):
//   gfh_k_sweep : residual + Jacobian columns (reverse mode, statically unrolled)
//   gfh_k_chi2  : residual only, all parameters passive, per-block sum of squares
//   gfh_k_omega : second directional derivative (forward mode val/d/dd)
bool generate_source(const Model& m, const std::vector<int32_t>& active, const GenConfig& cfg,
                     std::string* src, std::string* err);

}  // namespace gfh
