// device_text.h -- the hand-written device source of the generated translation units: each file of device/ as a
// NUL-terminated string, byte for byte (device_text.cpp embeds them at compile time; the library reads no file at run time).
#pragma once

namespace gfh {

extern const char kExp[];              // exp.hip: gfh_exp
extern const char kPowLn[];            // pow_ln.hip: gfh_pow_ln (models with x ** a, GFH_FAST_DIV)
extern const char kParsBlock[];        // pars_block.hip: the parameter block as kernel argument or device array
extern const char kUnseen[];           // unseen.hip: struct gfh_unseen, gfh_report_unseen (branching models; behind GFH_UNSEEN_CAP, unseen_report.h)
extern const char kSweep[];            // sweep.hip: layout, GFH_ROBUST, gfh_store64, gfh_k_sweep, the hand-off macros
extern const char kWaveSum[];          // wave_sum.hip: gfh_row_down, gfh_wave_sum (gram.hip and jtv.hip include the same file)
extern const char kFusedSweepGram[];   // fused_sweep_gram.hip: the fused STEP 1 + STEP 2 kernel in all its forms
extern const char kChi2[];             // chi2.hip: gfh_k_chi2
extern const char kOmega[];            // omega.hip: the tangent block of STEP 3, gfh_k_omega
extern const char kOmegaJt[];          // omega_jt.hip: gfh_k_omega_jt
extern const char kBatchWgSum[];       // batch_wg_sum.hip: gfh_b_sum_n, the cross-wave reducer of the 256-lane form of the batch kernels
extern const char kBatchCube[];        // batch_cube.hip: the data form and the load of the cube forms of the batch kernels (gfh_set_batch_cube)
extern const char kBatchFit[];         // batch_fit.hip: what the loops of the batch kernels share -- the data form, the three passes of a fit, the damped solve
extern const char kBatchFitKernels[];  // batch_fit_kernels.hip: gfh_k_fit_batch, gfh_k_batch_pass (behind batch_fit.hip: the two are the one text they were)
extern const char kBatchFitBounded[];  // batch_fit_bounded.hip: gfh_k_fit_batch_bounded, the loop inside a box -- in the bounded unit alone
extern const char kBatchCov[];         // batch_cov.hip: gfh_k_batch_cov, each fit's parameter covariance and standard errors
extern const char kBatchEval[];        // batch_eval.hip: gfh_k_batch_eval, the fitted curves, residuals and error bands of a range of fits
extern const char kEval[];             // eval.hip: gfh_k_eval and its three neighbours, the curves of a plain fit (units of GenConfig::eval alone)

}  // namespace gfh
