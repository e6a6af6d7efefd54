
// The whole fit of each spectrum (gadfit.F90:670-915).  Exit reasons as gfh_fit_result (0 max_iter, 1 chi2_abs, 2 chi2_rel, 5 rel_error,
// 7 lambda raised lam_incs + 1 times in a row), and 8: the damped matrix was not positive definite -- that fit ends with the
// parameters of its last accepted step, its neighbours go on.  uphill is 0 in a batch, so the acceptance test of gadfit.F90:761 is
// new_chi2 < old_chi2 and old_delta1 (read only by its factor (1 - beta)**uphill) is not kept.
//
// BARRIER INVARIANT (GFH_BLANES 256; the other forms have no barrier).  The barriers are those of gfh_b_sum_n: one at the end of
// gfh_b_chi2, of gfh_b_sweep and of gfh_b_omega, none inside their point loops.  The four waves of the workgroup must make the same
// sequence of these calls, so every branch or loop that encloses one is decided only by
//   (K) kernel arguments (o.*, n_fits),
//   (O) the fit's off[f], off[f + 1] (d.b, d.e; f = blockIdx.x is the workgroup's; in a cube 0 and the kernel argument n_points: (K)), or
//   (S) values that came out of gfh_b_sum_n -- the same LDS words added in the same order in every lane -- or were computed from such
//       values and (K), (O) by the same instruction sequence under contract(off): S, DTD, JTr, delta1, delta2, lambda, P, old_pars,
//       the chi2 values and the iteration count.  No per-lane quantity (d.lane, x, y, w, the accumulators before the sum) and nothing
//       read back from global memory that another wave wrote (status is write-only here) enters them.
// Line by line: the f >= n_fits return is per workgroup (K); for (;;) is left by gfh_b_solve's ok (S), by STEP 4's quit (S) and by
// STEP 5's exits (K, O: dof, S); `if (o.use_accth)` is (K); the STEP 4 loop's bound is (K) and its three arms are chosen by new_chi2 <
// old_chi2 (S) and i <= o.lam_incs (K).  `lds_img` is toggled once per gfh_b_sum_n and nowhere else, so it is the same in the four waves.
// A NaN or Inf in a spectrum therefore ends the fit with reason 8 at the same solve in all four waves.  The branches on d.lane == 0
// and on the lane inside gfh_b_sum_n enclose no barrier.  Lane 0 of wave 0 writes the parameters and the record.
// The cube's load (batch_cube.hip) adds only per-lane values -- the sample converted to double and the weight formed from it -- and
// none of them enters a branch that encloses a barrier: its selects (the threshold of SQRT_Y / PROPTO_Y, the clamp) sit inside GFH_BLOAD.
#if GFH_BMLE
// Under the Poisson estimator (GFH_BMLE; batch_fit.hip, gfh_b_dev) the arm adds only per-lane selects (w != 0, y == 0, the NaN of a
// term that has no value) and per-lane factors (1 / sqrt(f), the log) inside the point loops of gfh_b_sweep and gfh_b_chi2, which hold
// no barrier; what leaves those loops still goes through gfh_b_sum_n, so S and the deviance stay (S) and no per-lane value enters a
// branch that encloses a barrier.  The one new branch, a fit that STARTS with a NaN deviance ends with reason 8 in front of the loop,
// tests old_chi2 (S): the four waves skip the loop together.
#endif  // GFH_BMLE
#if GFH_BLOSS
// Under a loss (GFH_BLOSS; batch_fit.hip, gfh_b_ls) the kernels take inv_c = 1 / scale (K) behind their own arguments.  The loss adds
// per-lane selects (Huber's u^2 > 1) and per-lane factors inside the point loops of gfh_b_sweep and gfh_b_omega, which hold no barrier;
// what comes out of them still goes through gfh_b_sum_n, so S and J^T omega stay (S) and no per-lane value enters a branch that encloses
// a barrier.  The acceptance test stays on the plain chi2 of gfh_b_chi2 (lm_solver.cpp:438-465), which the loss does not reach.
extern "C" __global__ __launch_bounds__(256)
void gfh_k_fit_batch(GFH_BARGS, double* __restrict__ pars, const gfh_batch_opts o,
                     gfh_batch_rec* __restrict__ recs, const i64 n_fits, const double inv_c, int* __restrict__ status) {
#else  // GFH_BLOSS
extern "C" __global__ __launch_bounds__(256)
void gfh_k_fit_batch(GFH_BARGS, double* __restrict__ pars, const gfh_batch_opts o,
                     gfh_batch_rec* __restrict__ recs, const i64 n_fits, int* __restrict__ status) {
#endif  // GFH_BLOSS
#pragma clang fp contract(off)
  const i64 f = GFH_BFIT(threadIdx.x);
  if (f >= n_fits) return;
  constexpr int act[GFH_NA] = GFH_BACT;
  const gfh_bdata d = GFH_BDATA(f);
  double P[GFH_NP], old_pars[GFH_NA], DTD[GFH_NA], delta1[GFH_NA], delta2[GFH_NA], S[GFH_BNACC], JTr[GFH_NA];
#pragma unroll
  for (int k = 0; k < GFH_NP; k++) P[k] = gfh_uni(pars[f * GFH_NP + k]);
#pragma unroll
  for (int j = 0; j < GFH_NA; j++) { DTD[j] = o.dtd_min[j]; old_pars[j] = P[act[j]]; delta2[j] = 0.0; }      // gadfit.F90:641-646
  const i64 dof_ = (d.e - d.b) - GFH_NA;                                                     // gadfit.F90:648-657
  const double dof = dof_ == 0 ? 1.0 : (double)dof_;
  double lambda = o.lambda;
  int iterations = 0, exit_reason = -1, n_sweeps = 0, n_chi2 = 0, n_omega = 0;
  GFH_BIMG_INIT
  double old_chi2 = gfh_b_chi2(d, P, status GFH_BIMG), new_chi2 = 0.0, old_old_chi2 = 0.0;             // gadfit.F90:670
  n_chi2++;
#if GFH_BMLE
  if (!(old_chi2 == old_chi2)) exit_reason = 8;      // the first deviance is NaN (f <= 0, y < 0 or not finite): nothing to descend from
  else
#endif  // GFH_BMLE
  for (;;) {
#if GFH_BLOSS
    gfh_b_sweep(d, P, status, S, inv_c GFH_BIMG);                                              // STEP 1 + 2, gadfit.F90:675-701
#else  // GFH_BLOSS
    gfh_b_sweep(d, P, status, S GFH_BIMG);                                                     // STEP 1 + 2, gadfit.F90:675-701
#endif  // GFH_BLOSS
    n_sweeps++;
#pragma unroll
    for (int j = 0; j < GFH_NA; j++) {                                                        // gadfit.F90:702-710
      const double dj = S[GFH_BIDX(j, j)];
      DTD[j] = o.damp_plain ? dj : (DTD[j] > dj ? DTD[j] : dj);
      JTr[j] = S[GFH_BNP + j];
    }
    if (!gfh_b_solve(S, DTD, lambda, JTr, delta1)) { exit_reason = 8; break; }                // gadfit.F90:711-713
    if (o.use_accth) {                                                                        // STEP 3, gadfit.F90:715-743
      double DP[GFH_NP], JTo[GFH_NA];
#pragma unroll
      for (int k = 0; k < GFH_NP; k++) DP[k] = 0.0;
#pragma unroll
      for (int j = 0; j < GFH_NA; j++) DP[act[j]] = delta1[j];
#if GFH_BLOSS
      gfh_b_omega(d, P, DP, status, JTo, inv_c GFH_BIMG);
#else  // GFH_BLOSS
      gfh_b_omega(d, P, DP, status, JTo GFH_BIMG);
#endif  // GFH_BLOSS
      n_omega++;
      if (!gfh_b_solve(S, DTD, lambda, JTo, delta2)) { exit_reason = 8; break; }              // gadfit.F90:736-738 (the same matrix: the same factor)
      const double acc_ratio = __builtin_sqrt(gfh_b_dtd(delta2, DTD, delta2) / gfh_b_dtd(delta1, DTD, delta1));
      if (acc_ratio > o.accth) {
#pragma unroll
        for (int j = 0; j < GFH_NA; j++) delta2[j] = 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < GFH_NA; j++) P[act[j]] = P[act[j]] + delta1[j] + 0.5 * delta2[j];    // gadfit.F90:745-750
    bool quit = false;
    for (int i = 1; i <= o.lam_incs + 1; i++) {                                               // STEP 4, gadfit.F90:752-819
      new_chi2 = gfh_b_chi2(d, P, status GFH_BIMG);
      n_chi2++;
      if (new_chi2 < old_chi2) {                                                              // gadfit.F90:761
        lambda = lambda / o.lam_down;                                                         // gadfit.F90:780-782
        break;
      } else if (i <= o.lam_incs) {                                                           // gadfit.F90:785-808
        lambda = o.lam_up * lambda;
#pragma unroll
        for (int j = 0; j < GFH_NA; j++) P[act[j]] = old_pars[j];
        if (!gfh_b_solve(S, DTD, lambda, JTr, delta1)) { exit_reason = 8; quit = true; break; }
#pragma unroll
        for (int j = 0; j < GFH_NA; j++) P[act[j]] += delta1[j];
      } else {                                                                                // gadfit.F90:809-816
#pragma unroll
        for (int j = 0; j < GFH_NA; j++) P[act[j]] = old_pars[j];
        exit_reason = 7; quit = true; break;
      }
    }
    if (quit) break;
#pragma unroll
    for (int j = 0; j < GFH_NA; j++) old_pars[j] = P[act[j]];                                 // gadfit.F90:821-827
    old_old_chi2 = old_chi2;
    old_chi2 = old_chi2 < new_chi2 ? old_chi2 : new_chi2;
    iterations++;
    // STEP 5 (gadfit.F90:835-915), in the reference's order
    if (o.has_chi2_abs && old_chi2 / dof < o.chi2_abs) { exit_reason = 1; break; }
    if (o.has_chi2_rel && (old_old_chi2 - old_chi2) / old_chi2 < o.chi2_rel) { exit_reason = 2; break; }
    if (o.has_rel_error) {                                                                    // gadfit.F90:885-898
      bool all = true;
#pragma unroll
      for (int j = 0; j < GFH_NA; j++) all = all && !(__builtin_fabs(delta1[j] / P[act[j]]) > o.rel_error);
      if (all) { exit_reason = 5; break; }
    }
    if (o.has_max_iter && iterations >= o.max_iter) { exit_reason = 0; break; }              // gadfit.F90:911-915
  }
  if (d.lane == 0) {
#pragma unroll
    for (int j = 0; j < GFH_NA; j++) pars[f * GFH_NP + act[j]] = P[act[j]];
    gfh_batch_rec r;
    r.iterations = iterations; r.exit_reason = exit_reason; r.n_sweeps = n_sweeps; r.n_chi2 = n_chi2; r.n_omega = n_omega;
    r.dof = dof_ == 0 ? 1 : (dof_ > 2147483647LL ? 2147483647 : (int)dof_);
    r.lambda = lambda; r.chi2 = old_chi2;
    recs[f] = r;
  }
}

// STEP 1 + 2 only, at given parameters: each fit's J^T J [na x na] (both triangles), J^T r [na] and chi2 -- the "one pass" of
// callers with their own loop.  img [n_fits][na * na + na + 1].
extern "C" __global__ __launch_bounds__(256)
#if GFH_BLOSS
void gfh_k_batch_pass(GFH_BARGS, const double* __restrict__ pars, double* __restrict__ img,
                      const i64 n_fits, const double inv_c, int* __restrict__ status) {
#else  // GFH_BLOSS
void gfh_k_batch_pass(GFH_BARGS, const double* __restrict__ pars, double* __restrict__ img,
                      const i64 n_fits, int* __restrict__ status) {
#endif  // GFH_BLOSS
  const i64 f = GFH_BFIT(threadIdx.x);
  if (f >= n_fits) return;
  const gfh_bdata d = GFH_BDATA(f);
  double P[GFH_NP], S[GFH_BNACC];
#pragma unroll
  for (int k = 0; k < GFH_NP; k++) P[k] = gfh_uni(pars[f * GFH_NP + k]);
  GFH_BIMG_INIT
#if GFH_BLOSS
  gfh_b_sweep(d, P, status, S, inv_c GFH_BIMG);      // (256 lanes per fit: one barrier, reached by all four waves -- the return above is per workgroup)
#else  // GFH_BLOSS
  gfh_b_sweep(d, P, status, S GFH_BIMG);      // (256 lanes per fit: one barrier, reached by all four waves -- the return above is per workgroup)
#endif  // GFH_BLOSS
  if (d.lane == 0) {
    double* __restrict__ out = img + f * (GFH_NA * GFH_NA + GFH_NA + 1);
#pragma unroll
    for (int a = 0; a < GFH_NA; a++)
#pragma unroll
      for (int b = 0; b < GFH_NA; b++) out[a * GFH_NA + b] = a <= b ? S[GFH_BIDX(a, b)] : S[GFH_BIDX(b, a)];
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) out[GFH_NA * GFH_NA + a] = S[GFH_BNP + a];
    out[GFH_NA * GFH_NA + GFH_NA] = S[GFH_BNP + GFH_NA];
  }
}
