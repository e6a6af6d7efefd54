
// ---- Batched fits inside a box (GenConfig::batch_bounded; gfh_fit_batch_bounded): gfh_k_fit_batch (batch_fit_kernels.hip) with one box
// lower[j] <= p_act[j] <= upper[j] per batch, the same for every fit, in the order of the active set; -inf / +inf: no bound on that
// side.  A projected Levenberg-Marquardt loop with an active set, as MPFIT handles its limits.  A unit of its own behind batch_fit.hip:
// the text of the unbounded unit does not hold this file.  THE RULE (Bounds of a batch); everything not named
// here is gfh_k_fit_batch line for line:
//   1. Pinning.  After STEP 1+2, from the accepted parameters P and that sweep's J^T r (r = (y - f) w, so dchi2/dp_j = -2 J^T r_j):
//      active parameter j is PINNED for this iteration -- STEP 3 and every retrial of STEP 4 included -- when P_j == lower_j and
//      J^T r_j < 0, or P_j == upper_j and J^T r_j > 0: it sits on a wall and descent pushes through that wall.  Exact comparisons.
//   2. Solve.  Every solve of the iteration runs with the pinned rows and columns taken out (gfh_b_solve_pinned): their off-diagonal
//      entries and their right-hand side read as +0.0, their diagonal keeps S_jj + lambda DTD_j.  The factorisation and the
//      substitutions then perform the reduced system's operations on the reduced system's numbers -- every extra term is +-0.0 *
//      finite -- and delta_j = 0 exactly.  The DTD update, acc_ratio and the lambda logic are unchanged.
//   3. Projection.  Every trial point, P + delta1 + delta2 / 2 and the retrials old + delta1, is clamped per coordinate by two
//      selects (gfh_b_clamp); a NaN passes through and is rejected by new_chi2 < old_chi2 as it is without a box.
//   4. rel_error.  A coordinate whose accepted value sits on a bound does not hold the exit open; the others test |delta1_j / P_j|.
//   5. At the exit at_bound[f] gets bit j where the returned P_j == lower_j and bit 8 + j where it == upper_j.  The record is
//      gfh_batch_rec unchanged.
// With lower = -inf and upper = +inf everywhere no comparison above ever holds: pin is 0, every select takes the unbounded
// kernel's operand, and the fit returns gfh_k_fit_batch's bits.
struct gfh_batch_box { double lo[GFH_VALU_GRAM_MAX], hi[GFH_VALU_GRAM_MAX]; };
static_assert(GFH_VALU_GRAM_MAX <= 8, "at_bound: bit j lower, bit 8 + j upper");
// the pinned set as one value per fit: wave-uniform where the state is (the selects of the solve then test a scalar)
#if GFH_BLANES == 16
#define GFH_BPIN(v) (v)
#else
#define GFH_BPIN(v) __builtin_amdgcn_readfirstlane(v)
#endif
static __device__ __forceinline__ double gfh_b_clamp(const double v, const double lo, const double hi) { return v < lo ? lo : (v > hi ? hi : v); }
// gfh_b_solve (batch_fit.hip) operation for operation, the pinned rows and columns (bit j of pin) masked where S and rhs are read
static __device__ __forceinline__ bool gfh_b_solve_pinned(const double (&S)[GFH_BNACC], const double (&DTD)[GFH_NA], const double lambda,
                                                          const double (&rhs)[GFH_NA], const int pin, double (&out)[GFH_NA]) {
#pragma clang fp contract(off)
  double U[GFH_NA][GFH_NA];                                    // U[k][j], k <= j: column j of the upper factor
  bool ok = true;
#pragma unroll
  for (int j = 0; j < GFH_NA; j++) {
    double ajj = S[GFH_BIDX(j, j)] + lambda * DTD[j];
#pragma unroll
    for (int k = 0; k < j; k++) ajj -= U[k][j] * U[k][j];
    ok = ok && ajj > 0.0 && ajj < __builtin_inf();
    ajj = __builtin_sqrt(ajj); U[j][j] = ajj;
    const double rinv = 1.0 / ajj;
#pragma unroll
    for (int c = j + 1; c < GFH_NA; c++) {
      double t = (((pin >> j) | (pin >> c)) & 1 ? 0.0 : S[GFH_BIDX(j, c)]) + 0.0;
#pragma unroll
      for (int k = 0; k < j; k++) t -= U[k][j] * U[k][c];
      U[j][c] = t * rinv;
    }
  }
  if (!ok) return false;
#pragma unroll
  for (int i = 0; i < GFH_NA; i++) {
    double t = (pin >> i) & 1 ? 0.0 : rhs[i];
#pragma unroll
    for (int k = 0; k < i; k++) t -= U[k][i] * out[k];
    out[i] = t / U[i][i];
  }
#pragma unroll
  for (int k = GFH_NA - 1; k >= 0; k--) if (out[k] != 0.0) {
    out[k] /= U[k][k];
#pragma unroll
    for (int i = 0; i < k; i++) out[i] -= out[k] * U[i][k];
  }
#pragma unroll
  for (int i = 0; i < GFH_NA; i++) out[i] = gfh_uni(out[i]);
  return true;
}

// BARRIER INVARIANT (GFH_BLANES 256), continued from gfh_k_fit_batch: the calls that hold a barrier and the branches around them are
// that kernel's, and what is new encloses none.  Line by line: `pin` is computed by selects from P (S), J^T r (S) and box (K), and
// made wave-uniform from lane 0, whose bits are every lane's; gfh_b_solve_pinned's selects on pin (S) sit inside the solve, which
// holds no barrier, and its ok is (S) as gfh_b_solve's; gfh_b_clamp selects among P + delta (S) and box (K), so the trial points
// that gfh_b_chi2 is called at, and new_chi2 < old_chi2 behind it, stay (S); the rel_error exit tests P (S) against box (K);
// at_bound is written behind the loop under d.lane == 0, which encloses no barrier.  No per-lane value enters any of them.
#if GFH_BMLE
// Under the Poisson estimator (GFH_BMLE) rule 1 pins on the sign of the sweep's J^T r = sum g (y - f) / f, minus half the gradient of
// the deviance, and everything else is the rule unchanged; the start with a NaN deviance ends with reason 8 as in gfh_k_fit_batch.
#endif  // GFH_BMLE
#if GFH_BLOSS
// Under a loss (GFH_BLOSS) rule 1 pins on the sign of the sweep's loss-scaled J^T r -- the gradient of the cost the step descends --
// and everything else is the rule unchanged.  inv_c (K) reaches only the point loops of gfh_b_sweep and gfh_b_omega, which hold no barrier.
extern "C" __global__ __launch_bounds__(256)
void gfh_k_fit_batch_bounded(GFH_BARGS, double* __restrict__ pars, const gfh_batch_opts o, const gfh_batch_box box,
                             gfh_batch_rec* __restrict__ recs, int* __restrict__ at_bound, const i64 n_fits, const double inv_c, int* __restrict__ status) {
#else  // GFH_BLOSS
extern "C" __global__ __launch_bounds__(256)
void gfh_k_fit_batch_bounded(GFH_BARGS, double* __restrict__ pars, const gfh_batch_opts o, const gfh_batch_box box,
                             gfh_batch_rec* __restrict__ recs, int* __restrict__ at_bound, const i64 n_fits, int* __restrict__ status) {
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
  if (!(old_chi2 == old_chi2)) exit_reason = 8;      // the first deviance is NaN: as gfh_k_fit_batch
  else
#endif  // GFH_BMLE
  for (;;) {
#if GFH_BLOSS
    gfh_b_sweep(d, P, status, S, inv_c GFH_BIMG);                                              // STEP 1 + 2, gadfit.F90:675-701
#else  // GFH_BLOSS
    gfh_b_sweep(d, P, status, S GFH_BIMG);                                                     // STEP 1 + 2, gadfit.F90:675-701
#endif  // GFH_BLOSS
    n_sweeps++;
    int pin = 0;
#pragma unroll
    for (int j = 0; j < GFH_NA; j++) {                                                        // gadfit.F90:702-710
      const double dj = S[GFH_BIDX(j, j)];
      DTD[j] = o.damp_plain ? dj : (DTD[j] > dj ? DTD[j] : dj);
      JTr[j] = S[GFH_BNP + j];
      const double pj = P[act[j]];                                                            // rule 1
      pin |= ((pj == box.lo[j] && JTr[j] < 0.0) || (pj == box.hi[j] && JTr[j] > 0.0)) ? 1 << j : 0;
    }
    pin = GFH_BPIN(pin);
    if (!gfh_b_solve_pinned(S, DTD, lambda, JTr, pin, delta1)) { exit_reason = 8; break; }    // gadfit.F90:711-713, rule 2
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
      if (!gfh_b_solve_pinned(S, DTD, lambda, JTo, pin, delta2)) { exit_reason = 8; break; }  // gadfit.F90:736-738 (the same matrix: the same factor)
      const double acc_ratio = __builtin_sqrt(gfh_b_dtd(delta2, DTD, delta2) / gfh_b_dtd(delta1, DTD, delta1));
      if (acc_ratio > o.accth) {
#pragma unroll
        for (int j = 0; j < GFH_NA; j++) delta2[j] = 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < GFH_NA; j++) P[act[j]] = gfh_b_clamp(P[act[j]] + delta1[j] + 0.5 * delta2[j], box.lo[j], box.hi[j]);    // gadfit.F90:745-750, rule 3
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
        if (!gfh_b_solve_pinned(S, DTD, lambda, JTr, pin, delta1)) { exit_reason = 8; quit = true; break; }
#pragma unroll
        for (int j = 0; j < GFH_NA; j++) P[act[j]] = gfh_b_clamp(P[act[j]] + delta1[j], box.lo[j], box.hi[j]);
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
    if (o.has_rel_error) {                                                                    // gadfit.F90:885-898, rule 4
      bool all = true;
#pragma unroll
      for (int j = 0; j < GFH_NA; j++) {
        const double pj = P[act[j]];
        all = all && (pj == box.lo[j] || pj == box.hi[j] || !(__builtin_fabs(delta1[j] / pj) > o.rel_error));
      }
      if (all) { exit_reason = 5; break; }
    }
    if (o.has_max_iter && iterations >= o.max_iter) { exit_reason = 0; break; }              // gadfit.F90:911-915
  }
  if (d.lane == 0) {
    int at = 0;                                                                               // rule 5
#pragma unroll
    for (int j = 0; j < GFH_NA; j++) {
      const double pj = P[act[j]];
      pars[f * GFH_NP + act[j]] = pj;
      at |= (pj == box.lo[j] ? 1 << j : 0) | (pj == box.hi[j] ? 1 << (8 + j) : 0);
    }
    at_bound[f] = at;
    gfh_batch_rec r;
    r.iterations = iterations; r.exit_reason = exit_reason; r.n_sweeps = n_sweeps; r.n_chi2 = n_chi2; r.n_omega = n_omega;
    r.dof = dof_ == 0 ? 1 : (dof_ > 2147483647LL ? 2147483647 : (int)dof_);
    r.lambda = lambda; r.chi2 = old_chi2;
    recs[f] = r;
  }
}
