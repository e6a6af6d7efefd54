
// ---- Batched independent fits: MANY Levenberg-Marquardt fits of this model in one launch, GFH_BLANES lanes per fit from its first
// chi2 to its exit (gadfit.F90:670-915 restated per fit; lm.cpp gfh_fit is the host form of the same lines, lm_options.h the defaults of both).  256 threads whose fits
// never talk to each other: no atomics and, up to 64 lanes per fit, no LDS and no barrier; fit f = global thread index / GFH_BLANES.  Lane l of a fit takes points
// off[f] + l, + GFH_BLANES, ... of the fit's contiguous x, y, w (coalesced rows, no padding between fits); the lanes past the end of
// the last row re-read the fit's last point with w = 0.  STEP 1+2 is the per-lane outer product of the fused kernel's VALU form
// (GFH_NA <= GFH_VALU_GRAM_MAX) finished by gfh_b_sum, which leaves the same bits in every lane of the fit; every lane runs the damped
// solve and the lambda logic on them redundantly -- the same operations on the same numbers, so the same decisions -- which keeps the
// parameter block, the saved parameters and the normal equations in registers for the whole fit.
//   GFH_BLANES 64: a wave per fit, 4 fits per workgroup.  The sums come back as wave-uniform values (v_readfirstlane).
//   GFH_BLANES 16: a DPP row per fit, 4 fits per wave, 16 per workgroup -- for spectra of a few dozen points, where a wave per fit
//     keeps 48 lanes on w = 0.  The sums are reduced inside the row alone (gfh_b_sum below) and the state is per-lane, replicated
//     across the row; nothing crosses a row, so neighbouring fits of a wave do not see each other, and exits at different iterations
//     or spectra of different lengths inside a wave are ordinary divergence: a row is always wholly live or wholly gone.
//   GFH_BLANES 256: a workgroup per fit (fit f = blockIdx.x, grid = n_fits) -- for few, long spectra, where a wave per fit walks a
//     spectrum 64 points at a time on a quarter of the card.  A pass row is 256 points.  Each wave reduces its lanes' accumulators with
//     gfh_wave_sum as the wave form does; lane 0 of each wave writes the wave's partials to an LDS image [4][n], and after ONE workgroup
//     barrier every lane adds the four partials of each value in wave order, ((p0 + p1) + p2) + p3 (gfh_b_sum_n, batch_wg_sum.hip).  All four waves
//     then hold the same bits as wave-uniform values, and each runs the solve and the lambda logic redundantly, as every lane of a wave
//     does in the other forms.  Up to 64 points waves 1 ... 3 contribute exact +0.0 and the fit returns the wave form's bits.
//     What keeps the barriers matched is the BARRIER INVARIANT above gfh_k_fit_batch.
#define GFH_BNP (GFH_NA * (GFH_NA + 1) / 2)
#define GFH_BNACC (GFH_BNP + GFH_NA + 1)
#define GFH_BIDX(a, b) ((a) * GFH_NA - (a) * ((a) - 1) / 2 + ((b) - (a)))      // packed upper triangle, a <= b
struct gfh_batch_opts {          // the options of gfh_fit that the batch carries (batch.cpp fills it; absent values hold the reference's defaults)
  double lambda, lam_up, lam_down, accth, chi2_abs, chi2_rel, rel_error;
  double dtd_min[GFH_VALU_GRAM_MAX];
  int lam_incs, max_iter, has_max_iter, use_accth, has_chi2_abs, has_chi2_rel, has_rel_error, damp_plain;
};
struct gfh_batch_rec { int iterations, exit_reason, n_sweeps, n_chi2, n_omega, dof; double lambda, chi2; };

#if GFH_BLANES == 64
static __device__ __forceinline__ double gfh_uni(const double v) {      // lane 0's value as a wave-uniform one
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)b), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
static __device__ __forceinline__ double gfh_b_sum(const double t) { return gfh_uni(gfh_wave_sum(t)); }
#define GFH_BFIT(tid) ((i64)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)((tid) >> 6)))
#elif GFH_BLANES == 16
static __device__ __forceinline__ double gfh_uni(const double v) { return v; }      // the state is per-lane, replicated across the row
// lane l reads lane (l - N) mod 16 of its row of 16 (DPP row_ror:N): every lane has a source inside its own row
template <int N> static __device__ __forceinline__ double gfh_row_ror(const double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x120 | N, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x120 | N, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// the sum of a row in every lane of it: the rotation butterfly t_l += t_(l-8), (l-4), (l-2), (l-1) (indices mod 16).  After the
// level of distance d the values have period d in l (a + b and b + a are the same bits), so every lane ends with the same bits, and
// lane 0's are those of the row levels of gfh_wave_sum (wave_sum.hip) with some operands commuted.  gfx9 has no row_share to
// broadcast with, and v_readlane / ds_bpermute would cross rows.
static __device__ __forceinline__ double gfh_b_sum(double t) {
  t += gfh_row_ror<8>(t); t += gfh_row_ror<4>(t); t += gfh_row_ror<2>(t); t += gfh_row_ror<1>(t);
  return t;
}
#define GFH_BFIT(tid) ((i64)blockIdx.x * 16 + (i64)((tid) >> 4))
#elif GFH_BLANES == 256
// gfh_uni and the cross-wave reducer gfh_b_sum_n (LDS, one barrier) are batch_wg_sum.hip, emitted in front of this file in this form
// alone: the text of the other forms holds no LDS and no barrier
#define GFH_BFIT(tid) ((i64)blockIdx.x)
#else
#error "GFH_BLANES: 64 (a wave per fit), 16 (a DPP row per fit) or 256 (a workgroup per fit)"
#endif
// `img`, the LDS image of the next reduction, travels from the kernel to the three reducers in the workgroup form alone
#if GFH_BLANES == 256
static_assert(GFH_BWG_NACC == GFH_BNACC, "batch_wg_sum.hip sizes its LDS images for the sweep's accumulators");
#define GFH_BIMG_DECL , int& img
#define GFH_BIMG , lds_img
#define GFH_BIMG_INIT int lds_img = 0;
#else
#define GFH_BIMG_DECL
#define GFH_BIMG
#define GFH_BIMG_INIT
#endif
// The data form: a fit's points (gfh_bdata), the four data arguments of the two kernels (GFH_BARGS), a fit's gfh_bdata from them
// (GFH_BDATA) and the load (GFH_BLOAD), through which ALL point access goes.  Here the ragged form of gfh_set_batch_data: x, y, w
// back to back as doubles, fit f owns [off[f], off[f + 1]).  The cube forms (GFH_BCUBE, gfh_set_batch_cube) bring their own four in
// batch_cube.hip, emitted in front of this file: one shared grid, narrow samples, the weight formed in the load.
#ifndef GFH_BCUBE
struct gfh_bdata { const double* __restrict__ x; const double* __restrict__ y; const double* __restrict__ w; i64 b, e; int lane; };
#define GFH_BARGS const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ w, const i64* __restrict__ off
#define GFH_BDATA(f) {x, y, w, off[f], off[f + 1], (int)(threadIdx.x & (GFH_BLANES - 1))}
// the inputs of pass row i0 (uniform in the fit) for this lane; past the end: the last point with w = 0
#define GFH_BLOAD(X, Y, W, i0) { const i64 i_ = (i0) + d.lane; const i64 c_ = i_ < d.e ? i_ : d.e - 1; \
  X = d.x[c_]; Y = d.y[c_]; const double w_ = d.w[c_]; W = i_ < d.e ? w_ : 0.0; }
#endif

// STEP 1 + 2 (gadfit.F90:675-699) of one fit: S = [J^T J upper triangle, packed | J^T r | sum r^2]
static __device__ __forceinline__ void gfh_b_sweep(const gfh_bdata& d, const double* __restrict__ P, int* status, double (&S)[GFH_BNACC] GFH_BIMG_DECL) {
  double av[GFH_BNACC];
#pragma unroll
  for (int k = 0; k < GFH_BNACC; k++) av[k] = 0.0;
  double Xc, Yc, Wc;
  GFH_BLOAD(Xc, Yc, Wc, d.b)
  for (i64 i0 = d.b; i0 < d.e; i0 += GFH_BLANES) {
    double Xn, Yn, Wn;
    GFH_BLOAD(Xn, Yn, Wn, i0 + GFH_BLANES < d.e ? i0 + GFH_BLANES : i0)       // next row's inputs (the last row re-reads its own)
    double F, G[GFH_NA];
    gfh_point_grad(Xc, P, F, G, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i0 + d.lane));
    const double R = (Yc - F) * Wc;                            // gadfit.F90:682-683
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) G[a] = G[a] * Wc;         // gadfit.F90:689-690
    int p = 0;
#pragma unroll
    for (int a = 0; a < GFH_NA; a++)
#pragma unroll
      for (int b = a; b < GFH_NA; b++, p++) av[p] += G[a] * G[b];      // gadfit.F90:697
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) av[GFH_BNP + a] += G[a] * R;      // gadfit.F90:698
    av[GFH_BNP + GFH_NA] += R * R;
    Xc = Xn; Yc = Yn; Wc = Wn;
  }
#if GFH_BLANES == 256
  gfh_b_sum_n(av, S, img);
#else
#pragma unroll
  for (int k = 0; k < GFH_BNACC; k++) S[k] = gfh_b_sum(av[k]);
#endif
}
// chi2() (gadfit.F90:1015-1034): every parameter passive, value only
static __device__ __forceinline__ double gfh_b_chi2(const gfh_bdata& d, const double* __restrict__ P, int* status GFH_BIMG_DECL) {
  double acc = 0.0, Xc, Yc, Wc;
  GFH_BLOAD(Xc, Yc, Wc, d.b)
  for (i64 i0 = d.b; i0 < d.e; i0 += GFH_BLANES) {
    double Xn, Yn, Wn;
    GFH_BLOAD(Xn, Yn, Wn, i0 + GFH_BLANES < d.e ? i0 + GFH_BLANES : i0)
    const double r = (Yc - gfh_point_value(Xc, P, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i0 + d.lane))) * Wc;   // gadfit.F90:1024-1026
    acc += r * r;
    Xc = Xn; Yc = Yn; Wc = Wn;
  }
#if GFH_BLANES == 256
  const double part[1] = {acc};
  double sum[1];
  gfh_b_sum_n(part, sum, img);
  return sum[0];
#else
  return gfh_b_sum(acc);
#endif
}
// STEP 3 (gadfit.F90:715-735): omega_i = -f''_delta1(x_i) w_i and J^T omega with the Jacobian row recomputed, as gfh_k_omega_jt
static __device__ __forceinline__ void gfh_b_omega(const gfh_bdata& d, const double* __restrict__ P, const double* __restrict__ DP, int* status,
                                                   double (&JTo)[GFH_NA] GFH_BIMG_DECL) {
  double acc[GFH_NA], Xc, Yc, Wc;
#pragma unroll
  for (int a = 0; a < GFH_NA; a++) acc[a] = 0.0;
  GFH_BLOAD(Xc, Yc, Wc, d.b)
  for (i64 i0 = d.b; i0 < d.e; i0 += GFH_BLANES) {
    double Xn, Yn, Wn;
    GFH_BLOAD(Xn, Yn, Wn, i0 + GFH_BLANES < d.e ? i0 + GFH_BLANES : i0)
    double G[GFH_NA];
    const double om = -gfh_point_dd_grad(Xc, P, DP, G, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i0 + d.lane)) * Wc;   // gadfit.F90:722-723
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) {
      const double j = G[a] * Wc;                              // gadfit.F90:689-690
      acc[a] += j * om;                                        // gadfit.F90:734
    }
    Xc = Xn; Yc = Yn; Wc = Wn;
  }
  (void)Yc;
#if GFH_BLANES == 256
  gfh_b_sum_n(acc, JTo, img);
#else
#pragma unroll
  for (int a = 0; a < GFH_NA; a++) JTo[a] = gfh_b_sum(acc[a]);
#endif
}
// (J^T J + lambda DTD) out = rhs (gadfit.F90:711-713): potrf_upper_plain and potrs_upper of normal_eq.cpp operation for operation,
// unrolled, without contraction (the host has none), so that this solve and the host's return the same bits from the same
// sums.  false: a pivot that is not positive, or -- the one test the host's '!(ajj > 0.0)' does not make -- not finite: this fit's
// normal equations are not positive definite.
static __device__ __forceinline__ bool gfh_b_solve(const double (&S)[GFH_BNACC], const double (&DTD)[GFH_NA], const double lambda,
                                                   const double (&rhs)[GFH_NA], double (&out)[GFH_NA]) {
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
      double t = S[GFH_BIDX(j, c)] + 0.0;
#pragma unroll
      for (int k = 0; k < j; k++) t -= U[k][j] * U[k][c];
      U[j][c] = t * rinv;
    }
  }
  if (!ok) return false;
#pragma unroll
  for (int i = 0; i < GFH_NA; i++) {
    double t = rhs[i];
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
static __device__ __forceinline__ double gfh_b_dtd(const double (&a)[GFH_NA], const double (&DTD)[GFH_NA], const double (&b)[GFH_NA]) {
#pragma clang fp contract(off)
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < GFH_NA; i++) t += a[i] * (DTD[i] * b[i]);       // dot(a, matmul(DTD, b)), DTD diagonal
  return t;
}

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
extern "C" __global__ __launch_bounds__(256)
void gfh_k_fit_batch(GFH_BARGS, double* __restrict__ pars, const gfh_batch_opts o,
                     gfh_batch_rec* __restrict__ recs, const i64 n_fits, int* __restrict__ status) {
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
  for (;;) {
    gfh_b_sweep(d, P, status, S GFH_BIMG);                                                     // STEP 1 + 2, gadfit.F90:675-701
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
      gfh_b_omega(d, P, DP, status, JTo GFH_BIMG);
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
void gfh_k_batch_pass(GFH_BARGS, const double* __restrict__ pars, double* __restrict__ img,
                      const i64 n_fits, int* __restrict__ status) {
  const i64 f = GFH_BFIT(threadIdx.x);
  if (f >= n_fits) return;
  const gfh_bdata d = GFH_BDATA(f);
  double P[GFH_NP], S[GFH_BNACC];
#pragma unroll
  for (int k = 0; k < GFH_NP; k++) P[k] = gfh_uni(pars[f * GFH_NP + k]);
  GFH_BIMG_INIT
  gfh_b_sweep(d, P, status, S GFH_BIMG);      // (256 lanes per fit: one barrier, reached by all four waves -- the return above is per workgroup)
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
