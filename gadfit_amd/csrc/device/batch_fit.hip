
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
#if GFH_BLOSS
// The loss of a batch (GenConfig::batch_loss, gfh_set_batch_loss; DESIGN section 3a, Losses of a batch).  The lines between
// `#if GFH_BLOSS`, `#else  // GFH_BLOSS` and `#endif  // GFH_BLOSS` are chosen by the GENERATOR (codegen.cpp, resolve_batch_loss), not by the
// preprocessor: a linear-loss unit holds the #else arms alone and is byte for byte the text it was before a batch had a loss.
// sqrt(rho'(u^2)) of the reference's costs (lm_solver.cpp:255-284) at u = r / c, r = (y - f) w the weighted residual and inv_c = 1 / c
// the kernel argument: GFH_BLOSS 1 Cauchy, 2 Huber.  The sweep and the omega pass scale the residual and the Jacobian row by it as
// GFH_ROBUST (sweep.hip) does at c = 1; nothing is divided by c, and chi2() (gfh_b_chi2) stays the plain sum.  Where ls is 1.0 the
// two products change no bit.
static __device__ __forceinline__ double gfh_b_ls(const double r, const double inv_c) {
#pragma clang fp contract(off)
  const double u = r * inv_c;
#if GFH_BLOSS == 1
  return __builtin_sqrt(1.0 / (1.0 + u * u));
#else
  return u * u > 1.0 ? __builtin_sqrt(1.0 / __builtin_fabs(u)) : 1.0;
#endif
}
#endif  // GFH_BLOSS
#if GFH_BMLE
// The estimator of a batch (GenConfig::batch_estimator, gfh_set_batch_estimator; DESIGN section 3a, Estimator of a batch).  The lines
// between `#if GFH_BMLE`, `#else  // GFH_BMLE` and `#endif  // GFH_BMLE` are chosen by the GENERATOR as the loss's are (codegen.cpp,
// resolve_batch_loss), not by the preprocessor: a least-squares unit holds the #else arms alone and none of these lines.
// GFH_BMLE 1: the Poisson maximum-likelihood fit.  What the loop minimises is the deviance D = 2 sum [f - y + y ln(y / f)] over the
// points with w != 0 (the data form's weight is a mask here and nothing more), by Fisher scoring: the sweep's weight is
// m / sqrt(f(P)), m = (w != 0), so J^T J = sum g g^T / f and J^T r = sum g (y - f) / f, and the sweep's last sum and gfh_b_chi2 are D.
// One term of D: 2 f at y = 0; NaN where f <= 0, y < 0 or an operand is not finite (a NaN deviance is a rejected trial, and a fit that
// starts with one ends with reason 8); an exact +0.0 at a masked point and in the padding lanes, which re-read the last point with w = 0.
static __device__ __forceinline__ double gfh_b_dev(const double y, const double f, const double w) {
#pragma clang fp contract(off)
  const bool ok = f > 0.0 && f < __builtin_inf() && y >= 0.0 && y < __builtin_inf();
  const double t = y == 0.0 ? 2.0 * f : 2.0 * ((f - y) + y * log(y / f));
  return w != 0.0 ? (ok ? t : __builtin_nan("")) : 0.0;
}
#endif  // GFH_BMLE

#if GFH_BLOSS
// STEP 1 + 2 (gadfit.F90:675-699) of one fit under a loss: S = [J^T J upper triangle, packed | J^T r | sum r^2], J and the r of J^T r
// scaled by ls (lm_solver.cpp:303-317), the last entry the PLAIN sum r^2 (chi2() of lm_solver.cpp:513-529: what gfh_k_batch_pass
// returns and gfh_k_batch_cov scales by)
static __device__ __forceinline__ void gfh_b_sweep(const gfh_bdata& d, const double* __restrict__ P, int* status, double (&S)[GFH_BNACC], const double inv_c GFH_BIMG_DECL) {
#else  // GFH_BLOSS
// STEP 1 + 2 (gadfit.F90:675-699) of one fit: S = [J^T J upper triangle, packed | J^T r | sum r^2]
static __device__ __forceinline__ void gfh_b_sweep(const gfh_bdata& d, const double* __restrict__ P, int* status, double (&S)[GFH_BNACC] GFH_BIMG_DECL) {
#endif  // GFH_BLOSS
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
#if GFH_BLOSS
    const double r = (Yc - F) * Wc;                            // gadfit.F90:682-683
    double R, Wl;
    {
#pragma clang fp contract(off)
      const double ls = gfh_b_ls(r, inv_c);                    // lm_solver.cpp:303-317 (a per-lane select inside the point loop: no barrier here)
      R = r * ls; Wl = Wc * ls;
    }
#else  // GFH_BLOSS
#if GFH_BMLE
    double R, Wf;                                              // Fisher scoring: the pass at weights m / sqrt(f(P))
    {
#pragma clang fp contract(off)
      Wf = (Wc != 0.0 ? 1.0 : 0.0) / __builtin_sqrt(F);        // (a per-lane select and factor inside the point loop: no barrier here)
      R = (Yc - F) * Wf;                                       // gadfit.F90:682-683
    }
#else  // GFH_BMLE
    const double R = (Yc - F) * Wc;                            // gadfit.F90:682-683
#endif  // GFH_BMLE
#endif  // GFH_BLOSS
#pragma unroll
#if GFH_BLOSS
    for (int a = 0; a < GFH_NA; a++) G[a] = G[a] * Wl;         // gadfit.F90:689-690, lm_solver.cpp:303-317
#else  // GFH_BLOSS
#if GFH_BMLE
    for (int a = 0; a < GFH_NA; a++) G[a] = G[a] * Wf;         // gadfit.F90:689-690
#else  // GFH_BMLE
    for (int a = 0; a < GFH_NA; a++) G[a] = G[a] * Wc;         // gadfit.F90:689-690
#endif  // GFH_BMLE
#endif  // GFH_BLOSS
    int p = 0;
#pragma unroll
    for (int a = 0; a < GFH_NA; a++)
#pragma unroll
      for (int b = a; b < GFH_NA; b++, p++) av[p] += G[a] * G[b];      // gadfit.F90:697
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) av[GFH_BNP + a] += G[a] * R;      // gadfit.F90:698
#if GFH_BLOSS
    av[GFH_BNP + GFH_NA] += r * r;
#else  // GFH_BLOSS
#if GFH_BMLE
    av[GFH_BNP + GFH_NA] += gfh_b_dev(Yc, F, Wc);              // the deviance in the place of sum r^2
#else  // GFH_BMLE
    av[GFH_BNP + GFH_NA] += R * R;
#endif  // GFH_BMLE
#endif  // GFH_BLOSS
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
#if GFH_BMLE
    acc += gfh_b_dev(Yc, gfh_point_value(Xc, P, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i0 + d.lane)), Wc);   // the deviance in the place of chi2
#else  // GFH_BMLE
    const double r = (Yc - gfh_point_value(Xc, P, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i0 + d.lane))) * Wc;   // gadfit.F90:1024-1026
    acc += r * r;
#endif  // GFH_BMLE
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
#if GFH_BLOSS
// Under a loss omega stays unscaled and the recomputed row is the sweep's ls g w, ls from the residual at P (the sweep's parameters).
// gfh_point_dd_grad returns no value, so f comes from gfh_point_value: one more value evaluation per point and no point function of
// its own.  The compiler's figures decided that (Losses of a batch): a dd_grad that hands out its value keeps it
// live through the reverse sweep and cost the 8-active Cauchy unit a wave per SIMD that this form keeps.
static __device__ __forceinline__ void gfh_b_omega(const gfh_bdata& d, const double* __restrict__ P, const double* __restrict__ DP, int* status,
                                                   double (&JTo)[GFH_NA], const double inv_c GFH_BIMG_DECL) {
#else  // GFH_BLOSS
static __device__ __forceinline__ void gfh_b_omega(const gfh_bdata& d, const double* __restrict__ P, const double* __restrict__ DP, int* status,
                                                   double (&JTo)[GFH_NA] GFH_BIMG_DECL) {
#endif  // GFH_BLOSS
  double acc[GFH_NA], Xc, Yc, Wc;
#pragma unroll
  for (int a = 0; a < GFH_NA; a++) acc[a] = 0.0;
  GFH_BLOAD(Xc, Yc, Wc, d.b)
  for (i64 i0 = d.b; i0 < d.e; i0 += GFH_BLANES) {
    double Xn, Yn, Wn;
    GFH_BLOAD(Xn, Yn, Wn, i0 + GFH_BLANES < d.e ? i0 + GFH_BLANES : i0)
    double G[GFH_NA];
#if GFH_BLOSS
    double Wl;                                                 // (formed in front of dd_grad: fewer values live across the value's body)
    {
#pragma clang fp contract(off)
      const double r = (Yc - gfh_point_value(Xc, P, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i0 + d.lane))) * Wc;
      Wl = Wc * gfh_b_ls(r, inv_c);                            // (per-lane, inside the point loop: no barrier here)
    }
#endif  // GFH_BLOSS
    const double om = -gfh_point_dd_grad(Xc, P, DP, G, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i0 + d.lane)) * Wc;   // gadfit.F90:722-723
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) {
#if GFH_BLOSS
      const double j = G[a] * Wl;                              // gadfit.F90:689-690, lm_solver.cpp:303-317
#else  // GFH_BLOSS
      const double j = G[a] * Wc;                              // gadfit.F90:689-690
#endif  // GFH_BLOSS
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
