
// ---- Errors of a batch: each fit's parameter covariance (J^T J)^-1 and standard errors at given parameters, behind batch_fit.hip in
// every batch translation unit and written once against GFH_BLANES like the two kernels there.  STEP 1 + 2 at the parameters
// (gfh_b_sweep: the same sums as gfh_k_batch_pass, so the matrix inverted is bit for bit the one that kernel returns), then in
// registers, unrolled, without contraction and redundantly in every lane of the fit, as the solve is:
//   factor   J^T J = U^T U, U upper (no damping, no DTD: the matrix itself).  A pivot is accepted if it is positive and finite, the
//            test of gfh_b_solve; the first one that is not ends the fit with info = its index + 1.
//   invert   V = U^-1 in place, column by column: V_jj = 1 / U_jj, V_ij = -V_jj sum_{k = i .. j-1} V_ik U_kj (i ascending: row i reads
//            the entries of column j at and below it, which are still U's).
//   multiply C = V V^T in place, rows and columns ascending: C_ab = sum_{k >= b} V_ak V_bk, a <= b, reads only entries of V at or
//            behind the one it replaces.  Each entry is formed once and stored to both triangles: C is symmetric bit for bit.
//   scale    scale 0: C = (J^T J)^-1 (the reference's LMsolver::getInvJTJ).  scale 1: C chi2 / dof with chi2 the sweep's sum r^2
//            and dof the record's of gfh_k_fit_batch: n - na, 1 where that is 0.
//   sigma_j = sqrt(C_jj), of the scaled C under scale 1.
// cov [n_fits][na * na], sigma [n_fits][na], info [n_fits] (0, or j + 1: pivot j failed), in the caller's order of the active
// parameters (GFH_BACT is the order of G[] and so of S).  A fit whose pivot fails gets NaN in all of its cov and sigma; nothing of
// it reaches another fit.  All point access is the sweep's, through GFH_BLOAD: every data form is carried with nothing further.
// (256 lanes per fit: the sweep's one barrier is the kernel's one barrier -- the BARRIER INVARIANT above gfh_k_fit_batch.)
#if GFH_BLOSS
// Under a loss (GFH_BLOSS) the matrix is J^T J of the loss-scaled Jacobian -- what the reference's getInvJTJ holds after a robust fit --
// and under scale 1 it is multiplied by the PLAIN chi2 / dof, as gfh_covariance does on the plain path (errors.cpp): the sweep's last
// sum is the plain sum r^2 under a loss too (gfh_b_sweep), so no further pass is made.
extern "C" __global__ __launch_bounds__(256)
void gfh_k_batch_cov(GFH_BARGS, const double* __restrict__ pars, const int scale, double* __restrict__ cov, double* __restrict__ sigma,
                     int* __restrict__ info, const i64 n_fits, const double inv_c, int* __restrict__ status) {
#else  // GFH_BLOSS
extern "C" __global__ __launch_bounds__(256)
void gfh_k_batch_cov(GFH_BARGS, const double* __restrict__ pars, const int scale, double* __restrict__ cov, double* __restrict__ sigma,
                     int* __restrict__ info, const i64 n_fits, int* __restrict__ status) {
#endif  // GFH_BLOSS
#pragma clang fp contract(off)
  const i64 f = GFH_BFIT(threadIdx.x);
  if (f >= n_fits) return;
  const gfh_bdata d = GFH_BDATA(f);
  double P[GFH_NP], S[GFH_BNACC];
#pragma unroll
  for (int k = 0; k < GFH_NP; k++) P[k] = gfh_uni(pars[f * GFH_NP + k]);
  GFH_BIMG_INIT
#if GFH_BLOSS
  gfh_b_sweep(d, P, status, S, inv_c GFH_BIMG);      // (256 lanes per fit: THE barrier, reached by all four waves -- the return above is per workgroup)
#else  // GFH_BLOSS
  gfh_b_sweep(d, P, status, S GFH_BIMG);      // (256 lanes per fit: THE barrier, reached by all four waves -- the return above is per workgroup)
#endif  // GFH_BLOSS
  double W[GFH_BNP];                          // U, then V, then C: the packed upper triangle, GFH_BIDX
  int bad = 0;
#pragma unroll
  for (int j = 0; j < GFH_NA; j++) {          // potrf_upper_plain of normal_eq.cpp, as gfh_b_solve walks it
    double ajj = S[GFH_BIDX(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) ajj -= W[GFH_BIDX(k, j)] * W[GFH_BIDX(k, j)];
    if (bad == 0 && !(ajj > 0.0 && ajj < __builtin_inf())) bad = j + 1;
    ajj = __builtin_sqrt(ajj); W[GFH_BIDX(j, j)] = ajj;
    const double rinv = 1.0 / ajj;
#pragma unroll
    for (int c = j + 1; c < GFH_NA; c++) {
      double t = S[GFH_BIDX(j, c)];
#pragma unroll
      for (int k = 0; k < j; k++) t -= W[GFH_BIDX(k, j)] * W[GFH_BIDX(k, c)];
      W[GFH_BIDX(j, c)] = t * rinv;
    }
  }
#pragma unroll
  for (int j = 0; j < GFH_NA; j++) {          // V = U^-1
    const double vjj = 1.0 / W[GFH_BIDX(j, j)];
#pragma unroll
    for (int i = 0; i < j; i++) {
      double t = W[GFH_BIDX(i, i)] * W[GFH_BIDX(i, j)];
#pragma unroll
      for (int k = i + 1; k < j; k++) t += W[GFH_BIDX(i, k)] * W[GFH_BIDX(k, j)];
      W[GFH_BIDX(i, j)] = -(t * vjj);
    }
    W[GFH_BIDX(j, j)] = vjj;
  }
  const i64 dof_ = (d.e - d.b) - GFH_NA;       // gadfit.F90:648-657, as gfh_k_fit_batch reports it
  const double q = S[GFH_BNP + GFH_NA] / (dof_ == 0 ? 1.0 : (double)dof_);
#pragma unroll
  for (int a = 0; a < GFH_NA; a++)            // C = V V^T
#pragma unroll
    for (int b = a; b < GFH_NA; b++) {
      double t = W[GFH_BIDX(a, b)] * W[GFH_BIDX(b, b)];
#pragma unroll
      for (int k = b + 1; k < GFH_NA; k++) t += W[GFH_BIDX(a, k)] * W[GFH_BIDX(b, k)];
      if (scale) t = t * q;
      W[GFH_BIDX(a, b)] = bad ? __builtin_nan("") : t;
    }
  if (d.lane == 0) {
    double* __restrict__ out = cov + f * (GFH_NA * GFH_NA);
#pragma unroll
    for (int a = 0; a < GFH_NA; a++)
#pragma unroll
      for (int b = 0; b < GFH_NA; b++) out[a * GFH_NA + b] = a <= b ? W[GFH_BIDX(a, b)] : W[GFH_BIDX(b, a)];
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) sigma[f * GFH_NA + a] = __builtin_sqrt(W[GFH_BIDX(a, a)]);
    info[f] = bad;
  }
}
