
// ---- Curves of a batch: the fitted model, the weighted residuals and the 1-sigma band of the curve for a contiguous range of the
// batch's fits [first_fit, first_fit + n_fits_eval), behind batch_cov.hip in every batch translation unit and written once against
// GFH_BLANES, GFH_BARGS, GFH_BDATA and GFH_BLOAD like the three kernels in front of it.  Fit f = first_fit + k, k = the index
// GFH_BFIT gives; pars [n_fits_eval][GFH_NP] and cov [n_fits_eval][GFH_NA * GFH_NA] hold the rows of the evaluated fits only.
//   on the fit's own points (x_eval null): lane l walks points b + l, + GFH_BLANES, ... through GFH_BLOAD, a row ahead, as gfh_b_chi2
//     does; the lanes past the end of the last row compute on the clamped point and STORE NOTHING.  Per point, whichever is asked for:
//       model    = f(x_i; P)
//       residual = (y_i - f) w_i          (gadfit.F90:682-683, w the weight the load forms)
//       band     = sqrt(g^T C g), g[a] = df / dp_active(a) the unweighted gradient of gfh_point_grad in the caller's order (GFH_BACT)
//     in the data's own layout: ragged, one flat array with fit f at off[f] - off[first_fit]; a cube, [n_fits_eval][n_points].
//   on a caller's grid (x_eval [n_eval], shared by all fits): model and band as [n_fits_eval][n_eval]; the host refuses a residual.
// The band in a fixed order, without contraction: t_a = sum_b C[a][b] g[b] (b ascending), s2 = sum_a g[a] t_a (a ascending),
// band = sqrt(s2 < 0 ? 0 : s2); NaN propagates, so a fit whose covariance is NaN gets NaN bands while its model and residuals stay
// finite.  Null outputs are not written; which are null is uniform for the launch.  Without a band the value comes from
// gfh_point_value, with one from gfh_point_grad: the two may differ in the last bits of `model`.
// No reduction, no LDS, no barrier in any form: every lane owns its points, and every store is a plain store of a double per lane, a
// row of GFH_BLANES consecutive doubles per fit.  (256 lanes per fit: nothing here to add to the BARRIER INVARIANT.)
#ifdef GFH_BCUBE
#define GFH_BOUT(k) ((k) * n_points)
#else
#define GFH_BOUT(k) (off[first_fit + (k)] - off[first_fit])
#endif
static __device__ __forceinline__ double gfh_b_band(const double (&G)[GFH_NA], const double (&Cm)[GFH_NA * GFH_NA]) {
#pragma clang fp contract(off)
  double s2 = 0.0;
#pragma unroll
  for (int a = 0; a < GFH_NA; a++) {
    double t = 0.0;
#pragma unroll
    for (int b = 0; b < GFH_NA; b++) t += Cm[a * GFH_NA + b] * G[b];
    s2 += G[a] * t;
  }
  return __builtin_sqrt(s2 < 0.0 ? 0.0 : s2);
}
extern "C" __global__ __launch_bounds__(256)
void gfh_k_batch_eval(GFH_BARGS, const double* __restrict__ pars, const double* __restrict__ cov, const double* __restrict__ x_eval,
                      const i64 n_eval, const i64 first_fit, const i64 n_fits_eval, double* __restrict__ model,
                      double* __restrict__ residual, double* __restrict__ band, int* __restrict__ status) {
#pragma clang fp contract(off)
  const i64 k = GFH_BFIT(threadIdx.x);
  if (k >= n_fits_eval) return;
  const i64 f = first_fit + k;
  const gfh_bdata d = GFH_BDATA(f);
  double P[GFH_NP], Cm[GFH_NA * GFH_NA];
#pragma unroll
  for (int j = 0; j < GFH_NP; j++) P[j] = gfh_uni(pars[k * GFH_NP + j]);
  if (band) {
#pragma unroll
    for (int j = 0; j < GFH_NA * GFH_NA; j++) Cm[j] = cov[k * (GFH_NA * GFH_NA) + j];
  }
  if (x_eval) {                                  // the caller's grid: [n_fits_eval][n_eval]
    const i64 base = k * n_eval;
    for (i64 i0 = 0; i0 < n_eval; i0 += GFH_BLANES) {
      const i64 i = i0 + d.lane;
      const double X = x_eval[i < n_eval ? i : n_eval - 1];
      double F, G[GFH_NA];
      if (band) gfh_point_grad(X, P, F, G, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i));
      else F = gfh_point_value(X, P, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i));
      if (i < n_eval) {
        if (model) model[base + i] = F;
        if (band) band[base + i] = gfh_b_band(G, Cm);
      }
    }
    return;
  }
  const i64 base = GFH_BOUT(k) - d.b;            // the fit's own points, in the data's layout
  double Xc, Yc, Wc;
  GFH_BLOAD(Xc, Yc, Wc, d.b)
  for (i64 i0 = d.b; i0 < d.e; i0 += GFH_BLANES) {
    double Xn, Yn, Wn;
    GFH_BLOAD(Xn, Yn, Wn, i0 + GFH_BLANES < d.e ? i0 + GFH_BLANES : i0)       // next row's inputs (the last row re-reads its own)
    const i64 i = i0 + d.lane;
    double F, G[GFH_NA];
    if (band) gfh_point_grad(Xc, P, F, G, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i));
    else F = gfh_point_value(Xc, P, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i));
    if (i < d.e) {
      if (model) model[base + i] = F;
      if (residual) {
        // past the end the load gives w = 0; here i < d.e, so Wc is the point's weight
        residual[base + i] = (Yc - F) * Wc;      // gadfit.F90:682-683
      }
      if (band) band[base + i] = gfh_b_band(G, Cm);
    }
    Xc = Xn; Yc = Yn; Wc = Wn;
  }
}
