
// ---- Curves of a plain fit (gfh_eval): the fitted model, the weighted residuals and the 1-sigma band of the curve, in a translation
// unit of their own (GenConfig::eval) behind the model's point functions -- the default unit carries none of this text.
//   on the data's own points: gfh_k_sweep's walk of the padded tiles, one lane per slot -- tile_ds -> the dataset's parameter row
//     through GFH_PARS_AT and, under a band, the dataset's covariance block cov[ds] (GFH_NA x GFH_NA, gathered by the host through
//     Jacobian_indices, so that it holds the dataset's global and local columns and their coupling) at a wave-uniform address: the
//     compiler reads it through the scalar cache, a block per tile.  Per slot, whichever is asked for:
//       model    = f(x_i; P_d)
//       residual = (y_i - f) w_i          chi2()'s plain residual, gadfit.F90:682-683 -- under a robust loss too; the expression of gfh_k_chi2
//       band     = sqrt(g^T C_d g), g[a] = df / dp_active(a) the unweighted gradient of gfh_point_grad in the caller's order
//     into padded arrays [n_slots] (pad slots compute on their dataset's last point with w = 0); the host un-pads.
//   on a caller's grid (x_eval [n_eval], shared by all datasets): workgroup b takes dataset b / tiles_per_ds and the grid's tile
//     b % tiles_per_ds; the lanes past the end compute on the clamped point and STORE NOTHING; model and band [n_datasets][n_eval].
// The band in gfh_b_band's fixed order, without contraction: t_a = sum_b C[a][b] g[b] (b ascending), s2 = sum_a g[a] t_a (a ascending),
// band = sqrt(s2 < 0 ? 0 : s2); NaN propagates, so a NaN covariance gives NaN bands while model and residuals stay finite.
// Without a band the value comes from gfh_point_value, with one from gfh_point_grad: the last bits of `model` may differ between the
// two.  The band kernels and the plain ones are separate instantiations: the plain ones carry neither the gradient's registers nor
// the block.  No reduction, no LDS, no barrier, no atomics (the status word of the point functions aside): every lane owns its
// slot, and every store is a plain store of a double per lane, written once and streamed.
// The signatures take the sweep's argument groups for auxiliary columns, variant tapes, meshes and order; models with integrate() are
// refused by the host, so the last two are empty in every unit that exists.
#if GFH_PARG
#define GFH_E_PARS const gfh_parg& pars
#else
#define GFH_E_PARS const double* __restrict__ pars
#endif
static __device__ __forceinline__ double gfh_e_band(const double (&G)[GFH_NA], const double* __restrict__ Cd) {
#pragma clang fp contract(off)
  double s2 = 0.0;
#pragma unroll
  for (int a = 0; a < GFH_NA; a++) {
    double t = 0.0;
#pragma unroll
    for (int b = 0; b < GFH_NA; b++) t += Cd[a * GFH_NA + b] * G[b];
    s2 += G[a] * t;
  }
  return __builtin_sqrt(s2 < 0.0 ? 0.0 : s2);
}

template <bool BAND>
static __device__ __forceinline__ void gfh_e_data(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ w,
                                                  GFH_E_PARS, const int* __restrict__ tile_ds, const int n_tiles,
                                                  const double* __restrict__ cov, double* __restrict__ model, double* __restrict__ residual,
                                                  double* __restrict__ band, int* __restrict__ status, const double* __restrict__ aux,
                                                  const i64 lda GFH_MESH_KPARAMS GFH_ORDER_KPARAMS) {
  for (int tb = blockIdx.x; tb < n_tiles; tb += gridDim.x) {
    const int t = GFH_ORD(tb);
    const int ds = tile_ds[t];                                // wave-uniform: scalar loads
    const double* __restrict__ P = GFH_PARS_AT(ds);
    const i64 i = (i64)t * GFH_BLOCK + threadIdx.x;
    const double X = x[i];
    double F;
    if constexpr (BAND) {
      double G[GFH_NA];
      gfh_point_grad(X, P, F, G, status, aux + i, lda GFH_MESH_AT(i) GFH_SLOT(i));
      __builtin_nontemporal_store(gfh_e_band(G, cov + (i64)ds * (GFH_NA * GFH_NA)), band + i);
    } else {
      F = gfh_point_value(X, P, status, aux + i, lda GFH_MESH_AT(i) GFH_SLOT(i));
    }
    if (model) __builtin_nontemporal_store(F, model + i);
    if (residual) {
      const double r = (y[i] - F) * w[i];                     // gadfit.F90:682-683
      __builtin_nontemporal_store(r, residual + i);
    }
  }
}

#define GFH_E_DATA_ARGS const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ w, GFH_PARS_DECL, \
                        const int* __restrict__ tile_ds, const int n_tiles, const double* __restrict__ cov, double* __restrict__ model, \
                        double* __restrict__ residual, double* __restrict__ band, int* __restrict__ status, \
                        const double* __restrict__ aux, const i64 lda GFH_MESH_KPARAMS GFH_ORDER_KPARAMS
#if GFH_HAS_ORDER
#define GFH_E_DATA_PASS x, y, w, pars, tile_ds, n_tiles, cov, model, residual, band, status, aux, lda, mesh, mesh_mode, order, cost
#else
#define GFH_E_DATA_PASS x, y, w, pars, tile_ds, n_tiles, cov, model, residual, band, status, aux, lda
#endif
extern "C" __global__ __launch_bounds__(GFH_BLOCK) GFH_OCC
void gfh_k_eval(GFH_E_DATA_ARGS) { gfh_e_data<false>(GFH_E_DATA_PASS); }
extern "C" __global__ __launch_bounds__(GFH_BLOCK) GFH_OCC
void gfh_k_eval_band(GFH_E_DATA_ARGS) { gfh_e_data<true>(GFH_E_DATA_PASS); }

#if GFH_EVAL_GRID
// (one recorded path, no auxiliary columns, no integrals: what the batch kernels carry)
template <bool BAND>
static __device__ __forceinline__ void gfh_e_grid(const double* __restrict__ x_eval, const i64 n_eval, const int tiles_per_ds, GFH_E_PARS,
                                                  const double* __restrict__ cov, double* __restrict__ model, double* __restrict__ band,
                                                  int* __restrict__ status) {
  const int ds = blockIdx.x / tiles_per_ds, tg = blockIdx.x - ds * tiles_per_ds;      // wave-uniform
  const double* __restrict__ P = GFH_PARS_AT(ds);
  const i64 i = (i64)tg * GFH_BLOCK + threadIdx.x;
  const double X = x_eval[i < n_eval ? i : n_eval - 1];
  double F;
  if constexpr (BAND) {
    double G[GFH_NA];
    gfh_point_grad(X, P, F, G, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i));
    const double s = gfh_e_band(G, cov + (i64)ds * (GFH_NA * GFH_NA));
    if (i < n_eval) __builtin_nontemporal_store(s, band + (i64)ds * n_eval + i);
  } else {
    F = gfh_point_value(X, P, status, (const double*)nullptr, 0 GFH_MESH_NONE GFH_SLOT(i));
  }
  if (model && i < n_eval) __builtin_nontemporal_store(F, model + (i64)ds * n_eval + i);
}
#define GFH_E_GRID_ARGS const double* __restrict__ x_eval, const i64 n_eval, const int tiles_per_ds, GFH_PARS_DECL, \
                        const double* __restrict__ cov, double* __restrict__ model, double* __restrict__ band, int* __restrict__ status
extern "C" __global__ __launch_bounds__(GFH_BLOCK) GFH_OCC
void gfh_k_eval_grid(GFH_E_GRID_ARGS) { gfh_e_grid<false>(x_eval, n_eval, tiles_per_ds, pars, cov, model, band, status); }
extern "C" __global__ __launch_bounds__(GFH_BLOCK) GFH_OCC
void gfh_k_eval_grid_band(GFH_E_GRID_ARGS) { gfh_e_grid<true>(x_eval, n_eval, tiles_per_ds, pars, cov, model, band, status); }
#endif
