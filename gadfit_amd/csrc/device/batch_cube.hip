
// ---- The data form of a cube (gfh_set_batch_cube; GFH_BCUBE): every spectrum of the batch on ONE abscissa grid x [n_points], the
// samples y [n_fits][n_points] spectrum-major in a narrow type, the weight formed from y in the load.  Emitted in front of
// batch_fit.hip in the cube forms alone; it replaces that file's gfh_bdata, GFH_BARGS, GFH_BDATA and GFH_BLOAD and nothing else: the
// LM loop, the sweeps and the reducers are batch_fit.hip's one text.
//   GFH_BYTYPE 0 double, 1 float, 2 unsigned short: each converts to double exactly.
//   GFH_BERR   the weight, by the expressions of k_init_weights (kernels.hip; gadfit.F90:445-470): 0 NONE, 1 SQRT_Y, 2 PROPTO_Y,
//              3 INVERSE_Y, 4 USER -- a plain load of w [n_fits][n_points], the weights as used.  Under 0 ... 3 the kernels read no
//              weight array (w is null).
// Plain element loads: row f begins at y + f * n_points, which is aligned to the element and to nothing more (an odd n_points puts
// every other row of unsigned short on an odd 2-byte boundary).  The product f * n_points is 64-bit.  Everything added here is a
// per-lane value that enters no branch enclosing a barrier (the BARRIER INVARIANT above gfh_k_fit_batch).
#if GFH_BYTYPE == 0
typedef double gfh_by_t;
#elif GFH_BYTYPE == 1
typedef float gfh_by_t;
#elif GFH_BYTYPE == 2
typedef unsigned short gfh_by_t;
#else
#error "GFH_BYTYPE: 0 double, 1 float, 2 unsigned short"
#endif
#define GFH_BTHR (1e2 * 2.2250738585072014e-308)
#if GFH_BERR == 0
#define GFH_BWEIGHT(yy, c) 1.0
#elif GFH_BERR == 1
#define GFH_BWEIGHT(yy, c) (fabs(yy) < GFH_BTHR ? 0.0 : 1.0 / sqrt(yy))
#elif GFH_BERR == 2
#define GFH_BWEIGHT(yy, c) (fabs(yy) < GFH_BTHR ? 0.0 : 1.0 / yy)
#elif GFH_BERR == 3
#define GFH_BWEIGHT(yy, c) yy
#elif GFH_BERR == 4
#define GFH_BWEIGHT(yy, c) d.w[c]
#else
#error "GFH_BERR: 0 NONE, 1 SQRT_Y, 2 PROPTO_Y, 3 INVERSE_Y, 4 USER"
#endif
// x: the shared grid; y, w: the fit's own rows; b = 0, e = n_points
struct gfh_bdata { const double* __restrict__ x; const gfh_by_t* __restrict__ y; const double* __restrict__ w; i64 b, e; int lane; };
#define GFH_BARGS const double* __restrict__ x, const gfh_by_t* __restrict__ y, const double* __restrict__ w, const i64 n_points
#define GFH_BDATA(f) {x, y + (f) * n_points, GFH_BERR == 4 ? w + (f) * n_points : w, 0, n_points, (int)(threadIdx.x & (GFH_BLANES - 1))}
// the inputs of pass row i0 for this lane, as the ragged load: one row ahead, clamped to the last point, w = 0 past the end
#define GFH_BLOAD(X, Y, W, i0) { const i64 i_ = (i0) + d.lane; const i64 c_ = i_ < d.e ? i_ : d.e - 1; \
  X = d.x[c_]; Y = (double)d.y[c_]; const double w_ = GFH_BWEIGHT(Y, c_); W = i_ < d.e ? w_ : 0.0; }
