// The tangent block of STEP 3 (delta1 per parameter).  Parameters and tangents are wave-uniform; with more than 16 of each
// they no longer fit the scalar registers next to each other, and what the compiler then does with loop-invariant scalars
// is to park them in VGPR lanes and fetch them back with v_readlane_b32 every pass (216 of them per pass at 32 parameters: a
// quarter of the loop's VALU issue).  Re-reading the tangents through the scalar cache inside the loop (constant address
// space, pointer made opaque so the loads stay in the loop) costs four s_load_dwordx16 per pass instead.
typedef const double __attribute__((address_space(4))) * gfh_cptr;
#if GFH_PARG
// (by value with the kernel arguments: addressed through the kernarg segment itself -- x, w, pars, dpars are the first
// four parameters of both STEP 3 kernels, so dpars sits at 16 + sizeof(gfh_parg); taking the address of the parameter
// object instead would make the compiler copy it to scratch.  tests/test_cpu_generated_source.py checks the offset
// against the code object's metadata.)
#define GFH_DPARS_CONST(ds) ((gfh_cptr)((const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr() + 16 + sizeof(gfh_parg)) + (GFH_PARG == GFH_NP ? 0 : (ds) * GFH_NP))
#else
#define GFH_DPARS_CONST(ds) ((gfh_cptr)(unsigned long long)(dpars + (i64)(ds) * GFH_NP))
#endif
#if GFH_NP > 16
#define GFH_TANGENTS(DPl, ds)                                                                  \
  double DPl[GFH_NP];                                                                          \
  { gfh_cptr c_ = GFH_DPARS_CONST(ds); asm volatile("" : "+s"(c_));                            \
    _Pragma("unroll") for (int k_ = 0; k_ < GFH_NP; k_++) DPl[k_] = c_[k_]; }
#else
#define GFH_TANGENTS(DPl, ds) const double* __restrict__ DPl = GFH_DPARS_AT(ds);
#endif

// omega kernel (STEP 3, forward mode): a workgroup owns a CONTIGUOUS chunk of tiles.  When the whole chunk
// lies in one dataset (always, unless a dataset boundary falls inside it) the parameter block is
// fixed for the loop, so everything that depends on parameters only leaves the per-point code.  The host sizes
// the grid to what is resident at once (launch.cpp, resident_grid), so no workgroup waits for a second round.
extern "C" __global__ __launch_bounds__(GFH_BLOCK) GFH_OCC
void gfh_k_omega(const double* __restrict__ x, const double* __restrict__ w,
                 GFH_PARS_DECL, GFH_DPARS_DECL,
                 const int* __restrict__ tile_ds, const int n_tiles, double* __restrict__ omega, int* __restrict__ status,
                 const double* __restrict__ aux, const i64 lda GFH_MESH_KPARAMS GFH_ORDER_KPARAMS GFH_WSG_KPARAMS) {
  GFH_WSG_INIT
#if GFH_WSG
  // (workspaces in the global pool: the grid is capped at the pool's slots; a workgroup takes tiles blockIdx.x, + gridDim.x, ... of
  // the table sorted by cost, like gfh_k_sweep)
  for (int tb = blockIdx.x; tb < n_tiles; tb += gridDim.x) {
    const int t = GFH_ORD(tb);
    const double* __restrict__ P = GFH_PARS_AT(tile_ds[t]);
    const double* __restrict__ DP = GFH_DPARS_AT(tile_ds[t]);
    for (i64 i = (i64)t * GFH_TILE + threadIdx.x; i < (i64)(t + 1) * GFH_TILE; i += GFH_BLOCK)
      omega[i] = -gfh_point_dd(x[i], P, DP, status, aux + i, lda GFH_MESH_AT(i) GFH_SLOT(i)) * w[i];
  }
  return;
#endif
  // tiles split as evenly as integers allow: workgroup b takes [b n / G, (b + 1) n / G)
  const int bi = gridDim.x == (unsigned)n_tiles ? GFH_ORD(blockIdx.x) : (int)blockIdx.x;      // (one tile per workgroup: in the order of cost)
  const int t0 = (int)((i64)bi * n_tiles / gridDim.x), t1 = (int)((i64)(bi + 1) * n_tiles / gridDim.x);
  if (t0 >= t1) return;
  if (tile_ds[t0] == tile_ds[t1 - 1]) {
    const double* __restrict__ P = GFH_PARS_AT(tile_ds[t0]);
    const int ds0 = tile_ds[t0];                                 // delta1 scattered per dataset
    const i64 e = (i64)t1 * GFH_TILE;
    i64 i = (i64)t0 * GFH_TILE + threadIdx.x;
    double Xc = x[i], Wc = w[i];
    for (; i < e; i += GFH_BLOCK) {
      const i64 in = i + GFH_BLOCK < e ? i + GFH_BLOCK : i;       // next pass's inputs (the last pass re-reads its own)
      const double Xn = x[in], Wn = w[in];
      GFH_TANGENTS(DPl, ds0)
      omega[i] = -gfh_point_dd(Xc, P, DPl, status, aux + i, lda GFH_MESH_AT(i) GFH_SLOT(i)) * Wc;                  // gadfit.F90:722-723
      Xc = Xn; Wc = Wn;
    }
  } else {
    for (int t = t0; t < t1; t++) {
      const double* __restrict__ P = GFH_PARS_AT(tile_ds[t]);
      const double* __restrict__ DP = GFH_DPARS_AT(tile_ds[t]);
      for (i64 i = (i64)t * GFH_TILE + threadIdx.x; i < (i64)(t + 1) * GFH_TILE; i += GFH_BLOCK)
        omega[i] = -gfh_point_dd(x[i], P, DP, status, aux + i, lda GFH_MESH_AT(i) GFH_SLOT(i)) * w[i];
    }
  }
}
