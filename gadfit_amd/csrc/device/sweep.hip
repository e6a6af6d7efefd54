
// Device layout (DESIGN.md "Data layout"): slots are data points padded per dataset to a
// multiple of the tile so every tile is full and belongs to one dataset; pad slots carry
// w = 0.  x, y, w, res, omega: [n_slots]; J: [NA][ldj] (parameter-major: a wave's store of
// one Jacobian column is 64 consecutive doubles = one fully coalesced 512 B write).
#define GFH_TILE GFH_BLOCK

// Robust cost of the C++ solver (lm_solver.cpp:255-284, 303-317): the weighted residual and its
// Jacobian row are scaled by sqrt(rho'(res^2)); chi2() stays the plain sum (lm_solver.cpp:513-529).
#if GFH_LOSS == 1
#define GFH_ROBUST(R, Wv) { const double ls_ = sqrt(1.0 / (1.0 + (R) * (R))); R *= ls_; Wv *= ls_; }
#elif GFH_LOSS == 2
#define GFH_ROBUST(R, Wv) { const double ls_ = (R) * (R) > 1.0 ? sqrt(1.0 / fabs(R)) : 1.0; R *= ls_; Wv *= ls_; }
#else
#define GFH_ROBUST(R, Wv)
#endif

typedef double gfh_d4 __attribute__((ext_vector_type(4)));
typedef int gfh_v2i __attribute__((ext_vector_type(2)));

// One wave stores 64 consecutive doubles at a WAVE-UNIFORM base: buffer_store_dwordx2 with
// the descriptor in SGPRs (built by scalar adds) and a 32-bit lane offset -- no per-lane
// 64-bit address VALU work and half the address bytes through the vector-memory issue path.
static __device__ __forceinline__ void gfh_store64(double* base, const int lane8, const double v) {
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, 512, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(gfh_v2i, v), rs, lane8, 0, 2);   // aux 2 = nt: written once, streamed
}

extern "C" __global__ __launch_bounds__(GFH_BLOCK) GFH_OCC
void gfh_k_sweep(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ w,
                 GFH_PARS_DECL, const int* __restrict__ tile_ds, const int n_tiles,
                 double* __restrict__ res, double* __restrict__ J, const i64 ldj, int* __restrict__ status,
                 const double* __restrict__ aux, const i64 lda GFH_MESH_KPARAMS GFH_ORDER_KPARAMS GFH_WSG_KPARAMS) {
  GFH_WSG_INIT
  for (int tb = blockIdx.x; tb < n_tiles; tb += gridDim.x) {
    const int t = GFH_ORD(tb);
#if GFH_HAS_ORDER
    const unsigned long long c0_ = __builtin_amdgcn_s_memtime();
#endif
    const double* __restrict__ P = GFH_PARS_AT(tile_ds[t]);   // wave-uniform: scalar loads
    const i64 i = (i64)t * GFH_TILE + threadIdx.x;
    const i64 iw = (i64)t * GFH_TILE + 64 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // this wave's first slot
    const int lane8 = (threadIdx.x & 63) * 8;
    const double X = x[i], Y = y[i];
    double W = w[i];
    double F, G[GFH_NA];
    gfh_point_grad(X, P, F, G, status, aux + i, lda GFH_MESH_AT(i) GFH_SLOT(i));
    double R = (Y - F) * W;                     // gadfit.F90:682-683
    GFH_ROBUST(R, W)
    gfh_store64(res + iw, lane8, R);
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) gfh_store64(J + (i64)a * ldj + iw, lane8, G[a] * W);   // gadfit.F90:689-690
#if GFH_HAS_ORDER
    if (cost && threadIdx.x == 0) { const unsigned long long d_ = (__builtin_amdgcn_s_memtime() - c0_) >> 6; cost[t] = d_ < 0x7fffffffull ? (int)d_ : 0x7fffffff; }
#endif
  }
}

// Cross-workgroup hand-off without fences (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement &
// inter-workgroup visibility", valid forms and the table's first row): every handed-off byte is stored `sc1` (write-through,
// past the XCD's L2), every storing wave drains (`s_waitcnt vmcnt(0)`) before a workgroup barrier, one lane then adds to
// an agent-scope counter, and the workgroup whose add came last reads the bytes with `sc1` loads -- global_ instructions,
// never flat_: the pointers are cast to the global address space so the compiler cannot fall back to flat accesses.
#define GFH_GLOBAL(p) ((__attribute__((address_space(1))) __typeof__(*(p))*)(p))
#define GFH_ST_DEV(p, v) __hip_atomic_store(GFH_GLOBAL(p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define GFH_LD_DEV(p) __hip_atomic_load(GFH_GLOBAL(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define GFH_ST_SYS(p, v) __hip_atomic_store(GFH_GLOBAL(p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)

