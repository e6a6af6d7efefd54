
// STEP 3 in one pass (gadfit.F90:715-735): omega_i = -f''_delta1(x_i) w_i in forward mode AND
// J^T omega, with the Jacobian row of the point recomputed in registers (the reverse sweep of
// gfh_k_sweep over the forward values the forward-mode pass has just formed: the same expressions,
// so the same J_i) instead of re-read from HBM -- 8*p B/point
// of traffic less than J^T omega from the stored Jacobian, and STEP 3 no longer needs J in HBM
// at all.  One workgroup per gram block; the thread-to-point map, the order of additions, the wave
// and workgroup reductions are those of k_jtv (kernels.hip), so partial[b][a] is bitwise what
// k_jtv returns from the stored J.
extern "C" __global__ __launch_bounds__(256)
void gfh_k_omega_jt(const double* __restrict__ x, const double* __restrict__ w,
                    GFH_PARS_DECL, GFH_DPARS_DECL,
                    const i64* __restrict__ gb_start, const int* __restrict__ gb_slots, const int* __restrict__ gb_ds,
                    double* __restrict__ omega, double* __restrict__ partial, const int pstride, int* __restrict__ status,
                    const double* __restrict__ aux, const i64 lda) {
  const i64 s0 = gb_start[blockIdx.x], e = s0 + gb_slots[blockIdx.x];
  const double* __restrict__ P = GFH_PARS_AT(gb_ds[blockIdx.x]);
  const int ds0 = gb_ds[blockIdx.x];
  double acc[GFH_NA];
#pragma unroll
  for (int a = 0; a < GFH_NA; a++) acc[a] = 0.0;
  for (i64 i = s0 + threadIdx.x; i < e; i += 256) {
    const double X = x[i], W = w[i];                   // (no prefetch of the next pass here: at 32 parameters it would not fit 256 VGPRs)
    double G[GFH_NA];
    GFH_TANGENTS(DPl, ds0)
    const double om = -gfh_point_dd_grad(X, P, DPl, G, status, aux + i, lda GFH_MESH_NONE GFH_SLOT(i)) * W;    // gadfit.F90:722-723
    omega[i] = om;
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) {
      const double j = G[a] * W;                                                      // the stored J entry, gadfit.F90:689-690
      acc[a] += j * om;                                                               // gadfit.F90:734
    }
  }
  __shared__ double ws[GFH_NA][4];
#pragma unroll
  for (int a = 0; a < GFH_NA; a++) {
    const double v = gfh_wave_sum(acc[a]);
    if ((threadIdx.x & 63) == 0) ws[a][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < GFH_NA) partial[(i64)blockIdx.x * pstride + threadIdx.x] =
      ((ws[threadIdx.x][0] + ws[threadIdx.x][1]) + ws[threadIdx.x][2]) + ws[threadIdx.x][3];
}
