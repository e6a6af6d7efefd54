
// chi2() (gadfit.F90:1015-1034): every parameter passive, value only.  Same partition and thread-to-point
// map as the fused kernel -- one workgroup of GFH_FW waves per gram block, wave wv of pass k takes the 64 slots
// at s0 + 64 wv + k * 64 GFH_FW -- every lane sums its own points pass by pass, then the wave tree, the waves
// in order, the workgroups by slices of 32 and the datasets in order: the order of additions of the fused
// kernel's sum r^2, so chi2() is bitwise the sum a sweep at the same parameters returns (GFH_FAST_DIV = 1: the
// reference's own value-only and active division forms differ by rounding, AD:814-913).  The parameter block
// is fixed per workgroup, so parameter-only subexpressions (reciprocals of widths ...) leave the pass loop.
// The next pass's inputs are loaded before the current pass's value is computed.
// tail_mode 0: workgroup sums only; 1: the last workgroup to arrive adds them up into out[0]; 2: and posts
// {sum, status} to the host mailbox.  The hand-off is the release / acquire form (MI355X_MICROARCH.md,
// inter-workgroup visibility: valid for any number of workgroups per CU).
#define GFH_CW (GFH_NA <= GFH_FUSED_MAX ? GFH_FW : 8)      // (beyond that there is no fused kernel to agree with)
#define GFH_CTHREADS (64 * GFH_CW)
extern "C" __global__ __launch_bounds__(GFH_CTHREADS) GFH_OCC
void gfh_k_chi2(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ w,
                GFH_PARS_DECL, const i64* __restrict__ gb_start, const int* __restrict__ gb_slots,
                const int* __restrict__ gb_ds, double* __restrict__ res, double* partial, int* __restrict__ status,
                const double* __restrict__ aux, const i64 lda, const int* __restrict__ ds_first_gb, const int nd,
                double* out, double* host_out, unsigned long long* host_flag, unsigned* counter,
                const unsigned long long seq, const int tail_mode GFH_MESH_KPARAMS GFH_ORDER_KPARAMS GFH_WSG_KPARAMS) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __shared__ double ws[GFH_CW];
  __shared__ double sl_sum[512];
  __shared__ double ds_sum[16];
  __shared__ int role;
  GFH_WSG_INIT
#if GFH_WSG
  // (workspaces in the global pool: the grid is capped at the pool's slots and a workgroup takes gram blocks blockIdx.x, + gridDim.x, ...;
  // every sum is defined on the partition into gram blocks, so which workgroup does a block changes no bit)
  for (int bb_ = blockIdx.x, nb_ = ds_first_gb[nd]; bb_ < nb_; bb_ += gridDim.x) {
  const int B = GFH_ORD(bb_);
#else
  {
  const int B = GFH_ORD(blockIdx.x);                                       // the gram block this workgroup works on
#endif
  const i64 s0 = gb_start[B];                                              // gb_slots: a positive multiple of GFH_CTHREADS slots
  const double* __restrict__ P = GFH_PARS_AT(gb_ds[B]);
  // Two passes per trip; the inputs of a trip are loaded during the trip before it, i.e. two passes (about a
  // microsecond of arithmetic) ahead: one pass ahead is less than the latency of an HBM load under load, and the
  // waves of a workgroup run in step, so they would all wait for it together.
  const int np = gb_slots[B] / GFH_CTHREADS;                              // passes of this workgroup (wave-uniform)
  const double* __restrict__ xb = x + s0 + threadIdx.x; const double* __restrict__ yb = y + s0 + threadIdx.x;
  const double* __restrict__ wb = w + s0 + threadIdx.x; const double* __restrict__ ab = aux + s0 + threadIdx.x;
  double* __restrict__ rb = res + s0 + threadIdx.x;
  double X0 = xb[0], Y0 = yb[0], W0 = wb[0];
  const i64 o1 = np > 1 ? GFH_CTHREADS : 0;
  double X1 = xb[o1], Y1 = yb[o1], W1 = wb[o1];
  double s = 0.0;
  for (int k = 0; k < np; k += 2) {
    const i64 oa = (i64)(k + 2 < np ? k + 2 : k) * GFH_CTHREADS, ob = (i64)(k + 3 < np ? k + 3 : k) * GFH_CTHREADS;
    const double Xa = xb[oa], Ya = yb[oa], Wa = wb[oa], Xb = xb[ob], Yb = yb[ob], Wb = wb[ob];
    const i64 oc = (i64)k * GFH_CTHREADS;
    const double r0 = (Y0 - gfh_point_value(X0, P, status, ab + oc, lda GFH_MESH_AT(s0 + threadIdx.x + oc) GFH_SLOT(s0 + threadIdx.x + oc))) * W0;   // gadfit.F90:1024-1026
#if GFH_STORE_RES
    __builtin_nontemporal_store(r0, rb + oc);
#endif
    s += r0 * r0;
    if (k + 1 < np) {
      const double r1 = (Y1 - gfh_point_value(X1, P, status, ab + oc + GFH_CTHREADS, lda GFH_MESH_AT(s0 + threadIdx.x + oc + GFH_CTHREADS) GFH_SLOT(s0 + threadIdx.x + oc + GFH_CTHREADS))) * W1;
#if GFH_STORE_RES
      __builtin_nontemporal_store(r1, rb + oc + GFH_CTHREADS);
#endif
      s += r1 * r1;
    }
    X0 = Xa; Y0 = Ya; W0 = Wa; X1 = Xb; Y1 = Yb; W1 = Wb;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) ws[wv] = s;
  if (tail_mode) asm volatile("s_waitcnt vmcnt(0)\n" ::: "memory");       // this wave's status raise (if any) has landed
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = ws[0];
#pragma unroll
    for (int k = 1; k < GFH_CW; k++) tot += ws[k];
    partial[B] = tot;
  }
#if GFH_WSG
  __syncthreads();                                                        // (ws[] is written again in the next round)
#endif
  }
  if (threadIdx.x == 0) {
    if (tail_mode) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)\n" ::: "memory");
      const bool last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
      if (last) {
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch (stream-ordered)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)\n" ::: "memory");
      }
      role = last;
    }
  }
  if (!tail_mode) return;
  __syncthreads();
  if (!role) return;
  // level 1: slice sl of dataset d adds its workgroups b0+sl, b0+sl+32, ... in ascending order; level 2: the 32
  // slice sums in slice order; level 3: the datasets in order (k_reduce_partials + k_gather_sum, and the fused tail)
  double total = 0.0;
  constexpr int DPR = GFH_CTHREADS / 32 < 16 ? GFH_CTHREADS / 32 : 16;     // datasets per round
  for (int d0 = 0; d0 < nd; d0 += DPR) {
    const int dl = threadIdx.x >> 5, sl = threadIdx.x & 31;
    if (dl < DPR && d0 + dl < nd) {
      const int b1 = ds_first_gb[d0 + dl + 1];
      double a = 0.0;
      for (int b = ds_first_gb[d0 + dl] + sl; b < b1; b += 32) a += partial[b];
      sl_sum[dl * 32 + sl] = a;
    }
    __syncthreads();
    if (threadIdx.x < DPR && d0 + (int)threadIdx.x < nd) {
      double t = sl_sum[threadIdx.x * 32];
#pragma unroll
      for (int k = 1; k < 32; k++) t += sl_sum[threadIdx.x * 32 + k];
      ds_sum[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) for (int k = 0; k < DPR && d0 + k < nd; k++) total += ds_sum[k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = total;
    if (tail_mode == 1) out[1] = GFH_STATUS_SLOT(GFH_LD_DEV(status));      // the status slot of the cross-rank sum that follows
    if (tail_mode == 2) {
      GFH_ST_SYS(host_out, total);
      GFH_ST_SYS(host_out + 1, (double)GFH_LD_DEV(status));
      asm volatile("s_waitcnt vmcnt(0)\n" ::: "memory");
      __hip_atomic_store(GFH_GLOBAL(host_flag), seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

