
// (the fused kernels exist for up to 128 active parameters = 8 tiles, model.h kFusedMaxActive / fused_max_active; beyond that STEP 1 and STEP 2 run as
// gfh_k_sweep + k_gram_block launches; models whose quadrature workspaces are the global pool never run them: launch.cpp, fusable_model)
#if GFH_NA <= GFH_FUSED_MAX && !GFH_WSG
// Fused STEP 1 + STEP 2 (gadfit.F90:675-699): the sweep above plus J^T J / J^T r / sum r^2 of
// the same points on the FP64 matrix cores, so J is written once and never re-read.
// One wave = 64 points per pass.  After the AD body each lane holds its point's weighted
// gradient; the wave transposes it through a private LDS stage [row = parameter][col = point]
// (stride 66 doubles: the 16 rows x 2 columns a half-wave reads hit 32 distinct bank pairs)
// into v_mfma_f64_16x16x4_f64 fragments: lane (r = l&15, q = l>>4) reads stage[16t+r][4s+q]
// for k-step s; the same fragment is A operand of row tile t and B operand of column tile t.
// Workgroup partial layout is identical to k_gram's, so the reduction/assembly kernels are shared.
#define GFH_T ((GFH_NA + 15) / 16)
#define GFH_NPAIR (GFH_T * (GFH_T + 1) / 2)
// GFH_HALF: the stage holds 32 points (stride 34) and a pass runs as two half-passes -- lanes 0-31 stage their points and the
// matrix cores take k-steps 0-7, then lanes 32-63 and k-steps 8-15: the k-steps in the order of the full stage, so the same sums
// bit for bit, for half the LDS per wave (more waves per SIMD; the gradient of the upper half waits in registers meanwhile).
#if GFH_HALF
#define GFH_S 34
#define GFH_NH 2
#define GFH_KS 8
#else
#define GFH_S 66
#define GFH_NH 1
#define GFH_KS 16
#endif
// Descriptor of the fused kernel's tail (filled by the host, launch.cpp TailDesc).
struct gfh_tail {
  const int* ds_first_gb;          // [nd+1] first workgroup of each dataset
  const int* inv;                  // [nd][dim] inverse of Jacobian_indices
  double* slice;                   // [nd][32][pstride] slice sums
  double* G;                       // [nd][pstride] per-dataset Gram images
  double* packed;                  // [dim*dim + dim + 1]
  double* host_out;                // pinned result mailbox
  unsigned long long* host_flag;   // pinned sequence flag
  unsigned* counters;              // [1 + nd*32], zero between launches
  int nd, dim, n_slices, pad;
};

// GFH_FW waves per workgroup, kept in phase (__syncthreads between the AD phase and the matrix phase):
// on gfx950 FP64 VALU and FP64 MFMA share one datapath and mixing the two kinds from different waves of
// a SIMD costs throughput (tools/microbench/fp64_overlap.hip), so a SIMD runs one kind at a time.
#define GFH_FTHREADS (64 * GFH_FW)
// Without the Jacobian store (gfh_set_keep_jacobian) the kernel carries another name, so that
// profiles keep the two apart.
#if GFH_STORE_J
#define GFH_K_SWEEP_GRAM gfh_k_sweep_gram
#else
#define GFH_K_SWEEP_GRAM gfh_k_sweep_gram_nostore
#endif
extern "C" __global__ __launch_bounds__(GFH_FTHREADS)
void GFH_K_SWEEP_GRAM(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ w,
                      GFH_PARS_DECL, const i64* __restrict__ gb_start,
                      const int* __restrict__ gb_slots, const int* __restrict__ gb_ds,
                      double* __restrict__ res, double* __restrict__ J, const i64 ldj,
                      double* __restrict__ partial, const int pstride, int* __restrict__ status, const double* __restrict__ aux, const i64 lda,
                      const gfh_tail* __restrict__ tl, const unsigned long long seq, const int tail_mode) {
#if GFH_NA <= GFH_VALU_GRAM_MAX
  // Up to 8 active parameters a 16-row matrix tile would be half empty and the whole outer product of a point is
  // NA (NA + 1) / 2 + NA + 1 <= 45 multiply-adds: it stays on the VALU, in per-lane accumulators -- no LDS stage, no
  // transposition, no matrix instructions (16 of them per pass = 1024 cycles of the FP64 pipe against 180 here) -- and the
  // kernel is left with the store stream.  Every lane sums its own points pass by pass; wave tree and the waves in order
  // at the end (for sum r^2 that is gfh_k_chi2's order, as in the matrix path).  Same partial image as the matrix path.
  constexpr int NP_ = GFH_NA * (GFH_NA + 1) / 2, NACC = NP_ + GFH_NA + 1;
  __shared__ double red[GFH_FW][NACC];
  __shared__ double tot[NACC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const i64 s0 = gb_start[blockIdx.x];
  const i64 e = s0 + gb_slots[blockIdx.x];                   // multiple of GFH_FTHREADS slots
  const double* __restrict__ P = GFH_PARS_AT(gb_ds[blockIdx.x]);
  double av[NACC];
#pragma unroll
  for (int k = 0; k < NACC; k++) av[k] = 0.0;
  i64 iw = s0 + 64 * __builtin_amdgcn_readfirstlane(wv);
  double Xc = (x + iw)[lane], Yc = (y + iw)[lane], Wc = (w + iw)[lane];
  auto body = [&](const double XC, const double YC, const double WC) __attribute__((always_inline)) {
    double* __restrict__ Jw = J + iw;
    double F, G[GFH_NA];
    gfh_point_grad(XC, P, F, G, status, aux + iw + lane, lda GFH_MESH_NONE GFH_SLOT(iw + lane));
    double R = (YC - F) * WC;                               // gadfit.F90:682-683
    double Wl = WC;
    GFH_ROBUST(R, Wl)
    gfh_store64(res + iw, lane * 8, R);
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) {
      G[a] = G[a] * Wl;                                     // gadfit.F90:689-690
#if GFH_STORE_J
      gfh_store64(Jw + (i64)a * ldj, lane * 8, G[a]);
#endif
    }
    int p = 0;
#pragma unroll
    for (int a = 0; a < GFH_NA; a++)
#pragma unroll
      for (int b = a; b < GFH_NA; b++, p++) av[p] += G[a] * G[b];      // gadfit.F90:697
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) av[NP_ + a] += G[a] * R;          // gadfit.F90:698
    av[NP_ + GFH_NA] += R * R;
  };
  asm volatile("" :: "v"(Xc), "v"(Yc), "v"(Wc));             // (see the matrix path: keeps the per-pass wait a counted one)
  for (; iw < e; iw += GFH_FTHREADS) {
    const i64 in = iw + GFH_FTHREADS < e ? iw + GFH_FTHREADS : iw;
    const double Xn = (x + in)[lane], Yn = (y + in)[lane], Wn = (w + in)[lane];
    body(Xc, Yc, Wc);
    Xc = Xn; Yc = Yn; Wc = Wn;
  }
  // wave tree of the NACC sums: t_l += t_(l+32), += t_(l+16) through the LDS crossbar (ds_bpermute, what __shfl_down compiles to), then
  // += t_(l+8), (l+4), (l+2), (l+1) as DPP row shifts inside the 16 lanes of row 0 -- the additions __shfl_down's tree makes, the same
  // bits, with a third of the crossbar operations: 45 sums x 6 levels x 2 halves = 540 ds_bpermute per wave, all waves of the chip
  // at once at the end of the launch, were most of this kernel's epilogue (round 6)
#pragma unroll
  for (int k = 0; k < NACC; k++) {
    const double t = gfh_wave_sum(av[k]);
    if (lane == 0) red[wv][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int wq = 1; wq < GFH_FW; wq++) t += red[wq][threadIdx.x];
    tot[threadIdx.x] = t;
  }
  __syncthreads();
  double* out = partial + (i64)blockIdx.x * pstride;
  __shared__ double tail_img[273];                                   // (read by the single-workgroup tail below)
  for (int idx = threadIdx.x; idx < 273; idx += GFH_FTHREADS) {      // [16][16] tile (both triangles) | JTr[16] | rTr
    double t;
    if (idx < 256) {
      int a = idx >> 4, b = idx & 15;
      if (a > b) { const int t_ = a; a = b; b = t_; }
      t = b < GFH_NA ? tot[a * GFH_NA - a * (a - 1) / 2 + (b - a)] : 0.0;
    } else if (idx < 272) t = idx - 256 < GFH_NA ? tot[NP_ + idx - 256] : 0.0;
    else t = tot[NP_ + GFH_NA];
    GFH_ST_DEV(out + idx, t);
    tail_img[idx] = t;
  }
#elif GFH_COOP
  // ---- Workgroup-cooperative Gram (round 6): 81 ... 128 active parameters, 6 ... 8 tiles (model.h, fused_coop).  Up to 4 tiles every wave keeps ALL
  // T (T + 1) / 2 accumulator tiles for its own 64 points; that grows as T^2 (15 tiles = 120 registers at T = 5, 36 = 288 at T = 8)
  // next to a gradient of 2 NA registers that waits for the half-passes.  Here the waves still differentiate and stage their own
  // points (half stages: 32 points, stride 34) but after a barrier every wave reads ALL stages of the workgroup and owns a contiguous
  // run of the row-major list of tile pairs (GFH_CK = ceil(NPAIR / FW) of them: 4 ... 9 accumulator tiles): the registers stop
  // growing as T^2, nothing spills, and no cross-wave reduction of the pair images is left -- a pair's accumulator IS the workgroup's
  // sum.  Every pair is a plain v_mfma_f64_16x16x4_f64 on two fragments (the diagonal tiles too: their 4x4x4 form saves a third of
  // a tile's cycles but needs rotated fragments per owner); J^T r of tile t rides with the owner of pair (t, t) on the VALU; sum r^2
  // stays per lane over the lane's own points (gfh_k_chi2's order).  Points enter a pair's sum in the order stage of wave 0, 1, ...,
  // half 0 then half 1, pass by pass: fixed, so deterministic.
  constexpr int ROWS = 16 * GFH_T + 1;                       // parameters (padded to 16T) + residual row
  constexpr int STAGE = ROWS * GFH_S;
  constexpr int IMG = GFH_NPAIR * 256 + 16 * GFH_T + 1;      // the workgroup's sums (partial image)
  constexpr int EPI = GFH_T * 64 + 8 + IMG;                  // epilogue: J^T r fragments per tile | wave sums of r^2 | the image, laid over the stages
  static_assert(GFH_FW == 4, "the cooperative form is written for one wave per SIMD: GFH_CSTAGES / GFH_CPUT dispatch, coop_defines");
  __shared__ double lds[GFH_FW * STAGE > EPI ? GFH_FW * STAGE : EPI];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  double* __restrict__ st = lds + wv * STAGE;
  const i64 s0 = gb_start[blockIdx.x];
  const i64 e = s0 + gb_slots[blockIdx.x];                   // multiple of GFH_FTHREADS slots
  const double* __restrict__ P = GFH_PARS_AT(gb_ds[blockIdx.x]);
#pragma unroll
  for (int a = GFH_NA; a < 16 * GFH_T; a++) st[a * GFH_S + (lane & 31)] = 0.0;      // padding rows: zero once
  // this wave's pairs: a contiguous run of the row-major upper triangle (generator: coop_defines -- per wave W the macros
  // GFH_CLOAD_W(B, U): the fragments of the DISTINCT tiles its pairs touch, read once per k-step (a run of K pairs touches about
  // K / 2 + 2 tiles: a third of the 2 K reads a pair-by-pair form makes, and the LDS reads were this kernel's bottleneck);
  // GFH_CMMA_W(B): its matrix instructions and, for its diagonal pairs, J^T r on the VALU; GFH_CPUT_W: its part of the epilogue)
  constexpr int CK = GFH_CK;
  const int wvu = __builtin_amdgcn_readfirstlane(wv);
  gfh_d4 acc[CK];
  double accr[CK];
#pragma unroll
  for (int k = 0; k < CK; k++) { acc[k] = (gfh_d4){0.0, 0.0, 0.0, 0.0}; accr[k] = 0.0; }
  double accc = 0.0;
  i64 iw = s0 + 64 * __builtin_amdgcn_readfirstlane(wv);
  double Xc = (x + iw)[lane], Yc = (y + iw)[lane], Wc = (w + iw)[lane];
  asm volatile("" :: "v"(Xc), "v"(Yc), "v"(Wc));             // (see the matrix path below: keeps the per-pass wait a counted one)
  for (; iw < e; iw += GFH_FTHREADS) {
    const i64 in = iw + GFH_FTHREADS < e ? iw + GFH_FTHREADS : iw;
    const double Xn = (x + in)[lane], Yn = (y + in)[lane], Wn = (w + in)[lane];
    double F, G[GFH_NA];
    gfh_point_grad(Xc, P, F, G, status, aux + iw + lane, lda GFH_MESH_NONE GFH_SLOT(iw + lane));
    double R = (Yc - F) * Wc;                               // gadfit.F90:682-683
    double Wl = Wc;
    GFH_ROBUST(R, Wl)
    gfh_store64(res + iw, lane * 8, R);
    accc += R * R;                                          // every lane sums its own points pass by pass: the order gfh_k_chi2 uses
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) {
      G[a] = G[a] * Wl;                                     // gadfit.F90:689-690
#if GFH_STORE_J
      gfh_store64(J + iw + (i64)a * ldj, lane * 8, G[a]);
#endif
    }
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
      if ((lane >> 5) == h) {                                // this half's 32 points into the wave's stage
        st[16 * GFH_T * GFH_S + (lane & 31)] = R;
#pragma unroll
        for (int a = 0; a < GFH_NA; a++) st[a * GFH_S + (lane & 31)] = G[a];
      }
      __syncthreads();
      // 8 k-steps per stage, the stages in wave order; inside a stage the fragments of step u + 1 are read before the matrix
      // instructions of step u (the stage loop itself stays a loop: unrolled over all 8 FW steps the kernel spilled hundreds of registers)
#define GFH_CSTAGES(W_)                                                                                             \
      _Pragma("unroll 1") for (int sw = 0; sw < GFH_FW; sw++) {                                                     \
        const double* __restrict__ sb = lds + sw * STAGE;                                                           \
        double f[2][GFH_CND], fr[2];                                                                                 \
        GFH_CLOAD_##W_(0, 0)                                                                                        \
        _Pragma("unroll") for (int u = 0; u < 8; u++) {                                                             \
          /* the first matrix instruction of the step, THEN the next step's fragment reads (issued while it runs: a wave issues in   \
             order, and reads in front of the step's first matrix instruction cost their whole issue time), then the rest */         \
          __builtin_amdgcn_sched_barrier(0);                                                                        \
          if (u & 1) { GFH_CMMA0_##W_(1) } else { GFH_CMMA0_##W_(0) }                                               \
          __builtin_amdgcn_sched_barrier(0);                                                                        \
          if (u + 1 < 8) { if (u & 1) { GFH_CLOAD_##W_(0, u + 1) } else { GFH_CLOAD_##W_(1, u + 1) } }              \
          __builtin_amdgcn_sched_barrier(0);                                                                        \
          if (u & 1) { GFH_CMMA_##W_(1) } else { GFH_CMMA_##W_(0) }                                                 \
          __builtin_amdgcn_sched_barrier(0);                                                                        \
        }                                                                                                           \
      }
#define GFH_MFMA(A_, B_, C_) C_ = __builtin_amdgcn_mfma_f64_16x16x4f64(A_, B_, C_, 0, 0, 0)
      if (wvu == 0) { GFH_CSTAGES(0) }
      else if (wvu == 1) { GFH_CSTAGES(1) }
      else if (wvu == 2) { GFH_CSTAGES(2) }
      else { GFH_CSTAGES(3) }
      __syncthreads();
    }
    Xc = Xn; Yc = Yn; Wc = Wn;
  }
  // epilogue: the owners write their pairs straight into the workgroup's image (global partial + the LDS copy the one-workgroup tail reads)
  double* vecs = lds;
  double* wsum = lds + GFH_T * 64;
  double* tail_img = wsum + 8;
  double* out = partial + (i64)blockIdx.x * pstride;
#define GFH_CPUT(K_, PP_)                                                                                            \
  _Pragma("unroll") for (int j = 0; j < 4; j++) {       /* f64 16x16 C/D map: row = (l>>4) + 4*reg, column = l & 15 */ \
    const int idx = (PP_) * 256 + (q + 4 * j) * 16 + r;                                                              \
    GFH_ST_DEV(out + idx, acc[K_][j]);                                                                               \
    tail_img[idx] = acc[K_][j]; }
#define GFH_CPUTR(K_, T_) vecs[(T_) * 64 + lane] = accr[K_];
  if (wvu == 0) { GFH_CPUT_0 }
  else if (wvu == 1) { GFH_CPUT_1 }
  else if (wvu == 2) { GFH_CPUT_2 }
  else { GFH_CPUT_3 }
  {
    const double t = gfh_wave_sum(accc);                     // wave tree, then the waves in order: gfh_k_chi2's order
    if (lane == 0) wsum[wv] = t;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 16 * GFH_T; idx += GFH_FTHREADS) {
    const int t = idx >> 4, rr_ = idx & 15;
    const double sacc = ((vecs[t * 64 + rr_] + vecs[t * 64 + 16 + rr_]) + vecs[t * 64 + 32 + rr_]) + vecs[t * 64 + 48 + rr_];
    GFH_ST_DEV(out + GFH_NPAIR * 256 + idx, sacc);
    tail_img[GFH_NPAIR * 256 + idx] = sacc;
  }
  if (threadIdx.x == 0) {
    double sacc = wsum[0];
#pragma unroll
    for (int wq = 1; wq < GFH_FW; wq++) sacc += wsum[wq];
    GFH_ST_DEV(out + GFH_NPAIR * 256 + 16 * GFH_T, sacc);
    tail_img[GFH_NPAIR * 256 + 16 * GFH_T] = sacc;
  }
#else
  constexpr int ROWS = 16 * GFH_T + 1;                       // parameters (padded to 16T) + residual row
  constexpr int STAGE = ROWS * GFH_S;
  constexpr int RED = GFH_NPAIR * 256 + GFH_T * 64 + 4;      // cross-wave reduction image (as k_gram)
  constexpr int IMG = GFH_NPAIR * 256 + 16 * GFH_T + 1;      // the workgroup's own sums (partial image), kept for the single-workgroup tail
#if GFH_RED1
  // 5 tiles: ONE pair image that the waves add into in order + the waves' J^T r / r^T r vectors + the workgroup's sums,
  // laid over the stages once the pass loop is done (model.h, fused_lds_bytes_for)
  constexpr int VEC = GFH_T * 64 + 4;
  constexpr int RED1 = GFH_NPAIR * 256 + GFH_FW * VEC + IMG;
  __shared__ double lds[GFH_FW * STAGE > RED1 ? GFH_FW * STAGE : RED1];
#else
  __shared__ double lds[GFH_FW * (STAGE > RED ? STAGE : RED)];
#endif
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  double* __restrict__ st = lds + wv * STAGE;
  const i64 s0 = gb_start[blockIdx.x];
  const i64 e = s0 + gb_slots[blockIdx.x];                   // multiple of GFH_FTHREADS slots
  const double* __restrict__ P = GFH_PARS_AT(gb_ds[blockIdx.x]);

  // rows GFH_NA .. 16T-1 of the stage are padding: zero once
#pragma unroll
  for (int a = GFH_NA; a < 16 * GFH_T; a++) st[a * GFH_S + (lane & (64 / GFH_NH - 1))] = 0.0;

  gfh_d4 acc[GFH_NPAIR];
#pragma unroll
  for (int p = 0; p < GFH_NPAIR; p++) acc[p] = (gfh_d4){0.0, 0.0, 0.0, 0.0};
  // Diagonal tiles: only 10 of the 16 4x4 blocks of a symmetric 16x16 tile are distinct, and
  // v_mfma_f64_4x4x4_4b_f64 (four independent 4x4 blocks, 17.5 cycles against 64, tools/microbench/mfma_4x4.hip) takes
  // its A operand in exactly the fragment layout of the 16x16x4 form (lane = 16 k + 4 block + row).  With B = the same
  // fragment it yields the four diagonal blocks (b,b); with B read from rows rotated by one block, (b,b+1 mod 4) -- which is
  // (0,1) (1,2) (2,3) and (3,0) = (0,3) transposed; the remaining (0,2) (1,3) of TWO tiles share one more instruction whose
  // lanes of blocks 0,1 read the first tile and those of blocks 2,3 the second (rows rotated by two blocks for B).
  // 2.5 x 17.5 cycles per diagonal tile and k-step instead of 64.
  constexpr int NMIX = GFH_T / 2;
  double dga[GFH_T], dgb[GFH_T], dgm[NMIX + 1];
#pragma unroll
  for (int t = 0; t < GFH_T; t++) dga[t] = dgb[t] = 0.0;
#pragma unroll
  for (int m = 0; m <= NMIX; m++) dgm[m] = 0.0;
  const int r4 = (r + 4) & 15, r8 = (r + 8) & 15, hi = r >> 3;
  double accr[GFH_T];
#pragma unroll
  for (int t = 0; t < GFH_T; t++) accr[t] = 0.0;
  double accc = 0.0;

  // iw: first slot of this wave's pass, kept wave-uniform (SGPRs) so every global access is
  // "scalar base + lane*8": no per-lane 64-bit address arithmetic, 32-bit offsets to the TA
  i64 iw = s0 + 64 * __builtin_amdgcn_readfirstlane(wv);
  // every workgroup owns at least one whole pass (gb_slots is a positive multiple of GFH_FTHREADS)
  double Xc = (x + iw)[lane], Yc = (y + iw)[lane], Wc = (w + iw)[lane];
  // The first pass's inputs are consumed here, outside the loop.  vmcnt counts loads and stores in
  // issue order; if these loads were still pending at the loop header the compiler would have to
  // wait for the loop-carried inputs with vmcnt(2) -- correct for this entry path, but on the
  // back edge it means "every Jacobian store of the previous pass has completed": a full drain of
  // the store queue at the top of every pass.  With a clean entry state the wait inside the loop
  // is the counted one (the 3 prefetch loads are OLDER than the pass's stores).
  asm volatile("" :: "v"(Xc), "v"(Yc), "v"(Wc));
#if GFH_AD_PRIO
  __builtin_amdgcn_s_setprio(3);                             // (the AD phase of the first pass; GenConfig::store_j)
#endif
  for (; iw < e; iw += GFH_FTHREADS) {
    // prefetch the next pass's inputs before the long compute phase (the last pass re-reads its
    // own: no branch, so the number of memory operations in flight is the same on every path)
    const i64 in = iw + GFH_FTHREADS < e ? iw + GFH_FTHREADS : iw;
    const double Xn = (x + in)[lane], Yn = (y + in)[lane], Wn = (w + in)[lane];
    double* __restrict__ Jw = J + iw;
    double F, G[GFH_NA];
    gfh_point_grad(Xc, P, F, G, status, aux + iw + lane, lda GFH_MESH_NONE GFH_SLOT(iw + lane));
    double R = (Yc - F) * Wc;                               // gadfit.F90:682-683
    double Wl = Wc;
    GFH_ROBUST(R, Wl)
    gfh_store64(res + iw, lane * 8, R);
    accc += R * R;                                          // every lane sums its own points pass by pass: the order gfh_k_chi2 uses
#if !GFH_HALF
    st[16 * GFH_T * GFH_S + lane] = R;
#endif
#pragma unroll
    for (int a = 0; a < GFH_NA; a++) {
      G[a] = G[a] * Wl;                                     // gadfit.F90:689-690
#if !GFH_HALF
      st[a * GFH_S + lane] = G[a];
#endif
    }
#if GFH_STORE_J
    // phase alignment (the stage itself is wave-private): with the Jacobian stores in the matrix phase the kernel is faster when
    // the waves of a workgroup are in the same phase (0.53 against 0.58 ms); without them it is the FP64 pipe alone and any
    // barrier is idle time (0.352 against 0.334 ms)
    __syncthreads();
#endif
    // k-steps: the fragment reads of step s+1 are issued while the matrix instructions of step s run, so the
    // LDS latency hides under them (sched_barrier pins the order)
    double fn[GFH_T], f4n[GFH_T], man[NMIX + 1], mbn[NMIX + 1], rn;
#define GFH_FRAGS(S_)                                                                                            \
    _Pragma("unroll") for (int t = 0; t < GFH_T; t++) {                                                          \
      fn[t] = st[(16 * t + r) * GFH_S + 4 * (S_) + q];                                                           \
      f4n[t] = st[(16 * t + r4) * GFH_S + 4 * (S_) + q];                                                         \
    }                                                                                                            \
    _Pragma("unroll") for (int m = 0; m < NMIX; m++) {                                                           \
      man[m] = st[(16 * (2 * m + hi) + r) * GFH_S + 4 * (S_) + q];                                               \
      mbn[m] = st[(16 * (2 * m + hi) + r8) * GFH_S + 4 * (S_) + q];                                              \
    }                                                                                                            \
    if (GFH_T & 1) mbn[NMIX] = st[(16 * (GFH_T - 1) + r8) * GFH_S + 4 * (S_) + q];                               \
    rn = st[16 * GFH_T * GFH_S + 4 * (S_) + q];
#if GFH_AD_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
#pragma unroll
    for (int h = 0; h < GFH_NH; h++) {
#if GFH_HALF
      // this half's 32 points into the stage (the fragment reads of the half before are older LDS operations of this wave:
      // the LDS executes a wave's operations in order)
      if ((lane >> 5) == h) {
        st[16 * GFH_T * GFH_S + (lane & 31)] = R;
#pragma unroll
        for (int a = 0; a < GFH_NA; a++) st[a * GFH_S + (lane & 31)] = G[a];
      }
#endif
      // (the first k-step's reads stay a one-trip loop: written out straight they compile to another instruction order)
#pragma unroll
      for (int s = 0; s < 1; s++) { GFH_FRAGS(s) }
#pragma unroll
      for (int s = 0; s < GFH_KS; s++) {
        double fa[GFH_T], f4[GFH_T], ma[NMIX + 1], mb[NMIX + 1];
#pragma unroll
        for (int t = 0; t < GFH_T; t++) { fa[t] = fn[t]; f4[t] = f4n[t]; }
#pragma unroll
        for (int m = 0; m <= NMIX; m++) { ma[m] = man[m]; mb[m] = mbn[m]; }
        const double rr = rn;
        __builtin_amdgcn_sched_barrier(0);
        int p = 0;
#pragma unroll
        for (int ti = 0; ti < GFH_T; ti++)
#pragma unroll
          for (int tj = ti; tj < GFH_T; tj++, p++)
            if (tj > ti) acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ti], fa[tj], acc[p], 0, 0, 0);
        // the next step's fragment reads go out BEHIND this step's 64-cycle matrix instructions (issued, they run by themselves):
        // the wave's LDS instructions then cost the shared FP64 pipe no idle issue slots (round 5: no-store 0.3135 -> 0.299 ms,
        // stored 0.209 -> 0.178 ms at N = 4e6, against the reads in front of them)
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < GFH_KS) { GFH_FRAGS(s + 1) }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < GFH_T; t++) {
          dga[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(fa[t], fa[t], dga[t], 0, 0, 0);
          dgb[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(fa[t], f4[t], dgb[t], 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < NMIX; m++) dgm[m] = __builtin_amdgcn_mfma_f64_4x4x4f64(ma[m], mb[m], dgm[m], 0, 0, 0);
        if (GFH_T & 1) dgm[NMIX] = __builtin_amdgcn_mfma_f64_4x4x4f64(fa[GFH_T - 1], mb[NMIX], dgm[NMIX], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < GFH_T; t++) accr[t] += fa[t] * rr;
#if GFH_STORE_J
        // Jacobian columns leave for HBM a few per k-step, under the matrix instructions,
        // instead of as one burst that stalls the wave on a full store queue
#pragma unroll
        for (int a = (h * GFH_KS + s) * ((GFH_NA + 15) / 16); a < (h * GFH_KS + s + 1) * ((GFH_NA + 15) / 16) && a < GFH_NA; a++)
          gfh_store64(Jw + (i64)a * ldj, lane * 8, G[a]);
#endif
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#if GFH_AD_PRIO
    __builtin_amdgcn_s_setprio(3);
#endif
#if GFH_STORE_J
    __syncthreads();
#endif
    Xc = Xn; Yc = Yn; Wc = Wn;
  }

#if GFH_AD_PRIO
  __builtin_amdgcn_s_setprio(0);
#endif
#if GFH_RED1
  // cross-wave reduction, 5 tiles: the waves add their accumulators into ONE image in wave order -- ((w0 + w1) + w2) + w3,
  // the order in which the per-wave images of the smaller kernels are added -- then J^T r and r^T r from per-wave vectors as there
  __syncthreads();                                           // (every wave is done with its stage: the image lies over them)
  double* img1 = lds;
  double* vecs = lds + GFH_NPAIR * 256;
  double* tail_img = vecs + GFH_FW * VEC;
#define GFH_PUT(IDX_, V_) { if (first) img1[IDX_] = (V_); else img1[IDX_] += (V_); }
  for (int wq = 0; wq < GFH_FW; wq++) {
    if (wv == wq) {
      const bool first = wq == 0;
      int p = 0;
#pragma unroll
      for (int ti = 0; ti < GFH_T; ti++)
#pragma unroll
        for (int tj = ti; tj < GFH_T; tj++, p++) {
          if (tj > ti) {
#pragma unroll
            for (int j = 0; j < 4; j++) GFH_PUT(p * 256 + (q + 4 * j) * 16 + r, acc[p][j])
          } else {
            const int row = (r & 12) + q;
            GFH_PUT(p * 256 + row * 16 + r, dga[ti])
            GFH_PUT(p * 256 + row * 16 + r4, dgb[ti])
            GFH_PUT(p * 256 + r4 * 16 + row, dgb[ti])
          }
        }
#pragma unroll
      for (int m = 0; m < NMIX; m++) {
        const int t = 2 * m + hi, pd = t * GFH_T - t * (t - 1) / 2, row = (r & 12) + q;
        GFH_PUT(pd * 256 + row * 16 + r8, dgm[m])
        GFH_PUT(pd * 256 + r8 * 16 + row, dgm[m])
      }
      if ((GFH_T & 1) && !hi) {
        const int t = GFH_T - 1, pd = t * GFH_T - t * (t - 1) / 2, row = (r & 12) + q;
        GFH_PUT(pd * 256 + row * 16 + r8, dgm[NMIX])
        GFH_PUT(pd * 256 + r8 * 16 + row, dgm[NMIX])
      }
    }
    __syncthreads();
  }
#undef GFH_PUT
  {
    double* myvec = vecs + wv * VEC;
#pragma unroll
    for (int t = 0; t < GFH_T; t++) myvec[t * 64 + lane] = accr[t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) accc += __shfl_down(accc, off, 64);
    if (lane == 0) myvec[GFH_T * 64] = accc;
  }
  __syncthreads();
  double* out = partial + (i64)blockIdx.x * pstride;
  for (int idx = threadIdx.x; idx < GFH_NPAIR * 256; idx += GFH_FTHREADS) {
    const double sacc = img1[idx];
    GFH_ST_DEV(out + idx, sacc);
    tail_img[idx] = sacc;
  }
  for (int idx = threadIdx.x; idx < 16 * GFH_T; idx += GFH_FTHREADS) {
    const int t = idx >> 4, rr_ = idx & 15;
    double sacc = 0.0;
#pragma unroll
    for (int wq = 0; wq < 4 * GFH_FW; wq++) sacc += vecs[(wq >> 2) * VEC + t * 64 + (wq & 3) * 16 + rr_];
    GFH_ST_DEV(out + GFH_NPAIR * 256 + idx, sacc);
    tail_img[GFH_NPAIR * 256 + idx] = sacc;
  }
  if (threadIdx.x == 0) {
    double sacc = vecs[GFH_T * 64];
#pragma unroll
    for (int wq = 1; wq < GFH_FW; wq++) sacc += vecs[wq * VEC + GFH_T * 64];
    GFH_ST_DEV(out + GFH_NPAIR * 256 + 16 * GFH_T, sacc);
    tail_img[GFH_NPAIR * 256 + 16 * GFH_T] = sacc;
  }
#else
  // cross-wave reduction in fixed order (deterministic), same image as k_gram
  __syncthreads();
  double* mine = lds + wv * RED;
  {
    int p = 0;
#pragma unroll
    for (int ti = 0; ti < GFH_T; ti++)
#pragma unroll
      for (int tj = ti; tj < GFH_T; tj++, p++) {
        if (tj > ti) {
#pragma unroll
          for (int j = 0; j < 4; j++) mine[p * 256 + (q + 4 * j) * 16 + r] = acc[p][j];   // f64 16x16 C/D map: row = (l>>4) + 4*reg
        } else {
          // 4x4x4 C/D map: lane = 16 row + 4 block + column; both triangles of the tile image are filled
          const int row = (r & 12) + q;
          mine[p * 256 + row * 16 + r] = dga[ti];
          mine[p * 256 + row * 16 + r4] = dgb[ti];
          mine[p * 256 + r4 * 16 + row] = dgb[ti];
        }
      }
#pragma unroll
    for (int m = 0; m < NMIX; m++) {
      const int t = 2 * m + hi, pd = t * GFH_T - t * (t - 1) / 2, row = (r & 12) + q;
      mine[pd * 256 + row * 16 + r8] = dgm[m];
      mine[pd * 256 + r8 * 16 + row] = dgm[m];
    }
    if ((GFH_T & 1) && !hi) {             // (blocks 2,3 of the unpaired tile hold the transposes of blocks 0,1: one writer each)
      const int t = GFH_T - 1, pd = t * GFH_T - t * (t - 1) / 2, row = (r & 12) + q;
      mine[pd * 256 + row * 16 + r8] = dgm[NMIX];
      mine[pd * 256 + r8 * 16 + row] = dgm[NMIX];
    }
  }
#pragma unroll
  for (int t = 0; t < GFH_T; t++) mine[GFH_NPAIR * 256 + t * 64 + lane] = accr[t];
  // sum r^2: wave tree, then the waves in order -- the same tree and order as gfh_k_chi2, so chi2() at the
  // parameters of a sweep returns bitwise this sweep's sum
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) accc += __shfl_down(accc, off, 64);
  if (lane == 0) mine[GFH_NPAIR * 256 + GFH_T * 64] = accc;
  __syncthreads();
  double* out = partial + (i64)blockIdx.x * pstride;
  // (the sums also stay in LDS for the single-workgroup tail below: the pair images in tail_pairs, J^T r and r^T r behind them)
  __shared__ double tail_img[GFH_NPAIR * 256 + 16 * GFH_T + 1];
  for (int idx = threadIdx.x; idx < GFH_NPAIR * 256; idx += GFH_FTHREADS) {
    double sacc = lds[idx];
#pragma unroll
    for (int wq = 1; wq < GFH_FW; wq++) sacc += lds[wq * RED + idx];
    GFH_ST_DEV(out + idx, sacc);
    tail_img[idx] = sacc;
  }
  for (int idx = threadIdx.x; idx < 16 * GFH_T; idx += GFH_FTHREADS) {
    const int t = idx >> 4, rr_ = idx & 15;
    double sacc = 0.0;
#pragma unroll
    for (int wq = 0; wq < 4 * GFH_FW; wq++) sacc += lds[(wq >> 2) * RED + GFH_NPAIR * 256 + t * 64 + (wq & 3) * 16 + rr_];
    GFH_ST_DEV(out + GFH_NPAIR * 256 + idx, sacc);
    tail_img[GFH_NPAIR * 256 + idx] = sacc;
  }
  if (threadIdx.x == 0) {
    double sacc = lds[GFH_NPAIR * 256 + GFH_T * 64];
#pragma unroll
    for (int wq = 1; wq < GFH_FW; wq++) sacc += lds[wq * RED + GFH_NPAIR * 256 + GFH_T * 64];
    GFH_ST_DEV(out + GFH_NPAIR * 256 + 16 * GFH_T, sacc);
    tail_img[GFH_NPAIR * 256 + 16 * GFH_T] = sacc;
  }
#endif  // GFH_RED1
#endif  // GFH_NA <= GFH_VALU_GRAM_MAX
  if (!tail_mode) return;

  // ---- tail (STEP 2's sum over workgroups, gadfit.F90:698-699, and the scatter through
  // Jacobian_indices): what k_reduce_partials + k_assemble + k_publish do as three more launches,
  // done here by the workgroups that finish last, in exactly their order of additions (bitwise the
  // same numbers).  Level 1: the workgroups b0+sl, b0+sl+32, ... of a dataset form slice sl; the last
  // of them to arrive adds their partials in ascending order.  Level 2: the workgroup that completes
  // the last slice adds the 32 slice sums of every dataset in slice order, assembles the packed
  // [JTJ | JTres | chi2] and (tail_mode 2) writes it, the status word and the call's sequence number
  // into the host mailbox.
  // Cross-workgroup traffic (partials, slice sums, counters) moves ONLY through device-scope atomic
  // loads/stores (sc1: written through to / read from memory, past the per-XCD L2s, which are not
  // coherent with each other), each producer waiting for its stores to be acknowledged (vmcnt(0))
  // before its arrival is counted.  A release fence would do the same job by writing back the whole
  // L2 -- which in this kernel is full of dirty Jacobian lines: measured +50 us per launch.
  constexpr int W = GFH_NPAIR * 256 + 16 * GFH_T + 1;
  __shared__ int role;
  const int d = gb_ds[blockIdx.x];
  // Assembly of the packed [JTJ | JTres | chi2] from per-dataset images (source `src`, image of dataset dd at src + dd * stride,
  // datasets [d_lo, d_hi)), the scatter through Jacobian_indices, and (tail_mode 2) the host mailbox.
  auto assemble_and_post = [&](auto at, const int d_lo, const int d_hi) {       // at(dd, k): entry k of dataset dd's image
    const int dim = tl->dim;
    const i64 nn = (i64)dim * dim, total = nn + dim + 1;
    const int* __restrict__ inv = tl->inv;
    double* packed = tl->packed;
    double* host_out = tl->host_out;
    for (i64 idx = threadIdx.x; idx < total; idx += GFH_FTHREADS) {
      double v = 0.0;
      if (idx < nn) {
        const int col = (int)(idx / dim), row = (int)(idx % dim);
        for (int dd = d_lo; dd < d_hi; dd++) {
          int a = inv[dd * dim + row], b = inv[dd * dim + col];
          if (a < 0 || b < 0) continue;
          if (a > b) { const int t_ = a; a = b; b = t_; }     // upper triangle of tile pairs is stored
          const int ti = a >> 4, tj = b >> 4;
          const int p = ti * GFH_T - ti * (ti - 1) / 2 + (tj - ti);
          v += at(dd, p * 256 + (a & 15) * 16 + (b & 15));
        }
      } else if (idx < nn + dim) {
        const int row = (int)(idx - nn);
        for (int dd = d_lo; dd < d_hi; dd++) {
          const int a = inv[dd * dim + row];
          if (a >= 0) v += at(dd, GFH_NPAIR * 256 + a);
        }
      } else {
        for (int dd = d_lo; dd < d_hi; dd++) v += at(dd, GFH_NPAIR * 256 + 16 * GFH_T);
      }
      packed[idx] = v;
      if (tail_mode == 2) GFH_ST_SYS(host_out + idx, v);       // pinned host memory is uncached: the store goes straight out
    }
    if (tail_mode != 2) {
      // (one process per GPU: element `total` of the packed buffer is the status slot of the cross-rank sum that follows --
      // 0, 1, 4096, 2^24 by code, so the sum over the ranks still tells which codes occurred: comm.cpp, allreduce_sum)
      if (threadIdx.x == 0) packed[total] = GFH_STATUS_SLOT(GFH_LD_DEV(status));
      return;
    }
    // the status word travels with the data (every workgroup's status updates were acknowledged before its arrival was
    // counted, this workgroup's own before the barrier in front of this call): ONE wait for the stores to host memory, then the flag
    if (threadIdx.x == 0) GFH_ST_SYS(host_out + total, (double)GFH_LD_DEV(status));
    asm volatile("s_waitcnt vmcnt(0)\n" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(GFH_GLOBAL(tl->host_flag), seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  };
  if (gridDim.x == 1) {
    // One workgroup (the small fits most of gadfit's use consists of): its partial IS the sum over workgroups of its dataset --
    // the two levels of the hand-off below would add 0.0 to it twice and cost five round trips to memory.  The same numbers
    // (0.0 + t in the assembly, as there), bitwise.
    // The sums are still in LDS (tail_img, written next to the partial image above): no trip through memory either.
    __syncthreads();
    assemble_and_post([&](int, int k) { return tail_img[k]; }, d, d + 1);
    return;
  }
  const int b0 = tl->ds_first_gb[d], b1 = tl->ds_first_gb[d + 1];
  const int sl = ((int)blockIdx.x - b0) & 31;
  unsigned* cnt = tl->counters;
  asm volatile("s_waitcnt vmcnt(0)\n" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned members = (unsigned)((b1 - b0 - sl + 31) >> 5);
    const bool last = __hip_atomic_fetch_add(GFH_GLOBAL(cnt + 1 + d * 32 + sl), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1;
    if (last) GFH_ST_DEV(cnt + 1 + d * 32 + sl, 0u);          // ready for the next launch (stream-ordered)
    role = last;
  }
  __syncthreads();
  if (!role) return;
  {
    double* sdst = tl->slice + ((i64)d * 32 + sl) * pstride;
    for (int idx = threadIdx.x; idx < W; idx += GFH_FTHREADS) {
      double sacc = 0.0;
      for (int b = b0 + sl; b < b1; b += 32 * 16) {           // 16 loads in flight, added in ascending order
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = b + 32 * u < b1 ? GFH_LD_DEV(partial + (i64)(b + 32 * u) * pstride + idx) : 0.0;
#pragma unroll
        for (int u = 0; u < 16; u++) if (b + 32 * u < b1) sacc += v[u];
      }
      GFH_ST_DEV(sdst + idx, sacc);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)\n" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool last = __hip_atomic_fetch_add(GFH_GLOBAL(cnt), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)tl->n_slices - 1;
    if (last) GFH_ST_DEV(cnt, 0u);
    role = last;
  }
  __syncthreads();
  if (!role) return;
  const int nd = tl->nd;
  double* G = tl->G;                                          // written and read by this workgroup only
  for (int dd = 0; dd < nd; dd++) {
    const int nb = tl->ds_first_gb[dd + 1] - tl->ds_first_gb[dd];
    const double* ssrc = tl->slice + (i64)dd * 32 * pstride;
    for (int idx = threadIdx.x; idx < W; idx += GFH_FTHREADS) {
      double v[32];
#pragma unroll
      for (int k = 0; k < 32; k++) v[k] = k < nb ? GFH_LD_DEV(ssrc + (i64)k * pstride + idx) : 0.0;
      double t = v[0];
#pragma unroll
      for (int k = 1; k < 32; k++) t += v[k];
      G[(i64)dd * pstride + idx] = t;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)\n" ::: "memory");
  __syncthreads();
  assemble_and_post([&](int dd, int k) { return G[(i64)dd * pstride + k]; }, 0, nd);
}

#endif  // GFH_NA <= GFH_FUSED_MAX && !GFH_WSG
