// gram.hip -- STEP 2 from a stored Jacobian: J^T J / J^T r / sum r^2 per gram block on the FP64 matrix cores (gadfit.F90:695-699),
// as three kernel families and the rule that picks one (launch_gram).  All of them write the Gram image of gram_image.h, one per
// workgroup; assemble.hip sums and scatters them.
//
// Layout contract: J is [NA][ldj] parameter-major over padded slots; every
// gram block covers whole 256-slot tiles of ONE dataset; pad slots hold zeros in J and res.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "codegen.h"

namespace gfh {

typedef double double4_t __attribute__((ext_vector_type(4)));

// The wave tree gfh_wave_sum: the one definition that the generated kernels carry too (device_text.cpp embeds the same file)
#include "device/wave_sum.hip"

// --------------------------------------------------------------------------------------
// The steps of k_gram_block's epilogue up to 4 x 4 tiles: cross-wave reduction in LDS, fixed order (deterministic).  A wave's LDS
// image is [NACC tiles as in the Gram image][TR * 64 J^T r lane sums][4]; the images of the four waves lie `ws` doubles apart.
// (k_gram spells the same steps out: through these functions k_gram<2> measured 1 - 2 % slower, twice.)

// a wave's accumulator tiles into its image.  f64 16x16x4 C/D map: col = lane&15, row = (lane>>4) + 4*reg
template <int NACC>
static __device__ __forceinline__ void spill_tiles(double* mine, const double4_t (&acc)[NACC], const int r, const int q) {
#pragma unroll
  for (int p = 0; p < NACC; p++)
#pragma unroll
    for (int j = 0; j < 4; j++) mine[gram_tile_at(p, q + 4 * j, r)] = acc[p][j];
}
// element idx of the four wave images, waves in order
static __device__ __forceinline__ double sum_wave_images(const double* img, const int ws, const int idx) {
  return ((img[idx] + img[ws + idx]) + img[2 * ws + idx]) + img[3 * ws + idx];
}
// J^T r of row rr of tile t: the four lane quarters of the four waves' sums, in order (vec = the first wave's lane sums)
static __device__ __forceinline__ double jtr_row_sum(const double* vec, const int ws, const int t, const int rr) {
  double sacc = 0.0;
#pragma unroll
  for (int w = 0; w < 4; w++)
#pragma unroll
    for (int qq = 0; qq < 4; qq++) sacc += vec[w * ws + t * 64 + qq * 16 + rr];
  return sacc;
}

// --------------------------------------------------------------------------------------
// Gram kernel.  One wave owns 16x16 accumulator tiles of the (NA x NA) per-dataset Gram
// matrix; a k-step of v_mfma_f64_16x16x4_f64 consumes 4 data points.  Lane (r = l&15,
// q = l>>4) holds J[16t + r][n + 4q .. 4q+3] as one 32-byte load, i.e. a wave instruction
// reads 16 rows x 128 B (full cache lines).  The SAME fragment serves as A operand of row
// tile t and as B operand of column tile t (A[i][k] and B[k][j] have identical lane maps for
// a symmetric product), so each J element is loaded exactly once per wave.
// J^T r rides along on the VALU (2 FMAs per fragment), sum r^2 likewise.
//
// T = number of 16-row tiles (NA <= 16 T).
template <int T>
__global__ __launch_bounds__(256) void k_gram(const double* __restrict__ J, const i64 ldj, const int na,
                                              const double* __restrict__ res,
                                              const i64* __restrict__ gb_start, const int* __restrict__ gb_slots,
                                              double* __restrict__ partial, const int pstride) {
  constexpr int NPAIR = T * (T + 1) / 2;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const i64 s = gb_start[blockIdx.x];
  const i64 e = s + gb_slots[blockIdx.x];

  double4_t acc[NPAIR];
#pragma unroll
  for (int p = 0; p < NPAIR; p++) acc[p] = (double4_t){0.0, 0.0, 0.0, 0.0};
  double accr[T];
#pragma unroll
  for (int t = 0; t < T; t++) accr[t] = 0.0;
  double accc = 0.0;

  const double* jrow[T];
  bool valid[T];
#pragma unroll
  for (int t = 0; t < T; t++) {
    valid[t] = (16 * t + r) < na;
    jrow[t] = J + (i64)(valid[t] ? 16 * t + r : 0) * ldj;
  }

  // Register double buffer: the 4 (T + 1) fragment loads of the NEXT 64 points are in flight while the matrix instructions of
  // this pass run (the last pass re-reads its own: no branch).  Same thread-to-point map and order of additions as the
  // single-buffered loop this replaces (0.61 -> 0.47 ms at 32 columns: the pass was load latency + 48 MFMAs, back to back).
  auto load = [&](const i64 n, double4_t (&a)[4][T], double4_t (&rr)[4]) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const i64 c = n + 16 * u + 4 * q;
#pragma unroll
      for (int t = 0; t < T; t++) a[u][t] = *reinterpret_cast<const double4_t*>(jrow[t] + c);
      rr[u] = *reinterpret_cast<const double4_t*>(res + c);
    }
  };
  double4_t a[4][T], rr[4];
  i64 n = s + 64 * wv;
  constexpr bool kDouble = T <= 2;      // (3 and 4 tiles: two buffers would not fit 256 VGPRs next to 6 / 10 accumulator tiles)
  if (kDouble && n < e) load(n, a, rr);
  for (; n < e; n += 256) {
    double4_t an[4][T], rn[4];
    if (kDouble) load(n + 256 < e ? n + 256 : n, an, rn);
    else load(n, a, rr);
#pragma unroll
    for (int u = 0; u < 4; u++) {
#pragma unroll
      for (int t = 0; t < T; t++)
        if (!valid[t]) a[u][t] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        int p = 0;
#pragma unroll
        for (int ti = 0; ti < T; ti++)
#pragma unroll
          for (int tj = ti; tj < T; tj++, p++)
            acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][ti][j], a[u][tj][j], acc[p], 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < T; t++)
        accr[t] += a[u][t][0] * rr[u][0] + a[u][t][1] * rr[u][1] + a[u][t][2] * rr[u][2] + a[u][t][3] * rr[u][3];
      accc += rr[u][0] * rr[u][0] + rr[u][1] * rr[u][1] + rr[u][2] * rr[u][2] + rr[u][3] * rr[u][3];
    }
    if (kDouble) {
#pragma unroll
      for (int u = 0; u < 4; u++) {
#pragma unroll
        for (int t = 0; t < T; t++) a[u][t] = an[u][t];
        rr[u] = rn[u];
      }
    }
  }

  // cross-wave reduction in LDS, fixed order (deterministic).
  __shared__ double sm[4][NPAIR * 256 + T * 64 + 4];
  double* mine = sm[wv];
#pragma unroll
  for (int p = 0; p < NPAIR; p++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      // f64 16x16x4 C/D map: col = lane&15, row = (lane>>4) + 4*reg
      mine[p * 256 + (q + 4 * j) * 16 + r] = acc[p][j];
    }
#pragma unroll
  for (int t = 0; t < T; t++) mine[NPAIR * 256 + t * 64 + lane] = accr[t];
  if (r == 0) mine[NPAIR * 256 + T * 64 + q] = accc;
  __syncthreads();
  double* out = partial + (i64)blockIdx.x * pstride;
  constexpr int JTR = gram_jtr(0, T), RTR = gram_rtr(T);
  for (int idx = threadIdx.x; idx < NPAIR * 256; idx += 256)
    out[idx] = ((sm[0][idx] + sm[1][idx]) + sm[2][idx]) + sm[3][idx];
  for (int idx = threadIdx.x; idx < 16 * T; idx += 256) {
    const int t = idx >> 4, rr_ = idx & 15;
    double sacc = 0.0;
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
      for (int qq = 0; qq < 4; qq++) sacc += sm[w][NPAIR * 256 + t * 64 + qq * 16 + rr_];
    out[JTR + idx] = sacc;
  }
  if (threadIdx.x == 0) {
    double sacc = 0.0;
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
      for (int qq = 0; qq < 4; qq++) sacc += sm[w][NPAIR * 256 + T * 64 + qq];
    out[RTR] = sacc;
  }
}

// --------------------------------------------------------------------------------------
// Up to 8 active parameters: a 16-row matrix tile would be half empty (and half of every fragment load redundant), and
// the whole per-point outer product is NA (NA + 1) / 2 + NA + 1 <= 45 multiply-adds -- nothing next to the 8 (NA + 1)
// bytes the point costs to read.  So this is a plain streaming kernel: one lane per point, the NA Jacobian entries and
// the residual as coalesced loads (two points per lane in flight), every product accumulated per lane, 8 waves per gram
// block, wave tree + waves in order at the end.  Writes the partial image of k_gram<1>.
template <int NA>
__global__ __launch_bounds__(512) void k_gram_small(const double* __restrict__ J, const i64 ldj, const double* __restrict__ res,
                                                     const i64* __restrict__ gb_start, const int* __restrict__ gb_slots,
                                                     double* __restrict__ partial, const int pstride) {
  constexpr int NP = NA * (NA + 1) / 2, NACC = NP + NA + 1;
  const i64 s = gb_start[blockIdx.x], e = s + gb_slots[blockIdx.x];
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; k++) acc[k] = 0.0;
  // two points per trip (512 apart: gb_slots is a multiple of 512), their loads issued together
  for (i64 i = s + threadIdx.x; i < e; i += 1024) {
    const bool two = i + 512 < e;
    const i64 i2 = two ? i + 512 : i;
    double j[NA], k[NA];
#pragma unroll
    for (int a = 0; a < NA; a++) { j[a] = J[(i64)a * ldj + i]; k[a] = J[(i64)a * ldj + i2]; }
    const double r = res[i], r2 = res[i2];
    int p = 0;
#pragma unroll
    for (int a = 0; a < NA; a++)
#pragma unroll
      for (int b = a; b < NA; b++, p++) acc[p] += j[a] * j[b];
#pragma unroll
    for (int a = 0; a < NA; a++) acc[NP + a] += j[a] * r;
    acc[NP + NA] += r * r;
    if (two) {
      p = 0;
#pragma unroll
      for (int a = 0; a < NA; a++)
#pragma unroll
        for (int b = a; b < NA; b++, p++) acc[p] += k[a] * k[b];
#pragma unroll
      for (int a = 0; a < NA; a++) acc[NP + a] += k[a] * r2;
      acc[NP + NA] += r2 * r2;
    }
  }
  __shared__ double sm[8][NACC];
  __shared__ double tot[NACC];
#pragma unroll
  for (int k = 0; k < NACC; k++) {
    const double t = gfh_wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    double t = sm[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < 8; w++) t += sm[w][threadIdx.x];
    tot[threadIdx.x] = t;
  }
  __syncthreads();
  // the image at T = 1, an element per thread; tot = [upper triangle of the NA x NA product, row by row | J^T r | sum r^2]
  double* out = partial + (i64)blockIdx.x * pstride;
  constexpr int JTR = gram_jtr(0, 1), RTR = gram_rtr(1);
  const int idx = threadIdx.x;
  if (idx < JTR) {
    int a = idx >> 4, b = idx & 15;                          // (= gram_tile_at(0, a, b))
    if (a > b) { const int t = a; a = b; b = t; }
    out[idx] = b < NA ? tot[a * NA - a * (a - 1) / 2 + (b - a)] : 0.0;      // both triangles of the one 16 x 16 tile
  } else if (idx < RTR) out[idx] = idx - JTR < NA ? tot[NP + idx - JTR] : 0.0;
  else if (idx == RTR) out[idx] = tot[NP + NA];
}

// --------------------------------------------------------------------------------------
// More than 64 active parameters per dataset (T > 4 tiles): the Gram image is formed in blocks of up to
// 4 x 4 tiles, one launch per block pair (gi <= gj) of the upper triangle.  A launch loads the row tiles
// R0 .. R0+TR-1 and the column tiles C0 .. C0+TC-1 of J (the same fragments when the block is on the
// diagonal) and writes its tile pairs into the SAME per-workgroup partial image k_gram<T> would write
// (pair index from the global T), so the reduction and assembly kernels do not change.  Diagonal
// launches also carry J^T r of their rows; the first one carries sum r^2, added in gfh_k_chi2's order.
template <int TR, int TC, bool SYM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gram_block(const double* __restrict__ J, const i64 ldj, const int na,
                                                    const double* __restrict__ res, const i64* __restrict__ gb_start,
                                                    const int* __restrict__ gb_slots, double* __restrict__ partial,
                                                    const int pstride, const int T, const int R0, const int C0, const int cw) {
  constexpr int NACC = SYM ? TR * (TR + 1) / 2 : TR * TC;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const i64 s = gb_start[blockIdx.x];
  const i64 e = s + gb_slots[blockIdx.x];
  double4_t acc[NACC];
#pragma unroll
  for (int p = 0; p < NACC; p++) acc[p] = (double4_t){0.0, 0.0, 0.0, 0.0};
  double accr[TR];
#pragma unroll
  for (int t = 0; t < TR; t++) accr[t] = 0.0;
  const double* arow[TR]; bool aval[TR];
  const double* brow[TC]; bool bval[TC];
#pragma unroll
  for (int t = 0; t < TR; t++) { aval[t] = R0 + t < T && 16 * (R0 + t) + r < na; arow[t] = J + (i64)(aval[t] ? 16 * (R0 + t) + r : 0) * ldj; }
#pragma unroll
  for (int t = 0; t < TC; t++) { bval[t] = C0 + t < T && 16 * (C0 + t) + r < na; brow[t] = J + (i64)(bval[t] ? 16 * (C0 + t) + r : 0) * ldj; }
  for (i64 n = s + 64 * wv; n < e; n += 256) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const i64 c = n + 16 * u + 4 * q;
      double4_t a[TR], b[TC];
#pragma unroll
      for (int t = 0; t < TR; t++) { a[t] = *reinterpret_cast<const double4_t*>(arow[t] + c); if (!aval[t]) a[t] = (double4_t){0.0, 0.0, 0.0, 0.0}; }
      if (!SYM) {
#pragma unroll
        for (int t = 0; t < TC; t++) { b[t] = *reinterpret_cast<const double4_t*>(brow[t] + c); if (!bval[t]) b[t] = (double4_t){0.0, 0.0, 0.0, 0.0}; }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        int p = 0;
#pragma unroll
        for (int ti = 0; ti < TR; ti++)
#pragma unroll
          for (int tj = SYM ? ti : 0; tj < TC; tj++, p++)
            acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti][j], SYM ? a[tj][j] : b[tj][j], acc[p], 0, 0, 0);
      }
      if (SYM) {
        const double4_t rr = *reinterpret_cast<const double4_t*>(res + c);
#pragma unroll
        for (int t = 0; t < TR; t++) accr[t] += a[t][0] * rr[0] + a[t][1] * rr[1] + a[t][2] * rr[2] + a[t][3] * rr[3];
      }
    }
  }
  // sum r^2 (the launch with R0 == 0) in gfh_k_chi2's own map and order at the cw waves it runs with for this number of active
  // parameters (chi2.hip, GFH_CW: 8 beyond the fused kernel; a gram block is whole passes of 512 slots): this thread stands for threads
  // tid and tid + 256 of such a workgroup -- each sums its own points pass by pass --, then the wave tree, then the eight waves in
  // order.  cw == 4 (65 ... 128 active parameters, where this kernel runs for models with integrate() and under GADFIT_HIP_FUSED=0):
  // gfh_k_chi2 has this kernel's 256 threads, each sums its own points pass by pass, then the wave tree and the four waves in order.
  // With k_reduce_partials and the assembly above it that is the order of chi2(), so chi2() at a sweep's parameters is bitwise the
  // sweep's sum here too.
  __shared__ double c8[8];
  if (SYM && R0 == 0) {
    double lo = 0.0, hi = 0.0;
    if (cw == 4) {
      for (i64 i = s + threadIdx.x; i < e; i += 256) { const double r0 = res[i]; lo += r0 * r0; }
    } else {
      for (i64 i = s + threadIdx.x; i + 256 < e; i += 512) {
        const double r0 = res[i], r1 = res[i + 256];
        lo += r0 * r0; hi += r1 * r1;
      }
    }
    lo = gfh_wave_sum(lo); hi = gfh_wave_sum(hi);
    if (lane == 0) { c8[wv] = lo; c8[wv + 4] = hi; }
  }
  // Cross-wave sum, waves in order.  Up to 4 x 4 tiles every wave has an image of its own in LDS, as in k_gram; the wide blocks (5 or
  // 6 tiles in ONE launch: 15 / 21 pair images of 2 KB) add into one image wave after wave -- the same order of additions, a quarter
  // of the LDS -- and keep only their lane sums of J^T r apart, behind it.
  constexpr bool WIDE = TR > 4;
  constexpr int IMG = NACC * 256, VEC = TR * 64 + 4, WS = WIDE ? VEC : IMG + VEC;
  __shared__ double sm[WIDE ? IMG + 4 * VEC : 4 * WS];
  if constexpr (!WIDE) spill_tiles<NACC>(sm + wv * WS, acc, r, q);
  else {
    for (int w = 0; w < 4; w++) {
      if (wv == w) {
#pragma unroll
        for (int p = 0; p < NACC; p++)
#pragma unroll
          for (int j = 0; j < 4; j++) {
            double* e = &sm[gram_tile_at(p, q + 4 * j, r)];
            *e = w == 0 ? acc[p][j] : *e + acc[p][j];
          }
      }
      __syncthreads();
    }
  }
  double* vec = sm + IMG + wv * WS;
#pragma unroll
  for (int t = 0; t < TR; t++) vec[t * 64 + lane] = accr[t];
  __syncthreads();
  double* out = partial + (i64)blockIdx.x * pstride;
  {
    int p = 0;
    for (int ti = 0; ti < TR; ti++)
      for (int tj = SYM ? ti : 0; tj < TC; tj++, p++) {
        const int gi = R0 + ti, gj = C0 + tj;
        if (gi >= T || gj >= T) continue;
        double v;
        if constexpr (WIDE) v = sm[gram_tile(p) + threadIdx.x];
        else v = sum_wave_images(sm, WS, gram_tile(p) + threadIdx.x);
        out[gram_tile(gram_pair(gi, gj, T)) + threadIdx.x] = v;
      }
  }
  if (SYM) {
    for (int idx = threadIdx.x; idx < 16 * TR; idx += 256) {
      const int t = idx >> 4, rr_ = idx & 15;
      if (R0 + t >= T) continue;
      out[gram_jtr(16 * (R0 + t) + rr_, T)] = jtr_row_sum(sm + IMG, WS, t, rr_);
    }
    if (R0 == 0 && threadIdx.x == 0) {
      double sacc = c8[0];
#pragma unroll
      for (int w = 1; w < 8; w++) if (w < 4 || cw != 4) sacc += c8[w];
      out[gram_rtr(T)] = sacc;
    }
  }
}

// ---------------------------------------------------------------------------- launchers
// The rule (tests/gram_chain_cases.py, gram_launches, restates it): up to 8 active parameters k_gram_small<na>; up to 4 tiles
// k_gram<T>; 5 and 6 tiles ONE k_gram_block<T, T, sym> that reads J once; beyond that blocks of up to 4 x 4 tiles over the upper
// triangle, diagonal blocks first in every block row.  Every launch notes itself where a caller asks (gfh_debug_chain).
namespace {
struct GramArgs {
  hipStream_t st; const double* J; i64 ldj; int na; const double* res; const i64* gb_start; const int* gb_slots; int n_gb;
  double* partial; int ps; int T, cw; std::vector<GramLaunch>* note;
};
template <int NA> void launch_small(const GramArgs& g, int, int) {
  hipLaunchKernelGGL(k_gram_small<NA>, dim3(g.n_gb), dim3(512), 0, g.st, g.J, g.ldj, g.res, g.gb_start, g.gb_slots, g.partial, g.ps);
  if (g.note) g.note->push_back({0, NA, 0, 0, 0, 0});
}
template <int T> void launch_whole(const GramArgs& g, int, int) {
  hipLaunchKernelGGL(k_gram<T>, dim3(g.n_gb), dim3(256), 0, g.st, g.J, g.ldj, g.na, g.res, g.gb_start, g.gb_slots, g.partial, g.ps);
  if (g.note) g.note->push_back({1, T, 0, 0, 0, 0});
}
template <int TR, int TC, bool SYM> void launch_block(const GramArgs& g, int r0, int c0) {
  hipLaunchKernelGGL((k_gram_block<TR, TC, SYM>), dim3(g.n_gb), dim3(256), 0, g.st, g.J, g.ldj, g.na, g.res, g.gb_start, g.gb_slots,
                     g.partial, g.ps, g.T, r0, c0, g.cw);
  if (g.note) g.note->push_back({2, TR, TC, SYM ? 1 : 0, r0, c0});
}
typedef void (*GramLauncher)(const GramArgs&, int r0, int c0);
const GramLauncher kSmall[8] = {launch_small<1>, launch_small<2>, launch_small<3>, launch_small<4>,
                                launch_small<5>, launch_small<6>, launch_small<7>, launch_small<8>};
const GramLauncher kWhole[6] = {launch_whole<1>, launch_whole<2>, launch_whole<3>, launch_whole<4>,
                                launch_block<5, 5, true>, launch_block<6, 6, true>};
// blocks of the triangle by the tiles they really hold: tr = tc on the diagonal; off it always four whole row tiles -- only the last
// block row / column of the triangle is short
const GramLauncher kDiag[4] = {launch_block<1, 1, true>, launch_block<2, 2, true>, launch_block<3, 3, true>, launch_block<4, 4, true>};
const GramLauncher kOff[4] = {launch_block<4, 1, false>, launch_block<4, 2, false>, launch_block<4, 3, false>, launch_block<4, 4, false>};
}  // namespace

hipError_t launch_gram(hipStream_t st, int T, const double* J, i64 ldj, int na, const double* res,
                       const i64* gb_start, const int* gb_slots, int n_gb, double* partial, std::vector<GramLaunch>* note) {
  const GramArgs g{st, J, ldj, na, res, gb_start, gb_slots, n_gb, partial, gram_partial_stride(T), T, chi2_waves_for(na), note};
  if (na <= 8) { if (na >= 1) kSmall[na - 1](g, 0, 0); }
  else if (T <= 6) { if (T >= 1) kWhole[T - 1](g, 0, 0); }
  else {
    // The blocks at the edge are instantiated at the number of tiles they really hold (80 parameters = 5 tiles: a 4 x 4 diagonal
    // block, a 4 x 1 block and a 1 x 1 diagonal block -- 15 tile pairs and 160 column reads per point where three 4 x 4 launches made
    // 36 pairs and 256 reads, most of them on tiles that do not exist: 2.31 -> 1.32 ms at N = 4e6; 5 and 6 tiles in one launch at two
    // waves per SIMD: 0.62 ms, profiles/r04_p80.md)
    for (int gi = 0; gi < T; gi += 4)
      for (int gj = gi; gj < T; gj += 4) {
        const int tc = T - gj < 4 ? T - gj : 4;
        (gi == gj ? kDiag : kOff)[tc - 1](g, gi, gj);
      }
  }
  return hipGetLastError();
}

}  // namespace gfh
