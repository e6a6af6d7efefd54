// jtv.hip -- STEP 3 from a stored Jacobian: J^T v products (gadfit.F90:734, 849) per gram block, their two finishes (one launch
// with the mailbox post, or k_reduce_partials + k_assemble_vec + k_publish), and the cos(phi) sums (gadfit.F90:865-873).
//
// Layout contract: J is [NA][ldj] parameter-major over padded slots; every
// gram block covers whole 256-slot tiles of ONE dataset; pad slots hold zeros in J and res.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace gfh {

// The wave tree gfh_wave_sum: the one definition that the generated kernels carry too (device_text.cpp embeds the same file), so
// k_jtv here and gfh_k_omega_jt there add alike by construction.
#include "device/wave_sum.hip"

// --------------------------------------------------------------------------------------
// J^T v per gram block (v = omega or res).  partial[b][a], a < na.
// CB columns per sweep over the block's points: v[i] is loaded once per CB columns and CB + 1 independent loads
// per lane are in flight (with 2 workgroups per CU that is what keeps HBM busy: up to 32 columns = the whole
// Jacobian row of the headline model in ONE pass over v).  Every column keeps its own accumulator and its own
// order of additions, so the result does not depend on CB.
template <int CB>
__global__ __launch_bounds__(256) void k_jtv(const double* __restrict__ J, const i64 ldj, const int na,
                                             const double* __restrict__ v, const i64* __restrict__ gb_start,
                                             const int* __restrict__ gb_slots, double* __restrict__ partial,
                                             const int pstride) {
  const i64 s = gb_start[blockIdx.x], e = s + gb_slots[blockIdx.x];
  __shared__ double ws[CB][4];
  for (int a0 = 0; a0 < na; a0 += CB) {
    double acc[CB];
#pragma unroll
    for (int u = 0; u < CB; u++) acc[u] = 0.0;
    const double* __restrict__ Ja = J + (i64)a0 * ldj;
    // (gb_slots is a multiple of 512: two points per trip, their loads issued together; each accumulator still adds its
    // points in ascending order, so the sums are those of the one-point loop)
    if (a0 + CB <= na) {
      for (i64 i = s + threadIdx.x; i < e; i += 512) {
        const double v0 = v[i], v1 = v[i + 256];
        double j0[CB], j1[CB];
#pragma unroll
        for (int u = 0; u < CB; u++) { j0[u] = Ja[(i64)u * ldj + i]; j1[u] = Ja[(i64)u * ldj + i + 256]; }
#pragma unroll
        for (int u = 0; u < CB; u++) { acc[u] += j0[u] * v0; acc[u] += j1[u] * v1; }
      }
    } else {
      for (i64 i = s + threadIdx.x; i < e; i += 512) {
        const double v0 = v[i], v1 = v[i + 256];
        double j0[CB], j1[CB];
#pragma unroll
        for (int u = 0; u < CB; u++)
          if (a0 + u < na) { j0[u] = Ja[(i64)u * ldj + i]; j1[u] = Ja[(i64)u * ldj + i + 256]; }
#pragma unroll
        for (int u = 0; u < CB; u++)
          if (a0 + u < na) { acc[u] += j0[u] * v0; acc[u] += j1[u] * v1; }
      }
    }
#pragma unroll
    for (int u = 0; u < CB; u++) {
      const double t = gfh_wave_sum(acc[u]);
      if ((threadIdx.x & 63) == 0) ws[u][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < CB && a0 + (int)threadIdx.x < na)
      partial[(i64)blockIdx.x * pstride + a0 + threadIdx.x] =
          ((ws[threadIdx.x][0] + ws[threadIdx.x][1]) + ws[threadIdx.x][2]) + ws[threadIdx.x][3];
    __syncthreads();
  }
}

// out[dim] from per-dataset vectors V[d][width>=na] through inv
__global__ void k_assemble_vec(const double* __restrict__ V, const int width, const int nd, const int dim,
                               const int* __restrict__ inv, double* __restrict__ out) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= dim) return;
  double s = 0.0;
  for (int d = 0; d < nd; d++) { const int a = inv[d * dim + row]; if (a >= 0) s += V[(i64)d * width + a]; }
  out[row] = s;
}

// k_reduce_partials (width na) + k_assemble_vec + k_publish for a J^T v product as ONE single-workgroup launch
// (n_datasets * na <= 4096): the same slice sums, slice order and dataset order, so bitwise the same vector.
// host_out == nullptr: the vector stays on the device (several ranks: RCCL sums it, k_publish posts it).
__global__ __launch_bounds__(1024) void k_jtv_finish(const double* __restrict__ partial, const int pstride, const int na,
                                                     const int* __restrict__ ds_first_gb, const int nd, const int dim,
                                                     const int* __restrict__ inv, double* __restrict__ out,
                                                     const int* __restrict__ status, double* host_out,
                                                     unsigned long long* host_flag, const unsigned long long seq) {
  __shared__ double sm[32][33];
  __shared__ double V[4096];
  const int lane32 = threadIdx.x & 31, sl = threadIdx.x >> 5;
  for (int d = 0; d < nd; d++) {
    const int b0 = ds_first_gb[d], b1 = ds_first_gb[d + 1];
    for (int e0 = 0; e0 < na; e0 += 32) {
      const int el = e0 + lane32;
      double s = 0.0;
      if (el < na)
        for (int b = b0 + sl; b < b1; b += 32) s += partial[(i64)b * pstride + el];
      sm[sl][lane32] = s;
      __syncthreads();
      if (sl == 0 && el < na) {
        double t = sm[0][lane32];
#pragma unroll
        for (int k = 1; k < 32; k++) t += sm[k][lane32];
        V[d * na + el] = t;
      }
      __syncthreads();
    }
  }
  for (int row = threadIdx.x; row < dim; row += 1024) {
    double s = 0.0;
    for (int d = 0; d < nd; d++) { const int a = inv[d * dim + row]; if (a >= 0) s += V[d * na + a]; }
    out[row] = s;
    if (host_out) __builtin_nontemporal_store(s, host_out + row);
  }
  if (!host_out) return;
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    host_out[dim] = (double)*status;
    __threadfence_system();
    __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// cos(phi) sums (gadfit.F90:865-873): Jdelta_i = sum_a J[a][i]*dl[ds][a];
// partial[b][0..2] = {res.Jdelta, res.res, Jdelta.Jdelta}
__global__ __launch_bounds__(256) void k_cosphi(const double* __restrict__ J, const i64 ldj, const int na,
                                                const double* __restrict__ res, const double* __restrict__ dl /*[nd][na]*/,
                                                const i64* __restrict__ gb_start, const int* __restrict__ gb_slots,
                                                const int* __restrict__ gb_ds, double* __restrict__ partial,
                                                const int pstride) {
  const i64 s = gb_start[blockIdx.x], e = s + gb_slots[blockIdx.x];
  const double* d1 = dl + (i64)gb_ds[blockIdx.x] * na;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (i64 i = s + threadIdx.x; i < e; i += 256) {
    double jd = 0.0;
    for (int a = 0; a < na; a++) jd += J[(i64)a * ldj + i] * d1[a];
    const double r = res[i];
    s0 += r * jd; s1 += r * r; s2 += jd * jd;
  }
  __shared__ double ws[3][4];
  s0 = gfh_wave_sum(s0); s1 = gfh_wave_sum(s1); s2 = gfh_wave_sum(s2);
  if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = s0; ws[1][threadIdx.x >> 6] = s1; ws[2][threadIdx.x >> 6] = s2; }
  __syncthreads();
  if (threadIdx.x < 3) partial[(i64)blockIdx.x * pstride + threadIdx.x] =
      ((ws[threadIdx.x][0] + ws[threadIdx.x][1]) + ws[threadIdx.x][2]) + ws[threadIdx.x][3];
}

// ---------------------------------------------------------------------------- launchers
hipError_t launch_jtv(hipStream_t st, const double* J, i64 ldj, int na, const double* v, const i64* gb_start,
                      const int* gb_slots, int n_gb, double* partial, int pstride) {
  if (na <= 8) hipLaunchKernelGGL(k_jtv<8>, dim3(n_gb), dim3(256), 0, st, J, ldj, na, v, gb_start, gb_slots, partial, pstride);
  else if (na <= 16) hipLaunchKernelGGL(k_jtv<16>, dim3(n_gb), dim3(256), 0, st, J, ldj, na, v, gb_start, gb_slots, partial, pstride);
  else hipLaunchKernelGGL(k_jtv<32>, dim3(n_gb), dim3(256), 0, st, J, ldj, na, v, gb_start, gb_slots, partial, pstride);
  return hipGetLastError();
}

hipError_t launch_jtv_finish(hipStream_t st, const double* partial, int pstride, int na, const int* ds_first_gb, int nd, int dim,
                             const int* inv, double* out, const int* status, double* host_out, unsigned long long* host_flag,
                             unsigned long long seq) {
  hipLaunchKernelGGL(k_jtv_finish, dim3(1), dim3(1024), 0, st, partial, pstride, na, ds_first_gb, nd, dim, inv, out, status, host_out, host_flag, seq);
  return hipGetLastError();
}

hipError_t launch_assemble_vec(hipStream_t st, const double* V, int width, int nd, int dim, const int* inv, double* out) {
  hipLaunchKernelGGL(k_assemble_vec, dim3((dim + 255) / 256), dim3(256), 0, st, V, width, nd, dim, inv, out);
  return hipGetLastError();
}

hipError_t launch_cosphi(hipStream_t st, const double* J, i64 ldj, int na, const double* res, const double* dl,
                         const i64* gb_start, const int* gb_slots, const int* gb_ds, int n_gb, double* partial, int pstride) {
  hipLaunchKernelGGL(k_cosphi, dim3(n_gb), dim3(256), 0, st, J, ldj, na, res, dl, gb_start, gb_slots, gb_ds, partial, pstride);
  return hipGetLastError();
}

}  // namespace gfh
