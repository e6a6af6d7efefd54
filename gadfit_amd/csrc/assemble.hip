// assemble.hip -- from the workgroups' Gram images (gram.hip, or the fused kernel) to the packed image of the normal equations:
// the deterministic cross-workgroup reduction per dataset, and the scatter into the global (dim x dim) system via
// Jacobian_indices (gadfit.F90:615-628) in three forms that add the same terms in the same order (packed_walk.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "packed_walk.h"

namespace gfh {

#include "device/mailbox.hip"

// --------------------------------------------------------------------------------------
// Sum workgroup partials per dataset in a fixed order (=> bitwise reproducible).
// grid = (ceil(width/32), n_datasets), block = 1024 = 32 elements x 32 slices: slice s adds
// workgroups b0+s, b0+s+32, ... and the 32 slice sums are added in slice order.
__global__ __launch_bounds__(1024) void k_reduce_partials(const double* __restrict__ partial, const int pstride,
                                                          const int width, const int* __restrict__ ds_first_gb,
                                                          double* __restrict__ out /*[nd][width]*/) {
  const int d = blockIdx.y;
  const int el = blockIdx.x * 32 + (threadIdx.x & 31), sl = threadIdx.x >> 5;
  const int b0 = ds_first_gb[d], b1 = ds_first_gb[d + 1];
  double s = 0.0;
  if (el < width)
    for (int b = b0 + sl; b < b1; b += 32) s += partial[(i64)b * pstride + el];
  __shared__ double sm[32][33];
  sm[sl][threadIdx.x & 31] = s;
  __syncthreads();
  if (sl == 0 && el < width) {
    double t = sm[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < 32; k++) t += sm[k][threadIdx.x];
    out[(i64)d * width + el] = t;
  }
}

// --------------------------------------------------------------------------------------
// Scatter the per-dataset Grams into the global normal equations through Jacobian_indices.
// packed = [JTJ (dim*dim, column-major) | JTres (dim) | chi2].  One thread per output
// element, datasets visited in order (deterministic): the walks of packed_walk.h.
// grid = (ceil(dim/256), dim + 1): blockIdx.y = column of JTJ, or dim for the [JTres | chi2] tail; threads = rows
__global__ __launch_bounds__(256) void k_assemble(const double* __restrict__ G /*[nd][gw]*/, const int gw, const int T, const int nd,
                                                  const int dim, const int* __restrict__ inv /*[nd][dim]*/,
                                                  const int* __restrict__ owner /*[dim]*/, double* __restrict__ packed) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  const int col = blockIdx.y;
  const i64 nn = (i64)dim * dim;
  if (col < dim) {
    if (row < dim) packed[(i64)col * dim + row] = walk_entry(G, gw, T, nd, dim, inv, owner, row, col);
  } else if (row < dim) packed[nn + row] = walk_jtr(G, gw, T, nd, dim, inv, owner, row);
  else if (row == dim) packed[nn + dim] = walk_rtr(G, gw, T, nd);
}

// Pattern-only assembly for global fits: the normal equations of several datasets are block-arrow (the
// local parameters of different datasets do not couple), so only the entries (row <= col) that some
// dataset touches are formed and sent to the host: packed = [nnz values | JTres (dim) | chi2].  The value
// of an entry is the one k_assemble computes: the same walk.
__global__ __launch_bounds__(256) void k_assemble_sparse(const double* __restrict__ G, const int gw, const int T, const int nd,
                                                         const int dim, const int* __restrict__ inv, const int* __restrict__ owner,
                                                         const int* __restrict__ nz_row, const int* __restrict__ nz_col, const int nnz,
                                                         double* __restrict__ packed) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < nnz) packed[idx] = walk_entry(G, gw, T, nd, dim, inv, owner, nz_row[idx], nz_col[idx]);
  else if (idx < nnz + dim) packed[idx] = walk_jtr(G, gw, T, nd, dim, inv, owner, idx - nnz);
  else if (idx == nnz + dim) packed[idx] = walk_rtr(G, gw, T, nd);
}

// The same packed image from host-built source lists (packed_layout.cpp, build_gather_lists): k_assemble_sparse reaches a value
// through four dependent loads (pattern entry -> owner -> inv -> G), each ~2 us on an idle chip, which made it 24 us at config 3.
// Here meta[idx] names the single term or the list of terms of an element (packed_walk.h, gather_sum).
// host_out != nullptr (single rank): the values also go straight into the pinned result mailbox and the last workgroup to arrive
// posts the status word and the call's sequence number, as k_publish does -- one launch less per pass.
__global__ __launch_bounds__(256) void k_gather_sum(const double* __restrict__ G, const int* __restrict__ meta, const int* __restrict__ list,
                                                    const int n, double* __restrict__ out, const int* __restrict__ status, double* host_out,
                                                    unsigned* counter, unsigned long long* host_flag, const unsigned long long seq) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const double s = gather_sum(G, idx < n ? meta[idx] : kGatherNoTerm, list);
  if (idx < n) {
    out[idx] = s;
    if (host_out) __builtin_nontemporal_store(s, host_out + idx);
  }
  if (!host_out) return;
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0 && gfh_last_workgroup(counter)) gfh_mailbox_post(host_out, n, status, host_flag, seq);
}

// ---------------------------------------------------------------------------- launchers
hipError_t launch_reduce_partials(hipStream_t st, const double* partial, int pstride, int width,
                                  const int* ds_first_gb, int nd, double* out) {
  hipLaunchKernelGGL(k_reduce_partials, dim3((width + 31) / 32, nd), dim3(1024), 0, st, partial, pstride, width, ds_first_gb, out);
  return hipGetLastError();
}

hipError_t launch_assemble(hipStream_t st, const double* G, int gw, int T, int nd, int dim, const int* inv, const int* owner, double* packed) {
  // (dim + 1) threads in x for the tail row: one more than the rows, so ceil((dim + 1) / 256) blocks
  hipLaunchKernelGGL(k_assemble, dim3((unsigned)((dim + 1 + 255) / 256), (unsigned)(dim + 1)), dim3(256), 0, st, G, gw, T, nd, dim, inv, owner, packed);
  return hipGetLastError();
}

hipError_t launch_assemble_sparse(hipStream_t st, const double* G, int gw, int T, int nd, int dim, const int* inv, const int* owner,
                                  const int* nz_row, const int* nz_col, int nnz, double* packed) {
  hipLaunchKernelGGL(k_assemble_sparse, dim3((unsigned)((nnz + dim + 1 + 255) / 256)), dim3(256), 0, st, G, gw, T, nd, dim, inv, owner, nz_row, nz_col, nnz, packed);
  return hipGetLastError();
}

hipError_t launch_gather_sum(hipStream_t st, const double* G, const int* meta, const int* list, int n, double* out, const int* status,
                             double* host_out, unsigned* counter, unsigned long long* host_flag, unsigned long long seq) {
  hipLaunchKernelGGL(k_gather_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, G, meta, list, n, out, status, host_out, counter, host_flag, seq);
  return hipGetLastError();
}

}  // namespace gfh
