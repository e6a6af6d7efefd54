// kernels.hip -- the small hand-written gfx950 kernels beside the LM hot path that do not depend on the model: the result
// mailbox's publisher, the status word as an element of a cross-rank sum, the pad slots of the device layout and
// init_weights (gadfit.F90:445-470).  The hot path lies by stage in gram.hip (STEP 2 from a stored Jacobian), assemble.hip
// (reduction and the packed image) and jtv.hip (STEP 3, cos(phi)).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace gfh {

#include "device/mailbox.hip"

// The result mailbox (device/mailbox.hip) for a result that lies in device memory: the <= (dim^2+dim+1) doubles at src and the
// status word, 1024 values per workgroup.
__global__ __launch_bounds__(256) void k_publish(const double* __restrict__ src, const int n, const int* __restrict__ status,
                                                 double* host_out, unsigned* counter,
                                                 unsigned long long* host_flag, const unsigned long long seq) {
  for (int i = blockIdx.x * 1024 + threadIdx.x; i < n && i < (int)(blockIdx.x + 1) * 1024; i += 256)
    __builtin_nontemporal_store(src[i], host_out + i);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0 && gfh_last_workgroup(counter)) gfh_mailbox_post(host_out, n, status, host_flag, seq);
}

// The kernels' status word as one more element of a cross-rank sum: 0, 1 (quadrature workspace exhausted), 4096 (code 2),
// 2^24 (anything else) -- the sum over at most a few thousand ranks still tells which codes occurred.
__global__ void k_status_slot(const int* __restrict__ status, double* __restrict__ dst) {
  const int st = *status;
  dst[0] = st == 0 ? 0.0 : st == 1 ? 1.0 : st == 2 ? 4096.0 : 16777216.0;
}

// Pad slots of the device layout (every dataset's range is padded to whole tiles): a real abscissa of the same dataset (so f stays
// finite), y = 0, w = 0, is_pad = 1.  One workgroup per dataset; seg[d] = {first slot, number of real points, end slot}.
__global__ __launch_bounds__(256) void k_fill_pads(const i64* __restrict__ seg, double* __restrict__ x, double* __restrict__ y,
                                                   double* __restrict__ w, unsigned char* __restrict__ is_pad) {
  const i64 s0 = seg[3 * blockIdx.x], len = seg[3 * blockIdx.x + 1], s1 = seg[3 * blockIdx.x + 2];
  const double fill = len ? x[s0 + len - 1] : 0.0;
  for (i64 sl = s0 + len + threadIdx.x; sl < s1; sl += 256) { x[sl] = fill; y[sl] = 0.0; w[sl] = 0.0; is_pad[sl] = 1; }
}

// init_weights, gadfit.F90:445-470 (w holds sigma on entry for USER)
__global__ void k_init_weights(const int type, const i64 n, const double* __restrict__ y, double* __restrict__ w,
                               const unsigned char* __restrict__ is_pad) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (is_pad[i]) { w[i] = 0.0; return; }
  const double thr = 1e2 * 2.2250738585072014e-308;
  const double yy = y[i];
  double r;
  switch (type) {
    case 0: r = 1.0; break;
    case 1: r = fabs(yy) < thr ? 0.0 : 1.0 / sqrt(yy); break;
    case 2: r = fabs(yy) < thr ? 0.0 : 1.0 / yy; break;
    case 3: r = yy; break;
    default: r = 1.0 / w[i]; break;
  }
  w[i] = r;
}

// ---------------------------------------------------------------------------- launchers
hipError_t launch_publish(hipStream_t st, const double* src, int n, const int* status, double* host_out, unsigned* counter,
                          unsigned long long* host_flag, unsigned long long seq) {
  hipLaunchKernelGGL(k_publish, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, st, src, n, status, host_out, counter, host_flag, seq);
  return hipGetLastError();
}

hipError_t launch_status_slot(hipStream_t st, const int* status, double* dst) {
  hipLaunchKernelGGL(k_status_slot, dim3(1), dim3(1), 0, st, status, dst);
  return hipGetLastError();
}

hipError_t launch_fill_pads(hipStream_t st, int nd, const i64* seg, double* x, double* y, double* w, unsigned char* is_pad) {
  hipLaunchKernelGGL(k_fill_pads, dim3((unsigned)nd), dim3(256), 0, st, seg, x, y, w, is_pad);
  return hipGetLastError();
}

hipError_t launch_init_weights(hipStream_t st, int type, i64 n, const double* y, double* w, const unsigned char* is_pad) {
  hipLaunchKernelGGL(k_init_weights, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, type, n, y, w, is_pad);
  return hipGetLastError();
}

}  // namespace gfh
