// Result mailbox, device side.  The result of a pass is written by the device straight into pinned, host-coherent memory together
// with the kernels' status word; the last workgroup to finish then stores the call's sequence number into a host flag the calling
// thread spins on.  No copy engine, no completion-signal round trip: the host sees the result a few microseconds after the last
// kernel's stores.  A kernel that posts: nontemporal stores of its values into host_out, then
//   __threadfence_system(); __syncthreads(); if (threadIdx.x == 0 && gfh_last_workgroup(counter)) gfh_mailbox_post(...);
// (a single-workgroup kernel needs no counter).

// Did every other workgroup of this grid arrive before this one?  The last one leaves the counter ready for the next call
// (stream-ordered).  One thread per workgroup asks.
static __device__ __forceinline__ bool gfh_last_workgroup(unsigned* counter) {
  const unsigned arrived = atomicAdd(counter, 1u);
  if (arrived != gridDim.x - 1) return false;
  *counter = 0;
  return true;
}

// The status word behind the n values, a fence, then the sequence number as a release store: what the host waits for.
static __device__ __forceinline__ void gfh_mailbox_post(double* host_out, const int n, const int* __restrict__ status,
                                                        unsigned long long* host_flag, const unsigned long long seq) {
  host_out[n] = (double)*status;
  __threadfence_system();
  __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
