struct gfh_unseen { i64 slot; unsigned long long path; int n_guards; int pad; };
static __device__ __attribute__((noinline)) void gfh_report_unseen(int* STATUS, const i64 slot, const unsigned long long path, const int ng) {
  GFH_RAISE(STATUS, 3);
  const unsigned k = __hip_atomic_fetch_add((unsigned*)((char*)STATUS + 64), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (k < GFH_UNSEEN_CAP) { gfh_unseen* e = (gfh_unseen*)((char*)STATUS + 128) + k; e->slot = slot; e->path = path; e->n_guards = ng; e->pad = 0; }
}
