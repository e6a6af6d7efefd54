// comm.cpp -- the communicator: the RCCL ranks of a context (gfh_comm_*), the cross-rank sum of a pass (allreduce_sum), the result
// mailbox every result-returning call ends in (fetch_result / await_result), and the latency probes of both ways a sum can travel
// (ncclAllReduce; the ordered host sum of a device group, group.cpp).  It launches no model kernel and allocates nothing of its own
// beyond what devmem.cpp hands out.
#include "context_internal.h"
#include "group.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>

using namespace gfh;

// End of every result-returning call: k_publish (kernels.hip; device/mailbox.hip) moves n doubles at `src` and the
// kernels' status word into the pinned mailbox c->h_pinned and stores this call's sequence number
// into the host flag; the host spins on the flag.  Everything queued on the stream before it has
// finished when the flag flips (it is the last operation of the call).  hipStreamQuery is polled
// now and then so that a failed launch or a device fault ends the wait with an error.
int gfh::await_result(gfh_ctx* c, unsigned long long seq, size_t n, bool summed) {
  for (unsigned spin = 1;; spin++) {
    if (__atomic_load_n(c->h_flag, __ATOMIC_ACQUIRE) == seq) break;
    __builtin_ia32_pause();
    if ((spin & 0x3FF) == 0) {
      const hipError_t e = hipStreamQuery(c->stream);
      if (e == hipSuccess) {
        if (__atomic_load_n(c->h_flag, __ATOMIC_ACQUIRE) == seq) break;
        return fail(c, "result mailbox was not written");
      }
      if (e != hipErrorNotReady) return fail(c, std::string("HIP error while waiting for a result: ") + hipGetErrorString(e));
    }
  }
  // summed: the n doubles are a cross-rank sum whose element n is the sum of the ranks' encoded status words (allreduce_sum),
  // so a quadrature failure on one rank raises the reference's error on every rank (and none waits in a later collective)
  int st = (int)c->h_pinned[n + (summed ? 1 : 0)];
  if (summed && !st) { const double g = c->h_pinned[n]; st = g >= 16777216.0 ? 3 : g >= 4096.0 ? 2 : g >= 1.0 ? 1 : 0; }
  // member of a single-process device group: the sum over the members (co_sum, misc.F90:133-170) is taken here,
  // on the host, in rank order; the status word travels with it so every member raises the same error
  if (c->member_of && !c->comm && gfh::group_allreduce(c, c->h_pinned, n, &st)) return 1;
  return status_check(c, st);
}

int gfh::fetch_result(gfh_ctx* c, const double* src, size_t n, bool summed) {
  if (pinned_reserve(c, sizeof(double) * std::max<size_t>(n + 2, 4096))) return 1;
  const unsigned long long seq = ++c->mail_seq;
  unsigned* counter = reinterpret_cast<unsigned*>(c->status.as<char>() + 16);
  HIPCHK(c, launch_publish(c->stream, src, (int)(n + (summed ? 1 : 0)), c->status.as<int>(), c->h_pinned, counter, c->h_flag, seq));
  return await_result(c, seq, n, summed);
}

// co_sum (misc.F90:133-170) of n doubles at buf over the ranks: ONE ncclAllReduce per call site of the reference; the kernels'
// status word rides along as element n (buf has room for it), encoded so that the sum still tells the codes apart
int gfh::allreduce_sum(gfh_ctx* c, double* buf, size_t n, bool slot_written) {
  // (slot_written: the kernel that produced buf -- the fused kernel's or gfh_k_chi2's tail in mode 1 -- has put the slot there itself)
  if (!slot_written) HIPCHK(c, launch_status_slot(c->stream, c->status.as<int>(), buf + n));
  NCCLCHK(c, ncclAllReduce(buf, buf, n + 1, ncclDouble, ncclSum, c->comm, c->stream));
  c->timers.n_allreduce++;
  return 0;
}

// gfh_debug_allreduce_latency on one context (a rank with a communicator, or a member of a device group on its own thread)
static int allreduce_latency_one(gfh_ctx* c, int n, int rounds, double* out6) {
  std::vector<double> dev_us, host_us;
  dev_us.reserve((size_t)rounds); host_us.reserve((size_t)rounds);
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
  int nranks = 1;
  if (c->comm) {
    NEED_GPU(c);
    NCCLCHK(c, ncclCommCount(c->comm, &nranks));
    DevBuf buf;
    if (dev_alloc(c, buf, sizeof(double) * ((size_t)n + 2))) return 1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { if (e0) hipEventDestroy(e0); dev_free(buf); return fail(c, "hipEventCreate failed"); }
    int rc = 0;
    auto body = [&]() -> int {
      HIPCHK(c, hipMemsetAsync(buf.p, 0, sizeof(double) * ((size_t)n + 2), c->stream));
      // (a) the collective alone, between two events on an otherwise idle stream (the first rounds wake the ranks up and are dropped)
      const int warm = std::min(rounds, 20);
      for (int i = 0; i < warm + rounds; i++) {
        HIPCHK(c, hipEventRecord(e0, c->stream));
        NCCLCHK(c, ncclAllReduce(buf.p, buf.p, (size_t)n + 1, ncclDouble, ncclSum, c->comm, c->stream));
        HIPCHK(c, hipEventRecord(e1, c->stream));
        const double ms = ev_ms(e0, e1);
        if (i >= warm) dev_us.push_back(1e3 * ms);
      }
      // (b) as a pass pays it: enqueue the all-reduce, publish the sums into the host mailbox, spin on its flag
      for (int i = 0; i < warm + rounds; i++) {
        const auto t0 = now();
        NCCLCHK(c, ncclAllReduce(buf.p, buf.p, (size_t)n + 1, ncclDouble, ncclSum, c->comm, c->stream));
        if (fetch_result(c, static_cast<double*>(buf.p), (size_t)n, true)) return 1;
        if (i >= warm) host_us.push_back(us(t0, now()));
      }
      return 0;
    };
    rc = body();
    (void)hipStreamSynchronize(c->stream);
    hipEventDestroy(e0); hipEventDestroy(e1);
    dev_free(buf);
    if (rc) return 1;
  } else if (c->member_of) {
    nranks = c->nranks;
    std::vector<double> v((size_t)n + 1, 0.0);
    int st = 0;
    const int warm = std::min(rounds, 200);
    for (int i = 0; i < warm + rounds; i++) {
      for (int j = 0; j < n; j++) v[(size_t)j] = 1.0 + c->rank;
      const auto t0 = now();
      if (gfh::group_allreduce(c, v.data(), (size_t)n, &st)) return 1;
      if (i >= warm) { const double t = us(t0, now()); dev_us.push_back(t); host_us.push_back(t); }
    }
    if (v[0] != 0.5 * nranks * (nranks + 1)) return fail(c, "gfh_debug_allreduce_latency: wrong sum");
  } else {
    return fail(c, "gfh_debug_allreduce_latency needs a communicator (gfh_comm_init) or a device-group handle");
  }
  if (c->rank == 0 || !c->member_of) {
    std::sort(dev_us.begin(), dev_us.end()); std::sort(host_us.begin(), host_us.end());
    auto q = [](const std::vector<double>& s, double f) { return s.empty() ? 0.0 : s[std::min(s.size() - 1, (size_t)(f * (double)s.size()))]; };
    if (out6) {
      out6[0] = q(dev_us, 0.5); out6[1] = q(dev_us, 0.95); out6[2] = dev_us.empty() ? 0.0 : dev_us.front(); out6[3] = dev_us.empty() ? 0.0 : dev_us.back();
      out6[4] = q(host_us, 0.5); out6[5] = (double)nranks;
    }
  }
  return 0;
}

extern "C" {

// Test hook: member r sums bufs[r][0..n) over the group in place through the same barrier + ordered host sum the
// passes use (status[r] in, max over the members out); member `fail_member` (>= 0) fails before it reaches the
// barrier, which must release the others with an error instead of leaving them waiting.
int gfh_debug_group_allreduce(gfh_ctx* c, double* bufs, int n, int* status, int fail_member) {
  if (!c || !c->grp) return fail(c, "gfh_debug_group_allreduce needs a device-group handle");
  return gfh::group_run(c, [&](gfh_ctx* k, int r) -> int {
    if (r == fail_member) return fail(k, "member " + std::to_string(r) + " failed on purpose");
    return gfh::group_allreduce(k, bufs + (size_t)r * n, (size_t)n, status + r);
  });
}

int gfh_debug_group_latency(gfh_ctx* c, int n, int rounds, double* out2) {
  if (!c || !c->grp || n < 1 || rounds < 1 || !out2) return fail(c, "gfh_debug_group_latency needs a device-group handle, n >= 1, rounds >= 1");
  const int N = gfh_group_size(c);
  std::vector<std::vector<double>> bufs((size_t)N, std::vector<double>((size_t)n, 1.0));
  auto sums = [&](int count) {
    return gfh::group_run(c, [&](gfh_ctx* k, int r) -> int {
      int st = 0;
      for (int i = 0; i < count; i++) {
        for (int j = 0; j < n; j++) bufs[(size_t)r][(size_t)j] = 1.0 + r;         // (a member's pass leaves fresh numbers in its mailbox)
        if (gfh::group_allreduce(k, bufs[(size_t)r].data(), (size_t)n, &st)) return 1;
      }
      return 0;
    });
  };
  if (sums(std::min(rounds, 200))) return 1;                                       // (threads awake, pages touched)
  auto t0 = std::chrono::steady_clock::now();
  if (sums(rounds)) return 1;
  out2[0] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / rounds;
  const double want = 0.5 * N * (N + 1);
  for (int r = 0; r < N; r++) if (bufs[(size_t)r][0] != want || bufs[(size_t)r][(size_t)n - 1] != want) return fail(c, "gfh_debug_group_latency: wrong sum");
  t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < rounds; i++) if (gfh::group_run(c, [](gfh_ctx*, int) -> int { return 0; })) return 1;
  out2[1] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / rounds;
  return 0;
}

// ------------------------------------------------------------------------- communicator
int gfh_comm_unique_id(void* id) {
  static_assert(sizeof(ncclUniqueId) == GFH_UNIQUE_ID_BYTES, "unique id size");
  ncclUniqueId u;
  ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess) { set_global_error(std::string("ncclGetUniqueId: ") + ncclGetErrorString(r)); return 1; }
  memcpy(id, &u, sizeof u);
  return 0;
}

int gfh_comm_init(gfh_ctx* c, int nranks, int rank, const void* id) {
  NOT_FOR_GROUP(c, "gfh_comm_init (a device group is its own communicator)");
  if (c && c->member_of) return fail(c, "context belongs to a device group");
  NEED_GPU(c);
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(c, "bad communicator geometry");
  if (c->count) return fail(c, "gfh_comm_init must precede gfh_set_data");
  ncclUniqueId u; memcpy(&u, id, sizeof u);
  NCCLCHK(c, ncclCommInitRank(&c->comm, nranks, u, rank));
  c->nranks = nranks; c->rank = rank;
  return 0;
}

// How the cross-rank sums of this context travel: ranks of its RCCL communicator as RCCL itself reports them
// (ncclCommCount; 0 = no communicator: a single image, or a device group that sums on the host), and the number of
// all-reduces issued since gfh_reset_timers.
int gfh_comm_info(gfh_ctx* c, int* rccl_nranks, int64_t* n_allreduce) {
  if (!c) return 1;
  gfh_ctx* k = c->grp ? gfh::group_member(c, 0) : c;
  int n = 0;
  if (k->comm) NCCLCHK(c, ncclCommCount(k->comm, &n));
  if (rccl_nranks) *rccl_nranks = n;
  if (n_allreduce) *n_allreduce = k->timers.n_allreduce;
  return 0;
}

int gfh_debug_set_rank(gfh_ctx* c, int nranks, int rank) {
  if (!c) return 1;
  NOT_FOR_GROUP(c, "gfh_debug_set_rank");
  if (c->member_of) return fail(c, "context belongs to a device group");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(c, "bad communicator geometry");
  if (c->comm) return fail(c, "context already has a communicator");
  c->nranks = nranks; c->rank = rank;
  return 0;
}

int gfh_comm_init_from_env(gfh_ctx* c) {
  const char* nr = getenv("GADFIT_HIP_NRANKS");
  if (c && c->grp) return nr ? fail(c, "GADFIT_HIP_NRANKS (one process per GPU) and a device group exclude each other") : 0;
  if (!nr) return c ? 0 : 1;      // (before the device is needed: a context from gfh_create_begin may still be setting it up)
  NEED_GPU(c);
  if (atoi(nr) < 1) return fail(c, "GADFIT_HIP_NRANKS must be >= 1");
  const char* rk = getenv("GADFIT_HIP_RANK");
  const char* path = getenv("GADFIT_HIP_IDFILE");
  if (!rk || !path) return fail(c, "GADFIT_HIP_NRANKS needs GADFIT_HIP_RANK and GADFIT_HIP_IDFILE");
  const int nranks = atoi(nr), rank = atoi(rk);
  unsigned char id[GFH_UNIQUE_ID_BYTES];
  if (rank == 0) {
    if (gfh_comm_unique_id(id)) return fail(c, std::string(gfh_last_error(nullptr)));
    std::string tmp = std::string(path) + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f || fwrite(id, 1, sizeof id, f) != sizeof id) { if (f) fclose(f); return fail(c, "cannot write GADFIT_HIP_IDFILE"); }
    fclose(f);
    if (rename(tmp.c_str(), path) != 0) return fail(c, "cannot publish GADFIT_HIP_IDFILE");
  } else {
    bool ok = false;
    for (int tries = 0; tries < 6000 && !ok; tries++) {      // up to ~60 s
      FILE* f = fopen(path, "rb");
      if (f) { ok = fread(id, 1, sizeof id, f) == sizeof id; fclose(f); }
      if (!ok) { struct timespec ts = {0, 10 * 1000 * 1000}; nanosleep(&ts, nullptr); }
    }
    if (!ok) return fail(c, "timed out waiting for GADFIT_HIP_IDFILE");
  }
  const int rc = gfh_comm_init(c, nranks, rank, id);
  // (ncclCommInitRank is a rendezvous: when it has returned here every rank holds the id, and a file left behind would be read as
  // the id of the NEXT run that names the same path)
  if (rank == 0) (void)remove(path);
  return rc;
}

// How long ONE cross-rank sum of n doubles (+ the status slot) takes on this context's path, measured by the library itself:
// through ncclAllReduce (processes with a communicator; members of a device group with RCCL) or through the group's ordered
// host sum.  Collective: every rank (or the group handle) calls it with the same n and rounds.
int gfh_debug_allreduce_latency(gfh_ctx* c, int n, int rounds, double* out6) {
  if (!c || n < 1 || rounds < 1 || !out6) return fail(c, "gfh_debug_allreduce_latency: n >= 1, rounds >= 1");
  GROUP(c, allreduce_latency_one(k, n, rounds, r ? nullptr : out6));
  return allreduce_latency_one(c, n, rounds, out6);
}

}  // extern "C"
