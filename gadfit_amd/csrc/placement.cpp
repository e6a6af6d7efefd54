// placement.cpp -- where the Jacobian buffer and the data arrays lie: the allocation of the buffer (place_jacobian), the timed search
// over candidate allocations (place_jacobian_now) and the entry points that steer and report it.  Candidates are fresh blocks from
// devmem.cpp; the search times the launchers of launch.cpp and touches no other state of a pass.
#include "context_internal.h"
#include "group.h"
#include <algorithm>
#include <cstdlib>

using namespace gfh;

// The Jacobian buffer: `na` column streams ldj * 8 bytes apart, written concurrently by every workgroup -- the traffic that
// bounds the sweep.  How fast the part absorbs them is a matter of the physical pages behind the allocation, and that is the
// luck of the draw: over a row of fresh allocations of the 2.6 GB buffer of the headline size the store stream alone takes
// 0.41 ... 0.47 ms (the same virtual address, different pages, reads either) and the fused kernel 0.46 ... 0.52 ms -- what
// rounds 1 and 2 first read as a power state of the box.  So a large buffer is PLACED: allocated here, and once `placement_after`
// sweeps have written it (a job that has run that long is taken to run on: the search costs as much as 50-110 sweeps)
// up to `placement_tries` allocations are held at once (place_jacobian_now), each timed with four launches of
// the kernel that is about to run, the fastest kept, the others freed.
int gfh::place_jacobian(gfh_ctx* c, int na) {
  const size_t bytes = sizeof(double) * (size_t)na * (size_t)std::max<int64_t>(1, c->ldj);
  if (c->J.bytes >= bytes && c->J.p) return 0;
  if (dev_alloc(c, c->J, bytes)) return 1;
  c->place.n = 0; c->place.sweeps_on_J = 0;
  // (only where the kernel that writes the buffer is bound by its store stream: the sweeps of models with integrate() are bound by
  // the quadrature arithmetic, no placement could show in their time)
  c->place.pending = c->place.tries >= 2 && bytes >= kPlacedJacobianBytes && c->n_gb > 0 && !(c->has_model && c->model.has_integrals());
  return 0;
}

// see place_jacobian.  The parameters of the call are uploaded already: the candidates are timed on the kernel and the numbers
// that are about to run (no tail, nothing read back).  One-time cost per (re)allocation: ~3 ms per candidate at the headline size.
int gfh::place_jacobian_now(gfh_ctx* c, bool fused) {
  c->place.pending = false;
  const size_t bytes = c->J.bytes;
  size_t free_b = 0, total_b = 0;
  const int tries = std::min(c->place.tries, 16);
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess) return 0;
  if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return 0; }
  int rc = 0;
  // (c->J is always a whole candidate -- pointer, bytes and cap together -- never a pointer under another block's sizes)
  auto probe = [&](const DevBuf& b, int launches) -> double {
    c->J = b;
    hipEventRecord(e0, c->stream);
    for (int k = 0; k < launches && !rc; k++) rc = fused ? launch_model_sweep_gram(c) : launch_model_sweep(c);
    hipEventRecord(e1, c->stream);
    if (rc || hipEventSynchronize(e1) != hipSuccess) return 1e30;
    float ms = 0; hipEventElapsedTime(&ms, e0, e1);
    return (double)ms / launches;
  };
  std::vector<DevBuf> cand{c->J};
  void* const first = c->J.p;
  probe(cand[0], 8);                                   // common warm-up (the first launches after an idle gap run slow)
  // Stop at the first candidate on the fast side.  Where that side lies is measured, not assumed: a device-to-device copy inside
  // the first candidate (read + write bytes over its duration) gives this card's copy rate; in fast pages the fused kernel moves
  // its algorithmic bytes at 1.22-1.24 x that rate and the plain sweep at 1.33-1.39 x, in slow pages at 1.09-1.14 x and
  // 1.19-1.25 x (round 2's kernel rates, profiles/r02_placement_probe.txt, over that round's copy rate of 5.05 TB/s): the
  // thresholds sit between.  (Without a usable measurement: round 2's absolute rates.)
  const double algo = (double)(32 + 8 * c->cur_active.size()) * (double)c->n_slots;
  double copy_rate = 0.0;
  {
    const size_t half = (bytes / 2) & ~(size_t)255;
    for (int rep = 0; rep < 3 && half; rep++) {
      hipEventRecord(e0, c->stream);
      if (hipMemcpyAsync(static_cast<char*>(first) + half, first, half, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) { (void)hipGetLastError(); break; }
      hipEventRecord(e1, c->stream);
      if (hipEventSynchronize(e1) != hipSuccess) break;
      float ms = 0; hipEventElapsedTime(&ms, e0, e1);
      if (ms > 0) copy_rate = std::max(copy_rate, 2.0 * (double)half / (1e-3 * ms));
    }
  }
  c->place.copy_rate = copy_rate;
  // (round 6: the <= 8-parameter form of the fused kernel -- no LDS stage, no matrix phase, and since this round a short epilogue --
  // moves its bytes at 1.27-1.30 x the copy rate in fast pages and 1.12-1.15 x in slow ones: 0.149 against 0.167-0.174 ms at BASELINE
  // config 2, profiles/r06_valu_form_ab.txt; with the matrix form's 1.19 a candidate at 0.160 ms counted as fast and ended the search)
  const bool valu_form = fused && (int)c->cur_active.size() <= kValuGramMax;
  // (... and never below an absolute rate: the copy is made INSIDE the first candidate, so slow pages under it lower the bar for
  // themselves -- a bench line of this round kept 0.485 ms after two candidates because its copy ran at 4.7 TB/s, in a process whose
  // other kernels all ran fast; 6.3 TB/s is what fast pages give the fused kernel on every box met: 0.426-0.448 ms at the headline size)
  const double floor_rate = valu_form ? 6.3e12 : fused ? 6.3e12 : 6.6e12;
  const double good_rate = std::max(floor_rate, copy_rate > 1e12 ? (valu_form ? 1.25 : fused ? 1.19 : 1.30) * copy_rate : 0.0);
  const double good_ms = algo / good_rate * 1e3;
  std::vector<double> t{probe(cand[0], 4)};
  for (int k = 1; k < tries && !rc && t.back() > good_ms; k++) {
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < total_b / 2 || free_b < 2 * bytes + ((size_t)1 << 30)) break;   // (never crowd the card)
    DevBuf p;
    if (!dev_alloc_fresh(p, bytes)) break;
    cand.push_back(p); t.push_back(probe(cand.back(), 4));
    // (a kernel the pages do not matter to -- bound by its arithmetic, never near the rate above -- shows it after four candidates:
    // all within 1.5 % of each other.  The search ends there instead of trying every allocation for nothing.)
    if (t.size() == 4) {
      const double lo = *std::min_element(t.begin(), t.end()), hi = *std::max_element(t.begin(), t.end());
      if (hi - lo < 0.015 * lo) break;
    }
  }
  // the part's clocks are still ramping while the first candidates are timed (launches 3-40 after an idle gap): those are
  // timed again now that it has settled
  for (size_t k = 0; k < cand.size() && k < 8 && 8 + 4 * k < 40 && cand.size() > 1 && !rc; k++) t[k] = std::min(t[k], probe(cand[k], 4));
  size_t best = 0;
  for (size_t k = 1; k < t.size(); k++) if (t[k] < t[best]) best = k;
  for (size_t k = 0; k < cand.size(); k++) if (k != best) dev_free(cand[k]);
  c->J = cand[best];
  c->place.n = (int)t.size();
  c->place.ms[0] = t[best];
  for (size_t k = 0, o = 1; k < t.size() && o < 7; k++) if (k != best) c->place.ms[o++] = t[k];
  // Round 6: the kernel's OTHER streams -- x, y, w read, res written: 32 of the 32 + 8 p bytes per point, a third of the traffic at 8
  // parameters -- sit in allocations of their own, and the pages behind THEM decide as much: BASELINE config 2 ran at 0.150-0.152 ms
  // or at 0.169-0.173 ms from process to process with every candidate of the Jacobian buffer alike within the process
  // (profiles/r06_data_placement.txt).  So while the kernel is still on the slow side the four arrays are re-placed together: a
  // new set allocated, the contents copied device to device, the kernel timed, the faster set kept.  GADFIT_HIP_PLACE_DATA=0: not.
  static const bool place_data = [] { const char* e = getenv("GADFIT_HIP_PLACE_DATA"); return !e || atoi(e) != 0; }();
  c->place.data_n = 0;
  if (place_data && !rc && c->n_slots > 0 && c->x.p && c->y.p && c->w.p && c->res.p) {
    const size_t nb = sizeof(double) * (size_t)c->n_slots;
    double best_t = c->place.ms[0];
    int stale = 0;
    for (int k = 0; k < tries && !rc && best_t > good_ms; k++) {
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < total_b / 2 || free_b < 8 * nb + ((size_t)1 << 30)) break;
      DevBuf nw[4];                                    // (the set not in use: the new one until the swap, the old one after it)
      DevBuf* cur[4] = {&c->x, &c->y, &c->w, &c->res};
      bool ok = true;
      for (int a = 0; a < 4 && ok; a++) ok = dev_alloc_fresh(nw[a], std::max(nb, cur[a]->bytes));
      for (int a = 0; a < 4 && ok; a++) ok = hipMemcpyAsync(nw[a].p, cur[a]->p, cur[a]->bytes, hipMemcpyDeviceToDevice, c->stream) == hipSuccess;
      if (!ok) { (void)hipGetLastError(); hipStreamSynchronize(c->stream); for (int a = 0; a < 4; a++) dev_free(nw[a]); break; }
      for (int a = 0; a < 4; a++) std::swap(*cur[a], nw[a]);
      const double tk = std::min(probe(c->J, 4), probe(c->J, 4));
      c->place.data_n++;
      if (!rc && tk < best_t) { if (tk < 0.99 * best_t) stale = 0; best_t = tk; for (int a = 0; a < 4; a++) dev_free(nw[a]); }
      else { hipStreamSynchronize(c->stream); for (int a = 0; a < 4; a++) { std::swap(*cur[a], nw[a]); dev_free(nw[a]); } }
      if (++stale >= 4) break;                         // (four sets in a row that gained nothing: these arrays are not what holds the kernel)
    }
    c->place.data_ms = best_t;
    c->place.ms[0] = best_t;
  }
  hipEventDestroy(e0); hipEventDestroy(e1);
  return rc;
}

extern "C" {

int gfh_set_placement_tries(gfh_ctx* c, int tries) {
  if (!c) return 1;
  GROUP(c, gfh_set_placement_tries(k, tries));
  if (tries < 1 || tries > 16) return fail(c, "gfh_set_placement_tries: between 1 and 16");
  c->place.tries = tries;
  return 0;
}
int gfh_set_placement_after(gfh_ctx* c, int sweeps) {
  if (!c) return 1;
  GROUP(c, gfh_set_placement_after(k, sweeps));
  if (sweeps < 0) return fail(c, "gfh_set_placement_after: a number of sweeps >= 0");
  c->place.after = sweeps;
  return 0;
}
int gfh_get_placement(gfh_ctx* c, double* out8) {
  if (!c) return 1;
  if (c->grp) return gfh_get_placement(gfh::group_member(c, 0), out8);
  for (int k = 0; k < 7; k++) out8[k] = k < c->place.n ? c->place.ms[k] : 0.0;
  out8[7] = c->place.n ? 1e-9 * c->place.copy_rate : 0.0;      // GB/s of the copy the thresholds were scaled with
  return 0;
}

}  // extern "C"
