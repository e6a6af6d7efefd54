// ws_plan.cpp -- host-side planning of a quadrature model's workspaces and mesh records: what active.cpp and launch.cpp ask the
// generator's side before a launch.  Emits nothing.
#include "codegen.h"

namespace gfh {

// Where the workspaces live and how many intervals the translation unit carries (model.h, WsPlan).
// (scratch form: 8 NQ bytes more per interval and lane, small workspaces only; pool form: NQ more fields in the interval's row)
bool carries_gradients(int n_ipars, int ws, bool global) {
  const int nq = n_ipars > 0 ? n_ipars : 1;
  return global ? nq <= kWsgCarryMax : (nq <= 4 && ws <= 128);
}
int wsg_row_fields(const Model& m, int level) {
  int nq = 0;
  for (const Integral& in : m.integrals)
    if ((in.depth <= 1) == (level == 1)) { const int q = in.n_ipars > 0 ? in.n_ipars : 1; if (q <= kWsgCarryMax) nq = std::max(nq, q); }
  return 4 + nq;
}

static long ws_scratch_bytes(const Model& m, int ws1, int ws2) {
  int nq1 = 0, nq2 = 0; bool nested = false;
  for (const Integral& in : m.integrals) {
    const int nq = in.n_ipars > 0 ? in.n_ipars : 1;
    if (in.depth <= 1) nq1 = std::max(nq1, nq); else { nq2 = std::max(nq2, nq); nested = true; }
  }
  long b = (long)ws1 * (32 + (carries_gradients(nq1, ws1, false) ? 8 * nq1 : 0));
  if (nested) b += (long)ws2 * (32 + (carries_gradients(nq2, ws2, false) ? 8 * nq2 : 0));
  return b;
}

WsPlan plan_workspaces(const Model& m, int fast, bool grown) {
  WsPlan p{m.ws_size, m.ws_size_inner, false};
  if (!m.has_integrals()) return p;
  if (!grown && fast >= 2) {
    p.ws_size = std::min(fast, m.ws_size); p.ws_size_inner = std::min(fast, m.ws_size_inner);
    // (nested integrals with several bound parameters: both levels shrink together until the budget holds them)
    while (ws_scratch_bytes(m, p.ws_size, p.ws_size_inner) > kScratchBudget && std::max(p.ws_size, p.ws_size_inner) > 2) {
      const int top = std::max(p.ws_size, p.ws_size_inner) - 1;
      p.ws_size = std::min(p.ws_size, top); p.ws_size_inner = std::min(p.ws_size_inner, top);
    }
    return p;
  }
  p.global = ws_scratch_bytes(m, p.ws_size, p.ws_size_inner) > kScratchBudget;
  return p;
}

int mesh_sites(const Model& m) {
  if (!m.has_integrals()) return 0;
  int most = 0;
  for (int v = 0; v < m.n_variants(); v++) {
    int n = 0;
    for (const Node& nd : m.eval(v).nodes)
      if (nd.op == GFH_INTEGRATE) {
        const Integral& in = m.integrals[(size_t)nd.a];
        if (in.depth <= 1 && !(in.lower_inf && in.upper_inf) && n < kMeshSitesMax) n++;
      }
    most = std::max(most, n);
  }
  return most;
}

}  // namespace gfh
