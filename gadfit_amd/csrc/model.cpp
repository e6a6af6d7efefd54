// model.cpp -- the host-side copy of a gfh_tape: validation of what a front end hands over, the pooling of further recorded
// paths of the same eval() (variants, and further recordings of an integrand) and their bookkeeping.  No code generation here:
// codegen.cpp and the emit_*.cpp files lower a loaded Model to HIP source.
#include "model.h"
#include "../../include/gadfit_gk_tables.h"
#include <cstring>
#include <functional>

namespace gfh {

bool Model::load(const gfh_tape* t, std::string* err) {
  if (!t || t->n_subtapes < 1 || !t->sub) { *err = "empty tape"; return false; }
  n_pars = t->n_pars;
  sub.clear(); integrals.clear(); ipar_nodes.clear();
  int n_bind = 0;
  for (int i = 0; i < t->n_integrals; i++) {
    const gfh_integral& g = t->integrals[i];
    integrals.push_back({g.integrand, g.lower, g.upper, g.lower_inf, g.upper_inf, g.n_ipars,
                         g.ipar_off, g.depth, g.rel_error, g.abs_error});
    if (g.ipar_off + g.n_ipars > n_bind) n_bind = g.ipar_off + g.n_ipars;
    if (g.integrand < 1 || g.integrand >= t->n_subtapes) { *err = "integral refers to a missing sub-tape"; return false; }
  }
  for (int i = 0; i < n_bind; i++) ipar_nodes.push_back(t->ipar_nodes[i]);
  for (int s = 0; s < t->n_subtapes; s++) {
    const gfh_subtape& st = t->sub[s];
    SubTape o; o.result = st.result;
    if (st.n_nodes < 1 || st.result < 0 || st.result >= st.n_nodes) { *err = "malformed sub-tape"; return false; }
    for (int k = 0; k < st.n_nodes; k++) {
      const gfh_node& n = st.nodes[k];
      Node d{n.op, n.a, n.b, n.flags, n.c};
      auto bad_ref = [&](int r) { return r < 0 || r >= k; };
      switch (n.op) {
        case GFH_CONST: case GFH_X: case GFH_IVAR: break;
        case GFH_AUX:
          // (inside an integrand too: a real of the enclosing eval() that the integrand takes without passing it through pars(:))
          if (n.a < 0 || n.a >= t->n_aux) { *err = "auxiliary column out of range"; return false; }
          break;
        case GFH_PARAM: if (n.a < 0 || n.a >= n_pars) { *err = "parameter index out of range"; return false; } break;
        case GFH_IPARAM: if (n.a < 0) { *err = "bad integrand parameter"; return false; } break;
        case GFH_LIFT: case GFH_NEG: case GFH_POWI: case GFH_VAL:
          if (bad_ref(n.a)) { *err = "operand refers forward"; return false; } break;
        case GFH_ADD: case GFH_SUB: case GFH_MUL: case GFH_DIV: case GFH_POW:
          if (bad_ref(n.a) || bad_ref(n.b)) { *err = "operand refers forward"; return false; } break;
        case GFH_INTEGRATE: if (n.a < 0 || n.a >= t->n_integrals) { *err = "bad integral index"; return false; } break;
        case GFH_GUARD_GT: case GFH_GUARD_LT:
          // (inside an integrand, s != 0: decided per evaluation of the integrand -- Model::alts, emit_family)
          if (bad_ref(n.a) || bad_ref(n.b)) { *err = "operand refers forward"; return false; }
          break;
        default:
          if (n.op >= GFH_ABS && n.op <= GFH_ERF) { if (bad_ref(n.a)) { *err = "operand refers forward"; return false; } }
          else { *err = "unknown op code " + std::to_string(n.op); return false; }
      }
      o.nodes.push_back(d);
    }
    sub.push_back(std::move(o));
  }
  gk_points = t->gk_points ? t->gk_points : 15;
  n_aux = t->n_aux > 0 ? t->n_aux : 0;
  rel_error_outer = t->rel_error_outer; rel_error_inner = t->rel_error_inner;
  ws_size = t->ws_size > 0 ? t->ws_size : 1000;                       // NI:40 DEFAULT_WORKSPACE_SIZE
  ws_size_inner = t->ws_size_inner > 0 ? t->ws_size_inner : 1000;
  if (ws_size < 2 || ws_size_inner < 2) { *err = "quadrature workspace size must be at least 2"; return false; }
  // (any size the device's memory holds: workspaces beyond the scratch budget live in the context's global pool, plan_workspaces)
  if (ws_size > (1 << 22) || ws_size_inner > (1 << 22)) { *err = "quadrature workspace size beyond 4194304 intervals"; return false; }
  more_evals.clear(); hint_aux = -1; hint_cols.clear(); tape_variant.assign(1, 0);
  alts.assign(integrals.size(), {});
  // a guard has no value: nothing may use one as an operand, a bound, a binding or the result
  for (const SubTape& st : sub) {
    auto guard = [&](int k) { return k >= 0 && k < (int)st.nodes.size() && is_guard_op(st.nodes[(size_t)k].op); };
    bool bad = guard(st.result);
    for (const Node& nd : st.nodes) {
      switch (nd.op) {
        case GFH_CONST: case GFH_X: case GFH_AUX: case GFH_PARAM: case GFH_IVAR: case GFH_IPARAM: case GFH_GUARD_GT: case GFH_GUARD_LT: break;
        case GFH_INTEGRATE: {
          const Integral& in = integrals[(size_t)nd.a];
          if ((!in.lower_inf && guard(in.lower)) || (!in.upper_inf && guard(in.upper))) bad = true;
          for (int q = 0; q < in.n_ipars; q++) if (guard(ipar_nodes[(size_t)in.ipar_off + q])) bad = true;
          break;
        }
        case GFH_ADD: case GFH_SUB: case GFH_MUL: case GFH_DIV: case GFH_POW: if (guard(nd.a) || guard(nd.b)) bad = true; break;
        default: if (guard(nd.a)) bad = true; break;
      }
    }
    if (bad) { *err = "a comparison is used as a value"; return false; }
  }
  return true;
}

bool Model::has_guards() const {
  for (int v = 0; v < n_variants(); v++) for (const Node& nd : eval(v).nodes) if (is_guard_op(nd.op)) return true;
  return false;
}

namespace {
bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
}  // namespace
bool same_node(const Node& a, const Node& b) {
  return a.op == b.op && a.a == b.a && a.b == b.b && (a.flags & ~GFH_F_TAKEN) == (b.flags & ~GFH_F_TAKEN) && same_bits(a.c, b.c);
}
namespace {
bool same_subtape(const SubTape& a, const SubTape& b) {
  if (a.result != b.result || a.nodes.size() != b.nodes.size()) return false;
  for (size_t k = 0; k < a.nodes.size(); k++) if (!same_node(a.nodes[k], b.nodes[k]) || a.nodes[k].flags != b.nodes[k].flags) return false;
  return true;
}
}  // namespace

// Further recorded paths of the same eval().  Their integrand sub-tapes and integrate() call sites join the pool of variant 0
// (sub[1..], integrals, ipar_nodes), identical ones shared -- so one generated device function serves every variant that calls
// it, and an INTEGRATE node of two variants is the same operation exactly when it carries the same pooled index.
bool Model::load_variants(int n, const gfh_tape* const* t, int hint, std::string* err, const std::vector<int32_t>* cols) {
  if (n < 1 || !t || !t[0]) { *err = "no variant"; return false; }
  if (!load(t[0], err)) return false;
  n_tapes = n;
  tape_variant.assign((size_t)n, 0);
  for (int v = 1; v < n; v++) {
    Model o;
    if (!t[v]) { *err = "null variant"; return false; }
    if (!o.load(t[v], err)) { *err = "variant " + std::to_string(v) + ": " + *err; return false; }
    if (o.n_pars != n_pars) { *err = "variants disagree on the number of parameters"; return false; }
    if (o.gk_points != gk_points || o.rel_error_outer != rel_error_outer || o.rel_error_inner != rel_error_inner ||
        o.ws_size != ws_size || o.ws_size_inner != ws_size_inner) { *err = "variants disagree on the quadrature settings"; return false; }
    n_aux = std::max(n_aux, o.n_aux);
    std::vector<int> sub_map(o.sub.size(), -1), int_map(o.integrals.size(), -1);
    std::vector<char> busy(o.integrals.size(), 0);
    bool ok = true;
    // pooled index of the variant's integral i (its integrand pooled first; integrands may nest call sites: depth <= 2, NI:70)
    std::function<int(int)> pool_integral;
    auto pool_sub = [&](int s_) -> int {
      if (sub_map[(size_t)s_] >= 0) return sub_map[(size_t)s_];
      SubTape st = o.sub[(size_t)s_];
      for (Node& nd : st.nodes) if (nd.op == GFH_INTEGRATE) { nd.a = pool_integral(nd.a); if (nd.a < 0) return -1; }
      for (size_t k = 1; k < sub.size(); k++) if (same_subtape(sub[k], st)) return sub_map[(size_t)s_] = (int)k;
      sub.push_back(std::move(st));
      return sub_map[(size_t)s_] = (int)sub.size() - 1;
    };
    pool_integral = [&](int i) -> int {
      if (int_map[(size_t)i] >= 0) return int_map[(size_t)i];
      if (busy[(size_t)i]) { ok = false; *err = "recursive integrate() call site"; return -1; }
      busy[(size_t)i] = 1;
      Integral in = o.integrals[(size_t)i];
      in.integrand = pool_sub(in.integrand);
      busy[(size_t)i] = 0;
      if (in.integrand < 0) return -1;
      const int32_t* binds = o.ipar_nodes.data() + in.ipar_off;
      for (size_t k = 0; k < integrals.size(); k++) {
        const Integral& e = integrals[k];
        if (e.integrand == in.integrand && e.lower == in.lower && e.upper == in.upper && e.lower_inf == in.lower_inf && e.upper_inf == in.upper_inf &&
            e.n_ipars == in.n_ipars && e.depth == in.depth && same_bits(e.rel_error, in.rel_error) && same_bits(e.abs_error, in.abs_error) &&
            std::equal(binds, binds + in.n_ipars, ipar_nodes.begin() + e.ipar_off))
          return int_map[(size_t)i] = (int)k;
      }
      const int off = (int)ipar_nodes.size();
      ipar_nodes.insert(ipar_nodes.end(), binds, binds + in.n_ipars);
      in.ipar_off = off;
      integrals.push_back(in);
      return int_map[(size_t)i] = (int)integrals.size() - 1;
    };
    SubTape ev = o.sub[0];
    for (Node& nd : ev.nodes) if (nd.op == GFH_INTEGRATE) { nd.a = pool_integral(nd.a); if (nd.a < 0 || !ok) { if (err->empty()) *err = "bad integrate() call site"; return false; } }
    alts.resize(integrals.size());
    bool dup = false;
    for (int w = 0; w < n_variants() && !dup; w++) dup = same_subtape(eval(w), ev);
    if (dup) { *err = "variant " + std::to_string(v) + " repeats an earlier one"; return false; }
    // the same path through eval() as an earlier variant, with an integrand that took another path through ITS comparisons (the
    // call sites agree in everything but the integrand's sub-tape): not a variant of eval() but a further recording of that
    // integrand.  An integrand that calls integrate() itself is compared the same way, node by node (so the recordings of an INNER
    // integrand that compares AD variables end up at the inner call site).
    std::function<bool(int, int, std::vector<std::pair<int, int>>&)> same_site = [&](int Ia, int Ib, std::vector<std::pair<int, int>>& add) -> bool {
      if (Ia == Ib) return true;
      const Integral &x = integrals[(size_t)Ia], &y = integrals[(size_t)Ib];
      const bool site = x.lower == y.lower && x.upper == y.upper && x.lower_inf == y.lower_inf && x.upper_inf == y.upper_inf &&
                        x.n_ipars == y.n_ipars && x.depth == y.depth && same_bits(x.rel_error, y.rel_error) && same_bits(x.abs_error, y.abs_error) &&
                        std::equal(ipar_nodes.begin() + x.ipar_off, ipar_nodes.begin() + x.ipar_off + x.n_ipars, ipar_nodes.begin() + y.ipar_off);
      if (!site) return false;
      if (x.integrand == y.integrand) return true;
      const SubTape &sa = sub[(size_t)x.integrand], &sb = sub[(size_t)y.integrand];
      // the same recording of the integrand up to call sites inside it that are themselves the same site?
      if (sa.result == sb.result && sa.nodes.size() == sb.nodes.size()) {
        std::vector<std::pair<int, int>> inner;
        bool same = true, any_int = false;
        for (size_t k = 0; k < sa.nodes.size() && same; k++) {
          const Node &p = sa.nodes[k], &q = sb.nodes[k];
          if (same_node(p, q) && p.flags == q.flags) continue;
          if (p.op == GFH_INTEGRATE && q.op == GFH_INTEGRATE && p.b == q.b && p.flags == q.flags && same_site(p.a, q.a, inner)) { any_int = true; continue; }
          same = false;
        }
        if (same && any_int) { add.insert(add.end(), inner.begin(), inner.end()); return true; }
      }
      add.push_back({Ia, y.integrand});                  // another path through this integrand's own comparisons
      return true;
    };
    bool joined = false;
    for (int w = 0; w < n_variants() && !joined; w++) {
      const SubTape& e = eval(w);
      if (e.result != ev.result || e.nodes.size() != ev.nodes.size()) continue;
      std::vector<std::pair<int, int>> add;
      bool same = true, any_int = false;
      for (size_t k = 0; k < e.nodes.size() && same; k++) {
        const Node &p = e.nodes[k], &q = ev.nodes[k];
        if (same_node(p, q) && p.flags == q.flags) continue;
        if (p.op == GFH_INTEGRATE && q.op == GFH_INTEGRATE && p.b == q.b && p.flags == q.flags && p.a != q.a && same_site(p.a, q.a, add)) { any_int = true; continue; }
        same = false;
      }
      if (!same || !any_int) continue;
      for (auto& d : add) {
        std::vector<int32_t>& f = alts[(size_t)d.first];
        if (d.second != integrals[(size_t)d.first].integrand && std::find(f.begin(), f.end(), (int32_t)d.second) == f.end()) f.push_back((int32_t)d.second);
      }
      joined = true;
      tape_variant[(size_t)v] = w;
    }
    if (joined) continue;
    more_evals.push_back(std::move(ev));
    tape_variant[(size_t)v] = n_variants() - 1;
  }
  alts.resize(integrals.size());
  if (hint >= n_aux) { *err = "the per-point variant column lies outside the auxiliary columns"; return false; }
  hint_aux = hint < 0 ? -1 : hint;
  hint_cols.clear();
  if (cols && hint_aux >= 0 && (int)cols->size() == n) {
    for (int32_t cidx : *cols) if (cidx < 0 || cidx >= n_aux) { *err = "a per-point variant column lies outside the auxiliary columns"; return false; }
    hint_cols = *cols;
  }
  return true;
}

int Model::hint_col_of_variant(int v) const {
  if (hint_cols.empty()) return hint_aux;
  for (size_t t = 0; t < tape_variant.size(); t++) if (tape_variant[t] == v) return hint_cols[t];
  return hint_aux;
}
std::vector<int> Model::tapes_of_variant(int v) const {
  std::vector<int> out;
  for (size_t t = 0; t < tape_variant.size(); t++) if (tape_variant[t] == v) out.push_back((int)t);
  if (out.empty()) out.push_back(v);          // (a model set through gfh_set_model: tape 0 = variant 0)
  return out;
}

GkRule gk_rule(int points) {
  switch (points) {
    case 15: return {gk15_roots, gk15_wg, gk15_wk, 15};
    case 21: return {gk21_roots, gk21_wg, gk21_wk, 21};
    case 31: return {gk31_roots, gk31_wg, gk31_wk, 31};
    case 41: return {gk41_roots, gk41_wg, gk41_wk, 41};
    case 51: return {gk51_roots, gk51_wg, gk51_wk, 51};
    case 61: return {gk61_roots, gk61_wg, gk61_wk, 61};
  }
  return {nullptr, nullptr, nullptr, 0};
}

}  // namespace gfh

// The Gauss-Kronrod rule the kernels are generated with, for the Fortran layer's host-side integrate() (gadf_print and calls of
// eval() outside gadf_fit: numerical_integration.F90, host_integral): reference node order, even 1-based positions = Gauss nodes.
extern "C" __attribute__((visibility("default"))) int gfh_gk_rule(int points, double* roots, double* wg, double* wk) {
  const gfh::GkRule rule = gfh::gk_rule(points);
  if (!roots || !wg || !wk || !rule.n) return 1;
  for (int i = 0; i < points; i++) { roots[i] = rule.roots[i]; wk[i] = rule.wk[i]; }
  for (int i = 0; i < points / 2; i++) wg[i] = rule.wg[i];
  return 0;
}
