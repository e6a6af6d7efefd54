// emit_branching.cpp -- a model whose eval() or integrands branch: the decision tree over its recordings, the selectors and the dispatchers.
#include "codegen_internal.h"
#include "device_text.h"
#include "unseen_report.h"
#include <algorithm>
#include <functional>

namespace gfh {

namespace {

// ---------------------------------------------------------------------------------------
// Branching eval() (AD:315-395; gadfit.F90:679-690 evaluates eval() afresh at every point, so a model may take another
// branch from one point to the next and from one parameter set to the next).  Every recorded path is a straight-line
// tape ("variant") whose comparisons are guard nodes with the outcome they had on that path.  The variants of one model
// share their nodes up to the first guard that came out differently, so together they form a decision tree: walk the
// common nodes, evaluate the guard AT THE CURRENT PARAMETERS on the device, descend.  gfh_select is that walk with values
// only (every parameter passive, the reference's expression shapes: comparisons look at val alone); it returns the variant
// whose body the lane then runs, or -1 where the point takes a turn no recording has taken yet -- the lane then reports
// its slot and the outcomes so far (gfh_report_unseen), the host records eval() at that point along those outcomes, adds
// the variant and repeats the pass (passes.cpp, recover_unseen).
// Where two variants part ways WITHOUT a guard (a Fortran eval() that branches on the plain real x: invisible to the
// recorder), only the host can tell which points go where: a per-point column (Model::hint_aux) names the variant each
// point took when the columns were tabulated, and the walk follows it at such a fork.
struct TrieNode {
  int kind = 0;              // 0 leaf, 1 guard, 2 fork without a guard
  int rep = 0;               // a variant of this subtree: its nodes [from, to) are evaluated before the decision
  int from = 0, to = 0;
  int leaf = -1;             // kind 0: the variant
  int guard = -1;            // kind 1: node index of the guard in rep
  int child[2] = {-1, -1};   // kind 1: [outcome false, outcome true]; -1 = never recorded
  std::vector<int> kids;     // kind 2
  std::vector<int> members;  // variants below this node
};

struct Trie {
  const Model& m;
  std::vector<TrieNode> nodes;
  std::string err;
  bool forks = false;
  std::function<const SubTape&(int)> tape;       // the recordings the tree is built over: eval() of variant v, or the members of an integrand family
  explicit Trie(const Model& mm) : m(mm), tape([&mm](int v) -> const SubTape& { return mm.eval(v); }) {}
  Trie(const Model& mm, std::function<const SubTape&(int)> t) : m(mm), tape(std::move(t)) {}

  int build(const std::vector<int>& S, int pos) {
    TrieNode t; t.rep = S[0]; t.from = pos; t.members = S;
    int q = pos;
    for (;;) {
      bool any_end = false, all_end = true;
      for (int v : S) { if (q >= (int)tape(v).nodes.size()) any_end = true; else all_end = false; }
      if (all_end) {
        if (S.size() > 1) { err = "two variants record the same operations"; return -1; }
        t.kind = 0; t.leaf = S[0]; t.to = q;
        nodes.push_back(t); return (int)nodes.size() - 1;
      }
      bool same = !any_end;
      if (same) for (int v : S) if (!same_node(tape(v).nodes[(size_t)q], tape(S[0]).nodes[(size_t)q])) { same = false; break; }
      if (same && !is_guard_op(tape(S[0]).nodes[(size_t)q].op)) { q++; continue; }
      t.to = q;
      if (same) {                                   // the same comparison on every path through here
        t.kind = 1; t.guard = q;
        std::vector<int> side[2];
        for (int v : S) side[(tape(v).nodes[(size_t)q].flags & GFH_F_TAKEN) ? 1 : 0].push_back(v);
        const int me = (int)nodes.size(); nodes.push_back(t);
        for (int o = 0; o < 2; o++) if (!side[o].empty()) { const int c = build(side[o], q + 1); if (c < 0) return -1; nodes[(size_t)me].child[o] = c; }
        return me;
      }
      // different operations (or one path ends here): classes of equal next node
      t.kind = 2; forks = true;
      std::vector<std::vector<int>> cls;
      for (int v : S) {
        bool placed = false;
        for (auto& c : cls) {
          const int w = c[0];
          const bool ve = q >= (int)tape(v).nodes.size(), we = q >= (int)tape(w).nodes.size();
          if (ve || we ? (ve && we && tape(v).result == tape(w).result)
                       : same_node(tape(v).nodes[(size_t)q], tape(w).nodes[(size_t)q])) { c.push_back(v); placed = true; break; }
        }
        if (!placed) cls.push_back({v});
      }
      if (cls.size() < 2) { err = "two variants record the same operations"; return -1; }
      const int me = (int)nodes.size(); nodes.push_back(t);
      for (auto& c : cls) { const int k = build(c, q); if (k < 0) return -1; nodes[(size_t)me].kids.push_back(k); }
      return me;
    }
  }
};

// nodes of variant v whose values some guard of v needs (transitively)
std::vector<char> guard_needs_of(const Model& m, const SubTape& st) {
  std::vector<char> need(st.nodes.size(), 0);
  for (int k = (int)st.nodes.size() - 1; k >= 0; k--) {
    const Node& nd = st.nodes[(size_t)k];
    if (!is_guard_op(nd.op) && !need[(size_t)k]) continue;
    auto want = [&](int r) { if (r >= 0) need[(size_t)r] = 1; };
    switch (nd.op) {
      case GFH_CONST: case GFH_X: case GFH_AUX: case GFH_PARAM: case GFH_IVAR: case GFH_IPARAM: break;
      case GFH_INTEGRATE: {
        const Integral& in = m.integrals[(size_t)nd.a];
        if (!in.lower_inf) want(in.lower);
        if (!in.upper_inf) want(in.upper);
        for (int q = 0; q < in.n_ipars; q++) want(m.ipar_nodes[(size_t)in.ipar_off + q]);
        break;
      }
      case GFH_ADD: case GFH_SUB: case GFH_MUL: case GFH_DIV: case GFH_POW: case GFH_GUARD_GT: case GFH_GUARD_LT: want(nd.a); want(nd.b); break;
      default: want(nd.a); break;      // unary, LIFT, NEG, POWI
    }
  }
  return need;
}
std::vector<char> guard_needs(const Model& m, int v) { return guard_needs_of(m, m.eval(v)); }

}  // namespace

// gfh_select (see above).  PATH / NG: the outcomes of the guards passed so far and their number, for the report of an unseen turn.
bool emit_selector(const Model& m, std::ostringstream& s, std::string* err) {
  const int V = m.n_variants();
  Trie T(m);
  std::vector<int> all(V); for (int v = 0; v < V; v++) all[(size_t)v] = v;
  const int root = T.build(all, 0);
  if (root < 0) { *err = "gfh_set_model_variants: " + T.err; return false; }
  if (T.forks && m.hint_aux < 0) {
    *err = "the recorded variants of eval() part ways without a comparison of AD variables (control flow on plain real values): "
           "the per-point variant column is needed (gfh_set_model_variants, hint_aux)";
    return false;
  }
  std::vector<std::vector<char>> need((size_t)V);
  for (int v = 0; v < V; v++) need[(size_t)v] = guard_needs(m, v);
  const std::vector<char> none((size_t)std::max(1, m.n_pars), 0);
  s << "\n// A lane whose point takes a turn through eval() that no recorded variant covers: status 3 and one entry {slot, outcomes of\n"
       "// the guards passed, their number} in the report area behind the status word (context.h, kStatusBytes).\n"
       "#define GFH_UNSEEN_CAP " << kUnseenCap << "\n" << kUnseen;      // unseen.hip: struct gfh_unseen, gfh_report_unseen
  s << "\n// Which recorded path of eval() does this point take at these parameters?  (codegen.cpp, Trie)\n"
       "static __device__ __forceinline__ int gfh_select(const double X, const double* __restrict__ P, int* STATUS,\n"
       "                                                 const double* __restrict__ AXP, const i64 LDA, unsigned long long& PATH, int& NG) {\n"
       "  PATH = 0ull; NG = 0;\n  GFH_LANE_STASH\n";
  // (HV: the per-point variant column once a fork without a comparison has been passed.  The walk then ends on a variant the HOST
  // has seen this point take -- HV itself -- or reports the point: behind such a fork the recordings of one class need not share the
  // side of the plain real branch that set them apart (two of them may agree by accident in the node where a third differs, an
  // affine literal's slope in its last bit), so a leaf other than HV is not taken on the device's word alone; the host records the
  // point along the outcomes met, tabulates the column anew at the parameters of this pass, and the pass is repeated.)
  if (T.forks) s << "  int HV = -2;\n";
  bool ok = true;
  // `fail`: what a walk does where it cannot go on (a comparison comes out a way nobody recorded, a leaf the host has not seen this
  // point take): report the point -- or, inside a fork's kid, give up on that kid and try the next one (round 5).  Recordings may
  // part ways without a comparison for a reason that a LATER comparison settles (the same source line holding another per-point
  // column on either side of it): which kid is the point's cannot be read off a column alone then, but only one of the candidates
  // can be walked to a leaf that the host has seen the point take under the outcomes met on the way.
  int n_labels = 0;
  std::function<void(int, int, const std::string&, const std::string&)> walk = [&](int idx, int depth, const std::string& ind, const std::string& fail) {
    const TrieNode& t = T.nodes[(size_t)idx];
    auto failing = [&](int ng) { return fail.empty() ? "{ NG = " + std::to_string(ng) + "; return -1; }" : "{ " + fail + " }"; };
    {
      Gen g(m, m.eval(t.rep), false); g.mode = 0; g.ind = ind; g.analyse(none);
      for (int k = t.from; k < t.to; k++) {
        bool wanted = false;
        for (int v : t.members) if (need[(size_t)v][(size_t)k]) { wanted = true; break; }
        if (wanted) g.emit_value_node(k);
      }
      s << g.o.str();
    }
    if (t.kind == 0) {
      // (behind a fork the walk ends on a leaf the HOST has seen this point take under exactly these outcomes -- the column of the
      // leaf's own set of outcomes names a tape of this leaf -- or fails)
      if (T.forks) {
        s << ind << "if (HV != -2) { const int hl = (int)AXP[(i64)" << m.hint_col_of_variant(t.leaf) << " * LDA]; if (!(";
        const std::vector<int> tp = m.tapes_of_variant(t.leaf);
        for (size_t q = 0; q < tp.size(); q++) s << (q ? " || " : "") << "hl == " << tp[q];
        s << ")) " << failing(depth) << " }\n";
      }
      s << ind << "return " << t.leaf << ";\n";
      return;
    }
    if (t.kind == 1) {
      if (depth >= 64) { ok = false; *err = "more than 64 comparisons on one path through eval()"; return; }
      const Node& nd = m.eval(t.rep).nodes[(size_t)t.guard];
      s << ind << "const bool c" << t.guard << " = v" << nd.a << (nd.op == GFH_GUARD_GT ? " > " : " < ") << "v" << nd.b << ";      // AD:315-395: values only\n";
      s << ind << "PATH |= (c" << t.guard << " ? 1ull : 0ull) << " << depth << ";\n";
      for (int o = 1; o >= 0; o--) {
        s << ind << (o ? "if (c" + std::to_string(t.guard) + ") {\n" : "} else {\n");
        if (t.child[o] >= 0) walk(t.child[o], depth + 1, ind + "  ", fail);
        else s << ind << "  " << failing(depth + 1) << "\n";
      }
      s << ind << "}\n";
      return;
    }
    // A fork without a comparison.  Kid by kid: the column of the kid's own outcomes (its first recording's) must name a tape of the
    // kid -- the host has seen this point go there under those outcomes -- and the walk inside must reach a leaf; else the next kid.
    s << ind << "const unsigned long long pf" << idx << " = PATH;\n";
    for (size_t c = 0; c < t.kids.size(); c++) {
      const TrieNode& k = T.nodes[(size_t)t.kids[c]];
      const int lab = n_labels++;
      s << ind << "{\n" << ind << "  const int h" << idx << "_" << c << " = (int)AXP[(i64)" << m.hint_col_of_variant(k.members[0]) << " * LDA];      // the tape this point follows under that kid's outcomes\n";
      s << ind << "  if (";
      bool first = true;
      for (size_t q = 0; q < k.members.size(); q++)
        for (int tpi : m.tapes_of_variant(k.members[q])) { s << (first ? "" : " || ") << "h" << idx << "_" << c << " == " << tpi; first = false; }
      s << ") {\n" << ind << "    HV = h" << idx << "_" << c << ";\n";
      walk(t.kids[c], depth, ind + "    ", "goto gfh_next" + std::to_string(lab) + ";");
      s << ind << "  }\n" << ind << "}\n" << ind << "gfh_next" << lab << ": PATH = pf" << idx << ";\n";
    }
    s << ind << failing(depth) << "\n";
  };
  walk(root, 0, "  ", "");
  s << "}\n";
  return ok;
}

// The recordings of ONE integrand that compares AD variables (Model::alts): which of them is the path of this abscissa, and the four
// forms of the integrand (value, value + gradient, forward mode with and without a tangent on the integration variable) as
// dispatchers under the names gfh_sf<I>_* that call site I uses instead of gfh_s<S>_*.  The comparisons are decided on values, per
// evaluation, exactly as the reference's integrand decides them when the quadrature calls it (AD:315-395).  An abscissa whose
// outcomes no recording has raises status 2 (the host reports it: the recordings sampled the integration variable too coarsely).
bool emit_family(const Model& m, int I, std::ostringstream& s, std::string* err) {
  const Integral& in = m.integrals[(size_t)I];
  const std::vector<int> mem = family_members(m, I);
  const int M = (int)mem.size();
  Trie T(m, [&m, mem](int k) -> const SubTape& { return m.sub[(size_t)mem[(size_t)k]]; });
  std::vector<int> all((size_t)M); for (int k = 0; k < M; k++) all[(size_t)k] = k;
  const int root = T.build(all, 0);
  if (root < 0) { *err = "integrand recordings: " + T.err; return false; }
  if (T.forks) { *err = "the recordings of an integrand part ways without a comparison of AD variables (control flow on plain real values inside an integrand)"; return false; }
  std::vector<std::vector<char>> need((size_t)M);
  int nip = 0;
  for (int k = 0; k < M; k++) {
    need[(size_t)k] = guard_needs_of(m, m.sub[(size_t)mem[(size_t)k]]);
    for (const Node& nd : m.sub[(size_t)mem[(size_t)k]].nodes) if (nd.op == GFH_IPARAM && nd.a + 1 > nip) nip = nd.a + 1;
  }
  const std::vector<char> none((size_t)std::max(1, nip), 0);
  const std::string Is = std::to_string(I);
  s << "// integrand of call site " << I << ": " << M << " recorded path(s) through its comparisons\n"
       "static __device__ __forceinline__ int gfh_sf" << Is << "_sel(const double T, const double* __restrict__ Q) {\n";
  bool ok = true;
  std::function<void(int, const std::string&)> walk = [&](int idx, const std::string& ind) {
    const TrieNode& t = T.nodes[(size_t)idx];
    {
      Gen g(m, m.sub[(size_t)mem[(size_t)t.rep]], false); g.in_integrand = true; g.mode = 0; g.ind = ind; g.analyse(none);
      for (int k = t.from; k < t.to; k++) {
        bool wanted = false;
        for (int v : t.members) if (need[(size_t)v][(size_t)k]) { wanted = true; break; }
        if (wanted) g.emit_value_node(k);
      }
      s << g.o.str();
    }
    if (t.kind == 0) { s << ind << "return " << t.leaf << ";\n"; return; }
    if (t.kind != 1) { ok = false; return; }
    const Node& nd = m.sub[(size_t)mem[(size_t)t.rep]].nodes[(size_t)t.guard];
    s << ind << "if (v" << nd.a << (nd.op == GFH_GUARD_GT ? " > " : " < ") << "v" << nd.b << ") {      // AD:315-395: values only\n";
    if (t.child[1] >= 0) walk(t.child[1], ind + "  "); else s << ind << "  return -1;\n";
    s << ind << "} else {\n";
    if (t.child[0] >= 0) walk(t.child[0], ind + "  "); else s << ind << "  return -1;\n";
    s << ind << "}\n";
  };
  walk(root, "  ");
  s << "}\n";
  if (!ok) { *err = "integrand recordings: unexpected fork"; return false; }
  auto cases = [&](const std::string& call_tail, const std::string& on_miss) {
    s << "  switch (gfh_sf" << Is << "_sel(T, Q)) {\n";
    for (int k = 0; k < M; k++) s << "    case " << k << ": " << "gfh_s" << mem[(size_t)k] << call_tail << "\n";
    s << "    default: if (STATUS) GFH_RAISE(STATUS, 2); " << on_miss << "\n  }\n";
  };
  s << "static __device__ double gfh_sf" << Is << "_val(const double T, const double* __restrict__ Q, int* STATUS) {\n";
  s << "  switch (gfh_sf" << Is << "_sel(T, Q)) {\n";
  for (int k = 0; k < M; k++) s << "    case " << k << ": return gfh_s" << mem[(size_t)k] << "_val(T, Q, STATUS);\n";
  s << "    default: if (STATUS) GFH_RAISE(STATUS, 2); return 0.0;\n  }\n}\n";
  s << "static __device__ void gfh_sf" << Is << "_grad(const double T, const double* __restrict__ Q, double& F, double* __restrict__ GQ, int* STATUS) {\n"
       "  for (int j = 0; j < " << n_q(in) << "; j++) GQ[j] = 0.0;      // (a recording writes the entries of the pars(:) it reads)\n";
  cases("_grad(T, Q, F, GQ, STATUS); return;", "F = 0.0; for (int j = 0; j < " + std::to_string(n_q(in)) + "; j++) GQ[j] = 0.0; return;");
  s << "}\n";
  for (int ta = 0; ta < 2; ta++) {
    s << "static __device__ void gfh_sf" << Is << (ta ? "_fwdT" : "_fwd") << "(const double T, const double TD, const double TE, "
         "const double* __restrict__ Q, const double* __restrict__ QD, const double* __restrict__ QE, double& F, double& FD, double& FE, int* STATUS) {\n";
    cases(std::string(ta ? "_fwdT" : "_fwd") + "(T, TD, TE, Q, QD, QE, F, FD, FE, STATUS); return;", "F = 0.0; FD = 0.0; FE = 0.0; return;");
    s << "}\n";
  }
  s << "\n";
  return true;
}

std::vector<int> family_members(const Model& m, int I) {
  std::vector<int> mem{m.integrals[(size_t)I].integrand};
  if ((size_t)I < m.alts.size()) mem.insert(mem.end(), m.alts[(size_t)I].begin(), m.alts[(size_t)I].end());
  return mem;
}

bool site_is_family(const Model& m, int I) {
  if ((size_t)I < m.alts.size() && !m.alts[(size_t)I].empty()) return true;
  for (const Node& nd : m.sub[(size_t)m.integrals[(size_t)I].integrand].nodes) if (is_guard_op(nd.op)) return true;
  return false;
}

// The dispatcher of a branching model under the plain name of a point function: gfh_select, then the body of the variant it names.
void emit_dispatcher(const PointFn& f, int n_variants, std::ostringstream& s) {
  s << "\n" << point_head(f, "", " GFH_SLOT_DECL")
    << "  unsigned long long path; int ng;\n  switch (gfh_select(X, P, STATUS, AXP, LDA, path, ng)) {\n";
  const bool returns = f.ret[0] != 'v';
  for (int v = 0; v < n_variants; v++)
    s << "    case " << v << ": " << (returns ? "return " : "") << "gfh_point_" << f.name << "_v" << v << "(" << f.args << ", AXP, LDA GFH_MESH_PASS);" << (returns ? "" : " break;") << "\n";
  s << "    default:" << f.on_miss << "\n  }\n}\n";
}

bool Model::needs_hint() const {
  if (n_variants() < 2) return false;
  Trie T(*this);
  std::vector<int> all((size_t)n_variants());
  for (int v = 0; v < n_variants(); v++) all[(size_t)v] = v;
  return T.build(all, 0) >= 0 && T.forks;
}

}  // namespace gfh
