// codegen_internal.h -- what the files of the generator (codegen.cpp, emit_ad.cpp, emit_quadrature.cpp, emit_branching.cpp) need
// from one another.  Nothing else includes it: the generator's interface is codegen.h.
#pragma once
#include "codegen.h"
#include <sstream>
#include <string>
#include <vector>

namespace gfh {

// ---- emit_ad.cpp
std::string lit(double c);      // a double as a hex-float literal: exact

struct Gen {
  const Model& m;
  const SubTape& st;
  std::vector<char> is_real, act;   // per node
  std::ostringstream o;
  std::string ind = "  ";
  bool fast_div = true;             // one reciprocal per distinct denominator, products elsewhere
  std::vector<char> inv_done;

  Gen(const Model& mm, const SubTape& s, bool fast) : m(mm), st(s), fast_div(fast), inv_done(s.nodes.size(), 0) {}

  // n<k> = 1/v<k>, emitted at first use (straight-line code: v<k> is already defined)
  std::string inv(int k) {
    if (!inv_done[k]) { o << ind << "const double n" << k << " = 1.0 / " << v(k) << ";\n"; inv_done[k] = 1; }
    return "n" + std::to_string(k);
  }

  std::string v(int k) const { return "v" + std::to_string(k); }
  std::string b(int k) const { return "b" + std::to_string(k); }
  std::string d(int k) const { return "d" + std::to_string(k); }
  std::string dd(int k) const { return "e" + std::to_string(k); }

  // par_active: activity of PARAM nodes (eval tape) or of IPARAM nodes (integrand tapes)
  bool ivar_active = false;
  // the body of an integrand: the data point's abscissa and auxiliary columns (GFH_X / GFH_AUX nodes inside a sub-tape: a real the
  // user's integrand takes from the enclosing eval() without passing it through pars(:), numerical_integration.F90:195-201 evaluates the
  // integrand afresh in that scope) are not among its arguments -- they are read back from the lane's slot of the LDS stash that
  // the point functions fill (GFH_LANE_STASH)
  bool in_integrand = false;
  int mode = 0;   // 0 value, 1 reverse (grad), 2 forward (val,d,dd)
  // Mesh hand-over (emit_integral_site): the body of a point function hands every outermost single-piece integrate() call
  // site its 64-byte record of the lane's mesh; bodies of integrands and the selector pass none.
  bool mesh_top = false;
  int mesh_next = 0;
  std::string mesh_args(const Integral& in) {
    if (!mesh_top || in.depth > 1 || (in.lower_inf && in.upper_inf) || mesh_next >= kMeshSitesMax) return "nullptr, 0";
    return "MESH ? MESH + " + std::to_string(kMeshRecord * mesh_next++) + " : nullptr, MESH_MODE";
  }
  void analyse(const std::vector<char>& par_active);
  std::string powi_expr(const std::string& x, int n, const std::string& tmp);
  int variant(const Node& nd, int k) const;
  void emit_values();
  void emit_forward_all();
  void emit_value_node(int k);
  void emit_integrate_call(int k);
  void emit_reverse();
  void emit_dd_node(int k);
};

// entries of pars(:) an integrate() call binds, as the length of a device array (none: one unused entry)
inline int n_q(const Integral& in) { return in.n_ipars > 0 ? in.n_ipars : 1; }

// ---- emit_quadrature.cpp: everything a model with integrate() needs in front of its point functions -- the rule's tables, the
// workspace macros, and the functions of every call site that a recording reaches, each behind the call sites its integrand calls
bool emit_quadrature(const Model& m, const GenConfig& cfg, std::ostringstream& s, std::string* err);

// ---- emit_branching.cpp
// the sub-tapes call site I integrates: its integrand and the further recordings of it (Model::alts)
std::vector<int> family_members(const Model& m, int I);
// does call site I pick its integrand per evaluation (several recordings, or one that compares AD variables)?
bool site_is_family(const Model& m, int I);
bool emit_family(const Model& m, int I, std::ostringstream& s, std::string* err);       // gfh_sf<I>_sel and the dispatchers gfh_sf<I>_*
bool emit_selector(const Model& m, std::ostringstream& s, std::string* err);            // GFH_UNSEEN_CAP, the report, gfh_select

// One of the four functions of a data point, stated once: codegen.cpp derives the plain form and the _v<k> forms from it,
// emit_branching.cpp the dispatcher of a branching model.
struct PointFn {
  const char* name;       // gfh_point_<name>
  const char* ret;
  const char* comment;    // in front of a body of its own
  const char* params;     // between `P,` and the columns: its own parameters, with the line breaks of its signature
  const char* pad;        // ... and the indentation of the line that holds the columns
  const char* args;       // arguments of a forwarding call up to the columns
  const char* on_miss;    // what the dispatcher does where gfh_select finds no recorded path
  int mode;               // Gen::mode of the body
  bool reverse;           // the body ends with the reverse sweep and writes G
};
extern const PointFn kPointValue, kPointGrad, kPointDd, kPointDdGrad;
// `static __device__ ... gfh_point_<name><sfx>(... <slot>) {`
std::string point_head(const PointFn& f, const std::string& sfx, const std::string& slot);
void emit_dispatcher(const PointFn& f, int n_variants, std::ostringstream& s);

}  // namespace gfh
