// codegen.cpp -- lowers a model tape to HIP source for gfx950.
//
// What the reference does per data point (gadfit.F90:679-690): run the user's eval() with
// operator overloading, which appends every elemental to a run-time tape
// (automatic_differentiation.F90:451-479), then walk that tape backwards in ad_grad
// (AD:1476-1659).  The tape's STRUCTURE is the same for every point, so here it is unrolled
// at code-generation time: forward values and adjoints become named doubles that the
// compiler keeps in VGPRs (one lane = one data point), the op dispatch disappears, and the
// (advar,advar)/(advar,real)/(real,advar) variant of each elemental is chosen statically
// from the operands' static type and activity -- the same choice the reference makes at run
// time from `index /= 0` (AD:454-479 pattern).  Formulas follow the reference line by line
// (cited below) so results agree to rounding.
//
// Three kernels per (model, active set):
//   gfh_k_sweep  STEP 1 (gadfit.F90:675-693): res_i = (y_i-f)*w_i, J[a][i] = df/dp_a * w_i
//   gfh_k_chi2   chi2() (gadfit.F90:1015-1034): all parameters passive, res_i and sum res^2
//   gfh_k_omega  STEP 3 (gadfit.F90:715-731): omega_i = -f''_delta(x_i) * w_i, forward mode
//
// Only what depends on the tape is generated here: the point functions, the quadrature call sites, the selector and the
// #defines in front of them.  The kernels themselves are hand-written HIP that no tape changes; they are plain files under
// device/ (sweep.hip, fused_sweep_gram.hip, chi2.hip, omega.hip, omega_jt.hip, batch_fit.hip, batch_wg_sum.hip, ...), embedded by
// device_text.cpp and streamed into the translation unit by generate_source as they are.  Loading and validating a tape is
// model.cpp.
#include "model.h"
#include "device_text.h"
#include "../../include/gadfit_gk_tables.h"
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <functional>
#include <sstream>

namespace gfh {

namespace {

std::string lit(double c) {
  char b[64];
  if (std::isnan(c)) return "__builtin_nan(\"\")";
  if (std::isinf(c)) return c > 0 ? "__builtin_inf()" : "(-__builtin_inf())";
  snprintf(b, sizeof b, "%a", c);   // hex float: exact
  return b;
}

const char* fn_name(int op) {
  switch (op) {
    case GFH_ABS: return "fabs"; case GFH_EXP: return "gfh_exp"; case GFH_SQRT: return "sqrt";
    case GFH_LOG: return "log"; case GFH_SIN: return "sin"; case GFH_COS: return "cos";
    case GFH_TAN: return "tan"; case GFH_ASIN: return "asin"; case GFH_ACOS: return "acos";
    case GFH_ATAN: return "atan"; case GFH_SINH: return "sinh"; case GFH_COSH: return "cosh";
    case GFH_TANH: return "tanh"; case GFH_ASINH: return "asinh"; case GFH_ACOSH: return "acosh";
    case GFH_ATANH: return "atanh"; case GFH_ERF: return "erf";
  }
  return "?";
}

// 2/sqrt(pi) as the reference forms it: 2.0_kp/sqrtpi (AD:1633, gadf_constants.F90:29-33)
const char* TWO_OVER_SQRTPI = "(2.0/0x1.c5bf891b4ef6bp+0)";

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
  void analyse(const std::vector<char>& par_active) {
    int n = (int)st.nodes.size();
    is_real.assign(n, 0); act.assign(n, 0);
    for (int k = 0; k < n; k++) {
      const Node& nd = st.nodes[k];
      is_real[k] = (nd.flags & GFH_F_REAL) ? 1 : 0;
      switch (nd.op) {
        case GFH_PARAM: case GFH_IPARAM: act[k] = nd.a < (int)par_active.size() ? par_active[nd.a] : 0; break;
        case GFH_IVAR: act[k] = ivar_active; break;
        case GFH_INTEGRATE: {
          const Integral& in = m.integrals[nd.a];
          char a = 0;
          for (int j = 0; j < in.n_ipars; j++) a |= act[m.ipar_nodes[in.ipar_off + j]];
          if (!in.lower_inf) a |= act[in.lower];
          if (!in.upper_inf) a |= act[in.upper];
          act[k] = a;
          break;
        }
        case GFH_CONST: case GFH_X: case GFH_AUX: act[k] = 0; break;
        case GFH_GUARD_GT: case GFH_GUARD_LT: act[k] = 0; break;      // a comparison of values (AD:315-395): no value, no derivative
        case GFH_LIFT: act[k] = 0; break;
        case GFH_VAL: act[k] = 0; is_real[k] = 1; break;      // the %val of an advar: a plain real whatever the flags of a third-party tape say (no derivative flows through it)
        case GFH_ADD: case GFH_SUB: case GFH_MUL: case GFH_DIV: case GFH_POW:
          act[k] = (act[nd.a] || act[nd.b]) && !is_real[k]; break;
        default: act[k] = act[nd.a] && !is_real[k]; break;
      }
    }
  }

  // integer power by repeated squaring, same multiplication order as oracle powi()
  std::string powi_expr(const std::string& x, int n, const std::string& tmp) {
    if (n == 0) return "1.0";
    unsigned mag = n < 0 ? (unsigned)(-(long)n) : (unsigned)n;
    std::string r; std::string base = x; int lvl = 0;
    // emit temporaries for the squarings
    while (mag) {
      if (mag & 1u) r = r.empty() ? base : "(" + r + "*" + base + ")";
      mag >>= 1;
      if (mag) {
        std::string nb = tmp + "_s" + std::to_string(lvl++);
        o << ind << "const double " << nb << " = " << base << "*" << base << ";\n";
        base = nb;
      }
    }
    return n < 0 ? "(1.0/" + r + ")" : r;
  }

  // ---------------------------------------------------------------- forward values
  // variant of a binary op: 0 plain(real or both passive advar), 1 aa, 2 ar, 3 ra
  int variant(const Node& nd, int k) const {
    if (is_real[k]) return 0;
    bool ra_ = is_real[nd.a], rb_ = is_real[nd.b];
    if (!ra_ && !rb_) {
      if (act[nd.a] && act[nd.b]) return 1;
      if (act[nd.a]) return 2;
      if (act[nd.b]) return 3;
      return 0;
    }
    return ra_ ? 3 : 2;   // static overload (advar,real) / (real,advar), also when passive
  }

  void emit_values(bool) {
    int n = (int)st.nodes.size();
    for (int k = 0; k < n; k++) emit_value_node(k);
  }

  // forward mode: value and (d, dd) of each node together, in tape order (an integrate()
  // call needs the tangents of its bindings when it is evaluated)
  void emit_forward_all() {
    int n = (int)st.nodes.size();
    for (int k = 0; k < n; k++) { emit_value_node(k); if (act[k]) emit_dd_node(k); }
  }

  void emit_value_node(int k) {
    {
      const Node& nd = st.nodes[k];
      std::string lhs = ind + "const double " + v(k) + " = ";
      switch (nd.op) {
        case GFH_CONST: o << lhs << lit(nd.c) << ";\n"; break;
        case GFH_GUARD_GT: case GFH_GUARD_LT: break;                   // decided by gfh_select before this body runs
        case GFH_X: o << lhs << (in_integrand ? "gfh_lane_x[threadIdx.x];\n" : "X;\n"); break;
        case GFH_AUX:
          if (in_integrand) o << lhs << "gfh_lane_axp[threadIdx.x][(i64)" << nd.a << " * gfh_lane_lda];\n";
          else o << lhs << "AXP[(i64)" << nd.a << " * LDA];\n";
          break;
        case GFH_PARAM: o << lhs << "P[" << nd.a << "];\n"; break;
        case GFH_IVAR: o << lhs << "T;\n"; break;
        case GFH_IPARAM: o << lhs << "Q[" << nd.a << "];\n"; break;
        case GFH_INTEGRATE: emit_integrate_call(k); break;
        case GFH_LIFT: case GFH_VAL: o << lhs << v(nd.a) << ";\n"; break;
        case GFH_NEG: o << lhs << "-" << v(nd.a) << ";\n"; break;
        case GFH_ADD: o << lhs << v(nd.a) << " + " << v(nd.b) << ";\n"; break;
        case GFH_SUB: o << lhs << v(nd.a) << " - " << v(nd.b) << ";\n"; break;
        case GFH_MUL: o << lhs << v(nd.a) << " * " << v(nd.b) << ";\n"; break;
        case GFH_DIV: {
          int var = variant(nd, k);
          if (fast_div && !is_real[k]) {
            // reciprocal reuse: every division by v<b> (here and in the derivative code)
            // shares one 1/v<b>; differs from the reference's r/a = r/v (AD:892-913) by <= 1 ulp
            std::string nb = inv(nd.b);
            o << lhs << v(nd.a) << " * " << nb << ";\n";
          } else if (var == 1 || var == 2) {   // AD:814-841, 843-866: multiply by the reciprocal
            o << ind << "const double i" << k << " = 1.0 / " << v(nd.b) << ";\n";
            o << lhs << v(nd.a) << " * i" << k << ";\n";
          } else o << lhs << v(nd.a) << " / " << v(nd.b) << ";\n";   // AD:892-913, 839
          break;
        }
        case GFH_POW:
          if (fast_div && !is_real[k]) {
            // x**y together with ln x (the derivative code wants it: AD:975-980, 1534-1553): one extended-precision logarithm serves both
            o << ind << "double l" << k << ";\n";
            o << lhs << "gfh_pow_ln(" << v(nd.a) << ", " << v(nd.b) << ", l" << k << ");\n";
          } else o << lhs << "pow(" << v(nd.a) << ", " << v(nd.b) << ");\n";
          break;
        case GFH_POWI: { std::string e = powi_expr(v(nd.a), nd.b, "q" + std::to_string(k)); o << lhs << e << ";\n"; break; }
        default: o << lhs << fn_name(nd.op) << "(" << v(nd.a) << ");\n"; break;
      }
    }
  }

  // integrate(f, pars, lower, upper) call site (NI:193-630): the adaptive rule lives in the
  // generated gfh_int<I>_* functions; here the bindings are gathered and, in reverse mode,
  // the partials w.r.t. pars(:) and f at the bounds are kept for the return sweep.
  void emit_integrate_call(int k) {
    const Node& nd = st.nodes[k];
    const Integral& in = m.integrals[nd.a];
    const std::string I = std::to_string(nd.a), ks = std::to_string(k);
    o << ind << "double q" << ks << "[" << (in.n_ipars > 0 ? in.n_ipars : 1) << "];\n";
    for (int j = 0; j < in.n_ipars; j++) o << ind << "q" << ks << "[" << j << "] = " << v(m.ipar_nodes[in.ipar_off + j]) << ";\n";
    const std::string lo = in.lower_inf ? "0.0" : v(in.lower), hi = in.upper_inf ? "0.0" : v(in.upper);
    if (mode == 1 && act[k]) {
      o << ind << "double " << v(k) << ", g" << ks << "[" << (in.n_ipars > 0 ? in.n_ipars : 1) << "], fl" << ks << ", fh" << ks << ";\n";
      o << ind << "gfh_int" << I << "_grad<" << ((!in.lower_inf && act[in.lower]) ? "true" : "false") << ", " << ((!in.upper_inf && act[in.upper]) ? "true" : "false") << ">(" << lo << ", " << hi << ", q" << ks << ", " << v(k) << ", g" << ks << ", fl" << ks << ", fh" << ks << ", STATUS, " << mesh_args(in) << ");\n";
    } else if (mode == 2 && act[k]) {
      // forward mode (NI:425-437, 480-487, 527-534): tangents of pars(:) and of the bounds go in
      const int NQ = in.n_ipars > 0 ? in.n_ipars : 1;
      o << ind << "double qd" << ks << "[" << NQ << "], qe" << ks << "[" << NQ << "];\n";
      for (int j = 0; j < in.n_ipars; j++) {
        int bn = m.ipar_nodes[in.ipar_off + j];
        o << ind << "qd" << ks << "[" << j << "] = " << (act[bn] ? d(bn) : "0.0") << "; qe" << ks << "[" << j << "] = " << (act[bn] ? dd(bn) : "0.0") << ";\n";
      }
      const bool la = !in.lower_inf && act[in.lower], ua = !in.upper_inf && act[in.upper];
      o << ind << "double " << v(k) << ", " << d(k) << ", " << dd(k) << ";\n";
      o << ind << "gfh_int" << I << "_fwd<" << (la ? "true" : "false") << ", " << (ua ? "true" : "false") << ">(" << lo << ", "
        << (la ? d(in.lower) : "0.0") << ", " << (la ? dd(in.lower) : "0.0") << ", " << hi << ", " << (ua ? d(in.upper) : "0.0") << ", "
        << (ua ? dd(in.upper) : "0.0") << ", q" << ks << ", qd" << ks << ", qe" << ks << ", " << v(k) << ", " << d(k) << ", " << dd(k) << ", STATUS, " << mesh_args(in) << ");\n";
    } else {
      o << ind << "const double " << v(k) << " = gfh_int" << I << "_val(" << lo << ", " << hi << ", q" << ks << ", STATUS, " << mesh_args(in) << ");\n";
    }
  }

  // ---------------------------------------------------------------- reverse sweep, AD:1476-1659
  void emit_reverse() {
    int n = (int)st.nodes.size();
    for (int k = 0; k < n; k++) if (act[k]) o << ind << "double " << b(k) << " = 0.0;\n";
    if (!act[st.result]) return;
    o << ind << b(st.result) << " = 1.0;\n";                                   // AD:1490
    // The reference zeroes the adjoints and accumulates (AD:1482-1490).  The code is straight-line, so which contribution
    // to an adjoint is the first one is known here: it is assigned instead of added to 0.0 -- the same value (0.0 + t = t
    // for every t except t = -0.0, which it turns into +0.0: a Jacobian entry that is a zero keeps the sign of its last
    // factor), one FP64 add less per adjoint, which the compiler may not drop by itself under IEEE rules.
    std::vector<char> touched((size_t)n, 0);
    touched[(size_t)st.result] = 1;
    auto acc = [&](int tgt, const std::string& sign, const std::string& expr) {
      if (!touched[(size_t)tgt]) {
        touched[(size_t)tgt] = 1;
        o << ind << b(tgt) << " = " << (sign == "-" ? "-(" + expr + ")" : expr) << ";\n";
        return;
      }
      o << ind << b(tgt) << " = " << b(tgt) << " " << sign << " " << expr << ";\n";
    };
    for (int k = n - 1; k >= 0; k--) {
      if (!act[k]) continue;
      const Node& nd = st.nodes[k];
      const std::string bk = b(k);
      switch (nd.op) {
        case GFH_PARAM: case GFH_IPARAM: case GFH_IVAR: break;
        case GFH_INTEGRATE: {
          const Integral& in = m.integrals[nd.a];
          const std::string ks = std::to_string(k);
          for (int j = 0; j < in.n_ipars; j++) {
            int bn = m.ipar_nodes[in.ipar_off + j];
            if (act[bn]) acc(bn, "+", bk + "*g" + ks + "[" + std::to_string(j) + "]");
          }
          if (!in.upper_inf && act[in.upper]) acc(in.upper, "+", bk + "*fh" + ks);   // AD:1650-1653, 1638-1639
          if (!in.lower_inf && act[in.lower]) acc(in.lower, "-", bk + "*fl" + ks);   // AD:1645-1648, 1641-1642
          break;
        }
        case GFH_ADD: {
          int var = variant(nd, k);
          if (var == 1) { acc(nd.a, "+", bk); acc(nd.b, "+", bk); }          // AD:1496-1499
          else acc(var == 2 ? nd.a : nd.b, "+", bk);                            // AD:1500-1502
          break;
        }
        case GFH_SUB: {
          int var = variant(nd, k);
          if (var == 1) { acc(nd.a, "+", bk); acc(nd.b, "-", bk); }          // AD:1503-1506
          else if (var == 2) acc(nd.a, "+", bk);                               // AD:1500-1502
          else acc(nd.b, "-", bk);                                             // AD:1507-1509
          break;
        }
        case GFH_MUL: {
          int var = variant(nd, k);
          if (var == 1) { acc(nd.a, "+", bk + "*" + v(nd.b)); acc(nd.b, "+", bk + "*" + v(nd.a)); }  // AD:1510-1515
          else if (var == 2) acc(nd.a, "+", bk + "*" + v(nd.b));               // AD:1516-1520
          else acc(nd.b, "+", bk + "*" + v(nd.a));
          break;
        }
        case GFH_DIV: {
          int var = variant(nd, k);
          if (fast_div) {
            std::string nb = inv(nd.b);
            if (var == 1 || var == 2) acc(nd.a, "+", bk + "*" + nb);            // AD:1521-1523, 1516-1520
            if (var == 1 || var == 3) acc(nd.b, "-", bk + "*" + v(k) + "*" + nb); // AD:1524-1533 (c/v/v = y/v)
          } else if (var == 1) {                                                // AD:1521-1527
            acc(nd.a, "+", bk + "/" + v(nd.b));
            acc(nd.b, "-", bk + "*" + v(k) + "/" + v(nd.b));
          } else if (var == 2) acc(nd.a, "+", bk + "*i" + std::to_string(k));   // AD:1516-1520, const = inv
          else acc(nd.b, "-", bk + "*" + v(nd.a) + "/" + v(nd.b) + "/" + v(nd.b));  // AD:1528-1533
          break;
        }
        case GFH_POW: {
          int var = variant(nd, k);
          // (shared reciprocals: x**(y-1) = x**y / x, and ln x came with the value -- one pow and one log less per node than
          // the reference's expressions, <= 2 ulp from them)
          const std::string pm1 = fast_div ? "(" + v(k) + "*" + (var == 3 ? std::string() : inv(nd.a)) + ")" : "pow(" + v(nd.a) + ", " + v(nd.b) + " - 1.0)";
          const std::string lg = fast_div ? "l" + std::to_string(k) : "log(" + v(nd.a) + ")";
          if (var == 1) {                                                       // AD:1534-1541
            acc(nd.a, "+", bk + "*" + v(nd.b) + "*" + pm1);
            acc(nd.b, "+", bk + "*" + lg + "*" + v(k));                       // x1**x2 recomputed = y
          } else if (var == 2)                                                  // AD:1542-1547
            acc(nd.a, "+", bk + "*" + v(nd.b) + "*" + pm1);
          else                                                                  // AD:1548-1553
            acc(nd.b, "+", bk + "*" + lg + "*" + v(k));
          break;
        }
        case GFH_POWI: {                                                        // AD:1554-1558
          std::string e = powi_expr(v(nd.a), nd.b - 1, "r" + std::to_string(k));
          acc(nd.a, "+", bk + "*" + lit((double)nd.b) + "*" + e);
          break;
        }
        case GFH_ABS:                                                           // AD:1559-1567
          touched[(size_t)nd.a] = 1;
          o << ind << b(nd.a) << " = (" << v(nd.a) << " < 0.0) ? " << b(nd.a) << " - " << bk << " : " << b(nd.a) << " + " << bk << ";\n";
          break;
        case GFH_EXP: acc(nd.a, "+", bk + "*" + v(k)); break;                  // AD:1568-1571
        case GFH_SQRT: if (fast_div) { std::string nk = inv(k); acc(nd.a, "+", bk + "*0.5*" + nk); }
                       else acc(nd.a, "+", bk + "/2.0/" + v(k));
                       break;                                                   // AD:1572-1575
        case GFH_LOG: if (fast_div) { std::string na_ = inv(nd.a); acc(nd.a, "+", bk + "*" + na_); }
                      else acc(nd.a, "+", bk + "/" + v(nd.a));
                      break;                                                    // AD:1576-1579
        case GFH_SIN: acc(nd.a, "+", bk + "*cos(" + v(nd.a) + ")"); break;     // AD:1581-1584
        case GFH_COS: acc(nd.a, "-", bk + "*sin(" + v(nd.a) + ")"); break;     // AD:1585-1588
        case GFH_TAN: o << ind << "const double rc" << k << " = cos(" << v(nd.a) << ");\n";
                      acc(nd.a, "+", bk + "/(rc" + std::to_string(k) + "*rc" + std::to_string(k) + ")"); break;   // AD:1589-1592
        case GFH_ASIN: acc(nd.a, "+", bk + "/sqrt(1.0 - " + v(nd.a) + "*" + v(nd.a) + ")"); break;  // AD:1593-1596
        case GFH_ACOS: acc(nd.a, "-", bk + "/sqrt(1.0 - " + v(nd.a) + "*" + v(nd.a) + ")"); break;  // AD:1597-1600
        case GFH_ATAN: acc(nd.a, "+", bk + "/(1.0 + " + v(nd.a) + "*" + v(nd.a) + ")"); break;      // AD:1601-1604
        case GFH_SINH: acc(nd.a, "+", bk + "*cosh(" + v(nd.a) + ")"); break;   // AD:1606-1609
        case GFH_COSH: acc(nd.a, "+", bk + "*sinh(" + v(nd.a) + ")"); break;   // AD:1610-1613
        case GFH_TANH: o << ind << "const double rc" << k << " = cosh(" << v(nd.a) << ");\n";
                       acc(nd.a, "+", bk + "/(rc" + std::to_string(k) + "*rc" + std::to_string(k) + ")"); break;  // AD:1614-1617
        case GFH_ASINH: acc(nd.a, "+", bk + "/sqrt(" + v(nd.a) + "*" + v(nd.a) + " + 1.0)"); break; // AD:1618-1621
        case GFH_ACOSH: acc(nd.a, "+", bk + "/sqrt(" + v(nd.a) + "*" + v(nd.a) + " - 1.0)"); break; // AD:1622-1625
        case GFH_ATANH: acc(nd.a, "+", bk + "/(1.0 - " + v(nd.a) + "*" + v(nd.a) + ")"); break;     // AD:1626-1629
        case GFH_ERF: acc(nd.a, "+", bk + "*" + TWO_OVER_SQRTPI + "*gfh_exp(-(" + v(nd.a) + "*" + v(nd.a) + "))"); break; // AD:1631-1635
        default: break;
      }
    }
  }

  // ---------------------------------------------------------------- forward mode (val,d,dd)
  // Active nodes carry d<k> and e<k> (= dd).  Formulas: the `else` branches of AD:454-1459.
  void emit_dd_node(int k) {
    {
      const Node& nd = st.nodes[k];
      auto D = [&](const std::string& e) { o << ind << "const double " << d(k) << " = " << e << ";\n"; };
      auto E = [&](const std::string& e) { o << ind << "const double " << dd(k) << " = " << e << ";\n"; };
      const bool leaf = nd.op == GFH_PARAM || nd.op == GFH_IPARAM || nd.op == GFH_IVAR || nd.op == GFH_INTEGRATE;
      const std::string va = nd.a >= 0 && !leaf ? v(nd.a) : "", y = v(k);
      const std::string da = nd.a >= 0 && !leaf ? d(nd.a) : "", ea = nd.a >= 0 && !leaf ? dd(nd.a) : "";
      std::string ks = std::to_string(k);
      switch (nd.op) {
        case GFH_PARAM: D("DP[" + std::to_string(nd.a) + "]"); E("0.0"); break;   // gadfit.F90:719: %d = delta1, dd = 0
        case GFH_IPARAM: D("QD[" + std::to_string(nd.a) + "]"); E("QE[" + std::to_string(nd.a) + "]"); break;
        case GFH_IVAR: D("TD"); E("TE"); break;
        case GFH_INTEGRATE: break;   // d/dd were produced together with the value (emit_integrate_call)
        case GFH_ADD: {
          int var = variant(nd, k);
          if (var == 1) { D(d(nd.a) + " + " + d(nd.b)); E(dd(nd.a) + " + " + dd(nd.b)); }   // AD:468-469
          else { int s = var == 2 ? nd.a : nd.b; D(d(s)); E(dd(s)); }                           // AD:495-496, 540-541
          break;
        }
        case GFH_SUB: {
          int var = variant(nd, k);
          if (var == 1) { D(d(nd.a) + " - " + d(nd.b)); E(dd(nd.a) + " - " + dd(nd.b)); }   // AD:585-586
          else if (var == 2) { D(d(nd.a)); E(dd(nd.a)); }                                     // AD:616-617
          else { D("-" + d(nd.b)); E("-" + dd(nd.b)); }                                       // AD:661-662
          break;
        }
        case GFH_MUL: {
          int var = variant(nd, k);
          std::string x1 = v(nd.a), x2 = v(nd.b);
          if (var == 1) {                                                                       // AD:707-708
            D(x1 + "*" + d(nd.b) + " + " + d(nd.a) + "*" + x2);
            E(x1 + "*" + dd(nd.b) + " + 2.0*" + d(nd.a) + "*" + d(nd.b) + " + " + dd(nd.a) + "*" + x2);
          } else if (var == 2) { D(d(nd.a) + "*" + x2); E(dd(nd.a) + "*" + x2); }             // AD:736-737
          else { D(x1 + "*" + d(nd.b)); E(x1 + "*" + dd(nd.b)); }                              // AD:783-784
          break;
        }
        case GFH_DIV: {
          int var = variant(nd, k);
          if (fast_div) {
            std::string nb = inv(nd.b);
            if (var == 1) {
              D("(" + d(nd.a) + " - " + y + "*" + d(nd.b) + ")*" + nb);
              E("(" + dd(nd.a) + " - " + y + "*" + dd(nd.b) + " - 2.0*" + d(k) + "*" + d(nd.b) + ")*" + nb);
            } else if (var == 2) { D(d(nd.a) + "*" + nb); E(dd(nd.a) + "*" + nb); }
            else {
              D("-" + y + "*" + d(nd.b) + "*" + nb);
              E("(-" + y + "*" + dd(nd.b) + " - 2.0*" + d(k) + "*" + d(nd.b) + ")*" + nb);
            }
          } else if (var == 1) {                                                                // AD:830-831
            D("(" + d(nd.a) + " - " + y + "*" + d(nd.b) + ")*i" + ks);
            E("(" + dd(nd.a) + " - " + y + "*" + dd(nd.b) + " - 2.0*" + d(k) + "*" + d(nd.b) + ")*i" + ks);
          } else if (var == 2) { D(d(nd.a) + "*i" + ks); E(dd(nd.a) + "*i" + ks); }            // AD:861-862
          else {                                                                                // AD:907-908
            D("-" + y + "*" + d(nd.b) + "/" + v(nd.b));
            E("(-" + y + "*" + dd(nd.b) + " - 2.0*" + d(k) + "*" + d(nd.b) + ")/" + v(nd.b));
          }
          break;
        }
        case GFH_POW: {
          int var = variant(nd, k);
          std::string x1 = v(nd.a), x2 = v(nd.b);
          if (var == 1) {                                                                       // AD:975-980
            if (!fast_div) {
              o << ind << "const double l" << ks << " = log(" << x1 << ");\n";
              D(y + "*" + d(nd.b) + "*l" + ks + " + " + d(nd.a) + "*" + x2 + "*pow(" + x1 + ", " + x2 + " - 1.0)");
            } else D(y + "*" + d(nd.b) + "*l" + ks + " + " + d(nd.a) + "*" + x2 + "*(" + y + "*" + inv(nd.a) + ")");
            o << ind << "const double i" << ks << " = 1.0 / " << x1 << ";\n";
            E(d(k) + "*" + d(k) + "/" + y + " + " + y + "*(" + dd(nd.b) + "*l" + ks + " + (2.0*" + d(nd.b) + "*" + d(nd.a) +
              " + " + x2 + "*(" + dd(nd.a) + " - " + d(nd.a) + "*" + d(nd.a) + "*i" + ks + "))*i" + ks + ")");
          } else if (var == 2) {                                                                // AD:1005-1008
            if (!fast_div) D(d(nd.a) + "*" + x2 + "*pow(" + x1 + ", " + x2 + " - 1.0)");
            else D(d(nd.a) + "*" + x2 + "*(" + y + "*" + inv(nd.a) + ")");
            o << ind << "const double i" << ks << " = 1.0 / " << x1 << ";\n";
            E(d(k) + "*" + d(k) + "/" + y + " + " + y + "*" + x2 + "*(" + dd(nd.a) + " - " + d(nd.a) + "*" + d(nd.a) + "*i" + ks + ")*i" + ks);
          } else {                                                                              // AD:1076-1079
            if (!fast_div) o << ind << "const double l" << ks << " = log(" << x1 << ");\n";
            D(y + "*" + d(nd.b) + "*l" + ks);
            E(d(k) + "*" + d(k) + "/" + y + " + " + y + "*" + dd(nd.b) + "*l" + ks);
          }
          break;
        }
        case GFH_POWI: {                                                                        // AD:1051-1054
          std::string nn = lit((double)nd.b);
          if (fast_div && nd.b >= 1) {
            // x**n, n >= 1, without the reference's two divisions (d = y n dx / x, dd = d d / y + y n (ddx - dx dx / x) / x):
            // d = n x^(n-1) dx, dd = n ((n-1) x^(n-2) dx dx + x^(n-1) ddx) -- the same polynomial identities, finite at x = 0
            // where the reference's forward mode returns 0/0 (its reverse mode, AD:1554-1558, has the product form as well)
            if (nd.b == 1) { D(da); E(ea); break; }
            const std::string p1 = powi_expr(va, nd.b - 1, "f" + ks);
            D(nn + "*" + p1 + "*" + da);
            if (nd.b == 2) E(nn + "*(" + da + "*" + da + " + " + va + "*" + ea + ")");
            else {
              const std::string p2 = powi_expr(va, nd.b - 2, "g" + ks);
              E(nn + "*(" + lit((double)(nd.b - 1)) + "*" + p2 + "*" + da + "*" + da + " + " + p1 + "*" + ea + ")");
            }
            break;
          }
          o << ind << "const double i" << ks << " = 1.0 / " << va << ";\n";
          D(y + "*" + nn + "*" + da + "*i" + ks);
          E(d(k) + "*" + d(k) + "/" + y + " + " + y + "*" + nn + "*(" + ea + " - " + da + "*" + da + "*i" + ks + ")*i" + ks);
          break;
        }
        case GFH_ABS:                                                                           // AD:951-953
          o << ind << "const double s" << ks << " = copysign(1.0, " << va << ");\n";
          D(da + "*s" + ks); E(ea + "*s" + ks); break;
        case GFH_EXP: D(da + "*" + y); E(ea + "*" + y + " + " + da + "*" + d(k)); break;      // AD:1123-1124
        case GFH_SQRT:                                                                          // AD:1144-1146
          o << ind << "const double i" << ks << " = 1.0 / " << y << ";\n";
          D(da + "/2.0*i" + ks); E("(" + ea + "*i" + ks + " - " + d(k) + "*" + da + "/" + va + ")/2.0"); break;
        case GFH_LOG:                                                                           // AD:1166-1168
          o << ind << "const double i" << ks << " = 1.0 / " << va << ";\n";
          D(da + "*i" + ks); E("(" + ea + " - " + da + "*" + d(k) + ")*i" + ks); break;
        case GFH_SIN:                                                                           // AD:1188-1190
          o << ind << "const double c" << ks << " = cos(" << va << ");\n";
          D(da + "*c" + ks); E(ea + "*c" + ks + " - " + da + "*" + da + "*" + y); break;
        case GFH_COS:                                                                           // AD:1210-1212
          o << ind << "const double c" << ks << " = -sin(" << va << ");\n";
          D(da + "*c" + ks); E(ea + "*c" + ks + " - " + da + "*" + da + "*" + y); break;
        case GFH_TAN:                                                                           // AD:1232-1235
          o << ind << "const double t" << ks << " = 1.0 / cos(" << va << ");\n";
          o << ind << "const double c" << ks << " = t" << ks << "*t" << ks << ";\n";
          D(da + "*c" + ks); E(ea + "*c" + ks + " + 2.0*" + da + "*" + y + "*" + d(k)); break;
        case GFH_ASIN:                                                                          // AD:1255-1257
          o << ind << "const double t" << ks << " = 1.0 / sqrt(1.0 - " << va << "*" << va << ");\n";
          D(da + "*t" + ks); E("t" + ks + "*(" + ea + " + " + va + "*" + d(k) + "*" + d(k) + ")"); break;
        case GFH_ACOS:                                                                          // AD:1277-1279
          o << ind << "const double t" << ks << " = -1.0 / sqrt(1.0 - " << va << "*" << va << ");\n";
          D(da + "*t" + ks); E("t" + ks + "*(" + ea + " + " + va + "*" + d(k) + "*" + d(k) + ")"); break;
        case GFH_ATAN:                                                                          // AD:1299-1301
          o << ind << "const double t" << ks << " = 1.0 / (1.0 + " << va << "*" << va << ");\n";
          D(da + "*t" + ks); E(ea + "*t" + ks + " - 2.0*" + va + "*" + d(k) + "*" + d(k)); break;
        case GFH_SINH:                                                                          // AD:1321-1323
          o << ind << "const double c" << ks << " = cosh(" << va << ");\n";
          D(da + "*c" + ks); E(ea + "*c" + ks + " + " + y + "*" + da + "*" + da); break;
        case GFH_COSH:                                                                          // AD:1343-1345
          o << ind << "const double c" << ks << " = sinh(" << va << ");\n";
          D(da + "*c" + ks); E(ea + "*c" + ks + " + " + y + "*" + da + "*" + da); break;
        case GFH_TANH:                                                                          // AD:1365-1367
          o << ind << "const double h" << ks << " = cosh(" << va << ");\n";
          o << ind << "const double t" << ks << " = 1.0 / (h" << ks << "*h" << ks << ");\n";
          D(da + "*t" + ks); E(ea + "*t" + ks + " - 2.0*" + y + "*" + da + "*" + d(k)); break;
        case GFH_ASINH:                                                                         // AD:1387-1389
          o << ind << "const double t" << ks << " = 1.0 / sqrt(1.0 + " << va << "*" << va << ");\n";
          D(da + "*t" + ks); E("t" + ks + "*(" + ea + " - " + va + "*" + d(k) + "*" + d(k) + ")"); break;
        case GFH_ACOSH:                                                                         // AD:1409-1411
          o << ind << "const double t" << ks << " = 1.0 / sqrt(" << va << "*" << va << " - 1.0);\n";
          D(da + "*t" + ks); E("t" + ks + "*(" + ea + " - " + va + "*" + d(k) + "*" + d(k) + ")"); break;
        case GFH_ATANH:                                                                         // AD:1431-1433
          o << ind << "const double t" << ks << " = 1.0 / (1.0 - " << va << "*" << va << ");\n";
          D(da + "*t" + ks); E("(" + ea + " + 2.0*" + va + "*" + da + "*" + d(k) + ")*t" + ks); break;
        case GFH_ERF:                                                                           // AD:1453-1455
          o << ind << "const double t" << ks << " = " << TWO_OVER_SQRTPI << "*gfh_exp(-(" << va << "*" << va << "));\n";
          D(da + "*t" + ks); E("(" + ea + " - 2.0*" + da + "*" + da + "*" + va + ")*t" + ks); break;
        default: break;
      }
    }
  }
};


// ---------------------------------------------------------------------------------------
// integrate(): adaptive Gauss-Kronrod through AD on the device (numerical_integration.F90).
// Per integrand sub-tape S:   gfh_s<S>_val(T, Q)          value, everything passive (NI:238-239)
//                             gfh_s<S>_grad(T, Q, F, GQ)   value + d/dpars(:) by the unrolled reverse sweep
// Per call site I:            gfh_int<I>_val / _grad       interval bisection on values (NI:251-267), then
//                             the final pass over the intervals in storage order (NI:268-275)
// The per-lane interval workspace lives in scratch: GFH_WS1 intervals for outer, GFH_WS2 for inner integrals.  The reference's
// workspaces are user-sized, default 1000 (NI:40, 114-135); typical use is << 100, so the kernels are first compiled with
// min(100, the user's size) and a pass that exhausts that (STATUS = 1) is repeated by the host with kernels compiled at the
// user's size before the reference's error is raised (NI:282-283; passes.cpp, grow_workspace).
void emit_integrand_functions(const Model& m, int S, const GenConfig& cfg, std::ostringstream& s) {
  const SubTape& st = m.sub[S];
  int nip = 0;
  for (const Node& nd : st.nodes) if (nd.op == GFH_IPARAM && nd.a + 1 > nip) nip = nd.a + 1;
  std::vector<char> none(nip > 0 ? nip : 1, 0), all(nip > 0 ? nip : 1, 1);
  s << "static __device__ double gfh_s" << S << "_val(const double T, const double* __restrict__ Q, int* STATUS) {\n";
  { Gen g(m, st, cfg.fast_div); g.in_integrand = true; g.mode = 0; g.analyse(none); g.emit_values(false); s << g.o.str() << "  return " << g.v(st.result) << ";\n}\n\n"; }
  s << "static __device__ void gfh_s" << S << "_grad(const double T, const double* __restrict__ Q, double& F, double* __restrict__ GQ, int* STATUS) {\n";
  {
    Gen g(m, st, cfg.fast_div); g.in_integrand = true; g.mode = 1; g.analyse(all); g.emit_values(false); g.emit_reverse();
    s << g.o.str() << "  F = " << g.v(st.result) << ";\n";
    for (int j = 0; j < nip; j++) {
      std::string e;
      for (int k = 0; k < (int)st.nodes.size(); k++)
        if (st.nodes[k].op == GFH_IPARAM && st.nodes[k].a == j && g.act[k]) e += (e.empty() ? "" : " + ") + g.b(k);
      s << "  GQ[" << j << "] = " << (e.empty() ? "0.0" : e) << ";\n";
    }
    s << "}\n\n";
  }
  // forward mode: (val, d, dd) with tangents QD/QE of pars(:); TA = the integration variable
  // itself carries (TD, TE) -- only needed for f(bound) with an active bound (NI:431, 435)
  for (int ta = 0; ta < 2; ta++) {
    s << "static __device__ void gfh_s" << S << (ta ? "_fwdT" : "_fwd") << "(const double T, const double TD, const double TE, "
         "const double* __restrict__ Q, const double* __restrict__ QD, const double* __restrict__ QE, double& F, double& FD, double& FE, int* STATUS) {\n";
    Gen g(m, st, cfg.fast_div); g.in_integrand = true; g.mode = 2; g.ivar_active = ta != 0; g.analyse(all); g.emit_forward_all();
    s << g.o.str() << "  F = " << g.v(st.result) << ";\n";
    if (g.act[st.result]) s << "  FD = " << g.d(st.result) << "; FE = " << g.dd(st.result) << ";\n";
    else s << "  FD = 0.0; FE = 0.0;\n";
    s << "}\n\n";
  }
}

void emit_integral_site(const Model& m, int I, const GenConfig& cfg, std::ostringstream& s) {
  const Integral& in = m.integrals[I];
  const int S = in.integrand, NQ = in.n_ipars > 0 ? in.n_ipars : 1;
  const double rel = in.rel_error >= 0 ? in.rel_error : (in.depth <= 1 ? m.rel_error_outer : m.rel_error_inner);
  const double abst = in.abs_error >= 0 ? in.abs_error : 0.0;
  // (an integrand that compares AD variables: the dispatchers gfh_sf<I>_* of emit_family stand in for gfh_s<S>_*)
  bool fam = (size_t)I < m.alts.size() && !m.alts[(size_t)I].empty();
  for (const Node& nd : m.sub[(size_t)S].nodes) if (is_guard_op(nd.op)) fam = true;
  const std::string Is = std::to_string(I), Ss = fam ? "f" + std::to_string(I) : std::to_string(S);
  const std::string WS = in.depth <= 1 ? "GFH_WS1" : "GFH_WS2";      // outer / inner workspace (NI:220-226)
  // integrand with the (a,inf) / (-inf,b) maps applied (NI:314-318, 347-351): TK 0 none, 1: f(tb-1+1/t)/t**2, 2: f(tb+1-1/t)/t**2
  s << "template <int TK> static __device__ __forceinline__ double gfh_i" << Is << "_f(const double t, const double tb, const double* __restrict__ Q, int* STATUS) {\n"
       "  if (TK == 0) return gfh_s" << Ss << "_val(t, Q, STATUS);\n"
       "  const double arg = TK == 1 ? (tb - 1.0) + 1.0 / t : (tb + 1.0) - 1.0 / t;\n"
       "  return gfh_s" << Ss << "_val(arg, Q, STATUS) * (1.0 / (t * t));\n}\n";
  s << "template <int TK> static __device__ __forceinline__ void gfh_i" << Is << "_fg(const double t, const double tb, const double* __restrict__ Q, double& F, double* __restrict__ G, int* STATUS) {\n"
       "  if (TK == 0) { gfh_s" << Ss << "_grad(t, Q, F, G, STATUS); return; }\n"
       "  const double arg = TK == 1 ? (tb - 1.0) + 1.0 / t : (tb + 1.0) - 1.0 / t;\n"
       "  gfh_s" << Ss << "_grad(arg, Q, F, G, STATUS);\n"
       "  const double i2 = 1.0 / (t * t);\n  F *= i2;\n"
       "  for (int j = 0; j < " << NQ << "; j++) G[j] *= i2;\n}\n";
  // one Gauss-Kronrod panel on values (NI:636-664)
  s << "template <int TK> static __device__ double gfh_i" << Is << "_gk(const double lo, const double hi, const double tb, const double* __restrict__ Q, double& err, int* STATUS) {\n"
       "  const double scale = (hi - lo) / 2, shift = (lo + hi) / 2;\n  double sg = 0.0, y = 0.0;\n"
       "  for (int i = 1; i <= GFH_GK_N; i++) {\n"
       "    const double f = gfh_i" << Is << "_f<TK>(scale * gfh_gk_roots[i - 1] + shift, tb, Q, STATUS);\n"
       "    if ((i & 1) == 0) sg = sg + gfh_gk_wg[i / 2 - 1] * f;\n"
       "    y = y + gfh_gk_wk[i - 1] * f;\n  }\n"
       "  y = scale * y;\n  err = fabs(y - scale * sg);\n  return y;\n}\n";
  // the same panel with the gradient w.r.t. pars(:) of its Kronrod sum (unscaled, as the final pass of NI:268-275 forms it); the value
  // and the error estimate are the operations of _gk on the same integrand values, bit for bit
  s << "template <int TK> static __device__ double gfh_i" << Is << "_gkg(const double lo, const double hi, const double tb, const double* __restrict__ Q, double& err, double* __restrict__ GS, int* STATUS) {\n"
       "  const double scale = (hi - lo) / 2, shift = (lo + hi) / 2;\n  double sg = 0.0, y = 0.0;\n"
       "  for (int j = 0; j < " << NQ << "; j++) GS[j] = 0.0;\n"
       "  for (int i = 1; i <= GFH_GK_N; i++) {\n"
       "    double f, g[" << NQ << "];\n"
       "    gfh_i" << Is << "_fg<TK>(scale * gfh_gk_roots[i - 1] + shift, tb, Q, f, g, STATUS);\n"
       "    if ((i & 1) == 0) sg = sg + gfh_gk_wg[i / 2 - 1] * f;\n"
       "    y = y + gfh_gk_wk[i - 1] * f;\n"
       "    for (int j = 0; j < " << NQ << "; j++) GS[j] += gfh_gk_wk[i - 1] * g[j];\n  }\n"
       "  y = scale * y;\n  err = fabs(y - scale * sg);\n  return y;\n}\n";
  // The mesh of one piece: bisection on values (NI:251-267) -- or, when another pass at these very parameters has left the
  // record of its bisections (MM == 2: chi2() at the trial point before the sweep of the accepted step, the sweep before
  // STEP 3), their replay: the same midpoints in the same storage order without a single integrand evaluation, so
  // everything that follows sees bitwise the mesh a fresh bisection would build.  MM == 1: this pass leaves the record
  // (MS[0] = number of bisections or 255 = none, MS[1 + k] = the interval the k-th one split).
  // carry: the bisection evaluates every panel WITH the gradient of its Kronrod sum and keeps it per interval (gs[q][:]), so the
  // final pass over the intervals (NI:268-275) has nothing left to evaluate -- (2n - 1) panels with gradient instead of (2n - 1)
  // without plus n with.  The panel sums are the same operations on the same numbers whenever they are formed, so the result is
  // bitwise the two-phase one.  Only with the small workspace the kernels carry first (scratch: 8 NQ bytes more per interval).
  const int ws_value = in.depth <= 1 ? cfg.ws_size : cfg.ws_size_inner;
  const bool can_carry = carries_gradients(NQ, ws_value, cfg.ws_global);
  // the lane's workspace in the global pool: level 1 (outer integrals) first, level 2 behind it (GFH_WSG_L2)
  const std::string ws_decl = cfg.ws_global
      ? "  double* const wl_ = gfh_wsg_lane(" + std::string(in.depth <= 1 ? "0" : "GFH_WSG_L2") + ");\n  const long long row_ = " + std::string(in.depth <= 1 ? "GFH_WSG_ROW1" : "GFH_WSG_ROW2") +
        ";\n  const gfh_wsa lo{wl_, row_}, hi{wl_ + 64, row_}, er{wl_ + 128, row_}, sm{wl_ + 192, row_};\n"
      : "  double lo[" + WS + "], hi[" + WS + "], er[" + WS + "], sm[" + WS + "];\n";
  auto mesh_build = [&](bool need_sums, bool carry = false) {
    std::ostringstream b;
    // (pool form: the gradient of a panel goes to fields 4 .. 4 + NQ - 1 of the interval's row, through a local array the panel fills)
    const bool gpool = carry && cfg.ws_global;
    auto put = [&](const char* q) { return gpool ? std::string("; for (int j = 0; j < ") + std::to_string(NQ) + "; j++) wl_[(4 + j) * 64 + (long long)(" + q + ") * row_] = gl_[j]" : std::string(); };
    if (carry && !gpool) b << "  double gs[" << WS << "][" << NQ << "];\n  bool carried = false;\n";
    if (gpool) b << "  double gl_[" << NQ << "];\n  bool carried = false;\n";
    const std::string gk0 = carry ? "_gkg<TK>(lower, upper, tb, Q, er[0], " + std::string(gpool ? "gl_" : "gs[0]") + ", STATUS)" + put("0") : "_gk<TK>(lower, upper, tb, Q, er[0], STATUS)";
    const std::string gkm = carry ? "_gkg<TK>(aa, mid, tb, Q, er[mx], " + std::string(gpool ? "gl_" : "gs[mx]") + ", STATUS)" + put("mx") : "_gk<TK>(aa, mid, tb, Q, er[mx], STATUS)";
    const std::string gkn = carry ? "_gkg<TK>(mid, bb, tb, Q, er[n], " + std::string(gpool ? "gl_" : "gs[n]") + ", STATUS)" + put("n") : "_gk<TK>(mid, bb, tb, Q, er[n], STATUS)";
    b << ws_decl <<
         "  lo[0] = lower; hi[0] = upper;\n"
         "  int n = 1;\n"
         "  if (MM == 2 && MS && MS[0] != 255) {\n"
         "    const int ns = MS[0];\n"
         "    for (int k = 0; k < ns; k++) {\n"
         "      const int mx = MS[1 + k];\n"
         "      const double aa = lo[mx], bb = hi[mx], mid = (aa + bb) / 2;\n"
         "      hi[mx] = mid; lo[n] = mid; hi[n] = bb; n++;\n"
         "    }\n";
    if (need_sums) b << "    for (int q = 0; q < n; q++) sm[q] = gfh_i" << Is << "_gk<TK>(lo[q], hi[q], tb, Q, er[q], STATUS);\n";
    b << "  } else {\n"
         "    sm[0] = gfh_i" << Is << gk0 << ";\n"
         "    bool whole = true;\n"
         "    for (;;) {\n"
         "      if (n >= " << WS << ") { if (STATUS) GFH_RAISE(STATUS, 1); whole = false; break; }            // NI:282-283\n"
         "      int mx = 0;\n      for (int q = 1; q < n; q++) if (er[q] > er[mx]) mx = q;   // maxloc: first maximum\n"
         "      const double aa = lo[mx], bb = hi[mx], mid = (aa + bb) / 2;\n"
         "      sm[mx] = gfh_i" << Is << gkm << ";\n"
         "      sm[n] = gfh_i" << Is << gkn << ";\n"
         "      hi[mx] = mid; lo[n] = mid; hi[n] = bb;\n"
         "      if (MM == 1 && MS && n < " << kMeshRecord << ") MS[n] = (unsigned char)mx;\n"
         "      n++;\n"
         "      double es = 0.0, ss = 0.0;\n      for (int q = 0; q < n; q++) { es += er[q]; ss += sm[q]; }\n"
         "      if (es < " << lit(abst) << " || es / ss < " << lit(rel) << ") break;         // NI:264-267 (no abs() on the sum)\n"
         "    }\n"
         "    if (MM == 1 && MS) MS[0] = (whole && n <= " << kMeshRecord << ") ? (unsigned char)(n - 1) : (unsigned char)255;\n"
      << (carry ? "    carried = true;\n" : "") <<
         "  }\n";
    return b.str();
  };
  // adaptive piece: the mesh, then the final pass.  WITH_GRAD adds the pars(:) gradient.
  s << "template <int TK, bool WITH_GRAD> static __device__ double gfh_i" << Is << "_piece(const double lower, const double upper, const double tb, const double* __restrict__ Q, double* __restrict__ GQ, int* STATUS, unsigned char* __restrict__ MS, const int MM) {\n"
    << "  if (!WITH_GRAD) {\n" << mesh_build(true) <<
       "  double y = 0.0;\n"
       "  for (int q = 0; q < n; q++) y = y + sm[q];       // NI:270-275\n"
       "  return y;\n  } else {\n" << mesh_build(false, can_carry) <<
       "  double y = 0.0;\n"
       "  for (int j = 0; j < " << NQ << "; j++) GQ[j] = 0.0;\n"
    << (can_carry ?
       "  if (carried) {\n"
       "    for (int q = 0; q < n; q++) {\n"
       "      const double scale = (hi[q] - lo[q]) / 2;\n"
       "      y = y + sm[q];\n"
       "      for (int j = 0; j < " + std::to_string(NQ) + "; j++) GQ[j] += scale * " + (cfg.ws_global ? std::string("wl_[(4 + j) * 64 + (long long)q * row_]") : std::string("gs[q][j]")) + ";\n"
       "    }\n"
       "    return y;\n"
       "  }\n" : std::string()) <<
       "  for (int q = 0; q < n; q++) {\n"
       "    const double scale = (hi[q] - lo[q]) / 2, shift = (lo[q] + hi[q]) / 2;\n"
       "    double yk = 0.0, gk[" << NQ << "];\n    for (int j = 0; j < " << NQ << "; j++) gk[j] = 0.0;\n"
       "    for (int i = 1; i <= GFH_GK_N; i++) {\n"
       "      double f, g[" << NQ << "];\n"
       "      gfh_i" << Is << "_fg<TK>(scale * gfh_gk_roots[i - 1] + shift, tb, Q, f, g, STATUS);\n"
       "      yk = yk + gfh_gk_wk[i - 1] * f;\n"
       "      for (int j = 0; j < " << NQ << "; j++) gk[j] += gfh_gk_wk[i - 1] * g[j];\n    }\n"
       "    const double sq = scale * yk;      // (rounded before it is added, as the panel sums of the value-only pass are: chi2() at these\n"
       "    y = y + sq;                        //  parameters then returns bitwise this pass's sum r^2 -- the look-ahead schedule builds on that)\n"
       "    for (int j = 0; j < " << NQ << "; j++) GQ[j] += scale * gk[j];\n  }\n"
       "  return y;\n  }\n}\n";
  // site: compose the pieces for the bound kinds (NI:291-369)
  auto body = [&](bool grad) {
    std::string g = grad ? "true" : "false", GQ = grad ? "GQ" : "nullptr";
    std::ostringstream b;
    if (!in.lower_inf && !in.upper_inf) b << "  double y = gfh_i" << Is << "_piece<0, " << g << ">(lower, upper, 0.0, Q, " << GQ << ", STATUS, MS, MM);\n";
    else if (!in.lower_inf && in.upper_inf > 0) b << "  double y = gfh_i" << Is << "_piece<1, " << g << ">(0.0, 1.0, lower, Q, " << GQ << ", STATUS, MS, MM);\n";
    else if (!in.lower_inf && in.upper_inf < 0) b << "  double y = 0.0 - gfh_i" << Is << "_piece<2, " << g << ">(0.0, 1.0, lower, Q, " << GQ << ", STATUS, MS, MM);\n" << (grad ? "  for (int j = 0; j < " + std::to_string(NQ) + "; j++) GQ[j] = -GQ[j];\n" : "");
    else if (in.lower_inf < 0 && !in.upper_inf) b << "  double y = gfh_i" << Is << "_piece<2, " << g << ">(0.0, 1.0, upper, Q, " << GQ << ", STATUS, MS, MM);\n";
    else if (in.lower_inf > 0 && !in.upper_inf) b << "  double y = 0.0 - gfh_i" << Is << "_piece<1, " << g << ">(0.0, 1.0, upper, Q, " << GQ << ", STATUS, MS, MM);\n" << (grad ? "  for (int j = 0; j < " + std::to_string(NQ) + "; j++) GQ[j] = -GQ[j];\n" : "");
    else {   // both infinite: integrate_inf_real(lower, 0) + integrate_real_inf(0, upper), NI:367-368
      std::string g2 = grad ? "G2" : "nullptr";
      if (grad) b << "  double G2[" << NQ << "];\n";
      b << "  double y1 = " << (in.lower_inf < 0 ? "" : "0.0 - ") << "gfh_i" << Is << "_piece<" << (in.lower_inf < 0 ? 2 : 1) << ", " << g << ">(0.0, 1.0, 0.0, Q, " << GQ << ", STATUS, nullptr, 0);\n";
      if (grad && in.lower_inf > 0) b << "  for (int j = 0; j < " << NQ << "; j++) GQ[j] = -GQ[j];\n";
      b << "  double y2 = " << (in.upper_inf > 0 ? "" : "0.0 - ") << "gfh_i" << Is << "_piece<" << (in.upper_inf > 0 ? 1 : 2) << ", " << g << ">(0.0, 1.0, 0.0, Q, " << g2 << ", STATUS, nullptr, 0);\n";
      if (grad) b << "  for (int j = 0; j < " << NQ << "; j++) GQ[j] += " << (in.upper_inf > 0 ? "" : "-") << "G2[j];\n";
      b << "  double y = y1 + y2;\n";
    }
    return b.str();
  };
  // forward-mode piece: same mesh (values), final pass carries (d, dd) linearly through the rule
  s << "template <int TK> static __device__ void gfh_i" << Is << "_piece_fwd(const double lower, const double upper, const double tb, const double* __restrict__ Q, "
       "const double* __restrict__ QD, const double* __restrict__ QE, double& Y, double& YD, double& YE, int* STATUS, unsigned char* __restrict__ MS, const int MM) {\n"
    << mesh_build(false) <<
       "  double y = 0.0, yd = 0.0, ye = 0.0;\n"
       "  for (int q = 0; q < n; q++) {\n"
       "    const double scale = (hi[q] - lo[q]) / 2, shift = (lo[q] + hi[q]) / 2;\n"
       "    double yk = 0.0, ykd = 0.0, yke = 0.0;\n"
       "    for (int i = 1; i <= GFH_GK_N; i++) {\n"
       "      const double t = scale * gfh_gk_roots[i - 1] + shift;\n"
       "      double f, fd, fe;\n"
       "      if (TK == 0) gfh_s" << Ss << "_fwd(t, 0.0, 0.0, Q, QD, QE, f, fd, fe, STATUS);\n"
       "      else {\n"
       "        const double arg = TK == 1 ? (tb - 1.0) + 1.0 / t : (tb + 1.0) - 1.0 / t;\n"
       "        gfh_s" << Ss << "_fwd(arg, 0.0, 0.0, Q, QD, QE, f, fd, fe, STATUS);\n"
       "        const double i2 = 1.0 / (t * t); f *= i2; fd *= i2; fe *= i2;\n"
       "      }\n"
       "      yk = yk + gfh_gk_wk[i - 1] * f; ykd = ykd + gfh_gk_wk[i - 1] * fd; yke = yke + gfh_gk_wk[i - 1] * fe;\n"
       "    }\n"
       "    const double sq = scale * yk;\n"
       "    y = y + sq; yd = yd + scale * ykd; ye = ye + scale * yke;\n"
       "  }\n"
       "  Y = y; YD = yd; YE = ye;\n}\n";
  {
    std::ostringstream b;
    auto call = [&](int tk, const std::string& lo_, const std::string& hi_, const std::string& tb_, const std::string& sfx) {
      b << "  double y" << sfx << ", yd" << sfx << ", ye" << sfx << ";\n"
        << "  gfh_i" << Is << "_piece_fwd<" << tk << ">(" << lo_ << ", " << hi_ << ", " << tb_ << ", Q, QD, QE, y" << sfx << ", yd" << sfx << ", ye" << sfx << ", STATUS, "
        << (sfx.empty() ? "MS, MM" : "nullptr, 0") << ");\n";
    };
    if (!in.lower_inf && !in.upper_inf) call(0, "lower", "upper", "0.0", "");
    else if (!in.lower_inf && in.upper_inf > 0) call(1, "0.0", "1.0", "lower", "");
    else if (!in.lower_inf && in.upper_inf < 0) { call(2, "0.0", "1.0", "lower", ""); b << "  y = 0.0 - y; yd = -yd; ye = -ye;\n"; }
    else if (in.lower_inf < 0 && !in.upper_inf) call(2, "0.0", "1.0", "upper", "");
    else if (in.lower_inf > 0 && !in.upper_inf) { call(1, "0.0", "1.0", "upper", ""); b << "  y = 0.0 - y; yd = -yd; ye = -ye;\n"; }
    else {
      call(in.lower_inf < 0 ? 2 : 1, "0.0", "1.0", "0.0", "1");
      if (in.lower_inf > 0) b << "  y1 = 0.0 - y1; yd1 = -yd1; ye1 = -ye1;\n";
      call(in.upper_inf > 0 ? 1 : 2, "0.0", "1.0", "0.0", "2");
      if (in.upper_inf < 0) b << "  y2 = 0.0 - y2; yd2 = -yd2; ye2 = -ye2;\n";
      b << "  double y = y1 + y2, yd = yd1 + yd2, ye = ye1 + ye2;\n";
    }
    s << "template <bool LA, bool UA> static __device__ void gfh_int" << Is << "_fwd(const double lower, const double lowerD, const double lowerE, "
         "const double upper, const double upperD, const double upperE, const double* __restrict__ Q, const double* __restrict__ QD, "
         "const double* __restrict__ QE, double& Y, double& YD, double& YE, int* STATUS, unsigned char* __restrict__ MS, const int MM) {\n" << b.str();
    // Leibniz terms of active bounds (NI:425-437 / 480-487 / 527-534): f at the bound with the
    // bound passive (dummy) and with the bound active (dir_deriv)
    if (!in.lower_inf) s << "  if (LA) {\n    double f0, f0d, f0e, f1, f1d, f1e;\n"
         "    gfh_s" << Ss << "_fwd(lower, 0.0, 0.0, Q, QD, QE, f0, f0d, f0e, STATUS);\n"
         "    gfh_s" << Ss << "_fwdT(lower, lowerD, lowerE, Q, QD, QE, f1, f1d, f1e, STATUS);\n"
         "    yd = yd - lowerD * f0;\n    ye = ye - lowerE * f0 - lowerD * (f1d + f0d);\n  }\n";
    if (!in.upper_inf) s << "  if (UA) {\n    double f0, f0d, f0e, f1, f1d, f1e;\n"
         "    gfh_s" << Ss << "_fwd(upper, 0.0, 0.0, Q, QD, QE, f0, f0d, f0e, STATUS);\n"
         "    gfh_s" << Ss << "_fwdT(upper, upperD, upperE, Q, QD, QE, f1, f1d, f1e, STATUS);\n"
         "    yd = yd + upperD * f0;\n    ye = ye + upperE * f0 + upperD * (f1d + f0d);\n  }\n";
    s << "  Y = y; YD = yd; YE = ye;\n}\n";
  }
  s << "static __device__ double gfh_int" << Is << "_val(const double lower, const double upper, const double* __restrict__ Q, int* STATUS, unsigned char* __restrict__ MS, const int MM) {\n"
    << body(false) << "  return y;\n}\n";
  // LA / UA: the bound is an AD variable with a live adjoint -- only then is f evaluated THERE for the Leibniz term (NI:413-417), as
  // in the reference.  (An iterated integral int_0^x w(t) int_0^t f du dt would otherwise evaluate its inner integral over the empty
  // range [0, 0], whose error test 0/0 never passes: "Number of iterations was insufficient" where the reference computes nothing.)
  s << "template <bool LA, bool UA> static __device__ void gfh_int" << Is << "_grad(const double lower, const double upper, const double* __restrict__ Q, double& Y, double* __restrict__ GQ, double& FL, double& FH, int* STATUS, unsigned char* __restrict__ MS, const int MM) {\n"
    << body(true)
    << "  Y = y;\n"
    << "  FL = " << (in.lower_inf ? "0.0" : "LA ? gfh_s" + Ss + "_val(lower, Q, STATUS) : 0.0") << ";\n"
    << "  FH = " << (in.upper_inf ? "0.0" : "UA ? gfh_s" + Ss + "_val(upper, Q, STATUS) : 0.0") << ";\n}\n\n";
}


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
std::vector<char> guard_needs_of(const Model& m, const SubTape& st);
std::vector<char> guard_needs(const Model& m, int v) { return guard_needs_of(m, m.eval(v)); }
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
  std::vector<int> mem{in.integrand};
  if ((size_t)I < m.alts.size()) mem.insert(mem.end(), m.alts[(size_t)I].begin(), m.alts[(size_t)I].end());
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
       "  for (int j = 0; j < " << std::max(1, in.n_ipars) << "; j++) GQ[j] = 0.0;      // (a recording writes the entries of the pars(:) it reads)\n";
  cases("_grad(T, Q, F, GQ, STATUS); return;", "F = 0.0; for (int j = 0; j < " + std::to_string(std::max(1, in.n_ipars)) + "; j++) GQ[j] = 0.0; return;");
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

// does call site I pick its integrand per evaluation (several recordings, or one that compares AD variables)?
bool site_is_family(const Model& m, int I) {
  if ((size_t)I < m.alts.size() && !m.alts[(size_t)I].empty()) return true;
  for (const Node& nd : m.sub[(size_t)m.integrals[(size_t)I].integrand].nodes) if (is_guard_op(nd.op)) return true;
  return false;
}

}  // namespace

bool Model::needs_hint() const {
  if (n_variants() < 2) return false;
  Trie T(*this);
  std::vector<int> all((size_t)n_variants());
  for (int v = 0; v < n_variants(); v++) all[(size_t)v] = v;
  return T.build(all, 0) >= 0 && T.forks;
}

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

// The cooperative form of the fused kernel (GFH_COOP, 5 ... 8 tiles): its switch and, per wave W of the workgroup, the straight-line
// code of its share of the tile pairs -- a contiguous run of the row-major upper triangle:
//   GFH_CLOAD_W(B, U)  fragment reads of k-step U into buffer B: one per DISTINCT tile of the run + the residual row
//   GFH_CMMA_W(B)      one v_mfma_f64_16x16x4_f64 per pair; J^T r of tile t with the owner of pair (t, t)
//   GFH_CPUT_W         the wave's accumulators into the workgroup's image
static std::string coop_defines(int NA) {
  std::ostringstream o;
  const bool on = fused_coop(NA);
  o << "\n#define GFH_COOP " << (on ? 1 : 0);
  if (!on) return o.str();
  const int T = (NA + 15) / 16, npair = T * (T + 1) / 2, fw = fused_waves_for(NA);
  std::vector<std::pair<int, int>> pairs;
  for (int ti = 0; ti < T; ti++) for (int tj = ti; tj < T; tj++) pairs.push_back({ti, tj});
  int cnd = 0;
  std::ostringstream body;
  for (int w = 0, p0 = 0; w < fw; w++) {
    const int nk = npair / fw + (w < npair % fw ? 1 : 0);
    std::vector<int> tiles;                                   // distinct tiles of this wave's run, in order of first use
    auto slot = [&](int t) { for (size_t d = 0; d < tiles.size(); d++) if (tiles[d] == t) return (int)d; tiles.push_back(t); return (int)tiles.size() - 1; };
    std::ostringstream mma0, mma, put;
    for (int k = 0; k < nk; k++) {
      const int ti = pairs[(size_t)(p0 + k)].first, tj = pairs[(size_t)(p0 + k)].second;
      const int ia = slot(ti), ib = slot(tj);
      (k == 0 ? mma0 : mma) << " GFH_MFMA(f[B_][" << ia << "], f[B_][" << ib << "], acc[" << k << "]);";
      if (ti == tj) mma << " accr[" << k << "] += f[B_][" << ia << "] * fr[B_];";
      put << " GFH_CPUT(" << k << ", " << (p0 + k) << ")";
      if (ti == tj) put << " GFH_CPUTR(" << k << ", " << ti << ")";
    }
    body << "\n#define GFH_CLOAD_" << w << "(B_, U_) fr[B_] = sb[16 * GFH_T * GFH_S + 4 * (U_) + q];";
    for (size_t d = 0; d < tiles.size(); d++) body << " f[B_][" << d << "] = sb[(16 * " << tiles[d] << " + r) * GFH_S + 4 * (U_) + q];";
    body << "\n#define GFH_CMMA0_" << w << "(B_)" << mma0.str();
    body << "\n#define GFH_CMMA_" << w << "(B_)" << mma.str();
    body << "\n#define GFH_CPUT_" << w << put.str();
    cnd = std::max(cnd, (int)tiles.size());
    p0 += nk;
  }
  o << "\n#define GFH_CK " << (npair + fw - 1) / fw << "\n#define GFH_CND " << std::max(1, cnd) << body.str();
  return o.str();
}

// GenConfig::batch: the two kernels of batched independent fits, behind the point functions of the translation unit (batch.cpp is
// their host side and refuses what they do not carry before it comes here; the checks below keep the generator honest on its own).
static bool emit_batch_kernels(const Model& m, const std::vector<int32_t>& active, const GenConfig& cfg, std::ostringstream& s, std::string* err) {
  const int NA = (int)active.size();
  if (NA < 1 || NA > kValuGramMax) { *err = "batch kernels: 1 to " + std::to_string(kValuGramMax) + " active parameters"; return false; }
  if (m.has_integrals() || m.branching() || m.n_aux > 0) { *err = "batch kernels: models with integrate(), variant tapes or auxiliary columns are not carried"; return false; }
  if (cfg.finite_diff || cfg.loss != 0 || !cfg.omega_jt) { *err = "batch kernels: use_ad = 0, robust losses and GADFIT_HIP_OMEGA_JT=0 are not carried"; return false; }
  if (cfg.batch_lanes != 64 && cfg.batch_lanes != 16 && cfg.batch_lanes != 256) { *err = "batch kernels: 64, 16 or 256 lanes per fit"; return false; }
  s << "\n#define GFH_BATCH 1\n#define GFH_BACT {";
  for (int j = 0; j < NA; j++) s << (j ? ", " : "") << active[j];
  s << "}\n#define GFH_BLANES " << cfg.batch_lanes << "\n";
  if (cfg.batch_lanes == 256) s << kBatchWgSum;          // batch_wg_sum.hip: LDS and a barrier, in the text of the workgroup form alone
  s << kBatchFit;                   // batch_fit.hip: gfh_k_fit_batch, gfh_k_batch_pass, written once against GFH_BLANES
  return true;
}

bool generate_source(const Model& m, const std::vector<int32_t>& active, const GenConfig& cfg,
                     std::string* src, std::string* err) {
  const SubTape& st = m.sub[0];
  for (int v = 0; v < m.n_variants(); v++)
    for (const Node& nd : m.eval(v).nodes)
      if (nd.op == GFH_IVAR || nd.op == GFH_IPARAM) { *err = "integrand node in eval() tape"; return false; }
  const int NA = (int)active.size(), NP = m.n_pars;
  std::vector<char> pa(NP, 0), none(NP, 0);
  for (int a : active) { if (a < 0 || a >= NP) { *err = "active parameter out of range"; return false; } pa[a] = 1; }
  // adjoint source per active parameter: every PARAM node of that parameter
  std::ostringstream s;
  s << "// generated by libgadfit_hip codegen -- model with " << st.nodes.size() << " tape nodes, "
    << NP << " parameters, " << NA << " active\n";
  s << "#define GFH_OMEGA_JT " << (cfg.omega_jt ? 1 : 0) << "\n#define GFH_FW " << fused_waves_for(NA) << "\n#define GFH_HALF " << (fused_half_stage(NA) ? 1 : 0) << "\n#define GFH_RED1 " << (fused_single_image(NA) ? 1 : 0) << "\n#define GFH_FUSED_MAX " << kFusedMaxActive << coop_defines(NA) << "\n#define GFH_FAST_DIV " << (cfg.fast_div ? 1 : 0)
    << "\n#define GFH_STORE_J " << (cfg.store_j ? 1 : 0) << "\n#define GFH_STORE_RES " << (cfg.store_res ? 1 : 0) << "\n#define GFH_LOSS " << cfg.loss << "\n#define GFH_BLOCK " << cfg.block << "\n#define GFH_NP " << NP
    << "\n#define GFH_NA " << (NA > 0 ? NA : 1) << "\n#define GFH_VALU_GRAM_MAX " << kValuGramMax << "\n#define GFH_AD_PRIO " << (cfg.store_j ? 0 : 1) << "\n";
  s << "#define GFH_PARG " << cfg.kernarg_pars << "\n";
  s << kExp;                        // exp.hip: gfh_exp
  {
    bool has_pow = false;
    for (const SubTape& t_ : m.sub) for (const Node& nd : t_.nodes) if (nd.op == GFH_POW && !(nd.flags & GFH_F_REAL)) has_pow = true;
    for (const SubTape& t_ : m.more_evals) for (const Node& nd : t_.nodes) if (nd.op == GFH_POW && !(nd.flags & GFH_F_REAL)) has_pow = true;
    if (has_pow && cfg.fast_div) s << kPowLn;      // pow_ln.hip: gfh_pow_ln
  }
  bool lane_stash = false;          // some integrand reads the data point's abscissa or auxiliary columns (Gen::in_integrand)
  for (size_t k = 1; k < m.sub.size(); k++) for (const Node& nd : m.sub[k].nodes) if (nd.op == GFH_X || nd.op == GFH_AUX) lane_stash = true;
  s << "\ntypedef long long i64;\n// kernels raise the status word with an agent-scope atomic: visible to whichever workgroup posts it to the host\n#define GFH_RAISE(p, v) __hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)\n"
       "#define GFH_STATUS_SLOT(st) ((st) == 0 ? 0.0 : (st) == 1 ? 1.0 : (st) == 2 ? 4096.0 : 16777216.0)\n";
  if (lane_stash)
    s << "// what an integrand takes from the enclosing eval() without passing it through pars(:): the lane's abscissa and its auxiliary\n"
         "// columns, left here by the point functions (same thread writes and reads: program order)\n"
         "__shared__ double gfh_lane_x[512];\n__shared__ const double* gfh_lane_axp[512];\n__shared__ i64 gfh_lane_lda;\n"
         "#define GFH_LANE_STASH gfh_lane_x[threadIdx.x] = X; gfh_lane_axp[threadIdx.x] = AXP; gfh_lane_lda = LDA;\n";
  else s << "#define GFH_LANE_STASH\n";
  s << kParsBlock;                  // pars_block.hip: GFH_PARS_DECL / GFH_PARS_AT
  if (m.has_integrals()) {
    const double *roots = gk15_roots, *wg = gk15_wg, *wk = gk15_wk; int npts = 15;
    switch (m.gk_points) {
      case 21: roots = gk21_roots; wg = gk21_wg; wk = gk21_wk; npts = 21; break;
      case 31: roots = gk31_roots; wg = gk31_wg; wk = gk31_wk; npts = 31; break;
      case 41: roots = gk41_roots; wg = gk41_wg; wk = gk41_wk; npts = 41; break;
      case 51: roots = gk51_roots; wg = gk51_wg; wk = gk51_wk; npts = 51; break;
      case 61: roots = gk61_roots; wg = gk61_wg; wk = gk61_wk; npts = 61; break;
      default: break;
    }
    s << "// Gauss-Kronrod rule (numerical_integration.F90:139-171), reference node order: even 1-based = Gauss nodes\n";
    // (intervals an adaptive integral may use, per nesting level: ws(1) / ws(2) of the reference, NI:70, 84-98)
    s << "#define GFH_GK_N " << npts << "\n#define GFH_WS1 " << cfg.ws_size << "\n#define GFH_WS2 " << cfg.ws_size_inner << "\n";
    if (cfg.ws_global) {
      // Workspaces in the context's global pool (model.h, plan_workspaces; NI:40-51, 128-134: the reference's are heap arrays of the
      // user's size).  One slot per wave of the launch -- workgroup b's wave v owns slot b * waves-per-workgroup + v, the host caps
      // the grid at the slots there are and the kernels stride over their tiles -- laid out [level][interval][lo|hi|err|sum][lane]:
      // the wave's access to one field of one interval is one coalesced 512 B row.  The kernels post the pool's address in LDS.
      // (round 5: a level whose call sites carry their panels' gradients has one more field per integrand parameter in its rows --
      // wsg_row_fields, model.h -- so that the pool form spares the final pass its re-evaluation as the scratch form does)
      const long l2 = 64L * wsg_row_fields(m, 1) * cfg.ws_size;
      s << "#define GFH_WSG 1\n#define GFH_WSG_L2 " << l2 << "LL\n#define GFH_WSG_WAVE " << wsg_wave_doubles(m, cfg.ws_size, cfg.ws_size_inner) << "LL\n"
           "#define GFH_WSG_ROW1 " << 64L * wsg_row_fields(m, 1) << "LL\n#define GFH_WSG_ROW2 " << 64L * wsg_row_fields(m, 2) << "LL\n"
           "__shared__ double* gfh_wsg_base;\n"
           "struct gfh_wsa { double* p; long long row; __device__ __forceinline__ double& operator[](const int q) const { return p[(long long)q * row]; } };\n"
           "static __device__ __forceinline__ double* gfh_wsg_lane(const long long level) {\n"
           "  return gfh_wsg_base + ((long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * GFH_WSG_WAVE + level + (threadIdx.x & 63);\n}\n";
    }
    auto arr = [&](const char* name, const double* a, int n) {
      s << "static __device__ const double " << name << "[" << n << "] = {";
      for (int i = 0; i < n; i++) s << (i ? ", " : "") << lit(a[i]);
      s << "};\n";
    };
    arr("gfh_gk_roots", roots, npts); arr("gfh_gk_wg", wg, npts / 2); arr("gfh_gk_wk", wk, npts);
    s << "\n";
    // (call sites of different variants may share one integrand sub-tape, Model::load_variants: its functions are emitted once)
    std::vector<char> sub_done(m.sub.size(), 0);
    // call sites that some recording of eval() (or of an integrand) reaches; the pooled call sites of further recordings of an
    // integrand (Model::alts) only lent their sub-tapes
    std::vector<char> used(m.integrals.size(), 0);
    for (int v = 0; v < m.n_variants(); v++) for (const Node& nd : m.eval(v).nodes) if (nd.op == GFH_INTEGRATE) used[(size_t)nd.a] = 1;
    for (bool more = true; more;) {
      more = false;
      for (size_t I = 0; I < m.integrals.size(); I++) {
        if (!used[I]) continue;
        std::vector<int> mem{m.integrals[I].integrand};
        if (I < m.alts.size()) mem.insert(mem.end(), m.alts[I].begin(), m.alts[I].end());
        for (int sidx : mem) for (const Node& nd : m.sub[(size_t)sidx].nodes) if (nd.op == GFH_INTEGRATE && !used[(size_t)nd.a]) { used[(size_t)nd.a] = 1; more = true; }
      }
    }
    // a call site after the call sites its integrand (any recording of it) calls itself
    std::vector<char> site_done(m.integrals.size(), 0);
    bool ok_sites = true;
    std::function<void(int, int)> emit_site = [&](int I, int depth) {
      if (site_done[(size_t)I] || !ok_sites) return;
      if (depth > 4) { ok_sites = false; *err = "integrate() call sites refer to each other in a cycle"; return; }
      site_done[(size_t)I] = 1;
      std::vector<int> mem{m.integrals[(size_t)I].integrand};
      if ((size_t)I < m.alts.size()) mem.insert(mem.end(), m.alts[(size_t)I].begin(), m.alts[(size_t)I].end());
      for (int S : mem) for (const Node& nd : m.sub[(size_t)S].nodes) if (nd.op == GFH_INTEGRATE) emit_site(nd.a, depth + 1);
      if (!ok_sites) return;
      for (int S : mem) { if (!sub_done[(size_t)S]) emit_integrand_functions(m, S, cfg, s); sub_done[(size_t)S] = 1; }
      if (site_is_family(m, I) && !emit_family(m, I, s, err)) { ok_sites = false; return; }
      emit_integral_site(m, I, cfg, s);
    };
    for (int I = 0; I < (int)m.integrals.size() && ok_sites; I++) if (used[(size_t)I]) emit_site(I, 0);
    if (!ok_sites) return false;
  }
  // The model bodies.  A model with ONE recorded path and no comparison gets the four point functions below under their plain
  // names.  A branching model (Model::branching) gets them once per variant (suffix _v<k>), the selector, and dispatchers
  // under the plain names that take the lane's slot as one more argument (for the report of an unseen turn).
  // register cap of the plain kernels (GenConfig::waves_per_eu): models with integrate() are bound by VALU issue and want waves, not registers
  if (cfg.waves_per_eu > 0) s << "#define GFH_OCC __attribute__((amdgpu_waves_per_eu(" << cfg.waves_per_eu << ")))\n";
  else s << "#define GFH_OCC\n";
  const bool multi = m.branching();
  const int V = m.n_variants();
  s << (multi ? "#define GFH_SLOT_DECL , const i64 SLOT\n#define GFH_SLOT(i) , (i64)(i)\n#define GFH_SLOT_PASS , SLOT\n"
              : "#define GFH_SLOT_DECL\n#define GFH_SLOT(i)\n#define GFH_SLOT_PASS\n");
  // Mesh hand-over (emit_integral_site, mesh_build): models with integrate() carry a per-lane record pointer and a mode
  // (0 none, 1 this pass records its bisections, 2 it replays recorded ones) from the kernels down to the call sites.
  const int n_mesh = cfg.finite_diff ? 0 : mesh_sites(m);
  if (n_mesh > 0)
    s << "#define GFH_MESH_STRIDE " << kMeshRecord * n_mesh << "\n#define GFH_MESH_DECL , unsigned char* __restrict__ MESH, const int MESH_MODE\n"
         "#define GFH_MESH_PASS , MESH, MESH_MODE\n#define GFH_MESH_AT(i) , (mesh ? mesh + (i64)(i) * GFH_MESH_STRIDE : (unsigned char*)nullptr), mesh_mode\n"
         "#define GFH_MESH_NONE , (unsigned char*)nullptr, 0\n#define GFH_MESH_KPARAMS , unsigned char* __restrict__ mesh, const int mesh_mode\n";
  else
    s << "#define GFH_MESH_DECL\n#define GFH_MESH_PASS\n#define GFH_MESH_AT(i)\n#define GFH_MESH_NONE\n#define GFH_MESH_KPARAMS\n";
  // Order of dispatch (launch.cpp, build_orders): the cost of a point of a model with integrate() is the number of its bisections,
  // workgroups are dispatched in index order, and x-sorted data put the expensive tiles last -- they would run alone at the end.  The
  // plain kernels of such models take the tile / block a workgroup works on from a table sorted by measured cost, expensive first;
  // the sweep measures (shader clock per tile).  Which workgroup does a tile changes no result: every sum is defined on the fixed
  // partition.
  if (n_mesh > 0)        // (the same kernels that take the mesh arguments: the host passes both groups or neither)
    s << "#define GFH_HAS_ORDER 1\n#define GFH_ORDER_KPARAMS , const int* __restrict__ order, int* __restrict__ cost\n#define GFH_ORD(b) (order ? order[b] : (int)(b))\n";
  else
    s << "#define GFH_HAS_ORDER 0\n#define GFH_ORDER_KPARAMS\n#define GFH_ORD(b) ((int)(b))\n";
  // (kernels whose quadrature workspaces are the global pool take its address as their last argument and post it in LDS)
  if (m.has_integrals() && cfg.ws_global)
    s << "#define GFH_WSG_KPARAMS , double* __restrict__ wsg\n#define GFH_WSG_INIT if (threadIdx.x == 0) gfh_wsg_base = wsg; __syncthreads();\n";
  else
    s << "#define GFH_WSG 0\n#define GFH_WSG_KPARAMS\n#define GFH_WSG_INIT\n";
  const bool mesh_on = n_mesh > 0;
  const std::string A7 = "const double* __restrict__ AXP, const i64 LDA GFH_MESH_DECL";
  auto grad_expr = [&](const Gen& g, const SubTape& t, int j) {
    std::string e;
    for (int k = 0; k < (int)t.nodes.size(); k++)
      if (t.nodes[k].op == GFH_PARAM && t.nodes[k].a == active[j] && g.act[k]) e += (e.empty() ? "" : " + ") + g.b(k);
    return e.empty() ? std::string("0.0") : e;
  };
  auto emit_value_fn = [&](const SubTape& t, const std::string& sfx, const std::string& slot) {
    s << "\n// One data point, every parameter passive (chi2 path): value only.\n"
         "static __device__ __forceinline__ double gfh_point_value" << sfx << "(const double X, const double* __restrict__ P, int* STATUS,\n"
         "                                                         " << A7 << slot << ") {\n";
    s << "  GFH_LANE_STASH\n";
    Gen g(m, t, cfg.fast_div); g.mode = 0; g.mesh_top = mesh_on; g.analyse(none); g.emit_values(false);
    s << g.o.str() << "  return " << g.v(t.result) << ";\n}\n";
  };
  auto emit_grad_fn = [&](const SubTape& t, const std::string& sfx, const std::string& slot) {
    s << "\n// One data point, reverse mode: value F and gradient G[a] = dF/dp_active(a).\n"
         "static __device__ __forceinline__ void gfh_point_grad" << sfx << "(const double X, const double* __restrict__ P,\n"
         "                                                      double& F, double (&G)[GFH_NA], int* STATUS,\n"
         "                                                      " << A7 << slot << ") {\n";
    s << "  GFH_LANE_STASH\n";
    Gen g(m, t, cfg.fast_div); g.mode = 1; g.mesh_top = mesh_on; g.analyse(pa); g.emit_values(false); g.emit_reverse();
    s << g.o.str() << "  F = " << g.v(t.result) << ";\n";
    for (int j = 0; j < NA; j++) s << "  G[" << j << "] = " << grad_expr(g, t, j) << ";\n";
    s << "}\n";
  };
  auto emit_dd_fn = [&](const SubTape& t, const std::string& sfx, const std::string& slot) {
    s << "\n// One data point, forward mode: second directional derivative along DP (per-parameter d seeds).\n"
         "static __device__ __forceinline__ double gfh_point_dd" << sfx << "(const double X, const double* __restrict__ P,\n"
         "                                                      const double* __restrict__ DP, int* STATUS,\n"
         "                                                      " << A7 << slot << ") {\n";
    s << "  GFH_LANE_STASH\n";
    Gen g(m, t, cfg.fast_div); g.mode = 2; g.mesh_top = mesh_on; g.analyse(pa); g.emit_forward_all();
    s << g.o.str();
    if (g.act[t.result]) s << "  return " << g.dd(t.result) << ";\n"; else s << "  return 0.0;\n";
    s << "}\n";
  };
  if (multi) {
    s << "\n// A lane whose point takes a turn through eval() that no recorded variant covers: status 3 and one entry {slot, outcomes of\n"
         "// the guards passed, their number} in the report area behind the status word (context.h, kStatusBytes).\n"
         "#define GFH_UNSEEN_CAP " << 120 << "\n"
         "struct gfh_unseen { i64 slot; unsigned long long path; int n_guards; int pad; };\n"
         "static __device__ __attribute__((noinline)) void gfh_report_unseen(int* STATUS, const i64 slot, const unsigned long long path, const int ng) {\n"
         "  GFH_RAISE(STATUS, 3);\n"
         "  const unsigned k = __hip_atomic_fetch_add((unsigned*)((char*)STATUS + 64), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
         "  if (k < GFH_UNSEEN_CAP) { gfh_unseen* e = (gfh_unseen*)((char*)STATUS + 128) + k; e->slot = slot; e->path = path; e->n_guards = ng; e->pad = 0; }\n"
         "}\n";
    if (!emit_selector(m, s, err)) return false;
    for (int v = 0; v < V; v++) {
      const std::string sfx = "_v" + std::to_string(v);
      emit_value_fn(m.eval(v), sfx, "");
      if (!cfg.finite_diff) { emit_grad_fn(m.eval(v), sfx, ""); emit_dd_fn(m.eval(v), sfx, ""); }
    }
    s << "\nstatic __device__ __forceinline__ double gfh_point_value(const double X, const double* __restrict__ P, int* STATUS,\n"
         "                                                         " << A7 << " GFH_SLOT_DECL) {\n"
         "  unsigned long long path; int ng;\n  switch (gfh_select(X, P, STATUS, AXP, LDA, path, ng)) {\n";
    for (int v = 0; v < V; v++) s << "    case " << v << ": return gfh_point_value_v" << v << "(X, P, STATUS, AXP, LDA GFH_MESH_PASS);\n";
    s << "    default: gfh_report_unseen(STATUS, SLOT, path, ng); return 0.0;\n  }\n}\n";
    if (!cfg.finite_diff) {
      s << "\nstatic __device__ __forceinline__ void gfh_point_grad(const double X, const double* __restrict__ P,\n"
           "                                                      double& F, double (&G)[GFH_NA], int* STATUS,\n"
           "                                                      " << A7 << " GFH_SLOT_DECL) {\n"
           "  unsigned long long path; int ng;\n  switch (gfh_select(X, P, STATUS, AXP, LDA, path, ng)) {\n";
      for (int v = 0; v < V; v++) s << "    case " << v << ": gfh_point_grad_v" << v << "(X, P, F, G, STATUS, AXP, LDA GFH_MESH_PASS); break;\n";
      s << "    default:\n      F = 0.0;\n#pragma unroll\n      for (int a = 0; a < GFH_NA; a++) G[a] = 0.0;\n      gfh_report_unseen(STATUS, SLOT, path, ng);\n  }\n}\n";
      s << "\nstatic __device__ __forceinline__ double gfh_point_dd(const double X, const double* __restrict__ P,\n"
           "                                                      const double* __restrict__ DP, int* STATUS,\n"
           "                                                      " << A7 << " GFH_SLOT_DECL) {\n"
           "  unsigned long long path; int ng;\n  switch (gfh_select(X, P, STATUS, AXP, LDA, path, ng)) {\n";
      for (int v = 0; v < V; v++) s << "    case " << v << ": return gfh_point_dd_v" << v << "(X, P, DP, STATUS, AXP, LDA GFH_MESH_PASS);\n";
      s << "    default: gfh_report_unseen(STATUS, SLOT, path, ng); return 0.0;\n  }\n}\n";
    }
  }
  if (cfg.finite_diff) {
    // use_ad = .false. (gadfit.F90:684-687, 721-726): every parameter passive, the gradient by forward differences
    // (fitfunction.F90:155-174) and the second directional derivative by a central difference (188-203); the
    // value body is inlined once per evaluation the reference makes (it re-evaluates f(p); the value is the same).
    // (A branching model takes its branch afresh in each of those evaluations, as the reference's eval() does.)
    if (!multi) emit_value_fn(st, "", " GFH_SLOT_DECL");
    s << R"(
// One data point, finite differences (grad_finite, fitfunction.F90:155-174): step = sqrt(epsilon)*p, taken as
// (p + step) - p; G[a] = (f(p + step e_a) - f(p)) / step.
static __device__ __forceinline__ void gfh_point_grad(const double X, const double* __restrict__ P,
                                                      double& F, double (&G)[GFH_NA], int* STATUS,
                                                      const double* __restrict__ AXP, const i64 LDA GFH_MESH_DECL GFH_SLOT_DECL) {
  double Q[GFH_NP];
#pragma unroll
  for (int k = 0; k < GFH_NP; k++) Q[k] = P[k];
  F = gfh_point_value(X, Q, STATUS, AXP, LDA GFH_MESH_PASS GFH_SLOT_PASS);
)";
    for (int j = 0; j < NA; j++) {
      const int pj = active[j];
      // (fd_col_sets: the per-point columns of this evaluation are those the host tabulated at p + step e_j -- set 1 + j)
      const std::string axp = cfg.fd_col_sets && m.n_aux > 0 ? "AXP + (i64)" + std::to_string((j + 1) * m.n_aux) + " * LDA" : "AXP";
      s << "  { const double saved = Q[" << pj << "]; double step = 0x1p-26 * saved; Q[" << pj << "] = saved + step; step = Q[" << pj
        << "] - saved;\n    const double fp = gfh_point_value(X, Q, STATUS, " << axp << ", LDA GFH_MESH_PASS GFH_SLOT_PASS); Q[" << pj << "] = saved; G[" << j
        << "] = (fp - F) / step; }\n";
    }
    s << R"(}

// One data point, second directional derivative along DP by finite differences (dir_deriv_2nd_finite,
// fitfunction.F90:188-203): h = epsilon**(1/4); (f(p + h d) + f(p - h d) - 2 f(p)) / sqrt(epsilon).
static __device__ __forceinline__ double gfh_point_dd(const double X, const double* __restrict__ P,
                                                      const double* __restrict__ DP, int* STATUS,
                                                      const double* __restrict__ AXP, const i64 LDA GFH_MESH_DECL GFH_SLOT_DECL) {
  double Q[GFH_NP];
#pragma unroll
  for (int k = 0; k < GFH_NP; k++) Q[k] = P[k];
)";
    for (int j = 0; j < NA; j++) s << "  Q[" << active[j] << "] = P[" << active[j] << "] + 0x1p-13 * DP[" << active[j] << "];\n";
    s << "  double y = gfh_point_value(X, Q, STATUS, AXP, LDA GFH_MESH_PASS GFH_SLOT_PASS);\n";
    for (int j = 0; j < NA; j++) s << "  Q[" << active[j] << "] = P[" << active[j] << "] - 0x1p-13 * DP[" << active[j] << "];\n";
    s << "  y = y + gfh_point_value(X, Q, STATUS, AXP, LDA GFH_MESH_PASS GFH_SLOT_PASS);\n";
    for (int j = 0; j < NA; j++) s << "  Q[" << active[j] << "] = P[" << active[j] << "];\n";
    s << "  y = y - 2.0 * gfh_point_value(X, Q, STATUS, AXP, LDA GFH_MESH_PASS GFH_SLOT_PASS);\n  return y / 0x1p-26;\n}\n";
  } else if (!multi) {
    emit_grad_fn(st, "", " GFH_SLOT_DECL");
    emit_value_fn(st, "", " GFH_SLOT_DECL");
    emit_dd_fn(st, "", " GFH_SLOT_DECL");
  }
  // ---- the hand-written kernels, in this order (the model body above is the only generated part)
  s << kSweep << kWaveSum << kFusedSweepGram << kChi2 << kOmega;
  if (cfg.omega_jt && !cfg.finite_diff && !m.has_integrals() && cfg.loss == 0 && NA <= 64) {
    // One data point, forward mode AND reverse mode over ONE evaluation of the forward values: the second directional
    // derivative along DP and the gradient.  The forward values are the expressions of gfh_point_grad / gfh_point_dd (the same
    // emit_value_node), the reverse sweep is gfh_point_grad's, so G is bitwise the Jacobian row the sweep kernel stores.
    auto emit_dd_grad_fn = [&](const SubTape& t, const std::string& sfx, const std::string& slot) {
      s << "\nstatic __device__ __forceinline__ double gfh_point_dd_grad" << sfx << "(const double X, const double* __restrict__ P,\n"
           "                                                           const double* __restrict__ DP, double (&G)[GFH_NA], int* STATUS,\n"
           "                                                           " << A7 << slot << ") {\n";
      s << "  GFH_LANE_STASH\n";
      Gen g(m, t, cfg.fast_div); g.mode = 2; g.analyse(pa); g.emit_forward_all(); g.emit_reverse();
      s << g.o.str();
      for (int j = 0; j < NA; j++) s << "  G[" << j << "] = " << grad_expr(g, t, j) << ";\n";
      if (g.act[t.result]) s << "  return " << g.dd(t.result) << ";\n}\n";
      else s << "  return 0.0;\n}\n";
    };
    if (!multi) emit_dd_grad_fn(st, "", " GFH_SLOT_DECL");
    else {
      for (int v = 0; v < V; v++) emit_dd_grad_fn(m.eval(v), "_v" + std::to_string(v), "");
      s << "\nstatic __device__ __forceinline__ double gfh_point_dd_grad(const double X, const double* __restrict__ P,\n"
           "                                                           const double* __restrict__ DP, double (&G)[GFH_NA], int* STATUS,\n"
           "                                                           " << A7 << " GFH_SLOT_DECL) {\n"
           "  unsigned long long path; int ng;\n  switch (gfh_select(X, P, STATUS, AXP, LDA, path, ng)) {\n";
      for (int v = 0; v < V; v++) s << "    case " << v << ": return gfh_point_dd_grad_v" << v << "(X, P, DP, G, STATUS, AXP, LDA GFH_MESH_PASS);\n";
      s << "    default:\n#pragma unroll\n      for (int a = 0; a < GFH_NA; a++) G[a] = 0.0;\n      gfh_report_unseen(STATUS, SLOT, path, ng); return 0.0;\n  }\n}\n";
    }
  }
  if (cfg.omega_jt && !cfg.finite_diff && !m.has_integrals() && cfg.loss == 0 && NA <= 64) s << kOmegaJt;      // omega_jt.hip: gfh_k_omega_jt
  if (cfg.batch && !emit_batch_kernels(m, active, cfg, s, err)) return false;
  *src = s.str();
  return true;
}

}  // namespace gfh
