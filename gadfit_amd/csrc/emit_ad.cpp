// emit_ad.cpp -- the AD unroller: one tape as straight-line device code -- forward values, the reverse sweep, forward-mode (d, dd).
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
#include "codegen_internal.h"
#include <cmath>
#include <cstdio>

namespace gfh {

std::string lit(double c) {
  char b[64];
  if (std::isnan(c)) return "__builtin_nan(\"\")";
  if (std::isinf(c)) return c > 0 ? "__builtin_inf()" : "(-__builtin_inf())";
  snprintf(b, sizeof b, "%a", c);   // hex float: exact
  return b;
}

namespace {

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

}  // namespace

void Gen::analyse(const std::vector<char>& par_active) {
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
std::string Gen::powi_expr(const std::string& x, int n, const std::string& tmp) {
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
int Gen::variant(const Node& nd, int k) const {
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

void Gen::emit_values() {
  int n = (int)st.nodes.size();
  for (int k = 0; k < n; k++) emit_value_node(k);
}

// forward mode: value and (d, dd) of each node together, in tape order (an integrate()
// call needs the tangents of its bindings when it is evaluated)
void Gen::emit_forward_all() {
  int n = (int)st.nodes.size();
  for (int k = 0; k < n; k++) { emit_value_node(k); if (act[k]) emit_dd_node(k); }
}

void Gen::emit_value_node(int k) {
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

// integrate(f, pars, lower, upper) call site (NI:193-630): the adaptive rule lives in the
// generated gfh_int<I>_* functions; here the bindings are gathered and, in reverse mode,
// the partials w.r.t. pars(:) and f at the bounds are kept for the return sweep.
void Gen::emit_integrate_call(int k) {
  const Node& nd = st.nodes[k];
  const Integral& in = m.integrals[nd.a];
  const std::string I = std::to_string(nd.a), ks = std::to_string(k);
  o << ind << "double q" << ks << "[" << n_q(in) << "];\n";
  for (int j = 0; j < in.n_ipars; j++) o << ind << "q" << ks << "[" << j << "] = " << v(m.ipar_nodes[in.ipar_off + j]) << ";\n";
  const std::string lo = in.lower_inf ? "0.0" : v(in.lower), hi = in.upper_inf ? "0.0" : v(in.upper);
  if (mode == 1 && act[k]) {
    o << ind << "double " << v(k) << ", g" << ks << "[" << n_q(in) << "], fl" << ks << ", fh" << ks << ";\n";
    o << ind << "gfh_int" << I << "_grad<" << ((!in.lower_inf && act[in.lower]) ? "true" : "false") << ", " << ((!in.upper_inf && act[in.upper]) ? "true" : "false") << ">(" << lo << ", " << hi << ", q" << ks << ", " << v(k) << ", g" << ks << ", fl" << ks << ", fh" << ks << ", STATUS, " << mesh_args(in) << ");\n";
  } else if (mode == 2 && act[k]) {
    // forward mode (NI:425-437, 480-487, 527-534): tangents of pars(:) and of the bounds go in
    const int NQ = n_q(in);
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
void Gen::emit_reverse() {
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
void Gen::emit_dd_node(int k) {
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

}  // namespace gfh
