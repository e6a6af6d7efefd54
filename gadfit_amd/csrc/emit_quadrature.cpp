// emit_quadrature.cpp -- integrate() on the device: the integrand functions, the call sites, the rule tables and the workspaces.
#include "codegen_internal.h"
#include <functional>

namespace gfh {

namespace {

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
  { Gen g(m, st, cfg.fast_div); g.in_integrand = true; g.mode = 0; g.analyse(none); g.emit_values(); s << g.o.str() << "  return " << g.v(st.result) << ";\n}\n\n"; }
  s << "static __device__ void gfh_s" << S << "_grad(const double T, const double* __restrict__ Q, double& F, double* __restrict__ GQ, int* STATUS) {\n";
  {
    Gen g(m, st, cfg.fast_div); g.in_integrand = true; g.mode = 1; g.analyse(all); g.emit_values(); g.emit_reverse();
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

// The pieces of a call site by the kinds of its bounds (NI:291-369): one adaptive piece on [lo, hi] under the map TK of gfh_i<I>_f
// (0 none, 1 (a, inf), 2 (-inf, b)) about tb, negated where the bounds come the other way round; both bounds infinite:
// integrate_inf_real(lower, 0) + integrate_real_inf(0, upper), NI:367-368.
struct Piece { int tk; const char *lo, *hi, *tb; bool neg; };
std::vector<Piece> pieces_of(const Integral& in) {
  if (!in.lower_inf && !in.upper_inf) return {{0, "lower", "upper", "0.0", false}};
  if (!in.lower_inf) return {{in.upper_inf > 0 ? 1 : 2, "0.0", "1.0", "lower", in.upper_inf < 0}};
  if (!in.upper_inf) return {{in.lower_inf < 0 ? 2 : 1, "0.0", "1.0", "upper", in.lower_inf > 0}};
  return {{in.lower_inf < 0 ? 2 : 1, "0.0", "1.0", "0.0", in.lower_inf > 0}, {in.upper_inf > 0 ? 1 : 2, "0.0", "1.0", "0.0", in.upper_inf < 0}};
}

void emit_integral_site(const Model& m, int I, const GenConfig& cfg, std::ostringstream& s) {
  const Integral& in = m.integrals[I];
  const int S = in.integrand, NQ = n_q(in);
  const double rel = in.rel_error >= 0 ? in.rel_error : (in.depth <= 1 ? m.rel_error_outer : m.rel_error_inner);
  const double abst = in.abs_error >= 0 ? in.abs_error : 0.0;
  // (an integrand that compares AD variables: the dispatchers gfh_sf<I>_* of emit_family stand in for gfh_s<S>_*)
  const std::string Is = std::to_string(I), Ss = site_is_family(m, I) ? "f" + std::to_string(I) : std::to_string(S);
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
  // site: compose the pieces for the bound kinds (NI:291-369, pieces_of)
  const std::vector<Piece> pc = pieces_of(in);
  auto body = [&](bool grad) {
    const std::string g = grad ? "true" : "false", flip = "  for (int j = 0; j < " + std::to_string(NQ) + "; j++) GQ[j] = -GQ[j];\n";
    auto piece = [&](const Piece& p, const char* gq, const char* ms) {
      return std::string(p.neg ? "0.0 - " : "") + "gfh_i" + Is + "_piece<" + std::to_string(p.tk) + ", " + g + ">(" + p.lo + ", " + p.hi + ", " + p.tb + ", Q, " + gq + ", STATUS, " + ms + ");\n";
    };
    std::ostringstream b;
    if (pc.size() == 1) {
      b << "  double y = " << piece(pc[0], grad ? "GQ" : "nullptr", "MS, MM") << (grad && pc[0].neg ? flip : "");
      return b.str();
    }
    if (grad) b << "  double G2[" << NQ << "];\n";
    b << "  double y1 = " << piece(pc[0], grad ? "GQ" : "nullptr", "nullptr, 0") << (grad && pc[0].neg ? flip : "");
    b << "  double y2 = " << piece(pc[1], grad ? "G2" : "nullptr", "nullptr, 0");
    if (grad) b << "  for (int j = 0; j < " << NQ << "; j++) GQ[j] += " << (pc[1].neg ? "-" : "") << "G2[j];\n";
    b << "  double y = y1 + y2;\n";
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
    for (size_t q = 0; q < pc.size(); q++) {
      const Piece& p = pc[q];
      const std::string sfx = pc.size() == 1 ? "" : std::to_string(q + 1);
      b << "  double y" << sfx << ", yd" << sfx << ", ye" << sfx << ";\n"
        << "  gfh_i" << Is << "_piece_fwd<" << p.tk << ">(" << p.lo << ", " << p.hi << ", " << p.tb << ", Q, QD, QE, y" << sfx << ", yd" << sfx << ", ye" << sfx << ", STATUS, "
        << (sfx.empty() ? "MS, MM" : "nullptr, 0") << ");\n";
      if (p.neg) b << "  y" << sfx << " = 0.0 - y" << sfx << "; yd" << sfx << " = -yd" << sfx << "; ye" << sfx << " = -ye" << sfx << ";\n";
    }
    if (pc.size() == 2) b << "  double y = y1 + y2, yd = yd1 + yd2, ye = ye1 + ye2;\n";
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

}  // namespace

// the rule's tables and the workspace macros (GFH_GK_N, GFH_WS1 / GFH_WS2, and for the global pool GFH_WSG* with its accessors)
static void emit_rule_and_workspaces(const Model& m, const GenConfig& cfg, std::ostringstream& s) {
  GkRule r = gk_rule(m.gk_points);
  if (!r.n) r = gk_rule(15);
  s << "// Gauss-Kronrod rule (numerical_integration.F90:139-171), reference node order: even 1-based = Gauss nodes\n";
  // (intervals an adaptive integral may use, per nesting level: ws(1) / ws(2) of the reference, NI:70, 84-98)
  s << "#define GFH_GK_N " << r.n << "\n#define GFH_WS1 " << cfg.ws_size << "\n#define GFH_WS2 " << cfg.ws_size_inner << "\n";
  if (cfg.ws_global) {
    // Workspaces in the context's global pool (codegen.h, plan_workspaces; NI:40-51, 128-134: the reference's are heap arrays of the
    // user's size).  One slot per wave of the launch -- workgroup b's wave v owns slot b * waves-per-workgroup + v, the host caps
    // the grid at the slots there are and the kernels stride over their tiles -- laid out [level][interval][lo|hi|err|sum][lane]:
    // the wave's access to one field of one interval is one coalesced 512 B row.  The kernels post the pool's address in LDS.
    // (round 5: a level whose call sites carry their panels' gradients has one more field per integrand parameter in its rows --
    // wsg_row_fields, codegen.h -- so that the pool form spares the final pass its re-evaluation as the scratch form does)
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
  arr("gfh_gk_roots", r.roots, r.n); arr("gfh_gk_wg", r.wg, r.n / 2); arr("gfh_gk_wk", r.wk, r.n);
  s << "\n";
}

// call sites that some recording of eval() (or of an integrand) reaches; the pooled call sites of further recordings of an
// integrand (Model::alts) only lent their sub-tapes
static std::vector<char> reachable_sites(const Model& m) {
  std::vector<char> used(m.integrals.size(), 0);
  for (int v = 0; v < m.n_variants(); v++) for (const Node& nd : m.eval(v).nodes) if (nd.op == GFH_INTEGRATE) used[(size_t)nd.a] = 1;
  for (bool more = true; more;) {
    more = false;
    for (size_t I = 0; I < m.integrals.size(); I++) {
      if (!used[I]) continue;
      for (int sidx : family_members(m, (int)I)) for (const Node& nd : m.sub[(size_t)sidx].nodes) if (nd.op == GFH_INTEGRATE && !used[(size_t)nd.a]) { used[(size_t)nd.a] = 1; more = true; }
    }
  }
  return used;
}

bool emit_quadrature(const Model& m, const GenConfig& cfg, std::ostringstream& s, std::string* err) {
  emit_rule_and_workspaces(m, cfg, s);
  // (call sites of different variants may share one integrand sub-tape, Model::load_variants: its functions are emitted once)
  std::vector<char> sub_done(m.sub.size(), 0);
  const std::vector<char> used = reachable_sites(m);
  // a call site after the call sites its integrand (any recording of it) calls itself
  std::vector<char> site_done(m.integrals.size(), 0);
  bool ok_sites = true;
  std::function<void(int, int)> emit_site = [&](int I, int depth) {
    if (site_done[(size_t)I] || !ok_sites) return;
    if (depth > 4) { ok_sites = false; *err = "integrate() call sites refer to each other in a cycle"; return; }
    site_done[(size_t)I] = 1;
    const std::vector<int> mem = family_members(m, I);
    for (int S : mem) for (const Node& nd : m.sub[(size_t)S].nodes) if (nd.op == GFH_INTEGRATE) emit_site(nd.a, depth + 1);
    if (!ok_sites) return;
    for (int S : mem) { if (!sub_done[(size_t)S]) emit_integrand_functions(m, S, cfg, s); sub_done[(size_t)S] = 1; }
    if (site_is_family(m, I) && !emit_family(m, I, s, err)) { ok_sites = false; return; }
    emit_integral_site(m, I, cfg, s);
  };
  for (int I = 0; I < (int)m.integrals.size() && ok_sites; I++) if (used[(size_t)I]) emit_site(I, 0);
  return ok_sites;
}

}  // namespace gfh
