// model.h -- host-side copy of a gfh_tape: the recordings of a model as the generator and the host read them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/gadfit_tape.h"

namespace gfh {

struct Node { int32_t op, a, b, flags; double c; };
struct SubTape { std::vector<Node> nodes; int32_t result; };
struct Integral {
  int32_t integrand, lower, upper, lower_inf, upper_inf, n_ipars, ipar_off, depth;
  double rel_error, abs_error;
};

// A model is one or more recorded paths ("variants") through the user's eval() (gadfit_tape.h, guard nodes).  sub[0] is eval() of
// variant 0, sub[1..] the integrand sub-tapes of ALL variants (pooled; identical ones are shared), more_evals[v-1] eval() of variant v.
struct Model {
  int32_t n_pars = 0;
  std::vector<SubTape> sub;
  std::vector<SubTape> more_evals;
  std::vector<Integral> integrals;
  std::vector<int32_t> ipar_nodes;
  // alts[I]: further recordings (sub-tape indices) of the integrand of call site I -- an integrand that compares AD variables takes
  // its branch anew at every abscissa of the quadrature (AD:315-395), a recording follows one path through it; the recordings of a
  // call site that differ only in that path are pooled here and the device picks per evaluation (emit_branching.cpp, emit_family)
  std::vector<std::vector<int32_t>> alts;
  int32_t n_tapes = 1;          // recordings handed over (gfh_set_model_variants): variants of eval() + further recordings of integrands
  int32_t gk_points = 15;
  int32_t n_aux = 0;            // auxiliary per-point columns read by eval() (GFH_AUX)
  int32_t hint_aux = -1;        // the auxiliary column that names, per data point, the variant it took when the columns were tabulated
                                // (needed only where variants part ways WITHOUT a comparison: plain-real control flow on x)
  // Round 5: one such column PER SET OF OUTCOMES.  hint_cols[t] (per tape; empty: hint_aux for all): the column that holds, per data
  // point, the tape the point follows when the comparisons of AD variables on tape t's own path come out as on tape t -- a function of
  // the abscissa alone (the comparisons are given, only plain-real control flow is left), so it is tabulated once and a point that
  // changes sides at a comparison finds its leaf behind a fork without the host (gfh_set_variant_hint_columns, emit_branching.cpp emit_selector).
  std::vector<int32_t> hint_cols;
  std::vector<int32_t> tape_variant;      // tape t of the hand-over -> the variant of eval() it became (pooled integrand recordings join an earlier one)
  int32_t ws_size = 1000, ws_size_inner = 1000;   // quadrature workspaces the user asked for (NI:40, 128-134)
  double rel_error_outer = 0, rel_error_inner = 0;

  // copies and validates; returns false and sets err on malformed tapes
  bool load(const gfh_tape* t, std::string* err);
  bool load_variants(int n, const gfh_tape* const* t, int hint_aux, std::string* err, const std::vector<int32_t>* hint_cols = nullptr);
  int hint_col_of_variant(int v) const;      // the column a walk reads for variant v (the first tape that became v)
  std::vector<int> tapes_of_variant(int v) const;
  bool has_integrals() const { return !integrals.empty(); }
  int n_variants() const { return 1 + (int)more_evals.size(); }
  const SubTape& eval(int v) const { return v == 0 ? sub[0] : more_evals[(size_t)v - 1]; }
  bool has_guards() const;
  bool branching() const { return n_variants() > 1 || has_guards(); }
  // do the variants part ways somewhere without a comparison (so that only a per-point column can tell them apart)?
  bool needs_hint() const;
};

inline bool is_guard_op(int op) { return op == GFH_GUARD_GT || op == GFH_GUARD_LT; }
// same operation (guards: whatever their recorded outcome)
bool same_node(const Node& a, const Node& b);

// The Gauss-Kronrod rule of a point count (Model::gk_points; include/gadfit_gk_tables.h): n roots and Kronrod weights in the
// reference's node order, n / 2 Gauss weights.  n = 0: no such rule.
struct GkRule { const double *roots, *wg, *wk; int n; };
GkRule gk_rule(int points);


}  // namespace gfh
