// normal_eq.cpp -- the host solve of the damped normal equations (normal_eq.h): plain and blocked Cholesky, the block-arrow solver of
// global fits.  Plain C++ on doubles: no context, no device.
#include "normal_eq.h"
#include <algorithm>
#include <cmath>

namespace gfh {

// potr_f08 (gadfit_linalg.F90:36-57) = dpotrf('U') then dpotrs, column-major, in place.  Split so a
// factor can serve two right-hand sides: gadf_fit factorises the SAME matrix twice per accelerated
// iteration (gadfit.F90:712-713 and 737-738); reusing the factor gives bitwise the same delta2.
int potrf_upper_plain(int n, double* a) {
  auto A = [&](int i, int j) -> double& { return a[(size_t)j * n + i]; };
  for (int j = 0; j < n; j++) {
    double ajj = A(j, j);
    for (int k = 0; k < j; k++) ajj -= A(k, j) * A(k, j);
    if (!(ajj > 0.0)) return 1;
    ajj = std::sqrt(ajj); A(j, j) = ajj;
    const double rinv = 1.0 / ajj;
    // row j of U: one dot product per column c.  Four columns at a time for instruction-level
    // parallelism; every individual sum keeps the k = 0..j-1 order, so results are bitwise those
    // of the plain loop (and of the oracle's).
    const double* cj = a + (size_t)j * n;
    int c = j + 1;
    for (; c + 3 < n; c += 4) {
      const double *c0 = a + (size_t)c * n, *c1 = c0 + n, *c2 = c1 + n, *c3 = c2 + n;
      double s0 = c0[j], s1 = c1[j], s2 = c2[j], s3 = c3[j];
      for (int k = 0; k < j; k++) {
        const double v = cj[k];
        s0 -= v * c0[k]; s1 -= v * c1[k]; s2 -= v * c2[k]; s3 -= v * c3[k];
      }
      A(j, c) = s0 * rinv; A(j, c + 1) = s1 * rinv; A(j, c + 2) = s2 * rinv; A(j, c + 3) = s3 * rinv;
    }
    for (; c < n; c++) {
      double s = A(j, c);
      for (int k = 0; k < j; k++) s -= A(k, j) * A(k, c);
      A(j, c) = s * rinv;
    }
  }
  return 0;
}

// ---- blocked factorisation for the normal equations of global fits (dim = n_global + n_local *
// n_datasets reaches hundreds: BASELINE config 3 has dim 259, where the plain loop above needs 7.7 ms per
// solve -- 70 times the device pass it waits for).  Left-looking by block columns of NB: the block row
// [jb, jb+nb) x [jb, n) first receives the contributions of the rows above it (dot products of
// column pairs, contiguous in memory: the 2 x 4 micro-kernel below, AVX2+FMA where the CPU has it),
// then its diagonal block is factorised by the plain algorithm and the rest of the block row follows by
// forward substitution.  Same arithmetic per entry, different (fixed) order of additions.
namespace {
typedef double v4d __attribute__((ext_vector_type(4)));

__attribute__((target("avx2,fma"))) void dots_2x4_avx2(const double* a0, const double* a1, const double* const* b, int len, double* out) {
  v4d acc[2][4];
  for (int r = 0; r < 2; r++) for (int q = 0; q < 4; q++) acc[r][q] = (v4d){0.0, 0.0, 0.0, 0.0};
  int k = 0;
  for (; k + 3 < len; k += 4) {
    v4d va0, va1, vb;
    __builtin_memcpy(&va0, a0 + k, 32); __builtin_memcpy(&va1, a1 + k, 32);
    for (int q = 0; q < 4; q++) {
      __builtin_memcpy(&vb, b[q] + k, 32);
      acc[0][q] += va0 * vb; acc[1][q] += va1 * vb;
    }
  }
  for (int q = 0; q < 4; q++) {
    double s0 = ((acc[0][q][0] + acc[0][q][1]) + acc[0][q][2]) + acc[0][q][3];
    double s1 = ((acc[1][q][0] + acc[1][q][1]) + acc[1][q][2]) + acc[1][q][3];
    for (int kk = k; kk < len; kk++) { s0 += a0[kk] * b[q][kk]; s1 += a1[kk] * b[q][kk]; }
    out[q] = s0; out[4 + q] = s1;
  }
}

void dots_2x4_plain(const double* a0, const double* a1, const double* const* b, int len, double* out) {
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < len; k++) {
    const double x0 = a0[k], x1 = a1[k];
    for (int q = 0; q < 4; q++) { s[q] += x0 * b[q][k]; s[4 + q] += x1 * b[q][k]; }
  }
  for (int q = 0; q < 8; q++) out[q] = s[q];
}

int potrf_upper_blocked(int n, double* a) {
  static const bool avx2 = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
  void (*dots)(const double*, const double*, const double* const*, int, double*) = avx2 ? dots_2x4_avx2 : dots_2x4_plain;
  auto A = [&](int i, int j) -> double& { return a[(size_t)j * n + i]; };
  auto col = [&](int j) -> const double* { return a + (size_t)j * n; };
  constexpr int NB = 48;
  for (int jb = 0; jb < n; jb += NB) {
    const int nb = jb + NB < n ? NB : n - jb;
    // (1) A(i, c) -= sum_{k < jb} U(k, i) U(k, c) for i in the block row, c >= i
    if (jb > 0) {
      for (int i = jb; i < jb + nb; i += 2) {
        const int i1 = i + 1 < jb + nb ? i + 1 : i;          // odd block height: the second row repeats the first
        for (int c = i; c < n; c += 4) {
          const double* b[4]; int cc[4];
          for (int q = 0; q < 4; q++) { cc[q] = c + q < n ? c + q : c; b[q] = col(cc[q]); }
          double out[8];
          dots(col(i), col(i1), b, jb, out);
          for (int q = 0; q < 4; q++) {
            if (c + q >= n) break;
            A(i, c + q) -= out[q];
            if (i1 != i && c + q >= i1) A(i1, c + q) -= out[4 + q];
          }
        }
      }
    }
    // (2) diagonal block by the plain algorithm (rows/columns jb .. jb+nb-1, k from jb)
    for (int j = jb; j < jb + nb; j++) {
      double ajj = A(j, j);
      for (int k = jb; k < j; k++) ajj -= A(k, j) * A(k, j);
      if (!(ajj > 0.0)) return 1;
      ajj = std::sqrt(ajj); A(j, j) = ajj;
      const double rinv = 1.0 / ajj;
      // (3) row j of U beyond the diagonal, inside the block and to its right: forward substitution
      for (int c = j + 1; c < n; c++) {
        double sacc = A(j, c);
        const double *cj = col(j), *ccol = col(c);
        for (int k = jb; k < j; k++) sacc -= cj[k] * ccol[k];
        A(j, c) = sacc * rinv;
      }
    }
  }
  return 0;
}
}  // namespace

int potrf_upper(int n, double* a) {
  return n > 64 ? potrf_upper_blocked(n, a) : potrf_upper_plain(n, a);
}

void potrs_upper(int n, const double* a, double* b) {
  auto A = [&](int i, int j) -> double { return a[(size_t)j * n + i]; };
  for (int i = 0; i < n; i++) { double t = b[i]; for (int k = 0; k < i; k++) t -= A(k, i) * b[k]; b[i] = t / A(i, i); }
  for (int k = n - 1; k >= 0; k--) if (b[k] != 0.0) { b[k] /= A(k, k); for (int i = 0; i < k; i++) b[i] -= b[k] * A(i, k); }
}


void DampedSolver::find_structure(const int32_t* jac) {
  std::vector<int> owner(dim, -1);           // -1 unused, d = only dataset d, -2 = several datasets
  for (int d = 0; d < nd; d++) for (int j = 0; j < na; j++) {
    int& o_ = owner[jac[(size_t)d * na + j]];
    o_ = o_ == -1 ? d : (o_ == d ? d : -2);
  }
  lcols.clear(); gcols.clear(); loff.assign(nd + 1, 0);
  for (int d = 0; d < nd; d++) { for (int col = 0; col < dim; col++) if (owner[col] == d) lcols.push_back(col); loff[d + 1] = (int)lcols.size(); }
  for (int col = 0; col < dim; col++) if (owner[col] < 0) gcols.push_back(col);
  arrow_ = nd > 1 && dim > 16 && (int)lcols.size() >= dim / 2;
  if (!arrow_) return;
  const int ng = (int)gcols.size();
  udoff.assign(nd + 1, 0); wdoff.assign(nd + 1, 0);
  for (int d = 0; d < nd; d++) { const int nl = loff[d + 1] - loff[d]; udoff[d + 1] = udoff[d] + nl * nl; wdoff[d + 1] = wdoff[d] + nl * ng; }
  Ud.assign(udoff[nd], 0); Wd.assign(wdoff[nd], 0); Ug.assign((size_t)ng * ng, 0); ytmp.assign(dim, 0);
}
int DampedSolver::factor_arrow(double lambda) {
  const int ng = (int)gcols.size();
  for (int a = 0; a < ng; a++) for (int b = 0; b < ng; b++) Ug[(size_t)b * ng + a] = Mat(gcols[a], gcols[b], lambda);
  for (int d = 0; d < nd; d++) {
    const int nl = loff[d + 1] - loff[d];
    if (!nl) continue;
    const int* lc = &lcols[loff[d]];
    double* U = &Ud[udoff[d]]; double* W = &Wd[wdoff[d]];
    for (int a = 0; a < nl; a++) for (int b = 0; b < nl; b++) U[(size_t)b * nl + a] = Mat(lc[a], lc[b], lambda);
    if (potrf_upper_plain(nl, U)) return 1;
    // W = U^-T B, B[a][g] = Mat(lc[a], gcols[g]); column g of W by forward substitution with U^T
    for (int g = 0; g < ng; g++) {
      double* wg = W + (size_t)g * nl;
      for (int a = 0; a < nl; a++) {
        double t = Mat(lc[a], gcols[g], lambda);
        for (int k = 0; k < a; k++) t -= U[(size_t)a * nl + k] * wg[k];
        wg[a] = t / U[(size_t)a * nl + a];
      }
    }
    // S -= W^T W (upper triangle is what potrf reads; keep it symmetric anyway)
    for (int g = 0; g < ng; g++) for (int h = 0; h <= g; h++) {
      double t = 0.0;
      for (int k = 0; k < nl; k++) t += W[(size_t)h * nl + k] * W[(size_t)g * nl + k];
      Ug[(size_t)g * ng + h] -= t; if (h != g) Ug[(size_t)h * ng + g] -= t;
    }
  }
  return ng ? potrf_upper_plain(ng, Ug.data()) : 0;
}
void DampedSolver::solve_arrow(const double* rhs, double* out) {
  const int ng = (int)gcols.size();
  std::vector<double>& y = ytmp;
  std::vector<double> bg(ng);
  for (int g = 0; g < ng; g++) bg[g] = rhs[gcols[g]];
  // forward: y_d = U_d^-T b_d ; b_g -= W_d^T y_d
  for (int d = 0; d < nd; d++) {
    const int nl = loff[d + 1] - loff[d];
    const int* lc = nl ? &lcols[loff[d]] : nullptr; const double* U = nl ? &Ud[udoff[d]] : nullptr; const double* W = nl ? &Wd[wdoff[d]] : nullptr;
    double* yd = y.data() + loff[d];
    for (int a = 0; a < nl; a++) {
      double t = rhs[lc[a]];
      for (int k = 0; k < a; k++) t -= U[(size_t)a * nl + k] * yd[k];
      yd[a] = t / U[(size_t)a * nl + a];
    }
    for (int g = 0; g < ng; g++) { double t = 0.0; for (int k = 0; k < nl; k++) t += W[(size_t)g * nl + k] * yd[k]; bg[g] -= t; }
  }
  // global block: U_g^T U_g x_g = b_g
  if (ng) potrs_upper(ng, Ug.data(), bg.data());
  for (int g = 0; g < ng; g++) out[gcols[g]] = bg[g];
  // back: x_d = U_d^-1 (y_d - W_d x_g)
  for (int d = 0; d < nd; d++) {
    const int nl = loff[d + 1] - loff[d];
    if (!nl) continue;
    const int* lc = &lcols[loff[d]]; const double* U = &Ud[udoff[d]]; const double* W = &Wd[wdoff[d]];
    double* yd = y.data() + loff[d];
    for (int a = 0; a < nl; a++) { double t = yd[a]; for (int g = 0; g < ng; g++) t -= W[(size_t)g * nl + a] * bg[g]; yd[a] = t; }
    for (int a = nl - 1; a >= 0; a--) {
      double t = yd[a];
      for (int k = a + 1; k < nl; k++) t -= U[(size_t)k * nl + a] * yd[k];
      yd[a] = t / U[(size_t)a * nl + a];
      out[lc[a]] = yd[a];
    }
  }
}

void DampedSolver::setup(int nd_, int na_, const int32_t* jac, int dim_, bool use_structure) {
  nd = nd_; na = na_; dim = dim_;
  find_structure(jac);
  if (!use_structure) arrow_ = false;
  if (!arrow_) zero_image(lin, (size_t)dim * dim);       // (the dense factor; a global fit of many curves is solved block by block)
}

int DampedSolver::factor(const double* JTJ_, const double* DTD_, double lambda) {
  JTJ = JTJ_; DTD = DTD_;
  if (arrow_) return factor_arrow(lambda);
  for (int col = 0; col < dim; col++)                                  // gadfit.F90:711-713
    for (int row = 0; row < dim; row++)
      lin[(size_t)col * dim + row] = JTJ[(size_t)col * dim + row] + (row == col ? lambda * DTD[col] : 0.0);
  return potrf_upper(dim, lin.data());
}

void DampedSolver::solve(const double* rhs, double* out) {
  if (arrow_) { std::fill(out, out + dim, 0.0); solve_arrow(rhs, out); return; }
  std::copy(rhs, rhs + dim, out);
  potrs_upper(dim, lin.data(), out);
}

// ---- the covariance (J^T J)^-1 of a fit (LMsolver::getInvJTJ, lm_solver.cpp:551-585: dpptrf + dpptri there).  The three steps are
// those of the batch kernel gfh_k_batch_cov (device/batch_cov.hip), operation for operation: the upper factor with every pivot
// held to "positive and finite", V = U^-1 over it, C = V V^T with every entry formed once.  No contraction: one rounding per operation.
namespace {
#pragma clang fp contract(off)
int factor_checked(int n, double* a) {                    // a = U^T U, the upper triangle in place; j + 1: pivot j failed
  auto A = [&](int i, int j) -> double& { return a[(size_t)j * n + i]; };
  for (int j = 0; j < n; j++) {
    double ajj = A(j, j);
    for (int k = 0; k < j; k++) ajj -= A(k, j) * A(k, j);
    if (!(ajj > 0.0 && ajj < HUGE_VAL)) return j + 1;
    ajj = std::sqrt(ajj); A(j, j) = ajj;
    const double rinv = 1.0 / ajj;
    for (int c = j + 1; c < n; c++) {
      double t = A(j, c);
      for (int k = 0; k < j; k++) t -= A(k, j) * A(k, c);
      A(j, c) = t * rinv;
    }
  }
  return 0;
}
void invert_upper(int n, double* a) {                     // V = U^-1 over U, column by column
  auto V = [&](int i, int j) -> double& { return a[(size_t)j * n + i]; };
  for (int j = 0; j < n; j++) {
    const double vjj = 1.0 / V(j, j);
    for (int i = 0; i < j; i++) {
      double t = V(i, i) * V(i, j);
      for (int k = i + 1; k < j; k++) t += V(i, k) * V(k, j);
      V(i, j) = -(t * vjj);
    }
    V(j, j) = vjj;
  }
}
void times_transpose(int n, double* a) {                  // C = V V^T over V: each entry once, written to both triangles
  auto V = [&](int i, int j) -> double& { return a[(size_t)j * n + i]; };
  for (int b = 0; b < n; b++)
    for (int r = 0; r <= b; r++) {
      double t = V(r, b) * V(b, b);
      for (int k = b + 1; k < n; k++) t += V(r, k) * V(b, k);
      V(r, b) = t; V(b, r) = t;                           // (row b of V right of the diagonal is read until C(b, b), the last of column b)
    }
}
}  // namespace

int cholesky_inverse(int n, double* a) {
  if (const int info = factor_checked(n, a)) return info;
  invert_upper(n, a);
  times_transpose(n, a);
  return 0;
}

// The arrow form: with the local columns of dataset d as block A_d, their coupling to the global columns B_d and the global block S,
//   S' = S - sum_d W_d^T W_d, W_d = U_d^-T B_d (the Schur complement, as factor_arrow forms it), C_gg = S'^-1,
//   X_d = A_d^-1 B_d = V_d W_d,  Y_d = X_d C_gg,  C_dg = -Y_d,  C_dd' = [d = d'] A_d^-1 + Y_d X_d'^T.
int DampedSolver::invert_arrow(const double* A, double* cov) const {
#pragma clang fp contract(off)
  const int ng = (int)gcols.size();
  auto at = [&](int r, int c) { return r <= c ? A[(size_t)c * dim + r] : A[(size_t)r * dim + c]; };      // the upper triangle, as the dense form reads it
  auto out = [&](int r, int c, double v) { cov[(size_t)c * dim + r] = v; cov[(size_t)r * dim + c] = v; };
  std::vector<double> S((size_t)ng * ng), X((size_t)(wdoff.empty() ? 0 : wdoff[nd])), Y(X.size()), Ai((size_t)(udoff.empty() ? 0 : udoff[nd])), W;
  for (int a = 0; a < ng; a++) for (int b = 0; b < ng; b++) S[(size_t)b * ng + a] = at(gcols[a], gcols[b]);
  for (int d = 0; d < nd; d++) {
    const int nl = loff[d + 1] - loff[d];
    if (!nl) continue;
    const int* lc = lcols.data() + loff[d];
    double* U = Ai.data() + udoff[d]; double* Xd = X.data() + wdoff[d];
    for (int a = 0; a < nl; a++) for (int b = 0; b < nl; b++) U[(size_t)b * nl + a] = at(lc[a], lc[b]);
    if (const int info = factor_checked(nl, U)) return lc[info - 1] + 1;
    W.assign((size_t)nl * ng, 0.0);
    for (int g = 0; g < ng; g++) {                        // column g of W = U^-T B by forward substitution
      double* wg = W.data() + (size_t)g * nl;
      for (int a = 0; a < nl; a++) {
        double t = at(lc[a], gcols[g]);
        for (int k = 0; k < a; k++) t -= U[(size_t)a * nl + k] * wg[k];
        wg[a] = t / U[(size_t)a * nl + a];
      }
    }
    for (int g = 0; g < ng; g++) for (int h = 0; h <= g; h++) {
      double t = 0.0;
      for (int k = 0; k < nl; k++) t += W[(size_t)h * nl + k] * W[(size_t)g * nl + k];
      S[(size_t)g * ng + h] -= t;                         // (the upper triangle is what the factorisation reads)
    }
    invert_upper(nl, U);                                  // V_d
    for (int g = 0; g < ng; g++) for (int a = 0; a < nl; a++) {
      double t = 0.0;
      for (int k = a; k < nl; k++) t += U[(size_t)k * nl + a] * W[(size_t)g * nl + k];
      Xd[(size_t)g * nl + a] = t;
    }
    times_transpose(nl, U);                               // A_d^-1
  }
  if (ng) if (const int info = cholesky_inverse(ng, S.data())) return gcols[info - 1] + 1;
  for (int a = 0; a < ng; a++) for (int b = a; b < ng; b++) out(gcols[a], gcols[b], S[(size_t)b * ng + a]);
  for (int d = 0; d < nd; d++) {                          // Y_d = X_d C_gg, and the coupling blocks
    const int nl = loff[d + 1] - loff[d];
    const int* lc = lcols.data() + loff[d]; const double* Xd = X.data() + wdoff[d]; double* Yd = Y.data() + wdoff[d];
    for (int a = 0; a < nl; a++) for (int g = 0; g < ng; g++) {
      double t = 0.0;
      for (int h = 0; h < ng; h++) t += Xd[(size_t)h * nl + a] * S[(size_t)g * ng + h];
      Yd[(size_t)g * nl + a] = t;
      out(lc[a], gcols[g], -t);
    }
  }
  for (int d = 0; d < nd; d++) {
    const int nl = loff[d + 1] - loff[d];
    for (int e = d; e < nd; e++) {
      const int ne = loff[e + 1] - loff[e];
      for (int a = 0; a < nl; a++) for (int b = (e == d ? a : 0); b < ne; b++) {
        double t = e == d ? Ai[udoff[d] + (size_t)b * nl + a] : 0.0;
        for (int g = 0; g < ng; g++) t += Y[wdoff[d] + (size_t)g * nl + a] * X[wdoff[e] + (size_t)g * ne + b];
        out(lcols[loff[d] + a], lcols[loff[e] + b], t);
      }
    }
  }
  return 0;
}

int DampedSolver::invert(const double* A, double factor, double* cov, double* sigma) {
  const size_t n2 = (size_t)dim * dim;
  int info;
  if (arrow_) { std::fill(cov, cov + n2, 0.0); info = invert_arrow(A, cov); }      // (columns no dataset uses stay zero)
  else { std::copy(A, A + n2, cov); info = cholesky_inverse(dim, cov); }
  if (info) {
    std::fill(cov, cov + n2, std::nan("")); std::fill(sigma, sigma + dim, std::nan(""));
    return info;
  }
  if (factor != 1.0) for (size_t k = 0; k < n2; k++) cov[k] *= factor;
  for (int j = 0; j < dim; j++) sigma[j] = std::sqrt(cov[(size_t)j * dim + j]);
  return 0;
}

}  // namespace gfh
