// normal_eq.h -- the linear algebra of the damped normal equations (J^T J + lambda DTD) x = rhs on the host: the dense and the
// blocked Cholesky (potr_f08, gadfit_linalg.F90:36-57), the block-arrow solver of global fits, and the zero-initialised images they
// work on.  Knows nothing of a context or of the device: a factorisation that fails is a return value and the caller words the
// message (lm.cpp: the fit and the two exported helpers gfh_potr / gfh_solve_damped).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <utility>
#include <vector>

namespace gfh {

// dpotrf('U') and dpotrs, column-major, in place; potrf_* return 1 where the matrix is not positive definite
int potrf_upper_plain(int n, double* a);
int potrf_upper(int n, double* a);          // the plain loop up to n = 64, the blocked factorisation above
void potrs_upper(int n, const double* a, double* b);

// The dense dim x dim images of a fit.  A global fit of many curves writes and reads only the pattern of its normal equations
// (gfh_sweep's pattern-only transfer, the block-arrow solve): 4003 columns are 128 MB per image of which 1 MB is ever touched, and
// filling them with zeros was 40 ms per fit.  The memory comes zeroed from calloc (for sizes like these: fresh pages, which cost
// nothing until they are touched) and value-initialisation leaves it alone.
template <class T> struct ZeroAlloc {
  using value_type = T;
  ZeroAlloc() = default;
  template <class U> ZeroAlloc(const ZeroAlloc<U>&) {}
  T* allocate(size_t n) { void* p = calloc(n ? n : 1, sizeof(T)); if (!p) throw std::bad_alloc(); return static_cast<T*>(p); }
  void deallocate(T* p, size_t) { free(p); }
  template <class U> void construct(U*) {}
  template <class U, class A0, class... A> void construct(U* p, A0&& a0, A&&... a) { ::new (static_cast<void*>(p)) U(std::forward<A0>(a0), std::forward<A>(a)...); }
  template <class U> bool operator==(const ZeroAlloc<U>&) const { return true; }
  template <class U> bool operator!=(const ZeroAlloc<U>&) const { return false; }
};
using ZVec = std::vector<double, ZeroAlloc<double>>;
inline void zero_image(ZVec& v, size_t n) { ZVec().swap(v); v.resize(n); }

// The damped solve of a fit: factor() once per (JTJ, DTD, lambda), solve() once per right-hand side against that factor (gadf_fit
// factorises the same matrix twice per accelerated iteration, gadfit.F90:712-713 and 737-738; one factor gives bitwise the same delta2).
class DampedSolver {
 public:
  // jac [nd][na]: the column of every dataset's active parameters (Jacobian_indices); use_structure = false keeps the dense form
  void setup(int nd, int na, const int32_t* jac, int dim, bool use_structure = true);
  int factor(const double* JTJ, const double* DTD, double lambda);      // 1: not positive definite
  void solve(const double* rhs, double* out);                           // rhs and out [dim], distinct
  bool arrow() const { return arrow_; }
  // The covariance of the fit (LMsolver::getInvJTJ, lm_solver.cpp:551-585): cov [dim * dim] = (J^T J)^-1 of the matrix itself, no
  // damping and no DTD, dense, both triangles, symmetric bit for bit; sigma [dim] = sqrt of its diagonal.  The upper Cholesky factor
  // U, V = U^-1 and C = V V^T with every entry formed once -- densely, or where the arrow form is on block by block: the local blocks
  // one by one, the Schur complement of the global columns, then the blocks of the inverse from them.  Returns 0, or j + 1 where
  // the pivot of column j was not positive and finite (cov and sigma are then NaN throughout); under the arrow form the local
  // columns are eliminated first, dataset by dataset, and j is the failing pivot's column in the caller's numbering.  Every entry
  // is multiplied by `factor` (1: as it is) before sigma is taken.  Throws std::bad_alloc where its work space cannot be had.
  int invert(const double* JTJ, double factor, double* cov, double* sigma);

 private:
  int nd = 0, na = 0, dim = 0;
  const double *JTJ = nullptr, *DTD = nullptr;   // of the factor() in progress
  // ---- block-arrow structure of a global fit.  A column of J that only ONE dataset's rows touch (a
  // local parameter of that dataset) has no product with the local columns of any other dataset:
  // JTJ + lambda DTD = [diag(A_1 .. A_nd)  B; B^T  S] with A_d the local block of dataset d and S the
  // block of the global parameters.  The reference factorises it densely (doc/user_guide.tex:222-235
  // notes the structure is not used); at BASELINE config 3 (64 x 4 local + 3 global, dim 259) that is
  // 5.8 Mflop on the host per solve against a 0.1 ms device pass.  Here: U_d = chol(A_d),
  // W_d = U_d^-T B_d, S' = S - sum_d W_d^T W_d, U_g = chol(S') -- the Cholesky factor of the matrix with
  // the global columns ordered last, the zero blocks skipped.  Same solution up to rounding.
  std::vector<int> lcols, loff, gcols;        // local columns grouped by dataset (offsets loff[nd+1]); global columns
  std::vector<double> Ud, Wd, Ug, ytmp;       // factors: per dataset [nl*nl] and [nl*ng] (column-major), global [ng*ng]
  std::vector<int> udoff, wdoff;
  bool arrow_ = false;
  ZVec lin;                                   // the dense factor (not allocated where the arrow form is used)
  void find_structure(const int32_t* jac);
  double Mat(int row, int col, double lambda) const { return JTJ[(size_t)col * dim + row] + (row == col ? lambda * DTD[col] : 0.0); }
  int factor_arrow(double lambda);
  void solve_arrow(const double* rhs, double* out);
  int invert_arrow(const double* A, double* cov) const;
};

// In place, column-major n x n: the upper triangle of a symmetric matrix on entry, its inverse in both triangles on return (U, then
// V = U^-1 over it, then V V^T; one rounding per operation, sums in ascending index).  0, or j + 1 where pivot j was not positive and
// finite; the contents are then unspecified.
int cholesky_inverse(int n, double* a);

}  // namespace gfh
