// packed_layout.cpp -- see packed_layout.h.  Host-only, context-free.
#include "packed_layout.h"
#include "gram_image.h"
#include "packed_walk.h"
#include <algorithm>

namespace gfh {

bool compute_layout(int nd, int na, const int32_t* jac, int dim, bool sparse_ok, PackedLayout* L, std::string* err) {
  L->inv.assign((size_t)nd * dim, -1);
  for (int d = 0; d < nd; d++)
    for (int k = 0; k < na; k++) {
      const int col = jac[d * na + k];
      if (col < 0 || col >= dim) { *err = "Jacobian index out of range"; return false; }
      L->inv[(size_t)d * dim + col] = k;
    }
  // owner[col]: the single dataset that uses column col (local parameter) or -1 (several: global parameter)
  L->owner.assign(dim, -1);
  std::vector<int> users(dim, 0);
  for (int d = 0; d < nd; d++) for (int k = 0; k < na; k++) { const int col = jac[d * na + k]; if (users[col]++ == 0) L->owner[col] = d; }
  for (int col = 0; col < dim; col++) if (users[col] != 1) L->owner[col] = -1;
  if (nd == 1) std::fill(L->owner.begin(), L->owner.end(), 0);
  // pattern of the normal equations: (row <= col) pairs of columns that share a dataset, column-major order
  L->sparse = false; L->nnz = 0; L->nz_row.clear(); L->nz_col.clear();
  L->small = (int64_t)dim * dim * nd <= 65536;
  if (sparse_ok && nd > 1) {
    // the (row <= col) pairs some dataset couples, in column-major order (sorted keys: a dim x dim map costs 16 MB and 8e6 tests
    // per call at the 4003 columns of a 1000-curve fit)
    std::vector<int64_t> keys;
    keys.reserve((size_t)nd * na * (na + 1) / 2);
    for (int d = 0; d < nd; d++)
      for (int k = 0; k < na; k++) for (int m = 0; m < na; m++) {
        const int r_ = jac[d * na + k], c_ = jac[d * na + m];
        if (r_ <= c_) keys.push_back((int64_t)c_ * dim + r_);
      }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    for (const int64_t key : keys) { L->nz_row.push_back((int)(key % dim)); L->nz_col.push_back((int)(key / dim)); }
    L->nnz = (int)L->nz_row.size();
    L->sparse = 4 * ((int64_t)L->nnz + dim + 1) < (int64_t)dim * dim + dim + 1;      // worth it when the pattern is a quarter or less
  }
  return true;
}

bool build_gather_lists(const PackedLayout& L, int nd, int dim, int T, std::vector<int>* meta, std::vector<int>* list) {
  const int gw = gram_partial_stride(T);
  const bool lay_sparse = L.transfer_sparse();
  const int64_t n_img = (int64_t)L.packed_n(dim);
  meta->clear(); list->clear();
  if ((int64_t)nd * gw >= (int64_t(1) << 31) || n_img > (int64_t(1) << 18)) return false;
  meta->resize((size_t)n_img);
  std::vector<int> terms;
  auto put = [&](size_t idx) {
    if (terms.empty()) (*meta)[idx] = kGatherNoTerm;
    else if (terms.size() == 1) (*meta)[idx] = terms[0];
    else { (*meta)[idx] = -((int)list->size() + 1); list->push_back((int)terms.size()); list->insert(list->end(), terms.begin(), terms.end()); }
  };
  auto entry = [&](int row, int col) {
    terms.clear();
    for (int d = 0; d < nd; d++) {
      const int a = L.inv[(size_t)d * dim + row], b = L.inv[(size_t)d * dim + col];
      if (a >= 0 && b >= 0) terms.push_back(d * gw + gram_entry(a, b, T));
    }
  };
  const size_t nn = lay_sparse ? (size_t)L.nnz : (size_t)dim * dim;
  if (lay_sparse) for (int k = 0; k < L.nnz; k++) { entry(L.nz_row[k], L.nz_col[k]); put((size_t)k); }
  else for (int col = 0; col < dim; col++) for (int row = 0; row < dim; row++) { entry(row, col); put((size_t)col * dim + row); }
  for (int row = 0; row < dim; row++) {
    terms.clear();
    for (int d = 0; d < nd; d++) { const int a = L.inv[(size_t)d * dim + row]; if (a >= 0) terms.push_back(d * gw + gram_jtr(a, T)); }
    put(nn + row);
  }
  terms.clear();
  for (int d = 0; d < nd; d++) terms.push_back(d * gw + gram_rtr(T));
  put(nn + dim);
  if (list->empty()) list->push_back(0);
  return true;
}

}  // namespace gfh
