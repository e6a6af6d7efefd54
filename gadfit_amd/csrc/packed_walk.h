// packed_walk.h -- the value of one element of the packed image [J^T J or its pattern | J^T r | chi2] from the per-dataset Gram
// images G [nd][gw] (gram_image.h): the walks over the datasets that k_assemble and k_assemble_sparse make through owner / inv, and
// the sum over a host-built source list that k_gather_sum makes (packed_layout.cpp, build_gather_lists).  All of them add the same
// terms in dataset order, so the three kernels give the same bits; tests/host/packed_image_main.cpp runs these very functions on
// the host against each other and against a naive loop.  Plain C++ with GFH_HD, no HIP header.
#pragma once
#include "gram_image.h"

#if defined(__HIPCC__)
#define GFH_HD_INLINE GFH_HD inline
#else
#define GFH_HD_INLINE inline
#endif

namespace gfh {

#define GFH_ASM_CHUNK 8

// J^T J entry (row, col).  inv[d][col] = local active index or -1.
// owner[c] = the only dataset whose rows touch column c (a local parameter), or -1 (global parameter):
// an entry with a local row or column receives a contribution from that one dataset only, so the loop
// over datasets -- and with it the order of additions -- collapses to that term
GFH_HD_INLINE double walk_entry(const double* __restrict__ G, const int gw, const int T, const int nd, const int dim,
                                const int* __restrict__ inv, const int* __restrict__ owner, const int row, const int col) {
  const int orow = owner[row], ocol = owner[col];
  const int d0 = orow >= 0 ? orow : (ocol >= 0 ? ocol : 0);
  const int d1 = (orow >= 0 || ocol >= 0) ? d0 + 1 : nd;
  // GFH_ASM_CHUNK datasets per step: the index and value loads of a step are independent of each other (a
  // global x global entry walks all datasets, and one dependent load chain per dataset made k_assemble
  // 21 us at 64 datasets); the additions keep the dataset order
  double s = 0.0;
  for (int d = d0; d < d1; d += GFH_ASM_CHUNK) {
    double v[GFH_ASM_CHUNK]; bool ok[GFH_ASM_CHUNK];
#pragma unroll
    for (int u = 0; u < GFH_ASM_CHUNK; u++) {
      ok[u] = d + u < d1;
      const int a = ok[u] ? inv[(d + u) * dim + row] : -1, b = ok[u] ? inv[(d + u) * dim + col] : -1;
      ok[u] = a >= 0 && b >= 0;
      v[u] = ok[u] ? G[(long long)(d + u) * gw + gram_entry(a, b, T)] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < GFH_ASM_CHUNK; u++) if (ok[u]) s += v[u];
  }
  return s;
}

// J^T r element of a row
GFH_HD_INLINE double walk_jtr(const double* __restrict__ G, const int gw, const int T, const int nd, const int dim,
                              const int* __restrict__ inv, const int* __restrict__ owner, const int row) {
  const int orow = owner[row];
  const int d0 = orow >= 0 ? orow : 0, d1 = orow >= 0 ? orow + 1 : nd;
  double s = 0.0;
  for (int d = d0; d < d1; d += GFH_ASM_CHUNK) {
    double v[GFH_ASM_CHUNK]; bool ok[GFH_ASM_CHUNK];
#pragma unroll
    for (int u = 0; u < GFH_ASM_CHUNK; u++) {
      const int a = d + u < d1 ? inv[(d + u) * dim + row] : -1;
      ok[u] = a >= 0;
      v[u] = ok[u] ? G[(long long)(d + u) * gw + gram_jtr(a, T)] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < GFH_ASM_CHUNK; u++) if (ok[u]) s += v[u];
  }
  return s;
}

// sum r^2 over all datasets
GFH_HD_INLINE double walk_rtr(const double* __restrict__ G, const int gw, const int T, const int nd) {
  double s = 0.0;
  for (int d = 0; d < nd; d += GFH_ASM_CHUNK) {
    double v[GFH_ASM_CHUNK];
#pragma unroll
    for (int u = 0; u < GFH_ASM_CHUNK; u++) v[u] = d + u < nd ? G[(long long)(d + u) * gw + gram_rtr(T)] : 0.0;
#pragma unroll
    for (int u = 0; u < GFH_ASM_CHUNK; u++) if (d + u < nd) s += v[u];
  }
  return s;
}

// The same element from its source list: m >= 0 is the offset of the single term in G; m < 0 (and not kGatherNoTerm) points at
// [count, offsets...] in `list`, the terms in dataset order, added in chunks of 16 independent loads.
constexpr int kGatherNoTerm = (int)0x80000000;
GFH_HD_INLINE double gather_sum(const double* __restrict__ G, const int m, const int* __restrict__ list) {
  double s = 0.0;
  if (m >= 0) s += G[m];
  else if (m != kGatherNoTerm) {
    const int* __restrict__ L = list + (-(m + 1));
    const int cnt = L[0];
    for (int k = 0; k < cnt; k += 16) {
      int o[16]; double v[16];
#pragma unroll
      for (int u = 0; u < 16; u++) o[u] = k + u < cnt ? L[1 + k + u] : -1;
#pragma unroll
      for (int u = 0; u < 16; u++) v[u] = o[u] >= 0 ? G[o[u]] : 0.0;
#pragma unroll
      for (int u = 0; u < 16; u++) if (o[u] >= 0) s += v[u];
    }
  }
  return s;
}

}  // namespace gfh
