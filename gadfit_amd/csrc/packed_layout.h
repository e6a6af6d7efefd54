// packed_layout.h -- the layout of the packed image and the source lists that k_gather_sum forms it from.  Needs no context and no
// HIP header: prepare_active (active.cpp) uploads what these functions return, gfh_debug_packed_layout hashes it, and
// tests/host/packed_image_main.cpp runs them as a stand-alone program.
//
// What the ranks all-reduce after a sweep is the image `packed`: [JTJ (dim*dim, column-major) | JTres | chi2], or for global
// fits beyond the in-kernel tail's reach the pattern-only [nnz values | JTres | chi2].  ncclAllReduce needs the same length
// and the same meaning of every element on every rank, so the layout may depend only on what all ranks share -- the column
// map, dim, the number of datasets -- never on which points (or whether any) THIS rank holds.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

namespace gfh {

struct PackedLayout {
  std::vector<int> inv, owner, nz_row, nz_col;
  bool sparse = false;         // the pattern is a quarter of the dense image or less
  bool small = false;          // dim*dim*n_datasets <= 65536: dense image, assembled by the fused kernel's tail where it applies
  int nnz = 0;
  bool transfer_sparse() const { return sparse && !small; }
  size_t packed_n(int dim) const { return transfer_sparse() ? (size_t)nnz + dim + 1 : (size_t)dim * dim + dim + 1; }
};

// inv, owner and the pattern from the column map jac[nd][na]; false with *err set for a column outside [0, dim)
bool compute_layout(int nd, int na, const int32_t* jac, int dim, bool sparse_ok, PackedLayout* L, std::string* err);

// Source lists for k_gather_sum: where in G (the per-dataset Gram images, [nd][gram_partial_stride(T)]) the terms of every element of
// the packed image sit, in dataset order -- what k_assemble / k_assemble_sparse find through owner/inv at run time (packed_walk.h
// states both, and what meta and list mean).  Built for the layout the launch chain will use: pattern-only or dense.
// False, with nothing built, where an offset would not fit an int or the image has more than 2^18 elements: the chain then assembles.
bool build_gather_lists(const PackedLayout& L, int nd, int dim, int T, std::vector<int>* meta, std::vector<int>* list);

}  // namespace gfh
