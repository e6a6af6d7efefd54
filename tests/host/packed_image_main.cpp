// packed_image_main.cpp -- "same terms, same order" of the packed image as a program of its own.  The three ways the library forms
// an element of [J^T J or its pattern | J^T r | chi2] from the per-dataset Gram images are run on the host, over random images, and
// compared bit for bit:
//   (a) the walks through owner / inv (packed_walk.h) as k_assemble maps them for the dense image and k_assemble_sparse for the pattern,
//   (b) the source lists of build_gather_lists (packed_layout.cpp) summed by gather_sum, as k_gather_sum does,
//   (c) a naive loop over the datasets in order, with the offset into the Gram image counted out instead of computed.
// Built from gram_image.h, packed_walk.h and packed_layout.cpp alone: no context, no HIP header.  tests/test_cpu_packed_image_host.py
// compiles it under AddressSanitizer and UBSan (a source offset that leaves G is a finding); exit status 0 = every element agreed.
#include "gram_image.h"
#include "packed_walk.h"
#include "packed_layout.cpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace gfh;

namespace {

int failures = 0;

void expect(bool ok, const std::string& what) {
  if (!ok) { printf("FAILED: %s\n", what.c_str()); failures++; }
}

// values whose sum depends on the order of the additions: mixed signs, magnitudes over twelve decades
struct Rng {
  uint64_t s = 0x9e3779b97f4a7c15ull;
  uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
  double value() {
    const uint64_t r = next();
    double v = (double)(r >> 11) / 9007199254740992.0 - 0.5;
    for (unsigned k = (unsigned)(r & 15u); k > 3; k--) v *= 10.0;
    return v;
  }
};

bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

// the offset of entry (a, b) without gram_image.h: the pairs before (ti, tj) counted row by row of the upper triangle
int naive_entry(int a, int b, int T) {
  if (a > b) std::swap(a, b);
  const int ti = a / 16, tj = b / 16;
  int p = 0;
  for (int i = 0; i < ti; i++) p += T - i;
  p += tj - ti;
  return p * 256 + (a % 16) * 16 + b % 16;
}

// jac[nd][na] is the column map of one case; pattern = what the layout should come out as
void run_case(const char* name, int nd, int na, int dim, const std::vector<int32_t>& jac, bool sparse_ok, bool pattern) {
  const std::string tag = std::string(name) + (pattern ? " (pattern)" : " (dense)");
  PackedLayout L; std::string err;
  if (!compute_layout(nd, na, jac.data(), dim, sparse_ok, &L, &err)) { expect(false, tag + ": compute_layout: " + err); return; }
  expect(L.transfer_sparse() == pattern, tag + ": the form of the image");
  const int T = (na + 15) / 16, gw = gram_partial_stride(T), tiles = T * (T + 1) / 2 * 256;
  expect(gw % 4 == 0 && gw >= tiles + 16 * T + 1 && gw < tiles + 16 * T + 1 + 4, tag + ": stride");
  std::vector<int> meta, list;
  if (!build_gather_lists(L, nd, dim, T, &meta, &list)) { expect(false, tag + ": no source lists"); return; }
  const size_t n = L.packed_n(dim);
  expect(meta.size() == n, tag + ": length of meta");

  Rng rng;
  std::vector<double> G((size_t)nd * gw);
  for (double& g : G) g = rng.value();
  const int* inv = L.inv.data(); const int* owner = L.owner.data();

  auto naive_pair = [&](int row, int col) {
    double s = 0.0;
    for (int d = 0; d < nd; d++) {
      const int a = inv[(size_t)d * dim + row], b = inv[(size_t)d * dim + col];
      if (a >= 0 && b >= 0) s += G[(size_t)d * gw + naive_entry(a, b, T)];
    }
    return s;
  };
  int bad = 0;
  auto check = [&](size_t idx, double walked, double naive) {
    const double gathered = gather_sum(G.data(), meta[idx], list.data());
    if (!(same_bits(walked, gathered) && same_bits(walked, naive)) && bad++ < 5)
      printf("FAILED: %s: element %zu: walk %.17g, gather %.17g, naive %.17g\n", tag.c_str(), idx, walked, gathered, naive);
  };
  size_t nn;
  if (pattern) {          // k_assemble_sparse: thread idx < nnz takes entry (nz_row, nz_col)
    nn = (size_t)L.nnz;
    for (int k = 0; k < L.nnz; k++)
      check((size_t)k, walk_entry(G.data(), gw, T, nd, dim, inv, owner, L.nz_row[k], L.nz_col[k]), naive_pair(L.nz_row[k], L.nz_col[k]));
  } else {                // k_assemble: blockIdx.y = column, threads = rows, column-major
    nn = (size_t)dim * dim;
    for (int col = 0; col < dim; col++)
      for (int row = 0; row < dim; row++)
        check((size_t)col * dim + row, walk_entry(G.data(), gw, T, nd, dim, inv, owner, row, col), naive_pair(row, col));
  }
  for (int row = 0; row < dim; row++) {
    double s = 0.0;
    for (int d = 0; d < nd; d++) { const int a = inv[(size_t)d * dim + row]; if (a >= 0) s += G[(size_t)d * gw + tiles + a]; }
    check(nn + row, walk_jtr(G.data(), gw, T, nd, dim, inv, owner, row), s);
  }
  double s = 0.0;
  for (int d = 0; d < nd; d++) s += G[(size_t)d * gw + tiles + 16 * T];
  check(nn + dim, walk_rtr(G.data(), gw, T, nd), s);
  expect(nn + dim + 1 == n, tag + ": length of the image");
  failures += bad;
  printf("%-58s %6zu elements, %5zu list entries: %s\n", tag.c_str(), n, list.size(), bad ? "DIFFER" : "equal bits");
}

// nd datasets of n_glob shared columns (0 .. n_glob-1) followed by n_loc columns of their own
std::vector<int32_t> global_local(int nd, int n_glob, int n_loc, int* dim) {
  std::vector<int32_t> jac;
  for (int d = 0; d < nd; d++) {
    for (int k = 0; k < n_glob; k++) jac.push_back(k);
    for (int k = 0; k < n_loc; k++) jac.push_back(n_glob + d * n_loc + k);
  }
  *dim = n_glob + nd * n_loc;
  return jac;
}

}  // namespace

int main() {
  int dim;
  std::vector<int32_t> jac;
  // one dataset, two tiles: the pair index and the a > b swap
  jac = global_local(1, 17, 0, &dim);
  run_case("17 active, one dataset", 1, 17, dim, jac, true, false);
  // T = 3: an off-diagonal pair behind a full row of pairs
  jac = global_local(1, 33, 0, &dim);
  run_case("33 active, one dataset", 1, 33, dim, jac, true, false);
  // a global column over 9 datasets: a second, partly filled chunk of 8 in the walks
  jac = global_local(9, 1, 1, &dim);
  run_case("9 datasets, one global column", 9, 2, dim, jac, true, false);
  // over 17 datasets: a second chunk of 16 in the gather
  jac = global_local(17, 1, 1, &dim);
  run_case("17 datasets, one global column", 17, 2, dim, jac, true, false);
  // local and global columns: owner collapses the walk of every entry with a local row or column
  jac = global_local(3, 2, 2, &dim);
  run_case("3 datasets, global and local columns", 3, 4, dim, jac, true, false);
  // column 0 belongs to datasets 0 and 2: inv = -1 in the middle of its walk
  jac = {0, 1, 2, 3, 0, 4};
  run_case("a column two of three datasets use", 3, 2, 5, jac, true, false);
  // 17 datasets of one global and four local columns: beyond the small image, so the pattern travels; and the same layout dense
  jac = global_local(17, 1, 4, &dim);
  run_case("17 datasets, 1 + 4 columns", 17, 5, dim, jac, true, true);
  run_case("17 datasets, 1 + 4 columns", 17, 5, dim, jac, false, false);
  // a column outside the system is refused with a message
  { PackedLayout L; std::string err; const int32_t out_of_range[2] = {0, 2};
    expect(!compute_layout(1, 2, out_of_range, 2, true, &L, &err) && !err.empty(), "a column index past dim is refused"); }
  printf(failures ? "packed image: %d failure(s)\n" : "packed image: all equal\n", failures);
  return failures ? 1 : 0;
}
