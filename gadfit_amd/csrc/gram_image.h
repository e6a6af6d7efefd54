// gram_image.h -- the layout of one Gram image, stated once: what a Gram kernel writes per workgroup (`partial`), what
// k_reduce_partials sums per dataset (`G`) and what the assembling kernels and the host-built source lists of k_gather_sum read.
//   [pair (ti <= tj) of 16-row tiles][16][16] row-major, pairs row by row of the upper triangle | J^T r [16 T] | sum r^2 | pad to 4
// Plain C++: host code includes it as it is, device code gets the same functions as __host__ __device__.  No HIP header.
#pragma once

#if defined(__HIPCC__)
#define GFH_HD __host__ __device__ __attribute__((always_inline))      // (inlined before anything else: a kernel compiles as if it spelled the offset out)
#else
#define GFH_HD
#endif

namespace gfh {

GFH_HD constexpr int gram_npair(int T) { return T * (T + 1) / 2; }
// index of (i <= j) in the upper triangle of an n x n matrix stored row by row: the pair index of tiles (ti, tj) at n = T
GFH_HD constexpr int gram_pair(int ti, int tj, int T) { return ti * T - ti * (ti - 1) / 2 + (tj - ti); }
// tile p and its element (row, col)
GFH_HD constexpr int gram_tile(int p) { return p * 256; }
GFH_HD constexpr int gram_tile_at(int p, int row, int col) { return gram_tile(p) + row * 16 + col; }
// entry (a, b) of the dataset's J^T J, a and b local active indices: the upper triangle of tile pairs is stored
GFH_HD constexpr int gram_entry(int a, int b, int T) {
  if (a > b) { const int t = a; a = b; b = t; }
  return gram_tile_at(gram_pair(a >> 4, b >> 4, T), a & 15, b & 15);
}
GFH_HD constexpr int gram_jtr(int a, int T) { return gram_tile(gram_npair(T)) + a; }
GFH_HD constexpr int gram_rtr(int T) { return gram_jtr(16 * T, T); }
// doubles per image for T 16-row tiles
GFH_HD constexpr int gram_partial_stride(int T) { return (gram_rtr(T) + 1 + 3) & ~3; }

}  // namespace gfh
