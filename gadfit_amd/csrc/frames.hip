// frames.hip -- a piece of a frame-major stack into the cube the batch kernels read (gfh_batch_frames_put, batch_frames.cpp): the
// stage holds frames [first_frame, first_frame + n_frames) as they arrived, stage[n_frames][n_fits] with the fit index fastest; the
// cube is spectrum-major, cube[n_fits][n_points].  A transpose through LDS and nothing else: the elements move as integers of their
// width (2, 4 or 8 bytes), so NaN payloads, -0.0 and denormals arrive as they left, and no model enters.
//
// One 64 x 64 tile per trip of a workgroup of 256 (four waves).  Phase 1: wave r reads row p0 + r, r + 4, ... of the stage, lane
// t the fit f0 + t -- 64 consecutive elements per wave and load.  Phase 2: wave r writes row f0 + r, r + 4, ... of the cube, lane t
// the point first_frame + p0 + t -- again 64 consecutive elements.  In between the tile lies in LDS with its rows padded by one
// element (65), which spreads phase 2's column read over the banks (an unpadded row of 64 four-byte elements puts a column on one).
// Every access is of the element's own width, so a cube row may start on any boundary the element's alignment allows (an odd n_points
// puts every other uint16 row on an odd 2-byte boundary).
//
// All index products are 64-bit: f * n_points passes 2^31 from row 65536 on at 32769 points, p * n_fits for a large piece.  The tiles
// are walked by a bounded one-dimensional grid with a loop over a 64-bit tile index, the frame axis fastest (neighbouring workgroups
// write neighbouring stretches of the same cube rows), so neither HIP's limit on a grid dimension nor the 65535 of gridDim.y caps
// n_fits or n_frames.  The trip count depends on blockIdx alone and both barriers stand outside every edge guard: all 256 threads
// of a workgroup reach each of them, whatever part of the tile lies inside the piece.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace gfh {

namespace {
constexpr int kFrameTile = 64;
constexpr unsigned kFrameGridMax = 1u << 16;      // workgroups per launch at the most; the rest of the tiles by the loop

template <class T>
__global__ __launch_bounds__(256) void k_frames_to_cube(const T* __restrict__ stage, const i64 n_frames, const i64 n_fits,
                                                        T* __restrict__ cube, const i64 n_points, const i64 first_frame,
                                                        const i64 tiles_p, const i64 n_tiles) {
  __shared__ T tile[kFrameTile][kFrameTile + 1];
  const int t = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  for (i64 k = blockIdx.x; k < n_tiles; k += gridDim.x) {
    const i64 p0 = (k % tiles_p) * kFrameTile, f0 = (k / tiles_p) * kFrameTile;
    for (int r = r0; r < kFrameTile; r += 4) {
      const i64 p = p0 + r, f = f0 + t;
      if (p < n_frames && f < n_fits) tile[r][t] = stage[p * n_fits + f];
    }
    __syncthreads();
    for (int r = r0; r < kFrameTile; r += 4) {
      const i64 f = f0 + r, p = p0 + t;
      if (f < n_fits && p < n_frames) cube[f * n_points + first_frame + p] = tile[t][r];
    }
    __syncthreads();      // (the next trip writes the tile again)
  }
}

template <class T>
hipError_t launch_typed(hipStream_t st, const void* stage, i64 n_frames, i64 n_fits, void* cube, i64 n_points, i64 first_frame) {
  const i64 tiles_p = (n_frames + kFrameTile - 1) / kFrameTile, tiles_f = (n_fits + kFrameTile - 1) / kFrameTile;
  const i64 n_tiles = tiles_p * tiles_f;
  const unsigned grid = (unsigned)(n_tiles < (i64)kFrameGridMax ? n_tiles : (i64)kFrameGridMax);
  hipLaunchKernelGGL(k_frames_to_cube<T>, dim3(grid), dim3(256), 0, st, static_cast<const T*>(stage), n_frames, n_fits,
                     static_cast<T*>(cube), n_points, first_frame, tiles_p, n_tiles);
  return hipGetLastError();
}
}  // namespace

// stage [n_frames][n_fits] -> cube [n_fits][n_points] at columns [first_frame, first_frame + n_frames), elements of elem_bytes
// (2, 4 or 8).  The caller has checked 1 <= n_frames, 0 <= first_frame, first_frame + n_frames <= n_points and 1 <= n_fits: the
// kernel's guards keep every access inside stage and inside those columns of the cube's n_fits rows.
hipError_t launch_frames_to_cube(hipStream_t st, int elem_bytes, const void* stage, i64 n_frames, i64 n_fits, void* cube,
                                 i64 n_points, i64 first_frame) {
  if (n_frames < 1 || n_fits < 1 || first_frame < 0 || first_frame + n_frames > n_points) return hipErrorInvalidValue;
  if (elem_bytes == 2) return launch_typed<uint16_t>(st, stage, n_frames, n_fits, cube, n_points, first_frame);
  if (elem_bytes == 4) return launch_typed<uint32_t>(st, stage, n_frames, n_fits, cube, n_points, first_frame);
  if (elem_bytes == 8) return launch_typed<uint64_t>(st, stage, n_frames, n_fits, cube, n_points, first_frame);
  return hipErrorInvalidValue;
}

}  // namespace gfh
