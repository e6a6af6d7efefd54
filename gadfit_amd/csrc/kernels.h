// kernels.h -- launchers of the static (model-independent) kernels: gram.hip, assemble.hip, jtv.hip, frames.hip, kernels.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "gram_image.h"   // gram_partial_stride(T): doubles per workgroup partial for T 16-row tiles

namespace gfh {
typedef long long i64;

// one Gram launch as launch_gram notes it where it launches (gfh_debug_chain): kind 0 = k_gram_small<a>, 1 = k_gram<a>,
// 2 = k_gram_block<a, b, sym> at the tiles (r0, c0)
struct GramLaunch { int kind, a, b, sym, r0, c0; };
hipError_t launch_gram(hipStream_t st, int T, const double* J, i64 ldj, int na, const double* res,
                       const i64* gb_start, const int* gb_slots, int n_gb, double* partial, std::vector<GramLaunch>* note = nullptr);
hipError_t launch_reduce_partials(hipStream_t st, const double* partial, int pstride, int width,
                                  const int* ds_first_gb, int nd, double* out);
hipError_t launch_assemble(hipStream_t st, const double* G, int gw, int T, int nd, int dim, const int* inv, const int* owner, double* packed);
hipError_t launch_gather_sum(hipStream_t st, const double* G, const int* meta, const int* list, int n, double* out, const int* status,
                             double* host_out, unsigned* counter, unsigned long long* host_flag, unsigned long long seq);
hipError_t launch_assemble_sparse(hipStream_t st, const double* G, int gw, int T, int nd, int dim, const int* inv, const int* owner,
                                  const int* nz_row, const int* nz_col, int nnz, double* packed);
hipError_t launch_jtv(hipStream_t st, const double* J, i64 ldj, int na, const double* v, const i64* gb_start,
                      const int* gb_slots, int n_gb, double* partial, int pstride);
hipError_t launch_jtv_finish(hipStream_t st, const double* partial, int pstride, int na, const int* ds_first_gb, int nd, int dim,
                             const int* inv, double* out, const int* status, double* host_out, unsigned long long* host_flag,
                             unsigned long long seq);
hipError_t launch_assemble_vec(hipStream_t st, const double* V, int width, int nd, int dim, const int* inv, double* out);
hipError_t launch_cosphi(hipStream_t st, const double* J, i64 ldj, int na, const double* res, const double* dl,
                         const i64* gb_start, const int* gb_slots, const int* gb_ds, int n_gb, double* partial, int pstride);
hipError_t launch_publish(hipStream_t st, const double* src, int n, const int* status, double* host_out, unsigned* counter,
                          unsigned long long* host_flag, unsigned long long seq);
hipError_t launch_status_slot(hipStream_t st, const int* status, double* dst);
hipError_t launch_fill_pads(hipStream_t st, int nd, const i64* seg, double* x, double* y, double* w, unsigned char* is_pad);
// frames.hip: stage [n_frames][n_fits] transposed into columns [first_frame, first_frame + n_frames) of cube [n_fits][n_points];
// elem_bytes 2, 4 or 8
hipError_t launch_frames_to_cube(hipStream_t st, int elem_bytes, const void* stage, i64 n_frames, i64 n_fits, void* cube,
                                 i64 n_points, i64 first_frame);
hipError_t launch_init_weights(hipStream_t st, int type, i64 n, const double* y, double* w, const unsigned char* is_pad);
}  // namespace gfh
