// batch_data.cpp -- the batch of independent fits that a context holds: the spectra back to back (gfh_set_batch_data), a cube on one
// grid with narrow samples (gfh_set_batch_cube), or that cube from a frame-major stack, transposed on the device by frames.hip
// (gfh_batch_frames_begin, gfh_batch_frames_put, gfh_set_batch_frames).  Every setter checks its arguments, replaces the batch held
// and records the new geometry and form on the host before the device is asked for, so a compile-only context ends in "no GPU" with
// the geometry known to the argument checks of the calls (batch_calls.cpp).
#include "batch_internal.h"
#include <algorithm>
#include <exception>

using namespace gfh;

int gfh::check_context(gfh_ctx* c, const char* who) {
  if (!c) return 1;
  const std::string w(who);
  if (c->grp) return fail(c, w + " is not available on a device-group handle (the fits are independent: split the batch over the members' contexts)");
  if (c->nranks > 1) return fail(c, w + " is not available on a context with a communicator of more than one rank (the fits are independent: split the batch)");
  return 0;
}
// what gfh_debug_batch_form reports and the kernel cache keys on
int gfh::data_form(const gfh_ctx* c) { return c->batch.cube ? 1 + c->batch.y_type + 3 * c->batch.error_type : 0; }

namespace {

constexpr size_t elem_bytes(int y_type) { return y_type == 0 ? 8 : y_type == 1 ? 4 : 2; }
// The largest staging of gfh_set_batch_frames' default pieces (frames_per_put 0), samples and USER weights together.  Kept at the
// 256 MiB it was proposed with: every stack of the measured table (profiles/batch_frames.json; at most 262 MB)
// is ONE put under it, so the default there is the single put it was to be compared with, and the same stacks cut into eight puts
// took 0.15 ... 0.3 ms longer (about 30 us per further put) -- a stack above the bound pays that per 256 MiB, against 5 ms of upload.
// The measurement gave no reason for another value; it does not hold a smaller one to be worse by more than that.
constexpr int64_t kFramesStageBytes = (int64_t)256 << 20;

// on what context and what a cube can be, for the three calls that make one (gfh_set_batch_cube, gfh_batch_frames_begin,
// gfh_set_batch_frames): one order, one wording, each under its own name.  null_arg: a required pointer is NULL, `required` names them; has_w: -1 the call takes no w
int check_cube(gfh_ctx* c, const char* who, bool null_arg, const char* required, int64_t n_fits, int64_t n_points, int y_type, int error_type,
               int has_w) {
  if (check_context(c, who)) return 1;
  const std::string w(who);
  if (null_arg) return fail(c, w + ": null argument (" + required + " required)");
  if (n_fits < 1) return fail(c, w + ": a batch holds at least one fit");
  if (n_points < 1) return fail(c, w + ": a spectrum holds at least one point");
  if (n_fits > ((int64_t)1 << 31) - 4) return fail(c, w + ": more fits than one launch takes (2^31 - 4)");
  if (y_type < 0 || y_type > 2) return fail(c, w + ": unknown y_type " + std::to_string(y_type) + " (0 double, 1 float, 2 uint16_t)");
  if (error_type < 0 || error_type > 4)
    return fail(c, w + ": unknown error_type " + std::to_string(error_type) + " (0 NONE, 1 SQRT_Y, 2 PROPTO_Y, 3 INVERSE_Y, 4 USER)");
  if (has_w >= 0 && error_type == 4 && !has_w) return fail(c, w + ": error_type USER needs the weights w");
  if (has_w >= 0 && error_type != 4 && has_w) return fail(c, w + ": w is taken under error_type USER alone (the other types form the weights from y on the device)");
  if (n_points > INT64_MAX / 8 / n_fits) return fail(c, w + ": n_fits x n_points overflows");
  return 0;
}

// Replaces the batch held, on the host alone: waits for a pending upload, drains the stream if data is on the device, frees the
// blocks, ends a begun stack and records the new geometry and form -- ragged with its offsets, or (offsets NULL) a cube of
// shortest = longest = n_points in y_type under error_type.  The callers ask for the device after it.
int replace_batch(gfh_ctx* c, int64_t n_fits, const int64_t* offsets, int64_t shortest, int64_t longest, int y_type, int error_type) {
  if (join_pending(c)) return 1;
  if (c->device >= 0 && c->batch.on_device) { hipSetDevice(c->device); if (c->stream) hipStreamSynchronize(c->stream); }
  batch_free(c);
  c->batch.frames = false; c->batch.frame_put.clear(); c->batch.frames_missing = 0; c->batch.frames_kernel_ms = 0.0;
  c->batch.cube = !offsets; c->batch.y_type = y_type; c->batch.error_type = error_type;
  c->batch.n_fits = n_fits; c->batch.min_points = shortest; c->batch.max_points = longest;
  if (offsets) c->batch.off.assign(offsets, offsets + n_fits + 1); else c->batch.off.clear();
  return 0;
}
// the blocks of the cube held -- the grid, the samples in their type, the weights under USER alone -- and its grid on the stream
int cube_blocks(gfh_ctx* c, const double* x) {
  NEED_GPU(c);
  const size_t np = (size_t)c->batch.max_points, n = (size_t)c->batch.n_fits * np;
  if (dev_alloc(c, c->batch.x, sizeof(double) * np) || dev_alloc(c, c->batch.y, n * elem_bytes(c->batch.y_type))) return 1;
  if (c->batch.error_type == 4 && dev_alloc(c, c->batch.w, sizeof(double) * n)) return 1;
  copy_path_ready();
  HIPCHK(c, hipMemcpyAsync(c->batch.x.p, x, sizeof(double) * np, hipMemcpyHostToDevice, c->stream));
  return 0;
}

}  // namespace

extern "C" {

// The spectra of a batch, back to back: fit f owns points [offsets[f], offsets[f + 1]) of x, y, w (w: the weights as used in
// (y - f) * w, gadfit.F90:682-683).
int gfh_set_batch_data(gfh_ctx* c, int64_t n_fits, const int64_t* offsets, const double* x, const double* y, const double* w) try {
  if (check_context(c, "gfh_set_batch_data")) return 1;
  if (n_fits < 1) return fail(c, "gfh_set_batch_data: a batch holds at least one fit");
  if (n_fits > ((int64_t)1 << 31) - 4) return fail(c, "gfh_set_batch_data: more fits than one launch takes (2^31 - 4)");
  if (!offsets || !x || !y || !w) return fail(c, "gfh_set_batch_data: null argument");
  if (offsets[0] != 0) return fail(c, "gfh_set_batch_data: offsets must begin at 0");
  int64_t shortest = offsets[1] - offsets[0], longest = shortest;
  for (int64_t f = 0; f < n_fits; f++) {
    if (offsets[f + 1] < offsets[f]) return fail(c, "gfh_set_batch_data: offsets must ascend (fit " + std::to_string((long long)f) + " ends before it begins)");
    shortest = std::min(shortest, offsets[f + 1] - offsets[f]); longest = std::max(longest, offsets[f + 1] - offsets[f]);
  }
  if (replace_batch(c, n_fits, offsets, shortest, longest, 0, 0)) return 1;
  NEED_GPU(c);
  const size_t n = (size_t)offsets[n_fits], nb = sizeof(double) * std::max<size_t>(n, 1);
  if (dev_alloc(c, c->batch.x, nb) || dev_alloc(c, c->batch.y, nb) || dev_alloc(c, c->batch.w, nb) ||
      dev_alloc(c, c->batch.off_d, sizeof(int64_t) * (size_t)(n_fits + 1))) return 1;
  copy_path_ready();
  if (n) {
    HIPCHK(c, hipMemcpyAsync(c->batch.x.p, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->batch.y.p, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->batch.w.p, w, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(c->batch.off_d.p, offsets, sizeof(int64_t) * (size_t)(n_fits + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch.on_device = true;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_batch_data: ") + e.what()); }

// The same batch as a cube (include/gadfit_hip.h): one grid x [n_points] for every spectrum, the samples y [n_fits][n_points] in
// y_type (0 double, 1 float, 2 uint16_t), the weights formed in the kernels' load by error_type's rule -- no weight array anywhere --
// or, under USER (4), w [n_fits][n_points] as used.  The calls work on whichever data is held: a cube's kernels are translation
// units of their own.
int gfh_set_batch_cube(gfh_ctx* c, int64_t n_fits, int64_t n_points, const double* x, const void* y, int y_type, int error_type,
                       const double* w) try {
  if (check_cube(c, "gfh_set_batch_cube", !x || !y, "x and y are", n_fits, n_points, y_type, error_type, w != nullptr)) return 1;
  if (replace_batch(c, n_fits, nullptr, n_points, n_points, y_type, error_type) || cube_blocks(c, x)) return 1;
  const size_t n = (size_t)n_fits * (size_t)n_points;
  HIPCHK(c, hipMemcpyAsync(c->batch.y.p, y, n * elem_bytes(y_type), hipMemcpyHostToDevice, c->stream));
  if (w) HIPCHK(c, hipMemcpyAsync(c->batch.w.p, w, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch.on_device = true;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_batch_cube: ") + e.what()); }

// A cube that arrives frame by frame (include/gadfit_hip.h): instruments deliver F [n_points][n_fits], one image per abscissa with
// the pixel index fastest.  begin is gfh_set_batch_cube without the samples -- the same checks, the same state, the same blocks --
// and marks every frame as missing; gfh_batch_frames_put uploads a piece as it is stored and k_frames_to_cube (frames.hip)
// transposes it into the cube's columns.  Once no frame is missing nothing downstream knows where the cube came from.
int gfh_batch_frames_begin(gfh_ctx* c, int64_t n_fits, int64_t n_points, const double* x, int y_type, int error_type) try {
  if (check_cube(c, "gfh_batch_frames_begin", !x, "x is", n_fits, n_points, y_type, error_type, -1)) return 1;
  std::vector<unsigned char> flags((size_t)n_points, 0);          // (before anything is replaced: this can fail)
  if (replace_batch(c, n_fits, nullptr, n_points, n_points, y_type, error_type)) return 1;
  c->batch.frames = true; c->batch.frame_put.swap(flags); c->batch.frames_missing = n_points;
  if (cube_blocks(c, x)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch.on_device = true;
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_frames_begin: ") + e.what()); }

// Frames [first_frame, first_frame + n_frames) of the begun batch: y [n_frames][n_fits] in the begun sample type, w alike as doubles
// under USER.  In any order and any piece sizes; a frame put again holds the later data.  The piece is staged in blocks of its own
// size, which go when no frame is missing; the call returns after the stream has drained, so the caller's buffers are free again.
int gfh_batch_frames_put(gfh_ctx* c, int64_t first_frame, int64_t n_frames, const void* y, const double* w) try {
  if (check_context(c, "gfh_batch_frames_put")) return 1;
  if (!c->batch.frames)
    return fail(c, "gfh_batch_frames_put: no batch has been begun (gfh_batch_frames_begin; gfh_set_batch_data and gfh_set_batch_cube replace a begun batch)");
  const int64_t n_fits = c->batch.n_fits, n_points = c->batch.max_points;
  if (first_frame < 0) return fail(c, "gfh_batch_frames_put: first_frame is negative (" + std::to_string((long long)first_frame) + ")");
  if (n_frames < 1) return fail(c, "gfh_batch_frames_put: a piece holds at least one frame");
  if (first_frame > n_points - n_frames)
    return fail(c, "gfh_batch_frames_put: frames [" + std::to_string((long long)first_frame) + ", " + std::to_string((long long)first_frame) + " + " +
                   std::to_string((long long)n_frames) + ") reach past the " + std::to_string((long long)n_points) + " frames of the batch");
  if (!y) return fail(c, "gfh_batch_frames_put: null argument (y is required)");
  if (c->batch.error_type == 4 && !w) return fail(c, "gfh_batch_frames_put: error_type USER needs the weights w");
  if (c->batch.error_type != 4 && w) return fail(c, "gfh_batch_frames_put: w is taken under error_type USER alone (the other types form the weights from y on the device)");
  NEED_GPU(c);
  if (!c->batch.on_device) return fail(c, "gfh_batch_frames_put: the begun batch is not on the device (gfh_batch_frames_begin failed)");
  const size_t eb = elem_bytes(c->batch.y_type), ne = (size_t)n_frames * (size_t)n_fits;
  if (dev_alloc(c, c->batch.stage_y, ne * eb)) return 1;
  if (w && dev_alloc(c, c->batch.stage_w, ne * sizeof(double))) return 1;
  copy_path_ready();
  harvest_events(c);
  HIPCHK(c, hipMemcpyAsync(c->batch.stage_y.p, y, ne * eb, hipMemcpyHostToDevice, c->stream));
  if (w) HIPCHK(c, hipMemcpyAsync(c->batch.stage_w.p, w, ne * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  HIPCHK(c, launch_frames_to_cube(c->stream, (int)eb, c->batch.stage_y.p, n_frames, n_fits, c->batch.y.p, n_points, first_frame));
  if (w) HIPCHK(c, launch_frames_to_cube(c->stream, 8, c->batch.stage_w.p, n_frames, n_fits, c->batch.w.p, n_points, first_frame));
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch.frames_kernel_ms += ev_ms(c->ev[0], c->ev[1]);
  for (int64_t p = first_frame; p < first_frame + n_frames; p++)
    if (!c->batch.frame_put[(size_t)p]) { c->batch.frame_put[(size_t)p] = 1; c->batch.frames_missing--; }
  if (c->batch.frames_missing == 0) { dev_free(c->batch.stage_y); dev_free(c->batch.stage_w); }
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_batch_frames_put: ") + e.what()); }

// begin + puts of a whole stack y [n_points][n_fits] (w alike under USER), frames_per_put frames each; 0: the largest count whose
// staging -- samples and weights -- stays within kFramesStageBytes, but at least one frame
int gfh_set_batch_frames(gfh_ctx* c, int64_t n_fits, int64_t n_points, const double* x, const void* y, int y_type, int error_type,
                         const double* w, int64_t frames_per_put) try {
  if (check_cube(c, "gfh_set_batch_frames", !x || !y, "x and y are", n_fits, n_points, y_type, error_type, w != nullptr)) return 1;
  if (frames_per_put < 0) return fail(c, "gfh_set_batch_frames: frames_per_put is negative (0: pieces of at most " +
                                         std::to_string((long long)(kFramesStageBytes >> 20)) + " MiB of staging)");
  if (gfh_batch_frames_begin(c, n_fits, n_points, x, y_type, error_type)) return 1;
  const int64_t per_frame = n_fits * (int64_t)(elem_bytes(y_type) + (w ? sizeof(double) : 0));
  const int64_t step = frames_per_put ? frames_per_put : std::max<int64_t>(1, kFramesStageBytes / per_frame);
  for (int64_t p = 0, k; p < n_points; p += k) {
    k = std::min(step, n_points - p);
    if (gfh_batch_frames_put(c, p, k, static_cast<const char*>(y) + (size_t)p * (size_t)n_fits * elem_bytes(y_type),
                             w ? w + (size_t)p * (size_t)n_fits : nullptr)) return 1;
  }
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_set_batch_frames: ") + e.what()); }

// frames of the begun batch not yet put; -1: the batch held was not begun by gfh_batch_frames_begin
int64_t gfh_debug_batch_frames_missing(gfh_ctx* c) { return c && c->batch.frames ? c->batch.frames_missing : -1; }
// device time of the transposing kernels of every put since the last gfh_batch_frames_begin, in seconds (HIP events)
double gfh_debug_batch_frames_seconds(gfh_ctx* c) { return c && c->batch.frames ? 1e-3 * c->batch.frames_kernel_ms : 0.0; }

// Elements [first, first + count) of the cube held, as stored (row-major [n_fits][n_points]): which 0 the samples in their type, 1
// the USER weights as doubles.  For tests that hold the cube's bytes; frames not yet put read as whatever the block held.
int gfh_debug_batch_read(gfh_ctx* c, int which, int64_t first, int64_t count, void* dst) try {
  if (check_context(c, "gfh_debug_batch_read")) return 1;
  if (c->batch.n_fits < 1 || !c->batch.cube) return fail(c, "gfh_debug_batch_read: the context holds no cube (gfh_set_batch_cube, gfh_batch_frames_begin)");
  if (which != 0 && which != 1) return fail(c, "gfh_debug_batch_read: which is 0 (the samples) or 1 (the USER weights)");
  if (which == 1 && c->batch.error_type != 4) return fail(c, "gfh_debug_batch_read: the cube holds weights under error_type USER alone");
  if (first < 0 || count < 0 || first > c->batch.n_fits * c->batch.max_points - count)
    return fail(c, "gfh_debug_batch_read: elements [first, first + count) reach past the cube");
  if (!dst) return fail(c, "gfh_debug_batch_read: null argument");
  NEED_GPU(c);
  if (!c->batch.on_device) return fail(c, "gfh_debug_batch_read: no batch data on the device");
  const size_t eb = which ? sizeof(double) : elem_bytes(c->batch.y_type);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (count) HIPCHK(c, hipMemcpy(dst, (which ? c->batch.w : c->batch.y).as<char>() + (size_t)first * eb, (size_t)count * eb, hipMemcpyDeviceToHost));
  return 0;
} catch (const std::exception& e) { return fail(c, std::string("gfh_debug_batch_read: ") + e.what()); }

}  // extern "C"
