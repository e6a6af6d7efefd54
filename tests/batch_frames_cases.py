"""The inputs of tests/test_gpu_batch_frames.py and tests/test_cpu_batch_frames.py: batches that arrive as stacks of frames
(gfh_batch_frames_begin, gfh_batch_frames_put, gfh_set_batch_frames) -- F [n_points][n_fits], one image per abscissa with the fit
index fastest, transposed into the cube on the device.  Everything here is deterministic and needs no GPU.

STACKS.  stack(n_points, n_fits, dtype, seed) is F [n_points][n_fits]: element i (row-major) takes the low 16, 32 or 64 bits of
splitmix64 value i of the seed SEED + FRAMES_SEED + seed, AS BITS -- so any two elements differ with all but negligible probability
and a misplaced one shows -- and is then viewed as uint16, float32 or float64.  In the float types the flat positions 3 + 11 k,
k = 0 ... 7, as far as the stack reaches, are overwritten with SPECIALS[dtype][k]: a quiet NaN with payload 1, a signalling NaN with a
payload, a negative NaN with a wide payload, +inf, -inf, -0.0, the smallest denormal and the negative largest denormal.  (Random bits
alone hold NaNs too: one float32 in 256.)  Stacks are compared as integers of their width (as_bits), never as floats: NaN != NaN, and
-0.0 == 0.0.
The USER weights of a uint16 stack are a float64 stack of another seed: for the bytes of the cube their meaning is irrelevant.

WHAT A STACK IS HELD AGAINST: np.ascontiguousarray(F.T) (cube_of), what set_batch_cube would have been given; for the fits, the
cubes of tests/batch_cube_cases.py and their transposes (frames_of), on the same context."""
import numpy as np

from tests import batch_cube_cases as CC
from tests import models as M
from tests.batch_common import COUNTS

FRAMES_SEED = 5000000
BYTE_FITS = (1, 2, 31, 32, 33, 63, 64, 65, 129, 257)        # both sides of a 32- and of a 64-wide tile, odd row alignments
BYTE_POINTS = (1, 2, 31, 32, 33, 63, 64, 65, 129)
PIECE_POINTS, PIECE_FITS = 130, 67
EDGES = (0, 1, 31, 32, 33, 63, 64, 65, 130)                  # p0 < p1 of the neighbour check, in a stack of 130 frames
EDGE_FITS = (65, 129)
_UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
SPECIALS = {
    np.dtype(np.float32): np.array([0x7fc00001, 0x7f800123, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff],
                                   dtype=np.uint32),
    np.dtype(np.float64): np.array([0x7ff8000000000001, 0x7ff0000000000123, 0xfff8123456789abc, 0x7ff0000000000000, 0xfff0000000000000,
                                    0x8000000000000000, 0x0000000000000001, 0x800fffffffffffff], dtype=np.uint64),
}
# the cube forms whose fits are held to set_batch_cube's bit for bit: (lanes, lengths, [(y_type number, error_type)])
FIT_FORMS = ((64, (5, 65), [(yt, et) for yt in range(3) for et in CC.ERROR_TYPES]),
             (16, (17,), [(CC.Y_TYPES.index(t), et) for t, et in CC.ORACLE_FORMS] + [(2, CC.USER)]),
             (256, (257,), [(CC.Y_TYPES.index(t), et) for t, et in CC.ORACLE_FORMS] + [(2, CC.USER)]))


def as_bits(a):
    """an array of 2-, 4- or 8-byte elements as unsigned integers of that width"""
    a = np.ascontiguousarray(a)
    return a.view(_UINT[a.dtype.itemsize])


def stack(n_points, n_fits, dtype, seed=0):
    dtype = np.dtype(dtype)
    n = n_points * n_fits
    bits = M.splitmix64(n, M.SEED + FRAMES_SEED + seed).astype(_UINT[dtype.itemsize])          # (astype of unsigned integers keeps the low bits)
    if dtype in SPECIALS:
        at = 3 + 11 * np.arange(8)
        at = at[at < n]
        bits[at] = SPECIALS[dtype][:at.size]
    F = bits.view(dtype).reshape(n_points, n_fits)
    F.setflags(write=False)
    return F


def cube_of(F):
    """what set_batch_cube would have been given: the host transpose the frames calls spare"""
    return np.ascontiguousarray(F.T)


def frames_of(Y):
    """a cube of tests/batch_cube_cases.py as the stack an instrument would have delivered"""
    return np.ascontiguousarray(np.asarray(Y).T)


def read_cube(ctx, n_fits, n_points, which=0):
    """the whole cube held, [n_fits][n_points], as stored (Context.debug_batch_read)"""
    return ctx.debug_batch_read(which, 0, n_fits * n_points).reshape(n_fits, n_points)


def same_bytes(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(as_bits(got), as_bits(want))


def same_fit(p, r, p0, r0):
    """two results of fit_batch bit for bit: the parameters, lambda and chi2 as bits, the five counts and dof"""
    assert np.array_equal(as_bits(p), as_bits(p0))
    for f in COUNTS + ('dof',):
        assert np.array_equal(r[f], r0[f]), f
    assert np.array_equal(as_bits(r['lambda_']), as_bits(r0['lambda_'])) and np.array_equal(as_bits(r['chi2']), as_bits(r0['chi2']))
