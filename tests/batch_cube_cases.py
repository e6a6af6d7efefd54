"""The inputs of tests/test_gpu_batch_cube.py and tests/test_cpu_batch_cube.py: batches as data cubes (gfh_set_batch_cube) -- every
spectrum on one abscissa grid, samples in float64, float32 or uint16, the weights formed from y on the device.  Everything here is
deterministic and needs no GPU; the scenarios, the bounds and the selection rule (select) are those of tests/batch_common.py and
tests/batch_cases.py, imported, not restated.

COUNTS.  For a length n one grid x_i = 0.5 + 99.5 (i + 0.5) / n and six spectra s = 0 ... 5 of model_exp2:
    truth_s = CUBE_TRUTH (0.8 + 0.4 u),  u = (splitmix64(4, SEED + CUBE_SEED + 4000 (s + 1) + n) >> 11) / 2**53,
    f = exp2_numpy(truth_s, x),  counts = clip(round(f + sqrt(f + 1) normal(n, SEED + CUBE_SEED + 31 s + n)), 0, 65535)  as uint16.
CUBE_TRUTH = (3000, 2.5, 1500, 15): counts run from a few thousand at the head of a long spectrum to a few at its tail, and zeros
occur there (test_cpu_batch_cube.py asserts it), so the 0.0 arm of SQRT_Y / PROPTO_Y is exercised.
How truth and seed were chosen, by the oracle alone (the device never entered): under INVERSE_Y the weight IS the count, the head of
a spectrum carries the fit and a slow component far weaker than the fast one is barely determined -- with amplitudes (2500, 60) a
quarter of the INVERSE_Y fits disagreed with themselves beyond SELF_TOL under any seed.  Two components of comparable amplitude and
well separated decay times are determined under all of the weight rules; of the seeds 0, 10**6, 2 10**6, 3 10**6 tried with them the
last is kept: it drops 1, 0 and 1 of the 84 fits of the three forms of the oracle check and every length keeps five of its six
(cap: 5 %, four of six).
The float32 cube takes the same counts plus k / 16, k = 0 ... 15 (exact in float32: 16 + 4 bits), the float64 cube plus a double in
[0, 1); a zero count stays an exact zero in both, so that every sample type meets the 0.0 arm.
USER weights: w = 1 / sqrt(counts + 1), the weights as used.

WHAT A CUBE IS HELD AGAINST (check 1): the ragged form on the same context fed x tiled, Y.astype(float64) and the weights the
device's own gfh_init_weights establishes (established_weights), bit for bit."""
import functools

import numpy as np

from gadfit_amd.ad import trace_model
from tests import batch_cases as BC
from tests import models as M
from tests.batch_common import SCENARIOS, start_of

CUBE_TRUTH = np.array([3000.0, 2.5, 1500.0, 15.0])
CUBE_SEED = 3000000
ACTIVE = [0, 1, 2, 3]
LENGTHS = {64: (4, 5, 63, 64, 65, 129, 1000), 16: (4, 5, 15, 16, 17, 33), 256: (4, 255, 256, 257, 513, 1025)}
FIT_COUNTS = (1, 3, 5, 17)          # waves, rows and workgroups without a fit; odd rows of uint16 and float32 on every alignment
FIT_SCENARIOS = ('a', 'c')
Y_TYPES = (np.float64, np.float32, np.uint16)         # gfh_set_batch_cube's y_type 0, 1, 2
NONE, SQRT_Y, PROPTO_Y, INVERSE_Y, USER = range(5)    # gfh_init_weights' numbers
ERROR_TYPES = (NONE, SQRT_Y, PROPTO_Y, INVERSE_Y, USER)
N_SPECTRA = 6
# check 2: held against the oracle directly, each at 64 lanes over its lengths
ORACLE_FORMS = ((np.uint16, SQRT_Y), (np.float32, PROPTO_Y), (np.float64, INVERSE_Y))
ORACLE_CAP = 0.05                   # of the fits may fail the rule, and
ORACLE_KEEP = 4                     # every length keeps at least this many of its six
# check 3
LARGE_FITS = 2 ** 17 + 3            # of 33 uint16 points at 16 lanes, tiled from 66 spectra
LARGE_N = 33
HUGE_FITS, HUGE_N = 65537, 32769    # one pass at 256 lanes: more than 2**31 elements, tiled from three spectra


def grid(n):
    return 0.5 + 99.5 * (np.arange(n, dtype=np.float64) + 0.5) / n


def truth_of(n, s):
    u = (M.splitmix64(4, M.SEED + CUBE_SEED + 4000 * (s + 1) + n) >> np.uint64(11)).astype(np.float64) / 9007199254740992.0
    return CUBE_TRUTH * (0.8 + 0.4 * u)


@functools.lru_cache(maxsize=None)
def counts(n, n_spectra=N_SPECTRA):
    """uint16 [n_spectra][n]"""
    x = grid(n)
    out = np.empty((n_spectra, n), dtype=np.uint16)
    for s in range(n_spectra):
        f = M.exp2_numpy(truth_of(n, s), x)
        out[s] = np.clip(np.round(f + np.sqrt(f + 1.0) * M.normal(n, M.SEED + CUBE_SEED + 31 * s + n)), 0, 65535).astype(np.uint16)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cube(n, y_type, n_spectra=N_SPECTRA):
    """Y [n_spectra][n] in y_type, C-contiguous"""
    c = counts(n, n_spectra)
    y_type = np.dtype(y_type)
    if y_type == np.uint16:
        return c
    bits = M.splitmix64(c.size, M.SEED + 77 * n + 5).reshape(c.shape)
    if y_type == np.float32:
        frac = (bits >> np.uint64(60)).astype(np.float64) / 16.0
    else:
        frac = (bits >> np.uint64(11)).astype(np.float64) / 9007199254740992.0
    Y = (c.astype(np.float64) + np.where(c == 0, 0.0, frac)).astype(y_type)
    assert np.array_equal(Y.astype(np.float64), c.astype(np.float64) + np.where(c == 0, 0.0, frac))      # the conversion is exact
    Y.setflags(write=False)
    return Y


def user_weights(n, n_spectra=N_SPECTRA):
    return 1.0 / np.sqrt(counts(n, n_spectra).astype(np.float64) + 1.0)


def reference_weights(Y, error_type, w=None):
    """init_weights of the reference (gadfit.F90:445-470) in numpy, on y as doubles: independent of the device"""
    y = np.asarray(Y, dtype=np.float64)
    tiny = 1e2 * np.finfo(np.float64).tiny
    with np.errstate(divide='ignore', invalid='ignore'):
        if error_type == NONE:
            return np.ones_like(y)
        if error_type == SQRT_Y:
            return np.where(np.abs(y) < tiny, 0.0, 1.0 / np.sqrt(y))
        if error_type == PROPTO_Y:
            return np.where(np.abs(y) < tiny, 0.0, 1.0 / y)
        if error_type == INVERSE_Y:
            return y.copy()
    return np.asarray(w, dtype=np.float64)


def established_weights(ctx, x, Y, error_type, w=None):
    """the weights the device's own gfh_init_weights establishes for the rows of Y, [n_spectra][n]: set_data(x tiled, y, ones),
    init_weights(type), weights() on a plain context `ctx` with a model set; USER takes the given w"""
    if error_type == USER:
        return np.asarray(w, dtype=np.float64)
    y = np.ascontiguousarray(Y, dtype=np.float64)
    ctx.set_data(np.tile(x, y.shape[0]), y.ravel(), np.ones(y.size), [0, y.size])
    ctx.init_weights(error_type)
    return ctx.weights().reshape(y.shape)


def pick(n_fits, n_spectra=N_SPECTRA):
    """the spectra of a batch of n_fits, taken in turn"""
    return np.arange(n_fits) % n_spectra


def starts(n, off, n_spectra=N_SPECTRA):
    return np.array([start_of(truth_of(n, s), off) for s in range(n_spectra)])


def tape():
    return trace_model(M.model_exp2, 4)


def form_of(y_type, error_type):
    """what Context.batch_form_used reports after a launch on such a cube"""
    return ('cube', Y_TYPES.index(np.dtype(y_type).type), error_type)


@functools.lru_cache(maxsize=None)
def oracle_selection(y_index, error_type, name):
    """batch_cases.select over the six spectra of every 64-lane length, weights by reference_weights:
    {n: [(kept, oracle result, self-difference, margin)]}"""
    t = tape()
    off, kw = SCENARIOS[name]
    out = {}
    for n in LENGTHS[64]:
        x = grid(n)
        Y = cube(n, Y_TYPES[y_index]).astype(np.float64)
        W = reference_weights(Y, error_type)
        st = starts(n, off)
        out[n] = [BC.select(t, x, Y[s].copy(), W[s].copy(), st[s], ACTIVE, kw) for s in range(N_SPECTRA)]
    return out


def cube_units():
    """[(lanes, y_type number, error_type)]: every cube translation unit of model_exp2 with ACTIVE that the GPU tests ask for -- all 15
    loads at each of the three lane forms (the ragged units of the same set are tests/batch_form_cases.py's)"""
    return [(lanes, yt, et) for lanes in (64, 16, 256) for yt in range(3) for et in ERROR_TYPES]


def prepare_units(ctx, part=0, parts=1):
    """compiles cube_units() and the ragged units the tests compare them with on a context (compile-only contexts included): a cube of
    the type and rule is set, which such a context keeps before it ends in `no GPU`.  part, parts: every parts-th unit from the
    part-th on, so that several processes can share the list (build() does: a process compiles one unit at a time)"""
    from gadfit_amd import _lib
    ctx.set_model(tape())
    x = grid(4)
    for lanes, yt, et in cube_units()[part::parts]:
        ctx.set_batch_lanes(lanes)
        try:
            ctx.set_batch_cube(x, np.ones((1, 4), dtype=Y_TYPES[yt]), et, np.ones((1, 4)) if et == USER else None)
        except _lib.GadfitHipError as e:
            if 'no GPU' not in str(e):
                raise
        ctx.batch_prepare(ACTIVE)
    for lanes in (64, 16, 256):
        ctx.set_batch_lanes(lanes)
        try:
            ctx.set_batch_data([0, 4], x, x, x)
        except _lib.GadfitHipError as e:
            if 'no GPU' not in str(e):
                raise
        ctx.batch_prepare(ACTIVE)
    ctx.set_batch_lanes(64)
