"""The inputs of tests/test_gpu_batch_bounds.py, tests/test_cpu_batch_bounds.py and tests/test_cpu_batch_bounds_cases.py: batched fits
inside a box (gfh_fit_batch_bounded).  Everything here is deterministic, needs no GPU and is decided by the oracle alone: the device's
results never enter a rule of this module.  The scenarios, the bounds and the selection rule (select) are those of
tests/batch_common.py and tests/batch_cases.py, imported, not restated.

SPECTRA.  model_exp2, one spectrum per length of LENGTHS (the edges of the 16-, 64- and 256-lane rows, down to n = na); for the
spectrum of length n
    u = (splitmix64(4, SEED + BOUNDS_SEED + n) >> 11) / 2**53,  truth = EXP2_TRUTH (0.9 + 0.2 u),
    x, y, s = make_single(exp2_numpy, truth, n, 0.05, 100.0, seed=SEED + BOUNDS_SEED + 13 n),  weights 1 / s,
    start = start_of(truth, off) with the scenario's off (scenarios a, c, d; c carries accth).
model_exp4 with all 8 active: the first 16 spectra of batch_common.spectrum4 (128 ... 500 points).

PINNED CASES (test 4).  A case pins one parameter: it starts ON its bound and the reduced fit -- the oracle's fit of the other active
parameters with that one passive at the bound -- is pushed outward at every iterate.  A spectrum is KEPT for a case and a scenario when
 (i)  batch_cases.select keeps the reduced fit, and
 (ii) at the start and at every accepted iterate of the reduced fit (the oracle's fit with max_iter = 1 ... iterations) the
      full-active-set sweep() has J^T r pointing outward at the pinned parameter: > 0 at an upper, < 0 at a lower bound.
At least CAP = 12 of the 16 spectra must be kept per case and scenario (tests/test_cpu_batch_bounds_cases.py); the others leave
test 4 by this rule and no other.

RELEASED CASE (test 5).  p[3] starts ON upper[3] = 40 with the truth inside, so it is free from the first iteration.  A spectrum is
kept when the unbounded fit's trial points stay below the wall: at the start and at every accepted iterate k of the oracle's
unbounded fit, the steps of EVERY lambda the iteration could try (lambda_k lam_up^i, i = 0 ... lam_incs; a superset of those it does
try) are recomputed from the oracle's sweep() and omega() with its own Cholesky solve, and P_3 + delta1_3 and, under accth, P_3 +
delta1_3 + delta2_3 / 2 must all lie below 40 (1 - 1e-9), and J^T r_3 at the start must point inward (< 0).  The same cap applies.

MIXED CASE (test 6).  24 spectra of model_exp2 of MIXED_LENGTHS, upper[3] = 20, p[3] started inside at 15 while the truth's p[3] is
27 ... 33: the fit is clamped, pinned and possibly released on its way.  Which spectra its stationary-point check is made on:
MIXED_ROOM below."""
import functools

import numpy as np

from gadfit_amd.ad import trace_model
from oracle import binding as orc
from tests import batch_cases as BC
from tests import models as M
from tests.batch_common import SCENARIOS, spectrum4, start_of

BOUNDS_SEED = 7000000
LENGTHS = (4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 255, 256, 257, 300)
NAMES = ('a', 'c', 'd')
CAP = 12
INF = float('inf')


@functools.lru_cache(maxsize=None)
def tape2():
    return trace_model(M.model_exp2, 4)


@functools.lru_cache(maxsize=None)
def tape4():
    return trace_model(M.model_exp4, 8)


def spectrum(n):
    """(truth, x, y, weights) of the spectrum of length n"""
    u = (M.splitmix64(4, M.SEED + BOUNDS_SEED + n) >> np.uint64(11)).astype(np.float64) / 9007199254740992.0
    truth = M.EXP2_TRUTH * (0.9 + 0.2 * u)
    x, y, s = M.make_single(M.exp2_numpy, truth, n, 0.05, 100.0, seed=M.SEED + BOUNDS_SEED + 13 * n)
    return truth, x, y, 1.0 / s


@functools.lru_cache(maxsize=None)
def exp2_batch(lengths=LENGTHS):
    """(truths, Batch)"""
    sp = [spectrum(n) for n in lengths]
    return np.array([it[0] for it in sp]), BC.Batch([it[1:] for it in sp])


@functools.lru_cache(maxsize=None)
def exp4_batch():
    sp = [spectrum4(b) for b in range(16)]
    return np.array([it[0] for it in sp]), BC.Batch([it[1:] for it in sp])


def exp2_starts(off, lengths=LENGTHS):
    return np.array([start_of(t, off) for t in exp2_batch(lengths)[0]])


def exp4_starts(off):
    sign = np.where(np.arange(8) % 2 == 0, 1.0 + off, 1.0 - off)
    return exp4_batch()[0] * sign


def box(na, **at):
    """(lower, upper) of na active parameters, infinite but for lo<j> = v / hi<j> = v"""
    lo = np.full(na, -INF); hi = np.full(na, INF)
    for k, v in at.items():
        (lo if k[:2] == 'lo' else hi)[int(k[2:])] = v
    return lo, hi


class Pinned:
    """a case of test 4: `active` in the caller's order, position `j` of it pinned at `value`, an upper (side +1) or lower (-1) bound"""

    def __init__(self, key, model, active, j, side, value):
        self.key, self.model, self.active, self.j, self.side, self.value = key, model, list(active), j, side, value
        self.reduced = [a for k, a in enumerate(self.active) if k != j]

    def tape(self):
        return tape2() if self.model == 'exp2' else tape4()

    def batch(self):
        return (exp2_batch() if self.model == 'exp2' else exp4_batch())[1]

    def starts(self, off):
        s = (exp2_starts(off) if self.model == 'exp2' else exp4_starts(off)).copy()
        s[:, self.active[self.j]] = self.value
        return s

    def box(self):
        lo = np.full(len(self.active), -INF); hi = np.full(len(self.active), INF)
        (hi if self.side > 0 else lo)[self.j] = self.value
        return lo, hi

    def bit(self):
        return 1 << (self.j + (8 if self.side > 0 else 0))


# p[3] last in the active order; p[2] in the middle of it (the masked solve's middle row); p[3] listed second; model_exp4 with 8 active,
# p[2] at 1.5 under a truth of 2.7 ... 3.3 (of the candidates tried by the rule above, p[7] <= 20 kept 9 of 16 in scenario a, this one 16)
PINNED = (Pinned('hi3', 'exp2', [0, 1, 2, 3], 3, +1, 20.0),
          Pinned('hi2', 'exp2', [0, 1, 2, 3], 2, +1, 1.0),
          Pinned('hi3_second', 'exp2', [0, 3, 1, 2], 1, +1, 20.0),
          Pinned('exp4_hi2', 'exp4', [0, 1, 2, 3, 4, 5, 6, 7], 2, +1, 1.5))


def outward(case, x, y, w, start, kw, iterations):
    """rule (ii): the smallest outward cosine side * J^T r_j / sqrt(J^T J_jj chi2) over the start and the accepted iterates of the
    reduced fit; > 0: outward everywhere"""
    tape = case.tape()
    worst = INF
    for k in range(iterations + 1):
        p = orc.OracleProblem(tape, [x], [y], [w], [start], case.reduced, [0] * tape.n_pars)
        if k:
            p.fit(**dict(kw, max_iter=k))
        full = orc.OracleProblem(tape, [x], [y], [w], [p.pars.ravel()], case.active, [0] * tape.n_pars)
        JTJ, JTr, _, _ = full.sweep()
        chi2 = full.chi2()[0]
        worst = min(worst, case.side * JTr[case.j] / np.sqrt(JTJ[case.j, case.j] * chi2))
    return float(worst)


@functools.lru_cache(maxsize=None)
def pinned_selection(key, name):
    """[(kept, select's record of the reduced fit, diff, margin, outward cosine)] over the case's 16 spectra"""
    case = next(c for c in PINNED if c.key == key)
    off, kw = SCENARIOS[name]
    starts = case.starts(off)
    out = []
    for b, (x, y, w) in enumerate(case.batch().items):
        ok, one, diff, margin = BC.select(case.tape(), x, y, w, starts[b], case.reduced, kw)
        cos = outward(case, x, y, w, starts[b], kw, one[0][0])
        out.append((bool(ok and cos > 0.0), one, diff, margin, cos))
    return out


def expanded(case, sel):
    """the selection with the reduced fits' parameters (the full parameter rows the oracle returns) as fit_worst reads them"""
    return [(ok, one, diff, margin) for ok, one, diff, margin, _ in sel]


# ---- test 5: released at once ----------------------------------------------------------------------------------------------------
RELEASED_WALL = 40.0
ACTIVE = [0, 1, 2, 3]


def released_starts(off):
    s = exp2_starts(off).copy()
    s[:, 3] = RELEASED_WALL
    return s


def trial_max(tape, x, y, w, start, active, j, kw):
    """the largest value of active parameter j among the trial points the unbounded fit could make (see the module's text)"""
    lam_up = kw.get('lam_up', 10.0); lam_incs = kw.get('lam_incs', 2)
    accth = kw.get('accth')
    it = orc.OracleProblem(tape, [x], [y], [w], [start], active, [0] * tape.n_pars).fit(**kw).iterations
    DTD = np.zeros(len(active))
    worst = -INF
    for k in range(it + 1):
        p = orc.OracleProblem(tape, [x], [y], [w], [start], active, [0] * tape.n_pars)
        lam = kw.get('lambda_', 1.0)
        if k:
            lam = p.fit(**dict(kw, max_iter=k)).lambda_
        JTJ, JTr, _, JT = p.sweep(want_J=True)
        DTD = np.maximum(DTD, np.diag(JTJ))
        P = p.pars.ravel()[active]          # (an accepted iterate is one of the trial points of the iteration before; the start sits on the wall)
        for i in range(lam_incs + 1):
            A = JTJ + lam * lam_up ** i * np.diag(DTD)
            d1 = orc.potr(A, JTr)
            worst = max(worst, P[j] + d1[j])
            if i == 0 and accth is not None:
                d2 = orc.potr(A, p.omega(d1, JT)[1])
                worst = max(worst, P[j] + d1[j] + 0.5 * d2[j])
    return float(worst)


@functools.lru_cache(maxsize=None)
def released_selection(name):
    """[(kept, trial_max)] over the 16 spectra"""
    off, kw = SCENARIOS[name]
    starts = released_starts(off)
    out = []
    for b, (x, y, w) in enumerate(exp2_batch()[1].items):
        t = trial_max(tape2(), x, y, w, starts[b], ACTIVE, 3, kw)
        inward = orc.OracleProblem(tape2(), [x], [y], [w], [starts[b]], ACTIVE, [0] * 4).sweep()[1][3] < 0.0
        out.append((bool(inward and t < RELEASED_WALL * (1.0 - 1e-9)), t))
    return out


# ---- test 6: the mixed regime ------------------------------------------------------------------------------------------------------
MIXED_LENGTHS = (16, 17, 24, 30, 31, 33, 37, 48, 63, 64, 65, 80, 100, 127, 128, 129, 160, 200, 255, 256, 257, 300, 400, 500)
MIXED_WALL, MIXED_START = 20.0, 15.0
MIXED_KW = dict(lambda_=1.0, lam_incs=3, max_iter=200)
MIXED_CONVERGED_FROM = 37          # shorter spectra do not converge within 200 iterations in the reference either
# The stationary-point check of test 6 holds the device's end point to the end of the reference's REDUCED fit, which starts ON the
# wall.  It is made for the spectra on which the reference converges with room: from both starts it ends by giving up on lambda (exit
# 7, not max_iter) within half of max_iter.  The bounded fit starts inside the box and first has to reach the wall, iterations the
# reduced fit does not spend; a spectrum on which the reference itself needs all but one of the 200 says nothing about a fit that
# needs a few more.  Of the ragged spectra this keeps exactly n >= 37 (the reference needs at most 66 iterations there, and 200 without
# converging below); of the cube's six it keeps three and leaves out those on which the reference needs 146, 199 and more than 200.
MIXED_ROOM = MIXED_KW['max_iter'] // 2


def mixed_starts(off=0.05, p3=MIXED_START):
    s = exp2_starts(off, MIXED_LENGTHS).copy()
    s[:, 3] = p3
    return s


def mixed_batch():
    return exp2_batch(MIXED_LENGTHS)[1]


def stationarity(tape, x, y, w, pars, active, free):
    """|J^T r_a| / sqrt(J^T J_aa chi2) of the positions `free` of `active` at `pars`, and J^T r whole, by the oracle's sweep()"""
    p = orc.OracleProblem(tape, [x], [y], [w], [pars], active, [0] * tape.n_pars)
    JTJ, JTr, _, _ = p.sweep()
    chi2 = p.chi2()[0]
    return np.array([abs(JTr[a]) / np.sqrt(JTJ[a, a] * chi2) for a in free]), JTr, chi2


def reduced_reference(items, starts_at_wall):
    """per spectrum of items: (the parameters at the end of the oracle's reduced fit [0, 1, 2], p[3] passive at the wall, from
    starts_at_wall(0.05), under MIXED_KW; the largest free stationarity measure at that end; the spread of that fit's free parameters
    between the starts of offsets +5 % and -8 %, relative; CONVERGED: from both starts the reference gives up on lambda (exit 7)
    within MIXED_ROOM iterations)"""
    out = []
    for b, (x, y, w) in enumerate(items):
        ends, conv = [], True
        for off in (0.05, -0.08):
            p = orc.OracleProblem(tape2(), [x], [y], [w], [starts_at_wall(off)[b]], [0, 1, 2], [0] * 4)
            r = p.fit(**MIXED_KW)
            conv = conv and r.exit_reason == 7 and r.iterations <= MIXED_ROOM
            ends.append(p.pars.ravel().copy())
        g, _, _ = stationarity(tape2(), x, y, w, ends[0], ACTIVE, [0, 1, 2])
        out.append((ends[0], float(np.max(g)), float(np.max(np.abs(ends[0][:3] - ends[1][:3]) / np.abs(ends[0][:3]))), bool(conv)))
    return out


def unbounded_end(items, starts):
    """p[3] at the end of the oracle's unbounded fit of every spectrum under MIXED_KW"""
    out = []
    for b, (x, y, w) in enumerate(items):
        p = orc.OracleProblem(tape2(), [x], [y], [w], [starts[b]], ACTIVE, [0] * 4)
        p.fit(**MIXED_KW)
        out.append(float(p.pars.ravel()[3]))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def mixed_reference():
    return reduced_reference(mixed_batch().items, lambda off: mixed_starts(off, MIXED_WALL))


# ---- the cube of tests 3 and 6: six uint16 spectra of batch_cube_cases on one grid, the weights by SQRT_Y --------------------------
CUBE_N, CUBE_FITS, CUBE_ERROR = 129, 6, 1
CUBE_WALL, CUBE_START = 9.0, 7.0       # the truth's p[3] of the cube's spectra is 12 ... 18 (batch_cube_cases.CUBE_TRUTH)


def cube():
    """(x [n], Y [6][n] uint16)"""
    from tests import batch_cube_cases as CU
    return CU.grid(CUBE_N), np.ascontiguousarray(CU.cube(CUBE_N, np.uint16, CUBE_FITS))


def cube_items():
    """the cube as the oracle reads it: (x, y as doubles, the reference's SQRT_Y weights) per spectrum"""
    from tests import batch_cube_cases as CU
    x, Y = cube()
    return [(x, Y[s].astype(np.float64), CU.reference_weights(Y[s], CUBE_ERROR)) for s in range(CUBE_FITS)]


def cube_starts(off=0.05, p3=None):
    from tests import batch_cube_cases as CU
    s = CU.starts(CUBE_N, off, CUBE_FITS).copy()
    if p3 is not None:
        s[:, 3] = p3
    return s


@functools.lru_cache(maxsize=None)
def cube_reference():
    return reduced_reference(cube_items(), lambda off: cube_starts(off, CUBE_WALL))


# ---- every translation unit the GPU tests ask for ------------------------------------------------------------------------------------
def units():
    """[(tape, active list)]: each in the bounded unit and (but for the permuted order, which test 4 alone runs) in the four kernels' unit,
    on the three lane forms"""
    return [(tape2(), [0]), (tape2(), [0, 1, 2, 3]), (tape2(), [3, 1]), (tape2(), [0, 3, 1, 2]), (tape4(), list(range(8)))]


def prepare_units(ctx):
    """compiles them on the compile-only context ctx (build() and tests/test_cpu_batch_bounds.py), the cube's two at 64 lanes last"""
    for lanes in (64, 16, 256):
        ctx.set_batch_lanes(lanes)
        for tape, active in units():
            ctx.set_model(tape)
            ctx.batch_prepare(active, bounded=True)
            if active != [0, 3, 1, 2]:
                ctx.batch_prepare(active)
    ctx.set_batch_lanes(64)
    ctx.set_model(tape2())
    x, Y = cube()
    try:
        ctx.set_batch_cube(x, Y, CUBE_ERROR)
    except Exception as e:          # (a compile-only context keeps the form and ends in `no GPU`)
        if 'no GPU' not in str(e):
            raise
    ctx.batch_prepare(ACTIVE, bounded=True)
    ctx.batch_prepare(ACTIVE)
