"""The inputs of tests/test_cpu_batch_loss.py and tests/test_gpu_batch_loss.py: batched fits under a robust loss with a residual scale
(gfh_set_batch_loss), and the rule that selects which fits a device fit may be held against.  Everything here is deterministic, needs
no GPU and is decided by the oracle alone; the spectra, the starts, the active sets and the forms are those of tests/batch_cases.py,
tests/batch_common.py and tests/batch_form_cases.py, imported, not restated.

THE REFERENCE FOR A SCALE c.  The reference's costs switch at |r| = 1.  With the weights w / c the oracle's weighted residual is u = r / c,
so OracleProblem(loss=..., weights w / c) is the fit under the scale c: the same ls at every point, every sum 1 / c^2 times the
device's, and the damped solve, acc_ratio, the lambda logic and the exit tests commute with that factor.  oracle() builds that problem;
what it returns in sums and chi2 is multiplied by c^2 before it is compared (c = 1.345 does not round away: w / c differs from the
exact quotient by half an ulp per point, far below every bound here).

PART A: the 48 spectra of batch_cases.part2() (model_exp4, 128 ... 512 points).  In spectrum b the samples idx = arange(5 + b % 7, n, 17)
are displaced by +12 / w and -9 / w alternately (+12 sigma, -9 sigma): 7 ... 30 outliers per spectrum.  Starts: part2_starts(active, off).
PART B: batch_cases.spectrum_n(n, s) of model_exp2, s = 0, 1, at the edge lengths of each form of tests/batch_form_cases.py; idx =
arange(2 + s, n, 11) displaced by +12 sigma / -9 sigma alternately.  Starts 5 % off the truth, scenario conv.

THE SELECTION RULE is batch_cases.select with loss= passed to OracleProblem (select below restates its three conditions with the same
constants): equal counts at 1 and 3 images, parameters within SELF_TOL, min_margin > TOL_PASS.  What it keeps, evaluated on the CPU
(tests/test_cpu_batch_loss.py asserts it over exactly the cases the GPU module uses):
  conv, conv_acc: every fit of every active set for both losses at c = 1, 2 and 1.345 -- the cap is 0 dropped;
  far_acc with Cauchy at c = 1: at most 2 per set of 48 dropped.  far_acc is not used with Huber or with c = 2: the rule keeps as few as 14 of 48 there;
  Part B under conv: at most RANDOM_CAP = 5 % of a form's fits dropped."""
import functools

import numpy as np

from gadfit_amd.ad import trace_model
from oracle import binding as orc
from tests import batch_bounds_cases as BB
from tests import batch_cases as BC
from tests import models as M
from tests.batch_common import COUNTS, SCENARIOS, start_of

CAUCHY, HUBER = 1, 2
LOSSES = (CAUCHY, HUBER)
LOSS_NAMES = {CAUCHY: 'cauchy', HUBER: 'huber'}
SCALES = (1.0, 2.0, 1.345)
PASS_SCALES = (1.0, 1.345)
ARGS = {
    'conv': (0.05, dict(lambda_=1.0, max_iter=50, chi2_rel=1e-6)),
    'conv_acc': (0.05, dict(lambda_=1.0, max_iter=50, chi2_rel=1e-6, accth=0.9)),
    'far_acc': (0.3, dict(lambda_=1.0, max_iter=12, accth=0.9)),
}
CAP_A = {'conv': 0, 'conv_acc': 0, 'far_acc': 2}          # fits of a set of 48 that may fail the rule
SETS = [list(a) for a in BC.EXP4_SETS]
EDGE_SETS = [SETS[0], SETS[3], SETS[7]]                   # na = 1, 4, 8: what the 16- and 256-lane forms run
ACTIVE2 = [0, 1, 2, 3]


def displaced(y, w, first, step):
    """y with the samples first, first + step, ... moved by +12 / w and -9 / w alternately"""
    idx = np.arange(first, y.size, step)
    out = y.copy()
    out[idx] += np.where(np.arange(idx.size) % 2 == 0, 12.0, -9.0) / w[idx]
    return out


# ---- the oracle under a loss and a scale ----------------------------------------------------------------------------------------------
def oracle(tape, x, y, w, start, active, loss, c=1.0):
    return orc.OracleProblem(tape, [x], [y], [w / c], [start], list(active), [0] * tape.n_pars, loss=loss)


def _fit(tape, x, y, w, start, active, kw, loss, c, n_images):
    p = oracle(tape, x, y, w, start, active, loss, c)
    r = p.fit(n_images=n_images, **kw)
    return (tuple(int(getattr(r, f)) for f in COUNTS), p.pars.ravel().copy(), float(r.lambda_), float(r.chi2) * c * c), float(r.min_margin)


def select(tape, x, y, w, start, active, kw, loss, c=1.0):
    """batch_cases.select under a loss and a scale: (kept, ((counts), parameters, lambda, chi2 in the device's units), the parameters'
    relative difference between 1 and 3 images, the closest chi2 comparison)"""
    one, margin = _fit(tape, x, y, w, start, active, kw, loss, c, 1)
    three = _fit(tape, x, y, w, start, active, kw, loss, c, 3)[0]
    diff = float(np.max(np.abs(one[1] - three[1]) / np.abs(one[1])))
    return one[0] == three[0] and diff <= BC.SELF_TOL and margin > BC.MARGIN, one, diff, margin


def oracle_pass(tape, x, y, w, start, active, loss, c=1.0):
    """(J^T J, J^T r of the loss-scaled Jacobian and residual, the plain chi2) in the device's units"""
    p = oracle(tape, x, y, w, start, active, loss, c)
    JTJ, JTr, _, _ = p.sweep()
    return JTJ * (c * c), JTr * (c * c), p.chi2()[0] * (c * c)


def pass_worst(tape, items, starts, active, loss, c, JTJ, JTr, chi2):
    """a batch_pass under a loss against the oracle, scaled as batch_common.pass_worst scales: (the worst of J^T J and J^T r, the worst of chi2)"""
    worst, worst_chi = 0.0, 0.0
    for b, (x, y, w) in enumerate(items):
        JTJ0, JTr0, chi0 = oracle_pass(tape, x, y, w, starts[b], active, loss, c)
        d = np.diag(JTJ0)
        # J^T r is scaled by the loss-scaled residual's own norm bound: |J^T r_a| <= sqrt(J^T J_aa sum R^2) <= sqrt(J^T J_aa chi2)
        worst = max(worst, np.max(np.abs(JTJ[b] - JTJ0) / (np.sqrt(np.outer(d, d)) + 1e-300)),
                    np.max(np.abs(JTr[b] - JTr0) / (np.sqrt(d * chi0) + 1e-300)))
        worst_chi = max(worst_chi, abs(chi2[b] - chi0) / chi0)
        assert np.array_equal(JTJ[b], JTJ[b].T), b
    assert np.isfinite(worst) and np.isfinite(worst_chi)
    return worst, worst_chi


# ---- Part A -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def part_a():
    """(tape, Batch): batch_cases.part2's spectra with their outliers"""
    tape, _, clean = BC.part2()
    return tape, BC.Batch([(x, displaced(y, w, 5 + b % 7, 17), w) for b, (x, y, w) in enumerate(clean.items)])


def starts_a(active, name):
    return BC.part2_starts(list(active), ARGS[name][0])


@functools.lru_cache(maxsize=None)
def _selection_a(active, name, loss, c):
    tape, batch = part_a()
    st = starts_a(active, name)
    return [select(tape, *batch.items[b], st[b], list(active), ARGS[name][1], loss, c) for b in range(len(batch.items))]


def selection_a(active, name, loss, c=1.0):
    """the rule over Part A (cached: one evaluation serves every lane form)"""
    return _selection_a(tuple(active), name, int(loss), float(c))


def fit_cases(lanes):
    """[(name, active, loss, c)] of the fits against the oracle in one lane form"""
    sets = SETS if lanes == 64 else EDGE_SETS
    out = [(name, a, loss, c) for name in ('conv', 'conv_acc') for a in sets for loss in LOSSES for c in SCALES]
    if lanes == 64:
        out += [('far_acc', a, CAUCHY, 1.0) for a in SETS]
    return out


def pass_cases(lanes):
    sets = SETS if lanes == 64 else EDGE_SETS
    return [(a, loss, c) for a in sets for loss in LOSSES for c in PASS_SCALES]


@functools.lru_cache(maxsize=None)
def _linear_fit_a(active, name):
    tape, batch = part_a()
    st = starts_a(active, name)
    return [BC.oracle_fit(tape, *batch.items[b], st[b], list(active), ARGS[name][1], 1)[1] for b in range(len(batch.items))]


def linear_pars_a(active, name):
    """the oracle's LINEAR fits of Part A: what the robust ones must differ from"""
    return _linear_fit_a(tuple(active), name)


# ---- Part B -----------------------------------------------------------------------------------------------------------------------------
PART_B_SAMPLES = (0, 1)


@functools.lru_cache(maxsize=None)
def part_b(form):
    """(tape, [(n, s)], starts [k][4], Batch) at the form's edge lengths, short beside long"""
    order = [(n, s) for s in PART_B_SAMPLES for n in sorted(form.edges)]
    items, starts = [], []
    for n, s in order:
        truth, x, y, w, _ = BC.spectrum_n(n, s)
        items.append((x, displaced(y, w, 2 + s, 11), w))
        starts.append(start_of(truth, ARGS['conv'][0]))
    return trace_model(M.model_exp2, 4), order, np.array(starts), BC.Batch(items)


@functools.lru_cache(maxsize=None)
def selection_b(form, loss):
    tape, _, st, batch = part_b(form)
    return [select(tape, *item, st[k], ACTIVE2, ARGS['conv'][1], loss) for k, item in enumerate(batch.items)]


# ---- the bounded case: batch_bounds_cases' first pinned-throughout construction under Cauchy -----------------------------------------------
PINNED = BB.PINNED[0]             # 'hi3': p[3] of model_exp2 starts on its upper bound 20 and is pushed outward
PINNED_SCENARIO = 'a'


def _outward(case, x, y, w, start, kw, iterations, loss):
    """batch_bounds_cases.outward with the loss: rule 1 pins on the sign of the loss-scaled J^T r"""
    tape = case.tape()
    worst = BB.INF
    for k in range(iterations + 1):
        p = oracle(tape, x, y, w, start, case.reduced, loss)
        if k:
            p.fit(**dict(kw, max_iter=k))
        full = oracle(tape, x, y, w, p.pars.ravel(), case.active, loss)
        JTJ, JTr, _, _ = full.sweep()
        worst = min(worst, case.side * JTr[case.j] / np.sqrt(JTJ[case.j, case.j] * full.chi2()[0]))
    return float(worst)


@functools.lru_cache(maxsize=None)
def pinned_selection(loss=CAUCHY):
    """[(kept, select's record of the reduced fit, diff, margin)] over the case's 16 spectra: batch_bounds_cases.pinned_selection's two
    rules with the loss in both"""
    case = PINNED
    off, kw = SCENARIOS[PINNED_SCENARIO]
    starts = case.starts(off)
    out = []
    for b, (x, y, w) in enumerate(case.batch().items):
        ok, one, diff, margin = select(case.tape(), x, y, w, starts[b], case.reduced, kw, loss)
        cos = _outward(case, x, y, w, starts[b], kw, one[0][0], loss)
        out.append((bool(ok and cos > 0.0), one, diff, margin))
    return out


# ---- the cube: 8 fits x 37 points, uint16 under SQRT_Y, two cosmic-ray-sized steps per spectrum -------------------------------------------
CUBE_N, CUBE_FITS, CUBE_ERROR, CUBE_LOSS, CUBE_SCALE = 37, 8, 1, CAUCHY, 2.0


def cube():
    """(x [37], Y [8][37] uint16, starts [8][4]): batch_cube_cases' counts with samples 7 + s and 23 + s of spectrum s raised by 40 %
    of the spectrum's peak + 200 counts (tens of sigma under SQRT_Y)"""
    from tests import batch_cube_cases as CU
    Y = np.ascontiguousarray(CU.cube(CUBE_N, np.uint16, CUBE_FITS)).astype(np.int64)
    for s in range(CUBE_FITS):
        for k in (7 + s, 23 + s):
            Y[s, k] += int(0.4 * Y[s].max()) + 200
    assert Y.max() < 65536
    return CU.grid(CUBE_N), np.ascontiguousarray(Y.astype(np.uint16)), CU.starts(CUBE_N, 0.05, CUBE_FITS)


# ---- the linear units whose text must not change --------------------------------------------------------------------------------------------
TEXT_MODELS = {'exp2': (M.model_exp2, 4, [0, 1, 2, 3]), 'exp4': (M.model_exp4, 8, list(range(8)))}
TEXT_DATA = ('ragged', 'cube_uint16_sqrt_y')
TEXT_LANES = (16, 64, 256)


def hold_text_cube(ctx):
    """gives the compile-only context ctx the data form of a uint16 cube under SQRT_Y (the call ends in `no GPU` and keeps the form)"""
    try:
        ctx.set_batch_cube(np.linspace(0.5, 99.5, 20), np.ones((3, 20), dtype=np.uint16), 1)
    except Exception as e:
        if 'no GPU' not in str(e):
            raise


def text_key(model, data, lanes, bounded):
    return '%s/%s/%d/%s' % (model, data, lanes, 'bounded' if bounded else 'four')


# ---- every translation unit the GPU tests ask for ---------------------------------------------------------------------------------------------
def prepare_units(ctx_factory):
    """compiles the loss units of tests/test_gpu_batch_loss.py on compile-only contexts made by ctx_factory() (build() and
    tests/test_cpu_batch_loss.py); returns how many were asked for"""
    n = 0
    tape4 = part_a()[0]
    tape2 = trace_model(M.model_exp2, 4)
    c = ctx_factory()
    try:
        for loss in LOSSES:
            c.set_batch_loss(loss, 1.0)
            for lanes in (64, 16, 256):
                c.set_batch_lanes(lanes)
                c.set_model(tape4)
                for a in (SETS if lanes == 64 else EDGE_SETS):
                    c.batch_prepare(a); n += 1
                c.batch_prepare(SETS[7], bounded=True); n += 1
                c.set_model(tape2)
                c.batch_prepare(ACTIVE2); n += 1
                c.batch_prepare(ACTIVE2, bounded=True); n += 1
        c.set_batch_loss(0, 1.0)
        c.set_model(tape2)          # (the plain path's units of model_exp2 under set_loss: what Context.covariance runs in test 5)
        for loss in LOSSES:
            c.set_loss(loss)
            for store in (True, False):
                c.model_prepare_form(ACTIVE2, 1, store); n += 1
        c.set_loss(0)
    finally:
        c.close()
    c = ctx_factory()          # (a context keeps the data form it was given: the cube's units on one of their own)
    try:
        c.set_model(tape2)
        x, Y, _ = cube()
        try:
            c.set_batch_cube(x, Y, CUBE_ERROR)
        except Exception as e:
            if 'no GPU' not in str(e):
                raise
        c.set_batch_loss(CUBE_LOSS, CUBE_SCALE)
        for lanes in (64, 16, 256):
            c.set_batch_lanes(lanes)
            c.batch_prepare(ACTIVE2); n += 1
    finally:
        c.close()
    return n
