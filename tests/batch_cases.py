"""The inputs of tests/batch_form_suite.py and tests/test_gpu_batch_shapes.py that the three forms share, and the rule that selects which inputs a device fit may be
held against (tests/test_cpu_batch_cases.py runs the rule and the compilations without a GPU).  What differs per form -- the lengths
of Part 1 among it -- is the table of tests/batch_form_cases.py.  Everything here is deterministic and needs no GPU.

THE SELECTION RULE.  Past convergence, accept / reject in Levenberg-Marquardt is decided by rounding.  A fit is
compared with the device only if the oracle agrees with itself on it:
 1. its point sums cut into three images (n_images=3: another order of additions) give the same (iterations, n_sweeps, n_chi2,
    n_omega, exit_reason) as n_images=1,
 2. and fitted parameters within SELF_TOL = 1e-12 relative;
 3. every comparison 'new_chi2 < old_chi2' it makes in STEP 4, whether the step is then accepted or rejected, has
    |new_chi2 - old_chi2| / old_chi2 > MARGIN = TOL_PASS = 2e-13 (orc_fit_result.min_margin: the oracle reports the closest one).
    That comparison is the loop's one data-dependent decision, and two implementations that are held to TOL_PASS per pass are not
    held to the sign of a difference below it.  (1) does not see such a decision in a short spectrum, where three images add the
    same numbers in nearly the same order, nor where the implementations differ in how they round the model function and not in
    the order of the sum.
The rule is evaluated by the oracle alone; the device's results never enter it.  Cases that fail it leave the fit comparisons only
(their first pass is still compared), and each part has a cap on how many may.

Part 1: model_exp2, spectrum_n(n, s) with the lengths n at the edges of each form's row of lanes (tests/batch_form_cases.py).
Part 2: model_exp4, every active count 1 ... 8, lists in the caller's order.
Part 3: the whole operator set: p[0] e_0(p, x) + ... + p[4] e_4(p, x) with the random expressions of tests/test_gpu_random_models.py,
and one written model for the three operators those expressions never draw (erf, a bare abs, unary minus)."""
import functools

import numpy as np

from gadfit_amd import ad
from gadfit_amd.ad import trace_model
from oracle import binding as orc
from tests import models as M
from tests.batch_common import COUNTS, TOL_PASS, spectrum4
from tests.test_gpu_random_models import NP_, _rand_expr

SELF_TOL = 1e-12
MARGIN = TOL_PASS


def _fit(tape, x, y, w, start, active, kw, n_images):
    p = orc.OracleProblem(tape, [x], [y], [w], [start], active, [0] * tape.n_pars)
    r = p.fit(n_images=n_images, **kw)
    return (tuple(int(getattr(r, f)) for f in COUNTS), p.pars.ravel().copy(), float(r.lambda_), float(r.chi2)), float(r.min_margin)


def oracle_fit(tape, x, y, w, start, active, kw, n_images):
    """OracleProblem.fit of one spectrum: ((iterations, n_sweeps, n_chi2, n_omega, exit_reason), fitted parameters, lambda, chi2)"""
    return _fit(tape, x, y, w, start, active, kw, n_images)[0]


def select(tape, x, y, w, start, active, kw):
    """the selection rule: (kept, the n_images=1 result of oracle_fit, the parameters' relative difference between 1 and 3 images,
    the closest chi2 comparison of the n_images=1 fit)"""
    one, margin = _fit(tape, x, y, w, start, active, kw, 1)
    three = oracle_fit(tape, x, y, w, start, active, kw, 3)
    diff = float(np.max(np.abs(one[1] - three[1]) / np.abs(one[1])))
    return one[0] == three[0] and diff <= SELF_TOL and margin > MARGIN, one, diff, margin


class Batch:
    """spectra back to back, as set_batch_data takes them"""

    def __init__(self, items):
        self.items = items                                   # each (x, y, w)
        self.n = np.array([it[0].size for it in items])
        self.off = np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64)
        self.x = np.concatenate([it[0] for it in items]); self.y = np.concatenate([it[1] for it in items])
        self.w = np.concatenate([it[2] for it in items])

    def first(self, k):
        e = self.off[k]
        return self.off[:k + 1], self.x[:e], self.y[:e], self.w[:e]


# ---- Part 1: the spectra of model_exp2 (their lengths per form: tests/batch_form_cases.py) ------------------------------------------
def spectrum_n(n, s):
    u = (M.splitmix64(4, M.SEED + 3000 * (s + 1) + n) >> np.uint64(11)).astype(np.float64) / 9007199254740992.0
    truth = M.EXP2_TRUTH * (0.8 + 0.4 * u)
    x, y, sigma = M.make_single(M.exp2_numpy, truth, n, 0.5, 100.0, seed=M.SEED + 17 * s + n)
    return truth, x, y, 1.0 / sigma, sigma


# ---- Part 2: every active count, in the caller's order (model_exp4, the 48 spectra of batch_common.spectrum4) -------------------
EXP4_SETS = ([3], [0, 1], [6, 1, 4], [0, 2, 4, 6], [7, 0, 3, 2, 5], [0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 7])
# under 'short' the amplitudes alone ([0, 2, 4, 6]) are a linear fit: it converges in one step and then hangs on rounding (19 of its 48
# fits fail the rule), so the four-parameter set of 'short' is another one (tests/test_cpu_batch_cases.py holds the rule over it)
EXP4_SHORT_FOUR = [0, 1, 2, 3]
EXP4_ARGS = {
    'conv': (0.05, dict(lambda_=1.0, max_iter=50, chi2_rel=1e-6)),
    'short': (0.3, dict(lambda_=1e-6, max_iter=3, accth=0.9)),
}
# the caller's order reaches DTD_min, the G[] columns and GFH_BACT: the same fit under two orders of the same set.  J^T J's diagonal for
# parameters 6, 1, 4 at these starts lies in [4.8e4, 2.0e5], [4.0e3, 1.6e4], [4.0e3, 1.9e4], so of the first pair's values none
# reaches max(DTD_min, diag); the second pair's do for parameters 6 and 4 (tests/test_cpu_batch_cases.py asserts that they change
# every fit), and a value that lands on another column changes the fit grossly
EXP4_ORDER = {
    'small': (([6, 1, 4], [1e-3, 1e3, 1.0]), ([1, 4, 6], [1e3, 1.0, 1e-3])),
    'binding': (([6, 1, 4], [1e6, 1e3, 1e5]), ([1, 4, 6], [1e3, 1e5, 1e6])),
}
EXP4_ORDER_ARGS = (0.3, dict(lambda_=1.0, max_iter=3))


def exp4_sets(name):
    return [EXP4_SHORT_FOUR if name == 'short' and list(a) == [0, 2, 4, 6] else list(a) for a in EXP4_SETS]


@functools.lru_cache(maxsize=None)
def part2():
    """(tape, truths [48][8], Batch)"""
    sp = [spectrum4(b) for b in range(48)]
    return trace_model(M.model_exp4, 8), np.array([it[0] for it in sp]), Batch([it[1:4] for it in sp])


def part2_starts(active, off):
    starts = part2()[1].copy()
    sign = np.where(np.arange(8) % 2 == 0, 1.0 + off, 1.0 - off)
    starts[:, active] *= sign[active]
    return starts


@functools.lru_cache(maxsize=None)
def part2_selection(active, off, kw_items, dtd=None):
    """the rule over the 48 spectra (hashable arguments: active a tuple, kw_items = tuple(sorted(kw.items())), dtd a tuple or None)"""
    tape, _, batch = part2()
    kw = dict(kw_items)
    if dtd is not None:
        kw['DTD_min'] = list(dtd)
    starts = part2_starts(list(active), off)
    return [select(tape, *batch.items[b], starts[b], list(active), kw) for b in range(48)]


def part2_select(active, off, kw, dtd=None):
    return part2_selection(tuple(active), off, tuple(sorted(kw.items())), None if dtd is None else tuple(dtd))


# ---- Part 3: the whole operator set -------------------------------------------------------------------------------------------
RANDOM_SEEDS = tuple(range(32))
# _rand_expr indexes its table of unary functions with (op - 12) % 18 for op < 27, so erf, a bare abs and unary minus (entries 15, 16,
# 17) are never drawn: one written model brings them through the same comparisons under the seed number after the random ones
ERF_NEG_SEED = 32
OPERATOR_SEEDS = RANDOM_SEEDS + (ERF_NEG_SEED,)
ERF_NEG_ACTIVE = [4, 1, 0, 3, 2]
RANDOM_LENGTHS = (5, 6, 37, 64, 65, 200)
RANDOM_ARGS = {
    # acc_ratio > accth never holds, so delta2 is always kept: one iteration is old + delta1 + delta2 / 2 of a well-damped system
    'i': dict(lambda_=10.0, max_iter=1, accth=1e30),
    'ii': dict(lambda_=1.0, max_iter=3, accth=0.75),
    'iii': dict(lambda_=1e-3, max_iter=3),
}
RANDOM_CAP = 0.05                  # of the fit comparisons of Part 3 may fail the rule; none of the pass comparisons is dropped


def random_model(seed):
    def model(p, x):
        r = np.random.default_rng(1000 + seed)           # the same stream at every trace
        y = p[0] * _rand_expr(r, p, x, 3)
        for k in range(1, NP_):
            y = y + p[k] * _rand_expr(r, p, x, 3)
        return y
    return model


def model_erf_neg(p, x):
    """unary minus of an AD variable is recorded as 0.0 - a (as the reference's subtract_advar does), of a real expression in x as a
    NEG node: both are here"""
    return p[0] * ad.erf(p[1] * x - 1.0) + p[2] * (-abs(p[3] - x)) + p[4] * ad.erf((-x) / p[1])


def model_values(tape, pars, x):
    """f(pars, x) as the oracle evaluates it: sweep()'s residuals are (y - f) w"""
    p = orc.OracleProblem(tape, [x], [np.zeros_like(x)], [np.ones_like(x)], [pars], [0], [0] * tape.n_pars)
    return -p.sweep()[2]


@functools.lru_cache(maxsize=None)
def part3(seed):
    """(tape, active list, starts [8][5], Batch): one batch of eight spectra and one active list per seed"""
    tape = trace_model(model_erf_neg if seed == ERF_NEG_SEED else random_model(seed), NP_)
    g = np.random.default_rng(5000 + seed)
    active = [int(v) for v in g.permutation(NP_)[:int(g.integers(1, NP_ + 1))]]
    if seed == ERF_NEG_SEED:
        active = list(ERF_NEG_ACTIVE)
    items, starts = [], []
    for _ in range(8):
        n = int(g.choice(RANDOM_LENGTHS))
        x = np.sort(g.uniform(0.3, 1.6, n))
        truth = g.uniform(0.6, 1.8, NP_)
        w = 20.0 * g.uniform(0.5, 2.0, n)
        y = model_values(tape, truth, x) + g.standard_normal(n) / w
        starts.append(truth * g.uniform(0.9, 1.1, NP_))
        items.append((x, y, w))
    return tape, active, np.array(starts), Batch(items)


@functools.lru_cache(maxsize=None)
def part3_selection(seed, name):
    tape, active, starts, batch = part3(seed)
    return [select(tape, *batch.items[b], starts[b], active, RANDOM_ARGS[name]) for b in range(8)]


# ---- every batch translation unit the GPU tests ask for -----------------------------------------------------------------------
# a seed of Part 3 whose model has an advar ** advar or real ** advar node (the generated source then calls gfh_pow_ln) and four active
# parameters: its pass is repeated on a context created under GADFIT_HIP_FAST_DIV=0, where pow, log and the divisions are the library's
RANDOM_POW_SEED = 5


def part2_units():
    """[(tape, active list)] of Part 2: the ten active lists, whichever form runs them"""
    seen = []
    for a in [a for name in sorted(EXP4_ARGS) for a in exp4_sets(name)] + [o[0] for pair in EXP4_ORDER.values() for o in pair]:
        if list(a) not in seen:
            seen.append(list(a))
    return [(part2()[0], a) for a in seen]


def operator_units():
    """[(tape, active list)] of Part 3 under the default switches; RANDOM_POW_SEED's unit is asked for once more under GADFIT_HIP_FAST_DIV=0"""
    return [part3(seed)[:2] for seed in OPERATOR_SEEDS]
