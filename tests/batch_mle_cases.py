"""The inputs of tests/test_cpu_batch_mle.py and tests/test_gpu_batch_mle.py: batched fits under the Poisson maximum-likelihood estimator
(gfh_set_batch_estimator(1)), their reference and the rule that selects which fits a device fit may be held against count for count.
Everything here is deterministic and needs no GPU; nothing a device returns enters the rule.

THE SPECTRA.  model_exp2 with its four parameters active at the lengths LENGTHS: n = na and the row edges of the three lane forms.  The
counts are Poisson draws by inverse CDF (a sequential search on the CDF) from splitmix64 uniforms; no numpy generator is used.  The means
are exp2_numpy(truth * s, x), s on the two amplitudes, in two regimes: s = 1 ('low': a few counts per bin at the head, mostly zeros
behind it) and s = 40 ('high').  The grid is that of tests/batch_cube_cases.py.  A second set, model_exp4 with its eight parameters
active, holds four spectra of 128 ... 300 points at s = 40.

THE REFERENCE PASS at parameters P.  f comes from orc.eval_reverse point by point; OracleProblem(..., w = m / sqrt(f)).sweep(n_images) is
the reference's own least-squares pass at those weights and gives alpha = sum g g^T / f and beta = sum g (y - f) / f: Fisher scoring has
no second statement here.  The deviance D = 2 sum [f - y + y ln(y / f)] over the unmasked points (2 f at y = 0; NaN where f <= 0, y < 0
or an operand is not finite) is summed in numpy.longdouble.

THE REFERENCE FIT is the loop of gfh_k_fit_batch (device/batch_fit_kernels.hip) restated over those passes with orc.potr, in the style
of lm_loop_cases.lm_iterate_restated: the first deviance (NaN: exit 8), the sweep, the running maximum of alpha's diagonal, the damped
solve (not positive definite: exit 8), the trials with new < old, lambda / lam_down and lam_up * lambda, exit 7, and STEP 5's chi2_abs,
chi2_rel, rel_error and max_iter in the reference's order, with D in the place of chi2.  It returns the counts, the parameters, lambda,
D and two margins: the closest relative distance of any `new < old` from equality, and of any fired or unfired exit test from its
threshold.

THE RULE.  A fit is KEPT if the reference at n_images = 1 and at 3 (and with the points reversed: below) gives equal counts, parameters within SELF_TOL = TOL_FIT / 10, every
acceptance margin > ACCEPT_MARGIN = 1e-9 and every exit margin > EXIT_MARGIN = 1e-3.  The margins are conditions, as in lm_loop_cases:
the deviance's rounding sits near 1e-14 relative on these inputs.  One condition is added, because that last sentence does not hold
where a fit interpolates its points (n = na: D falls to 1e-7 and below while its terms stay of order one): every deviance the loop
evaluates must be RESOLVED in doubles, bound / D <= RESOLVED = TOL_FIT / TOL_PASS = 500 with bound = 2 sum (|f - y| + |y ln(y / f)|) the
cancellation bound of the sum.  A pass is held to TOL_PASS x bound absolute, so D is known to TOL_FIT relative only up to that ratio, and
the acceptance margin of 1e-9 then stands 1e4 above the rounding of either side.  And one evaluation is added to the two: the reference
with the POINTS REVERSED, held to the same conditions against n_images = 1.  Cutting a sum of four or five points into three images
reorders nothing, so for the shortest spectra the first condition compared the reference with itself bit for bit -- and the all-zero
spectrum of n = 4, whose alpha has kappa_2 = 1e12 on the way to f = 0, passed it while the reversed sum moves its parameters by 1e-7
(scenario b) and 6e-4 (d).  Both additions are decided by the reference alone, like the rest.
At most one fit in five may be dropped per scenario (CAP).  The
scenarios are batch_common.SCENARIOS a, b and d; c carries accth, which the estimator refuses."""
import functools

import numpy as np

from gadfit_amd.ad import trace_model
from oracle import binding as orc
from tests import batch_cases as BC
from tests import batch_cube_cases as CU
from tests import models as M
from tests.batch_common import SCENARIOS, TOL_FIT, TOL_PASS, start_of

LSQ, POISSON = 0, 1
ACTIVE = [0, 1, 2, 3]
ACTIVE8 = list(range(8))
LENGTHS = (4, 5, 15, 16, 17, 33, 63, 64, 65, 129, 255, 256, 257, 513)
REGIMES = {'low': 1.0, 'high': 40.0}
NAMES = ('a', 'b', 'd')
SELF_TOL = TOL_FIT / 10
ACCEPT_MARGIN = 1e-9
EXIT_MARGIN = 1e-3
RESOLVED = TOL_FIT / TOL_PASS
CAP = 0.2
MLE_SEED = 9000000
EXP4_LENGTHS = (128, 185, 243, 300)
EXP4_NAMES = ('a', 'b')
FORM_LENGTHS = {16: (4, 5, 15, 16, 17, 33), 64: (4, 5, 63, 64, 65, 129), 256: (4, 255, 256, 257, 513)}


@functools.lru_cache(maxsize=None)
def tape2():
    return trace_model(M.model_exp2, 4)


@functools.lru_cache(maxsize=None)
def tape4():
    return trace_model(M.model_exp4, 8)


def uniforms(n, seed):
    return (M.splitmix64(n, seed) >> np.uint64(11)).astype(np.float64) / 9007199254740992.0


def poisson_counts(mean, u):
    """one Poisson draw per mean by inverse CDF: the smallest k with CDF(k) >= u, found by a sequential search"""
    out = np.zeros(mean.size)
    for i, (mu, ui) in enumerate(zip(mean, u)):
        k, p = 0, np.exp(-mu)
        c = p
        while ui > c and k < 100000:
            k += 1
            p *= mu / k
            c += p
        out[i] = k
    return out


def scaled_truth(truth, s):
    return truth * np.where(np.arange(truth.size) % 2 == 0, s, 1.0)


def truth_of(n, regime, seed=0):
    u = uniforms(4, M.SEED + MLE_SEED + 5000 * (seed + 1) + n)
    return scaled_truth(M.EXP2_TRUTH * (0.8 + 0.4 * u), REGIMES[regime])


@functools.lru_cache(maxsize=None)
def spectrum(n, regime, seed=0):
    """(truth, x, y, w): counts of model_exp2 on n points; w = 1 everywhere (a mask that masks nothing)"""
    truth = truth_of(n, regime, seed)
    x = CU.grid(n)
    y = poisson_counts(M.exp2_numpy(truth, x), uniforms(n, M.SEED + MLE_SEED + 37 * seed + 11 * n + (1 if regime == 'low' else 2)))
    for a in (truth, x, y):
        a.setflags(write=False)
    return truth, x, y, np.ones(n)


@functools.lru_cache(maxsize=None)
def spectrum4(k):
    n = EXP4_LENGTHS[k]
    u = uniforms(8, M.SEED + MLE_SEED + 7000 * (k + 1))
    truth = scaled_truth(M.EXP4_TRUTH * (0.9 + 0.2 * u), 40.0)
    x = 0.05 + 99.95 * (np.arange(n, dtype=np.float64) + 0.5) / n
    y = poisson_counts(M.exp4_numpy(truth, x), uniforms(n, M.SEED + MLE_SEED + 13 * k + 3))
    return truth, x, y, np.ones(n)


def order(lengths=LENGTHS):
    """[(n, regime)] in batch order: short beside long, both regimes of a length side by side"""
    ln = sorted(lengths)
    seq = []
    while ln:
        seq.append(ln.pop(0))
        if ln:
            seq.append(ln.pop())
    return [(n, r) for n in seq for r in ('low', 'high')]


@functools.lru_cache(maxsize=None)
def batch(lengths=LENGTHS):
    """(order, Batch, truths): the spectra of model_exp2 back to back"""
    od = order(lengths)
    sp = [spectrum(n, r) for n, r in od]
    return od, BC.Batch([(x, y, w) for _, x, y, w in sp]), np.array([t for t, _, _, _ in sp])


def starts(lengths, off):
    return np.array([start_of(t, off) for t in batch(lengths)[2]])


@functools.lru_cache(maxsize=None)
def batch4():
    sp = [spectrum4(k) for k in range(len(EXP4_LENGTHS))]
    return BC.Batch([(x, y, w) for _, x, y, w in sp]), np.array([t for t, _, _, _ in sp])


def starts4(off):
    return np.array([t * np.where(np.arange(8) % 2 == 0, 1.0 + off, 1.0 - off) for t in batch4()[1]])


# ---- the reference pass --------------------------------------------------------------------------------------------------------------
def model_values(tape, x, P):
    mask = [0] * tape.n_pars
    return np.array([orc.eval_reverse(tape, float(xv), P, mask)[0] for xv in x])


def deviance_terms(y, f, m):
    """the terms of D in longdouble, and the terms of its cancellation bound |f - y| + |y ln(y / f)|"""
    yl, fl = np.asarray(y, dtype=np.longdouble), np.asarray(f, dtype=np.longdouble)
    with np.errstate(divide='ignore', invalid='ignore'):
        lg = np.where(yl == 0, np.longdouble(0), yl * np.log(yl / fl))
        t = np.where(yl == 0, 2 * fl, 2 * ((fl - yl) + lg))
        bad = ~((fl > 0) & np.isfinite(fl) & (yl >= 0) & np.isfinite(yl))
        t = np.where(bad, np.longdouble('nan'), t)
        bound = np.abs(fl - yl) + np.abs(lg)
    keep = np.asarray(m) != 0
    return np.where(keep, t, np.longdouble(0)), np.where(keep, bound, np.longdouble(0))


def deviance(tape, x, y, m, P):
    """(D, its cancellation bound 2 sum (|f - y| + |y ln(y / f)|)) at P"""
    t, bound = deviance_terms(y, model_values(tape, x, P), m)
    return float(np.sum(t)), float(2 * np.sum(bound))


def reference_pass(tape, x, y, m, P, active, n_images=1):
    """(alpha, beta, D, the cancellation bound 2 sum (|f - y| + |y ln(y / f)|) of D) at P"""
    f = model_values(tape, x, P)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.where(np.asarray(m) != 0, 1.0, 0.0) / np.sqrt(f)
    p = orc.OracleProblem(tape, [x], [y], [w], [P], list(active), [0] * tape.n_pars)
    A, b, _, _ = p.sweep(n_images)
    t, bound = deviance_terms(y, f, m)
    return A, b, float(np.sum(t)), float(2 * np.sum(bound))


# ---- the reference fit ---------------------------------------------------------------------------------------------------------------
def _solve(A, DTD, lam, b):
    """the damped solve, or None where the matrix is not positive definite (or not finite)"""
    Ad = A + lam * np.diag(DTD)
    if not (np.all(np.isfinite(Ad)) and np.all(np.isfinite(b))):
        return None
    try:
        d = orc.potr(Ad, b)
    except Exception:
        return None
    return d if np.all(np.isfinite(d)) else None


def restated_fit(tape, x, y, m, start, active, kw, n_images=1):
    """gfh_k_fit_batch's loop under GFH_BMLE over reference_pass: ((iterations, n_sweeps, n_chi2, n_omega, exit_reason), parameters,
    lambda, D, the acceptance margin, the exit margin, the largest bound / D of the deviances evaluated)"""
    active = list(active)
    na = len(active)
    lam, lam_up, lam_down, lam_incs = float(kw.get('lambda_', 1.0)), float(kw.get('lam_up', 10.0)), float(kw.get('lam_down', 10.0)), int(kw.get('lam_incs', 2))
    max_iter = int(kw['max_iter'])
    P = np.array(start, dtype=np.float64)
    old = P[active].copy()
    DTD = np.zeros(na)
    dof_ = int(x.size) - na
    dof = 1.0 if dof_ == 0 else float(dof_)
    accept, exits = np.inf, np.inf
    old_D, bound = deviance(tape, x, y, m, P)
    unresolved = bound / old_D if old_D == old_D else 0.0
    it, n_sweeps, n_chi2, reason = 0, 0, 1, -1
    if old_D != old_D:
        reason = 8
    while reason < 0:
        A, b, _, _ = reference_pass(tape, x, y, m, P, active, n_images)
        n_sweeps += 1
        DTD = np.maximum(DTD, np.diag(A))
        delta = _solve(A, DTD, lam, b)
        if delta is None:
            reason = 8
            break
        P[active] = P[active] + delta
        new_D = 0.0
        for i in range(1, lam_incs + 2):
            new_D, bound = deviance(tape, x, y, m, P)
            n_chi2 += 1
            if new_D == new_D:
                accept = min(accept, abs(new_D - old_D) / old_D)
                unresolved = max(unresolved, bound / new_D)
            if new_D < old_D:
                lam = lam / lam_down
                break
            elif i <= lam_incs:
                lam = lam_up * lam
                P[active] = old
                delta = _solve(A, DTD, lam, b)
                if delta is None:
                    reason = 8
                    break
                P[active] = P[active] + delta
            else:
                P[active] = old
                reason = 7
                break
        if reason >= 0:
            break
        old = P[active].copy()
        old_old, old_D = old_D, min(old_D, new_D)
        it += 1
        if 'chi2_abs' in kw:
            v, thr = old_D / dof, float(kw['chi2_abs'])
            exits = min(exits, abs(v - thr) / abs(thr))
            if v < thr:
                reason = 1
                break
        if 'chi2_rel' in kw:
            v, thr = (old_old - old_D) / old_D, float(kw['chi2_rel'])
            exits = min(exits, abs(v - thr) / abs(thr))
            if v < thr:
                reason = 2
                break
        if 'rel_error' in kw:
            v, thr = np.abs(delta / P[active]), float(kw['rel_error'])
            exits = min(exits, float(np.min(np.abs(v - thr) / abs(thr))))
            if not np.any(v > thr):
                reason = 5
                break
        if it >= max_iter:
            reason = 0
            break
    return (it, n_sweeps, n_chi2, 0, reason), P, lam, old_D, float(accept), float(exits), float(unresolved)


def select(tape, x, y, m, start, active, kw):
    """the rule: (kept, (counts, parameters, lambda, D) of the n_images = 1 fit, the parameters' relative difference between 1 and 3
    images, (acceptance margin, exit margin, the largest bound / D))"""
    one = restated_fit(tape, x, y, m, start, active, kw, 1)
    others = (restated_fit(tape, x, y, m, start, active, kw, 3),
              restated_fit(tape, np.ascontiguousarray(x[::-1]), np.ascontiguousarray(y[::-1]), np.ascontiguousarray(np.asarray(m)[::-1]), start, active, kw, 1))
    act = list(active)
    with np.errstate(divide='ignore', invalid='ignore'):
        diff = float(max(np.max(np.abs(one[1][act] - o[1][act]) / np.abs(one[1][act])) for o in others))
    every = (one,) + others
    margins = (min(f[4] for f in every), min(f[5] for f in every), max(f[6] for f in every))
    ok = (all(o[0] == one[0] for o in others) and diff <= SELF_TOL and margins[0] > ACCEPT_MARGIN and margins[1] > EXIT_MARGIN
          and margins[2] <= RESOLVED)
    return bool(ok), one[:4], diff, margins


@functools.lru_cache(maxsize=None)
def selection(name, lengths=LENGTHS):
    """the rule over the batch of model_exp2 under scenario `name`, in batch order (cached: one evaluation serves every lane form)"""
    off, kw = SCENARIOS[name]
    _, b, _ = batch(lengths)
    st = starts(lengths, off)
    return [select(tape2(), x, y, w, st[k], ACTIVE, kw) for k, (x, y, w) in enumerate(b.items)]


def form_selection(name, lanes):
    """selection() restricted to the lengths of a lane form: the fits of batch(FORM_LENGTHS[lanes]), each taken from the one evaluation"""
    full = {k: s for k, s in zip(order(), selection(name))}
    return [full[k] for k in order(FORM_LENGTHS[lanes])]


@functools.lru_cache(maxsize=None)
def selection4(name):
    off, kw = SCENARIOS[name]
    b, _ = batch4()
    st = starts4(off)
    return [select(tape4(), x, y, w, st[k], ACTIVE8, kw) for k, (x, y, w) in enumerate(b.items)]


# ---- the estimator's reason: the bias of 1 / sqrt(y) weights at a few counts per bin --------------------------------------------------
BIAS_N, BIAS_SPECTRA, BIAS_ACTIVE = 64, 64, [0, 2]
BIAS_KW = dict(lambda_=1.0, max_iter=50, chi2_rel=1e-10)


def bias_spectrum(seed):
    """(truth, x, y): the s = 1 regime with ONE truth for all seeds, so that the mean over the seeds is an estimate of the bias"""
    truth = scaled_truth(M.EXP2_TRUTH, REGIMES['low'])
    x = CU.grid(BIAS_N)
    return truth, x, poisson_counts(M.exp2_numpy(truth, x), uniforms(BIAS_N, M.SEED + MLE_SEED + 100003 * (seed + 1)))


# ---- data forms, isolation, bounds ---------------------------------------------------------------------------------------------------
CUBE_N = {16: 33, 64: 65, 256: 257}
CUBE_FITS = 5


def cube(lanes):
    """(x [n], Y [5][n] uint16, starts [5][4], the same as ragged items): spectra of the 'high' regime of one length, seeds 0 ... 4"""
    n = CUBE_N[lanes]
    sp = [spectrum(n, 'high', s) for s in range(CUBE_FITS)]
    Y = np.ascontiguousarray(np.array([y for _, _, y, _ in sp]).astype(np.uint16))
    assert np.array_equal(Y.astype(np.float64), np.array([y for _, _, y, _ in sp]))
    return sp[0][1].copy(), Y, np.array([start_of(t, 0.05) for t, _, _, _ in sp]), [(x, y, w) for _, x, y, w in sp]


ISOLATION_FITS, ISOLATION_N = 7, {16: 33, 64: 65, 256: 257}
ISOLATION_BAD = (3, 5)


def isolation(lanes):
    """(items, starts) of 7 fits of the 'high' regime: fit 3 holds a negative sample, fit 5 starts with a negative amplitude -- that of
    the slow component, so that the model is negative in the tail of every grid and the first deviance is NaN"""
    n = ISOLATION_N[lanes]
    sp = [spectrum(n, 'high', 10 + s) for s in range(ISOLATION_FITS)]
    items = [(x.copy(), y.copy(), w.copy()) for _, x, y, w in sp]
    items[3][1][n // 2] = -1.0
    st = np.array([start_of(t, 0.05) for t, _, _, _ in sp])
    st[5, 2] = -st[5, 2]
    return items, st


WALL_ACTIVE = [0, 1, 2]          # the decay time of the second component stays passive: with its amplitude at 0 the counts say nothing of it
WALL_KW = dict(lambda_=1.0, max_iter=200)          # no exit test: the loop runs until no trial lowers D any more (exit 7), a converged fit


def wall_case(lanes):
    """(items, starts, lower, upper) over WALL_ACTIVE: four spectra of the 'high' regime whose counts hold the FIRST component alone, lower
    = 0 on both amplitudes, the second amplitude starting on its wall.  Behind the first component's few decay times every bin is
    empty, and there a positive second amplitude only adds its 2 f to D: the data push it through the wall (the GPU module asserts
    beta < 0 from the reference at the start and at the end)."""
    n = ISOLATION_N[lanes]
    items, st = [], []
    for s in range(4):
        truth = np.array(truth_of(n, 'high', 20 + s))
        truth[2] = 0.0
        x = CU.grid(n)
        y = poisson_counts(M.exp2_numpy(truth, x), uniforms(n, M.SEED + MLE_SEED + 53 * s + n + 7))
        start = start_of(truth, 0.05)
        start[2] = 0.0
        items.append((x, y, np.ones(n))); st.append(start)
    inf = float('inf')
    return items, np.array(st), np.array([0.0, -inf, 0.0]), np.array([inf, inf, inf])


# ---- every translation unit the GPU tests ask for -------------------------------------------------------------------------------------
def prepare_units(ctx_factory):
    """compiles the Poisson units of tests/test_gpu_batch_mle.py on compile-only contexts made by ctx_factory() (build() and
    tests/test_cpu_batch_mle.py); returns how many were asked for"""
    n = 0
    c = ctx_factory()
    try:
        c.set_batch_estimator(POISSON)
        for lanes in (64, 16, 256):
            c.set_batch_lanes(lanes)
            c.set_model(tape2())
            c.batch_prepare(ACTIVE); n += 1
            c.batch_prepare(ACTIVE, bounded=True); n += 1
            c.batch_prepare(WALL_ACTIVE, bounded=True); n += 1
        c.set_batch_lanes(64)
        c.set_model(tape4())
        c.batch_prepare(ACTIVE8); n += 1
    finally:
        c.close()
    c = ctx_factory()          # (a context keeps the data form it was given: the cube's units, which the frames share, on one of their own)
    try:
        c.set_model(tape2())
        c.set_batch_estimator(POISSON)
        for lanes in (64, 16, 256):
            x, Y, _, _ = cube(lanes)
            try:
                c.set_batch_cube(x, Y, 0)
            except Exception as e:
                if 'no GPU' not in str(e):
                    raise
            c.set_batch_lanes(lanes)
            c.batch_prepare(ACTIVE); n += 1
    finally:
        c.close()
    return n
