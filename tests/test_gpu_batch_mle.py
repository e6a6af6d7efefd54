"""Batched fits under the Poisson maximum-likelihood estimator on the device (gfh_set_batch_estimator(1); the GFH_BMLE arm of the batch
kernels).  Inputs, the reference pass (the oracle's least-squares pass at the weights 1 / sqrt(f), the deviance in longdouble), the
restated reference fit and the selection rule: tests/batch_mle_cases.py; tests/test_cpu_batch_mle.py runs the rule over the same cases
without a GPU.  Every unit asked for is one the build has compiled.  Every launch asserts the estimator and the lane form it ran under.

1. batch_pass at the starts against the reference pass on 64, 16 and 256 lanes: alpha and beta scaled as batch_common.pass_worst
   scales them within TOL_PASS; D against longdouble within TOL_PASS x 2 sum (|f - y| + |y ln(y / f)|), the bound of the term's cancellation.
2. Whole fits against the restated reference on the three forms: counts, dof and exit reasons equal on the kept fits, lambda within
   TOL_LAMBDA, parameters and D within TOL_FIT.
3. The same counts as a uint16 cube under NONE and as frames: the ragged form's bits.
4. A batch of 7 with a negative sample in fit 3 and a negative amplitude at the start of fit 5: those end with exit 8 or 7, the other
   five are bit for bit what they are in a batch without them.
5. After estimator 1 and then 0 a least-squares fit is bit for bit that of a context that never heard of the setting.
6. Under an infinite box fit_batch_bounded returns fit_batch's bits; with lower = 0 on both amplitudes and a start on the wall pushed
   outward at_bound has the bit and the free parameters are a stationary point of the reduced system.
7. fit_batch_errors: cov against the longdouble inverse of the oracle's alpha at the fitted parameters within the bound of
   tests/test_gpu_batch_cov.py; under scale=True it is cov times D / dof.
The observed maxima go where the other batch modules' go (GADFIT_BATCH_OBSERVE), under mle_*."""
import numpy as np
import pytest

from tests import batch_cases as BC
from tests import batch_cov_cases as CV
from tests import batch_mle_cases as MC
from tests.batch_common import SCENARIOS, TOL_FIT, TOL_PASS, check_fit, context, fit_worst, observe, same_bits, same_pass

pytestmark = pytest.mark.gpu

FORMS = (64, 16, 256)
INF = float('inf')
A4 = MC.ACTIVE
KW_A = SCENARIOS['a'][1]


def _used(c, lanes, estimator=MC.POISSON):
    assert c.batch_estimator_used() == estimator and c.batch_lanes_used() == lanes


def _pass_worst(tape, items, starts, active, JTJ, JTr, D):
    """a batch_pass under the estimator against the reference pass: (the worst of alpha and beta, scaled as batch_common.pass_worst
    scales them; the worst of |D - D0| over the cancellation bound of D0)"""
    worst, worst_d = 0.0, 0.0
    for b, (x, y, w) in enumerate(items):
        A0, b0, D0, bound = MC.reference_pass(tape, x, y, w, starts[b], active)
        d = np.diag(A0)
        worst = max(worst, np.max(np.abs(JTJ[b] - A0) / (np.sqrt(np.outer(d, d)) + 1e-300)),
                    np.max(np.abs(JTr[b] - b0) / (np.sqrt(d * D0) + 1e-300)))
        worst_d = max(worst_d, abs(D[b] - D0) / bound)
        assert np.array_equal(JTJ[b], JTJ[b].T), b
    assert np.isfinite(worst) and np.isfinite(worst_d)
    return worst, worst_d


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_one_pass_against_the_reference(lanes):
    lengths = MC.FORM_LENGTHS[lanes]
    _, batch, _ = MC.batch(lengths)
    st = MC.starts(lengths, SCENARIOS['a'][0])
    c = context(MC.tape2(), batch)
    try:
        JTJ, JTr, D = c.batch_pass(st, A4, lanes_per_fit=lanes, estimator='poisson')
        _used(c, lanes)
    finally:
        c.close()
    w, wd = _pass_worst(MC.tape2(), batch.items, st, A4, JTJ, JTr, D)
    observe(**{'mle_pass_lanes%d_sums' % lanes: w, 'mle_pass_lanes%d_deviance_over_bound' % lanes: wd})
    assert w < TOL_PASS and wd < TOL_PASS


def test_one_pass_with_eight_active_parameters():
    batch, _ = MC.batch4()
    st = MC.starts4(SCENARIOS['a'][0])
    c = context(MC.tape4(), batch)
    try:
        JTJ, JTr, D = c.batch_pass(st, MC.ACTIVE8, lanes_per_fit=64, estimator=1)
        _used(c, 64)
    finally:
        c.close()
    w, wd = _pass_worst(MC.tape4(), batch.items, st, MC.ACTIVE8, JTJ, JTr, D)
    observe(mle_pass_na8_sums=w, mle_pass_na8_deviance_over_bound=wd)
    assert w < TOL_PASS and wd < TOL_PASS


def test_a_masked_point_leaves_every_sum():
    """w = 0 is the mask: a spectrum with points masked gives the pass of the spectrum without them, to the bound of a pass (the lanes
    add in another order); the value of a non-zero weight does not matter bit for bit"""
    truth, x, y, w = MC.spectrum(65, 'high')
    keep = np.ones(65, dtype=bool); keep[[3, 17, 64]] = False
    masked = np.where(keep, 7.5, 0.0)
    y_bad = y.copy(); y_bad[~keep] = -5.0          # what is masked may hold anything
    batch = BC.Batch([(x, y, w), (x, y_bad, masked), (x[keep], y[keep], w[keep])])
    st = np.tile(truth * 1.05, (3, 1))
    c = context(MC.tape2(), batch)
    try:
        JTJ, JTr, D = c.batch_pass(st, A4, lanes_per_fit=64, estimator=1)
        _used(c, 64)
    finally:
        c.close()
    assert np.all(np.isfinite(D)) and D[1] < D[0]
    d = np.diag(JTJ[2])
    assert np.max(np.abs(JTJ[1] - JTJ[2]) / np.sqrt(np.outer(d, d))) < TOL_PASS and np.max(np.abs(JTr[1] - JTr[2]) / np.sqrt(d * D[2])) < TOL_PASS
    assert abs(D[1] - D[2]) < TOL_PASS * MC.reference_pass(MC.tape2(), x[keep], y[keep], w[keep], st[2], A4)[3]


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', MC.NAMES)
@pytest.mark.parametrize('lanes', FORMS)
def test_fits_against_the_restated_reference(lanes, name):
    lengths = MC.FORM_LENGTHS[lanes]
    off, kw = SCENARIOS[name]
    _, batch, _ = MC.batch(lengths)
    c = context(MC.tape2(), batch)
    try:
        pars, res, _ = c.fit_batch(MC.starts(lengths, off), A4, lanes_per_fit=lanes, estimator='poisson', **kw)
        _used(c, lanes)
    finally:
        c.close()
    sel = MC.form_selection(name, lanes)
    assert sum(1 for s in sel if not s[0]) <= MC.CAP * len(sel)
    assert np.all(res['n_omega'] == 0)
    check_fit('mle_lanes%d' % lanes, name, fit_worst(sel, pars, res, batch.n, 4), TOL_FIT, TOL_FIT)


@pytest.mark.parametrize('name', MC.EXP4_NAMES)
def test_fits_with_eight_active_parameters(name):
    off, kw = SCENARIOS[name]
    batch, _ = MC.batch4()
    c = context(MC.tape4(), batch)
    try:
        pars, res, _ = c.fit_batch(MC.starts4(off), MC.ACTIVE8, lanes_per_fit=64, estimator=1, **kw)
        _used(c, 64)
    finally:
        c.close()
    sel = MC.selection4(name)
    assert sum(1 for s in sel if not s[0]) <= MC.CAP * len(sel)
    check_fit('mle_na8', name, fit_worst(sel, pars, res, batch.n, 8), TOL_FIT, TOL_FIT)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_a_uint16_cube_under_none_and_frames_return_the_ragged_forms_bits(lanes):
    x, Y, st, items = MC.cube(lanes)
    ragged = context(MC.tape2(), BC.Batch(items))
    cube = context(MC.tape2())
    frames = context(MC.tape2())
    try:
        p0, r0, _ = ragged.fit_batch(st, A4, lanes_per_fit=lanes, estimator=1, **KW_A)
        _used(ragged, lanes)
        assert ragged.batch_form_used() == 'ragged'
        pass0 = ragged.batch_pass(st, A4)
        _used(ragged, lanes)
        assert np.all(r0['iterations'] > 0) and np.all(np.isfinite(r0['chi2']))
        cube.set_batch_cube(x, Y, 0)
        frames.set_batch_frames(x, np.ascontiguousarray(Y.T), 0)
        for c in (cube, frames):
            p, r, _ = c.fit_batch(st, A4, lanes_per_fit=lanes, estimator=1, **KW_A)
            _used(c, lanes)
            assert c.batch_form_used() == ('cube', 2, 0)
            same_bits(p, r, p0, r0)
            same_pass(c.batch_pass(st, A4), pass0)
            _used(c, lanes)
    finally:
        for c in (ragged, cube, frames):
            c.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_a_fit_that_cannot_start_leaves_its_neighbours_alone(lanes):
    items, st = MC.isolation(lanes)
    good = [k for k in range(MC.ISOLATION_FITS) if k not in MC.ISOLATION_BAD]
    whole = context(MC.tape2(), BC.Batch(items))
    clean = context(MC.tape2(), BC.Batch([items[k] for k in good]))
    try:
        p, r, _ = whole.fit_batch(st, A4, lanes_per_fit=lanes, estimator=1, **KW_A)
        _used(whole, lanes)
        p0, r0, _ = clean.fit_batch(st[good], A4, lanes_per_fit=lanes, estimator=1, **KW_A)
        _used(clean, lanes)
    finally:
        whole.close(); clean.close()
    for k in MC.ISOLATION_BAD:
        assert int(r['exit_reason'][k]) in (8, 7), (k, r[k])
        assert int(r['iterations'][k]) == 0
    assert np.array_equal(p[5], st[5])          # nothing was accepted: the start comes back
    assert np.all(r0['iterations'] > 0) and np.all(np.isin(r0['exit_reason'], (0, 2)))
    same_bits(p[good], r[good], p0, r0)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_nothing_of_the_estimator_stays_behind(lanes):
    lengths = MC.FORM_LENGTHS[lanes]
    _, batch, _ = MC.batch(lengths)
    st = MC.starts(lengths, SCENARIOS['a'][0])
    plain = context(MC.tape2(), batch)          # a context that never heard of the setting
    c = context(MC.tape2(), batch)
    try:
        p0, r0, _ = plain.fit_batch(st, A4, lanes_per_fit=lanes, **KW_A)
        _used(plain, lanes, MC.LSQ)
        pass0 = plain.batch_pass(st, A4)
        p1, r1, _ = c.fit_batch(st, A4, lanes_per_fit=lanes, estimator=1, **KW_A)
        _used(c, lanes)
        p, r, _ = c.fit_batch(st, A4, estimator=0, **KW_A)
        _used(c, lanes, MC.LSQ)
        same_bits(p, r, p0, r0)
        same_pass(c.batch_pass(st, A4), pass0)
        _used(c, lanes, MC.LSQ)
        assert not np.array_equal(p1, p0)          # (the two estimators are two fits)
    finally:
        plain.close(); c.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_an_infinite_box_returns_fit_batchs_bits(lanes):
    lengths = MC.FORM_LENGTHS[lanes]
    _, batch, _ = MC.batch(lengths)
    c = context(MC.tape2(), batch)
    try:
        for name in ('a', 'd'):
            off, kw = SCENARIOS[name]
            st = MC.starts(lengths, off)
            p0, r0, _ = c.fit_batch(st, A4, lanes_per_fit=lanes, estimator=1, **kw)
            _used(c, lanes)
            p, r, at, _ = c.fit_batch_bounded(st, A4, [-INF] * 4, [INF] * 4, **kw)
            _used(c, lanes)
            same_bits(p, r, p0, r0)
            assert np.all(at == 0)
    finally:
        c.close()


@pytest.mark.parametrize('lanes', FORMS)
def test_an_amplitude_on_its_wall_stays_there_and_the_rest_is_stationary(lanes):
    items, st, lower, upper = MC.wall_case(lanes)
    # by the reference alone: at the start the data push the second amplitude through its wall (beta < 0 at p = lower)
    for b, (x, y, w) in enumerate(items):
        assert MC.reference_pass(MC.tape2(), x, y, w, st[b], MC.WALL_ACTIVE)[1][2] < 0.0
    c = context(MC.tape2(), BC.Batch(items))
    try:
        p, r, at, _ = c.fit_batch_bounded(st, MC.WALL_ACTIVE, lower, upper, lanes_per_fit=lanes, estimator=1, **MC.WALL_KW)
        _used(c, lanes)
    finally:
        c.close()
    worst = 0.0
    for b, (x, y, w) in enumerate(items):
        assert int(at[b]) & (1 << 2) and p[b, 2] == 0.0 and p[b, 0] > 0.0 and not int(at[b]) & 1, (b, at[b], p[b])
        assert p[b, 3] == st[b, 3]          # passive
        A, beta, D, _ = MC.reference_pass(MC.tape2(), x, y, w, p[b], MC.WALL_ACTIVE)
        assert beta[2] < 0.0          # still pushed outward at the end: the pin is the solution's
        worst = max(worst, float(np.max(np.abs(beta[:2]) / np.sqrt(np.diag(A)[:2] * D))))
    observe(**{'mle_wall_lanes%d_stationarity' % lanes: worst})
    assert worst <= 1e-6


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_errors_are_the_inverse_fisher_matrix(lanes):
    lengths = tuple(n for n in MC.FORM_LENGTHS[lanes] if n >= 15)
    od, batch, _ = MC.batch(lengths)
    st = MC.starts(lengths, SCENARIOS['a'][0])
    c = context(MC.tape2(), batch)
    try:
        p0, r0, _ = c.fit_batch(st, A4, lanes_per_fit=lanes, estimator=1, **KW_A)
        _used(c, lanes)
        p, r, (cov, sigma, info), _ = c.fit_batch_errors(st, A4, scale=False, **KW_A)
        _used(c, lanes)
        same_bits(p, r, p0, r0)
        _, _, (cov1, sigma1, info1), _ = c.fit_batch_errors(st, A4, scale=True, **KW_A)
        _used(c, lanes)
        _, _, D = c.batch_pass(p, A4)
        _used(c, lanes)
    finally:
        c.close()
    r_host = CV.r_host()
    worst, compared = 0.0, 0
    for f, (x, y, w) in enumerate(batch.items):
        A, _, D0, bound = MC.reference_pass(MC.tape2(), x, y, w, p[f], A4)
        kap = CV.kappa(A)
        assert abs(D[f] - D0) <= TOL_PASS * bound and abs(r['chi2'][f] - D0) <= TOL_PASS * bound
        if info[f] == 0:
            # under scale=True: the same matrix times D / dof with D the sweep's own sum, the operation the kernel makes
            assert info1[f] == 0 and np.array_equal(cov1[f], cov[f] * (D[f] / float(r['dof'][f])))
            assert np.array_equal(sigma[f], np.sqrt(np.diag(cov[f]))) and np.array_equal(sigma1[f], np.sqrt(np.diag(cov1[f])))
        if not kap <= CV.KAPPA_MAX:
            continue
        assert info[f] == 0, (od[f], info[f])
        err = CV.scaled_error(cov[f], CV.longdouble_inverse(A), CV.scale_of(A))
        limit = (4 * TOL_PASS + 10.0 * r_host * CV.EPS) * kap
        assert err <= limit, (od[f], err, limit)
        worst = max(worst, err / limit); compared += 1
    assert compared >= len(batch.items) // 2
    observe(**{'mle_cov_lanes%d_over_bound' % lanes: worst})
