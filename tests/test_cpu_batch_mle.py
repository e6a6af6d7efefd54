"""CPU tests of the estimator of a batch (gfh_set_batch_estimator, Context.set_batch_estimator, the estimator= argument of the batch
calls; GenConfig::batch_estimator): the setter's refusals and persistence, the three combinations the launching calls refuse before the
device is asked for, the text of the units (a least-squares unit holds no line of the Poisson arm and is the same text before and after
the setting was used), the Poisson units compiled for gfx950 on a compile-only context, and the reference of
tests/batch_mle_cases.py held to itself: the rule's share per scenario, the stationarity of the restated fit, and the reason the
estimator exists -- at a few counts per bin its amplitudes are less biased than those of the SQRT_Y least-squares fit of the same
counts.  tests/test_gpu_batch_mle.py holds the device to that reference."""
import numpy as np
import pytest

from gadfit_amd import _lib
from oracle import binding as orc
from tests import batch_cube_cases as CU
from tests import batch_mle_cases as MC
from tests import models as M

INF = float('inf')
A4 = [0, 1, 2, 3]


def _ctx():
    c = _lib.Context(-1)
    c.set_model(MC.tape2())
    return c


def _data(c, sizes=(10, 12, 9)):
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    with pytest.raises(_lib.GadfitHipError, match='no GPU'):
        c.set_batch_data(off, np.linspace(0.5, 9.5, n), np.ones(n), np.ones(n))
    return len(sizes)


def test_the_setter_refuses_by_name_and_a_refused_call_leaves_the_setting():
    c = _lib.Context(-1)          # needs neither a GPU nor a model
    try:
        assert c.batch_estimator() == 0 and c.batch_estimator_used() is None
        for value, held in ((1, 1), (0, 0), ('poisson', 1), ('lsq', 0), (1, 1)):
            c.set_batch_estimator(value)
            assert c.batch_estimator() == held
        for bad in (-1, 2, 17):
            with pytest.raises(_lib.GadfitHipError, match=r'gfh_set_batch_estimator: unknown estimator %d \(0: least squares, 1: poisson\)' % bad):
                c.set_batch_estimator(bad)
            assert c.batch_estimator() == 1
        with pytest.raises(_lib.GadfitHipError, match="unknown estimator 'cash'"):
            c.set_batch_estimator('cash')
        assert c.batch_estimator() == 1
        c.set_model(MC.tape2())
        assert '#define GFH_BMLE 1\n' in c.batch_source(A4)
        assert c.batch_estimator_used() is None          # a setting is no launch
    finally:
        c.close()


def test_the_keyword_of_the_calls_sets_the_estimator_and_none_leaves_it():
    c = _ctx()
    try:
        nf = _data(c)
        start = np.tile(M.EXP2_TRUTH, (nf, 1))
        for call in (lambda **kw: c.fit_batch(start, A4, max_iter=2, **kw), lambda **kw: c.fit_batch_errors(start, A4, max_iter=2, **kw),
                     lambda **kw: c.fit_batch_bounded(start, A4, [-INF] * 4, [INF] * 4, max_iter=2, **kw),
                     lambda **kw: c.batch_pass(start, A4, **kw), lambda **kw: c.batch_covariance(start, A4, **kw)):
            c.set_batch_estimator(0)
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                call(estimator='poisson')
            assert c.batch_estimator() == 1          # it stays set
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                call()                                 # None leaves the setting
            assert c.batch_estimator() == 1
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                call(estimator=0)
            assert c.batch_estimator() == 0
            with pytest.raises(_lib.GadfitHipError, match='unknown estimator 3'):
                call(estimator=3)
            assert c.batch_estimator() == 0
    finally:
        c.close()


def test_the_three_combinations_are_refused_before_the_device_is_asked_for():
    c = _ctx()
    try:
        nf = _data(c)
        start = np.tile(M.EXP2_TRUTH, (nf, 1))
        fits = (('gfh_fit_batch', lambda **kw: c.fit_batch(start, A4, max_iter=2, **kw)),
                ('gfh_fit_batch_errors', lambda **kw: c.fit_batch_errors(start, A4, max_iter=2, **kw)),
                ('gfh_fit_batch_bounded', lambda **kw: c.fit_batch_bounded(start, A4, [-INF] * 4, [INF] * 4, max_iter=2, **kw)))
        others = (('gfh_batch_pass', lambda **kw: c.batch_pass(start, A4)), ('gfh_batch_covariance', lambda **kw: c.batch_covariance(start, A4)),
                  ('gfh_batch_eval', lambda **kw: c.batch_eval(start, A4)), ('gfh_batch_source', lambda **kw: c.batch_source(A4)),
                  ('gfh_batch_prepare', lambda **kw: c.batch_prepare(A4)), ('gfh_batch_prepare_bounded', lambda **kw: c.batch_prepare(A4, bounded=True)))
        c.set_batch_estimator(1)
        # 1. with a batch loss
        for loss in (1, 2):
            c.set_batch_loss(loss, 1.345)
            for who, call in fits + others:
                with pytest.raises(_lib.GadfitHipError, match=who + r': the poisson estimator \(gfh_set_batch_estimator\) together with a batch loss'):
                    call()
        c.set_batch_loss(0, 1.0)
        # 2. with accth
        for who, call in fits:
            with pytest.raises(_lib.GadfitHipError, match=who + r': accth \(geodesic acceleration\) is not carried under the poisson estimator'):
                call(accth=0.9)
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):          # accth = 0 switches STEP 3 off, as everywhere
                call(accth=0.0)
        # 3. a residual from batch_eval; model and band go through to the device
        with pytest.raises(_lib.GadfitHipError, match=r'gfh_batch_eval: the weighted residual has no meaning under the poisson estimator'):
            c.batch_eval(start, A4, residuals=True)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.batch_eval(start, A4, cov=np.tile(np.eye(4), (nf, 1, 1)))
        # each of them is a refusal of the combination: under least squares the same calls get as far as the device
        c.set_batch_estimator(0)
        c.set_batch_loss(1, 1.345)
        for who, call in fits:
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                call(accth=0.9)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.batch_eval(start, A4, residuals=True)
        # ... and what was pinned before stays: the unknown loss, the LM policies
        with pytest.raises(_lib.GadfitHipError, match=r'unknown loss 3'):
            c.set_batch_loss(3, 1.0)
        c.set_batch_loss(0, 1.0)
        c.set_batch_estimator(1)
        with pytest.raises(_lib.GadfitHipError, match='nielsen'):
            c.fit_batch(start, A4, max_iter=2, nielsen=1)
    finally:
        c.close()


@pytest.mark.parametrize('lanes', [16, 64, 256])
@pytest.mark.parametrize('bounded', [False, True])
def test_a_least_squares_unit_holds_none_of_the_new_lines(lanes, bounded):
    c = _ctx()
    try:
        c.set_batch_lanes(lanes)
        before = c.batch_source(A4, bounded=bounded)
        assert 'GFH_BMLE' not in before and 'gfh_b_dev' not in before
        c.set_batch_estimator(1)
        poisson = c.batch_source(A4, bounded=bounded)
        assert '#define GFH_BMLE 1\n' in poisson and 'gfh_b_dev' in poisson
        # the generator resolved every region: no directive of either kind is left for the preprocessor
        assert not [ln for ln in poisson.split('\n') if ln.startswith('#') and ('GFH_BMLE' in ln or 'GFH_BLOSS' in ln) and ln != '#define GFH_BMLE 1']
        assert ('gfh_k_fit_batch_bounded' in poisson) == bounded
        c.set_batch_estimator(0)
        assert c.batch_source(A4, bounded=bounded) == before
        # under a loss the text holds none of the Poisson arm either
        c.set_batch_loss(1, 1.0)
        assert 'GFH_BMLE' not in c.batch_source(A4, bounded=bounded)
    finally:
        c.close()


def test_the_poisson_units_of_the_gpu_module_compile_for_gfx950():
    assert MC.prepare_units(lambda: _lib.Context(-1)) == 13


@pytest.mark.parametrize('name', MC.NAMES)
def test_every_scenario_keeps_its_share(name):
    sel = MC.selection(name)
    assert len(sel) == 2 * len(MC.LENGTHS)
    dropped = [(k, s[2], s[3]) for k, s in zip(MC.order(), sel) if not s[0]]
    print('scenario %s: %d of %d dropped %s' % (name, len(dropped), len(sel), dropped))
    assert len(dropped) <= MC.CAP * len(sel)
    for lanes, lengths in MC.FORM_LENGTHS.items():          # ... and in every lane form's share of the lengths
        sub = MC.form_selection(name, lanes)
        assert len(sub) == 2 * len(lengths) and sum(1 for s in sub if not s[0]) <= MC.CAP * len(sub)
    exits = sorted(set(s[1][0][4] for s in sel if s[0]))
    print('scenario %s: exit reasons of the kept fits %s' % (name, exits))
    assert all(s[1][0][3] == 0 for s in sel)          # no omega pass under this estimator


@pytest.mark.parametrize('name', MC.EXP4_NAMES)
def test_the_eight_parameter_set_keeps_its_share(name):
    sel = MC.selection4(name)
    assert len(sel) == 4 and sum(1 for s in sel if not s[0]) <= MC.CAP * len(sel)


def test_the_three_scenarios_reach_acceptances_rejections_and_three_exits():
    """what the kept fits cover, decided by the reference alone: accepted and rejected trials, and the exits 0, 2 and 7"""
    kept = [s for name in MC.NAMES for s in MC.selection(name) if s[0]]
    exits = set(s[1][0][4] for s in kept)
    assert {0, 2, 7} <= exits
    assert any(c[2] > c[1] + 1 and c[0] > 0 for c in (s[1][0] for s in kept))          # a rejected trial inside a fit that goes on


def test_the_deviance_of_the_reference_is_the_stated_formula():
    y = np.array([0.0, 3.0, 1.0, 2.0, 5.0, 4.0])
    f = np.array([0.5, 2.0, 1.0, -1.0, np.inf, 4.5])
    m = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 2.0])
    t, _ = MC.deviance_terms(y, f, m)
    want = [2 * 0.5, 2 * (2.0 - 3.0 + 3.0 * np.log(1.5)), 0.0, 0.0, 0.0, 2 * (4.5 - 4.0 + 4.0 * np.log(4.0 / 4.5))]
    assert np.allclose(np.asarray(t, dtype=np.float64), want, rtol=0, atol=2e-15)          # (`want` is formed in doubles: terms of order one that cancel)
    for yy, ff in ((1.0, 0.0), (1.0, -2.0), (0.0, -2.0), (-1.0, 2.0), (np.nan, 2.0), (1.0, np.nan), (1.0, np.inf), (np.inf, 1.0), (0.0, 0.0)):
        assert np.isnan(float(MC.deviance_terms(np.array([yy]), np.array([ff]), np.ones(1))[0][0])), (yy, ff)


def test_the_converged_restated_fit_is_a_stationary_point_of_the_deviance():
    """chi2_rel = 1e-10: |beta_j| <= 1e-6 sqrt(alpha_jj D) at the fitted parameters, in both regimes.  The exit test itself bounds the
    scaled gradient only near sqrt(chi2_rel) = 1e-5 (one step lowers D by about beta^T alpha^-1 beta); 1e-6 asks that the last steps
    were Newton steps of a well-determined fit, whose decrease falls quadratically through the threshold.  So the spectra are those from
    255 points on, where the counts determine all four parameters (shorter ones crawl along a valley: 100 iterations do not end them)."""
    kw = dict(lambda_=1.0, max_iter=100, chi2_rel=1e-10)
    checked = 0
    for n in (255, 256, 257, 513):
        for regime in ('low', 'high'):
            truth, x, y, w = MC.spectrum(n, regime)
            counts, P, lam, D, _, _, _ = MC.restated_fit(MC.tape2(), x, y, w, truth * np.array([1.05, 0.95, 1.05, 0.95]), A4, kw)
            assert counts[4] == 2, (n, regime, counts)
            A, b, D1, _ = MC.reference_pass(MC.tape2(), x, y, w, P, A4)
            assert abs(D1 - D) <= 1e-12 * D
            worst = np.max(np.abs(b) / np.sqrt(np.diag(A) * D))
            print('n = %d %s: iterations %d, D = %.6g, worst |beta| / sqrt(alpha D) = %.2e' % (n, regime, counts[0], D, worst))
            assert worst <= 1e-6
            checked += 1
    assert checked == 8


def test_the_poisson_fit_is_less_biased_than_sqrt_y_least_squares_at_a_few_counts_per_bin():
    """the s = 1 regime over 64 seeded spectra, the two amplitudes active and the decay times at their truths: the mean relative
    amplitude error of the restated Poisson fit against that of the oracle's least-squares fit under SQRT_Y weights of the same counts,
    zero bins at the cube's clamp (weight 0).  Of the reference alone: this is why the estimator exists."""
    tape = MC.tape2()
    err_p, err_l = [], []
    for seed in range(MC.BIAS_SPECTRA):
        truth, x, y = MC.bias_spectrum(seed)
        assert y.max() <= 20 and np.sum(y == 0) >= MC.BIAS_N // 4          # a few counts per bin, many zeros
        counts, P, _, _, _, _, _ = MC.restated_fit(tape, x, y, np.ones(y.size), truth, MC.BIAS_ACTIVE, MC.BIAS_KW)
        assert counts[4] in (2, 7), (seed, counts)
        w = CU.reference_weights(y, CU.SQRT_Y)
        assert np.array_equal(w == 0.0, y == 0.0)
        p = orc.OracleProblem(tape, [x], [y], [w], [truth], MC.BIAS_ACTIVE, [0] * 4)
        r = p.fit(**MC.BIAS_KW)
        assert r.exit_reason in (2, 7), (seed, r.exit_reason)          # (7: converged, then a comparison of two equal chi2)
        err_p.append((P[MC.BIAS_ACTIVE] - truth[MC.BIAS_ACTIVE]) / truth[MC.BIAS_ACTIVE])
        err_l.append((p.pars.ravel()[MC.BIAS_ACTIVE] - truth[MC.BIAS_ACTIVE]) / truth[MC.BIAS_ACTIVE])
    bias_p, bias_l = np.mean(err_p, axis=0), np.mean(err_l, axis=0)
    print('mean relative amplitude error over %d spectra: poisson %s, sqrt_y least squares %s' % (MC.BIAS_SPECTRA, bias_p, bias_l))
    assert np.all(np.abs(bias_p) < np.abs(bias_l))
    assert abs(np.mean(bias_p)) < abs(np.mean(bias_l))


def test_the_session_calls_check_the_estimator_argument():
    from gadfit_amd import gadfit as G
    for bad in (2, -1, 'cash', True, 1.5):
        with pytest.raises(G.GadfitError, match='estimator must be None, 0 or'):
            G._batch_estimator('gadf_fit_batch', bad)
    assert [G._batch_estimator('w', v) for v in (None, 0, 1, 'lsq', 'poisson')] == [0, 0, 1, 0, 1]
