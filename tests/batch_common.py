"""What the batch tests share (tests/test_gpu_batch.py, tests/batch_form_suite.py and the three forms' modules,
tests/test_gpu_batch_cube.py, their inputs modules and their CPU modules): the scenarios, the bounds, the spectra of model_exp4,
the record of observed maxima and the comparisons against the oracle and bit for bit.  No test module is imported for any of it.

GADFIT_BATCH_OBSERVE=<file>: the observed maxima of every module of ONE pytest process are written there as JSON (tools/bench_batch.py
puts them into profiles/batch_fits.json, profiles/batch_rows.json and profiles/batch_workgroup.json)."""
import json
import os

import numpy as np

from gadfit_amd import _lib
from oracle import binding as orc
from tests import models as M

TOL_PASS = 2e-13          # the project's per-pass bound (tests/test_gpu_parity.py)
TOL_LAMBDA = 1e-14        # the same decisions give the same products of lam_up / lam_down
# fitted parameters and chi2: north_star's bound is 1e-10; observed 2.0e-13 and 1.7e-13 (profiles/batch_fits.json, observed_maxima_against_the_oracle), and the oracle
# against itself with its point sums in another order differs by 1.7e-13 on these inputs, so 10 x observed would sit at what a
# reordered sum does: the assertion stays at 3e-12
TOL_PARS = 3e-12
TOL_CHI2 = 3e-12
TOL_FIT = 1e-10           # north_star's bound on fitted parameters and chi2
SCENARIOS = {
    'a': (0.05, dict(lambda_=1.0, max_iter=50, chi2_rel=1e-6)),
    'b': (0.4, dict(lambda_=1e-6, max_iter=4)),
    'c': (0.4, dict(lambda_=1e-6, accth=0.9, max_iter=4)),
    'd': (0.4, dict(lambda_=1e-6, max_iter=40, chi2_rel=1e-4)),
}
COUNTS = ('iterations', 'n_sweeps', 'n_chi2', 'n_omega', 'exit_reason')
_OBSERVED = {}            # one per process: the record tools rely on several modules writing one file


def observe(**kw):
    for k, v in kw.items():
        _OBSERVED[k] = max(_OBSERVED.get(k, 0.0), float(v))
        print('observed %s = %.3e' % (k, float(v)))
    path = os.environ.get('GADFIT_BATCH_OBSERVE')
    if path:
        with open(path, 'w') as fh:
            json.dump(_OBSERVED, fh, indent=1, sort_keys=True)


def start_of(truth, off):
    return truth * np.where(np.arange(4) % 2 == 0, 1.0 + off, 1.0 - off)


def spectrum4(b):
    """spectrum b of model_exp4 (the inputs are described in tests/test_gpu_batch.py): (truth, x, y, weights)"""
    u = (M.splitmix64(8, M.SEED + 2000 * (b + 1)) >> np.uint64(11)).astype(np.float64) / 9007199254740992.0
    truth = M.EXP4_TRUTH * (0.9 + 0.2 * u)
    x, y, s = M.make_single(M.exp4_numpy, truth, 128 + (53 * b) % 385, 0.05, 100.0, seed=M.SEED + 7 * b + 3)
    return truth, x, y, 1.0 / s


def context(tape, batch=None):
    c = _lib.Context(0)
    c.set_model(tape)
    if batch is not None:
        c.set_batch_data(batch.off, batch.x, batch.y, batch.w)
    return c


def same_bits(p, r, p0, r0):
    """two results of fit_batch: parameters, counts and dof equal, lambda and chi2 bit for bit"""
    assert np.array_equal(p, p0)
    for f in COUNTS + ('dof',):
        assert np.array_equal(r[f], r0[f]), f
    assert np.array_equal(r['lambda_'].view(np.uint64), r0['lambda_'].view(np.uint64))
    assert np.array_equal(r['chi2'].view(np.uint64), r0['chi2'].view(np.uint64))


def same_pass(a, b):
    """two results of batch_pass (J^T J, J^T r, chi2) bit for bit"""
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))


def pass_worst(tape, items, starts, active, JTJ, JTr, chi2):
    """a batch_pass against OracleProblem.sweep, fit by fit, scaled as test_gpu_batch.test_one_pass_against_the_oracle scales it"""
    worst = 0.0
    for b, (x, y, w) in enumerate(items):
        p = orc.OracleProblem(tape, [x], [y], [w], [starts[b]], active, [0] * tape.n_pars)
        JTJ0, JTr0, _, _ = p.sweep()
        chi0, _ = p.chi2()
        d = np.diag(JTJ0)
        worst = max(worst, np.max(np.abs(JTJ[b] - JTJ0) / (np.sqrt(np.outer(d, d)) + 1e-300)),
                    np.max(np.abs(JTr[b] - JTr0) / (np.sqrt(d * chi0) + 1e-300)), abs(chi2[b] - chi0) / chi0)
        assert np.array_equal(JTJ[b], JTJ[b].T), b
    assert np.isfinite(worst)
    return worst


def fit_worst(sel, pars, res, n_points, na):
    """fit_batch against the oracle's fits of the selection (kept cases): the counts and dof equal; returns the worst relative
    differences of lambda, the parameters and chi2"""
    worst = dict(lam=0.0, pars=0.0, chi2=0.0)
    mismatches, kept = [], 0
    for b, (ok, (counts, p0, lam0, chi0), _, _) in enumerate(sel):
        assert int(res['dof'][b]) == max(int(n_points[b]) - na, 1), b          # n = na: dof 0 is reported as 1 (gadfit.F90:648-657)
        if not ok:
            continue
        kept += 1
        got = tuple(int(res[f][b]) for f in COUNTS)
        if got != counts:
            mismatches.append((b, got, counts))
            continue
        worst['lam'] = max(worst['lam'], abs(res['lambda_'][b] - lam0) / lam0)
        worst['pars'] = max(worst['pars'], np.max(np.abs(pars[b] - p0) / np.abs(p0)))
        worst['chi2'] = max(worst['chi2'], abs(res['chi2'][b] - chi0) / chi0)
    assert kept > 0, 'the rule kept no fit of this batch: nothing was compared'
    assert not mismatches, '%d of %d kept fits differ in (iterations, n_sweeps, n_chi2, n_omega, exit_reason): %s' % (len(mismatches), kept, mismatches[:8])
    assert all(np.isfinite(v) for v in worst.values())
    return worst


def check_fit(prefix, key, worst, tol_pars, tol_chi2):
    """records a fit_worst under <prefix>_<key>_{lambda,pars,chi2} and holds it to the bounds"""
    observe(**{'%s_%s_lambda' % (prefix, key): worst['lam'], '%s_%s_pars' % (prefix, key): worst['pars'], '%s_%s_chi2' % (prefix, key): worst['chi2']})
    assert worst['lam'] <= TOL_LAMBDA and worst['pars'] < tol_pars and worst['chi2'] < tol_chi2
