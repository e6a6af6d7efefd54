"""gfh_k_fit_batch_bounded held to the restated reference of its five rules (tests/batch_bounds_rule_cases.py; run by the reference
alone in tests/test_cpu_batch_bounds_rule.py) on the three lane forms: every case of the table, least squares, under Cauchy and Huber
and under the Poisson estimator, each form on the fits of the case at its own lengths, one launch per case and form.

For the fits the rule keeps: the counts and dof equal, at_bound equal, lambda within TOL_LAMBDA, the parameters and chi2 (the deviance
under the estimator) within TOL_PARS and TOL_CHI2 -- the project's bounds (tests/batch_common.py) -- and a parameter returned on a
wall is the wall's bits.  For every fit, the dropped ones too: finite, inside the box, at_bound the exact comparison on what came back;
and on 64 lanes the batch reversed returns every fit's bits.  The cube of tests/batch_bounds_cases.py runs a_hi3's box and options
under the same rule.  Every unit asked for is one the build has compiled."""
import numpy as np
import pytest

from tests import batch_bounds_cases as BB
from tests import batch_bounds_rule_cases as R
from tests.batch_common import TOL_CHI2, TOL_PARS, check_fit, context, fit_worst, same_bits

pytestmark = pytest.mark.gpu

FORMS = (64, 16, 256)


def _device(case, lanes, idx):
    """the case's fits idx as one batch on a context of its own: (parameters, records, at_bound)"""
    items = case.batch().items
    sub = BB.BC.Batch([items[k] for k in idx])
    how = case.how()
    if 'scale' in how:
        how['loss_scale'] = how.pop('scale')
    lo, hi = case.box()
    c = context(case.tape(), sub)
    try:
        p, r, at, _ = c.fit_batch_bounded(case.starts()[idx], case.active(), lo, hi, lanes_per_fit=lanes, **how, **case.kw)
        assert c.batch_lanes_used() == lanes
    finally:
        c.close()
    return p, r, at


def _at_bound(p, active, lo, hi):
    at = np.zeros(p.shape[0], dtype=np.int64)
    for j, a in enumerate(active):
        at |= np.where(p[:, a] == lo[j], 1 << j, 0) | np.where(p[:, a] == hi[j], 1 << (8 + j), 0)
    return at


def _held(key, sel, p, r, at, n_points, active, lo, hi, prefix):
    """the assertions on one launch: sel in the launch's order"""
    act = list(active)
    # every fit, kept or dropped: finite, in the box, at_bound exact on what came back
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(r['chi2'])) and np.all(np.isfinite(r['lambda_']))
    assert np.all(p[:, act] >= lo) and np.all(p[:, act] <= hi)
    assert at.dtype == np.int32 and np.array_equal(at, _at_bound(p, act, lo, hi))
    kept = [b for b, s in enumerate(sel) if s[0]]
    # a parameter on a wall at 0 is compared as bits (below), not as 0 / 0: both sides read 1 in fit_worst's quotient
    ref = []
    pc = p.copy()
    for b, s in enumerate(sel):
        p0 = s[1][1].copy()
        both = (p0 == 0.0) & (p[b] == 0.0)
        p0[both] = 1.0; pc[b, both] = 1.0
        ref.append((s[0], (s[1][0], p0, s[1][2], s[1][3]), s[2], s[3]))
    for b in kept:          # (before the bound, so that a miss can be read against the reference's own spread of that fit)
        d = float(np.max(np.abs(pc[b] - ref[b][1][1]) / np.abs(ref[b][1][1])))
        if d >= TOL_PARS:
            print('%s %s fit %d (n = %d): parameters off the reference by %.2e, the reference against itself by %.2e' % (prefix, key, b, n_points[b], d, sel[b][2]))
    worst = fit_worst(ref, pc, r, n_points, len(act))
    for b in kept:
        assert int(at[b]) == sel[b][4].at_bound, (b, int(at[b]), sel[b][4].at_bound)
        for j, a in enumerate(act):
            for bit, wall in ((1 << j, lo[j]), (1 << (8 + j), hi[j])):
                if int(at[b]) & bit:
                    assert p[b, a].view(np.uint64) == np.float64(wall).view(np.uint64), (b, j)
    check_fit(prefix, key, worst, TOL_PARS, TOL_CHI2)
    return kept


@pytest.mark.parametrize('key', R.KEYS)
@pytest.mark.parametrize('lanes', FORMS)
def test_the_device_against_the_restated_rule(lanes, key):
    case = R.case(key)
    idx = case.form(lanes)
    full = R.selection(key)
    sel = [full[k] for k in idx]
    lo, hi = case.box()
    p, r, at = _device(case, lanes, idx)
    kept = _held(key, sel, p, r, at, case.batch().n[idx], case.active(), lo, hi, 'bounds_rule_lanes%d' % lanes)
    assert len(idx) - len(kept) <= R.CAP * len(idx)
    print('%s, %d lanes: %d of %d kept; exits %s, at_bound %s' % (key, lanes, len(kept), len(idx), sorted(set(r['exit_reason'].tolist())), sorted(set(at.tolist()))))


@pytest.mark.parametrize('key', R.KEYS)
def test_the_batch_reversed_returns_every_fits_bits(key):
    case = R.case(key)
    idx = case.form(64)
    p, r, at = _device(case, 64, idx)
    pr, rr, ar = _device(case, 64, idx[::-1])
    same_bits(pr[::-1], rr[::-1], p, r)
    assert np.array_equal(ar[::-1], at)


def test_the_cube_against_the_restated_rule():
    sel = R.cube_selection()
    lo, hi = BB.box(4, hi3=BB.CUBE_WALL)
    x, Y = BB.cube()
    c = context(BB.tape2())
    try:
        c.set_batch_cube(x, Y, BB.CUBE_ERROR)
        p, r, at, _ = c.fit_batch_bounded(BB.cube_starts(0.05, BB.CUBE_START), R.ACTIVE, lo, hi, lanes_per_fit=64, **R.A_KW)
        assert c.batch_form_used() == ('cube', 2, BB.CUBE_ERROR) and c.batch_lanes_used() == 64
    finally:
        c.close()
    kept = _held('cube', sel, p, r, at, np.full(BB.CUBE_FITS, BB.CUBE_N), R.ACTIVE, lo, hi, 'bounds_rule')
    assert BB.CUBE_FITS - len(kept) <= R.CAP * BB.CUBE_FITS
