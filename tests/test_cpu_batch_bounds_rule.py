"""The statement of the bounded batch fit's rule (tests/batch_bounds_rule_cases.py) held by the reference alone, without a GPU: what
tests/test_gpu_batch_bounds_rule.py holds the device against is decided, and shown to be worth holding it against, here.

 1. The cap: of every case, and of the fits of it that each lane form runs, at most one in five is dropped by the rule.
 2. Coverage: each case shows what it is in the table for on at least a quarter of its kept fits; over all cases the kept fits hold
    every exit reason 0, 2, 5, 7 with a non-empty final at_bound, a lower and an upper bit, a clamped retrial, and a pin in position 0,
    in a middle position and in the last.
 3. Each rule is noticed: each of the nine altered rules M1 ... M9 changes the counts, at_bound or the parameters beyond TOL_FIT of at
    least NOTICED_MIN kept fits; and an altered fit that the unaltered one did not `touch` is the unaltered fit.
 4. With an infinite box the restated loop returns batch_cases.oracle_fit's counts and parameters exactly, and it is deterministic."""
import numpy as np
import pytest

from tests import batch_bounds_cases as BB
from tests import batch_bounds_rule_cases as R
from tests import batch_cases as BC
from tests.batch_common import SCENARIOS

FORMS = (64, 16, 256)


def _kept(key):
    return [k for k, s in enumerate(R.selection(key)) if s[0]]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', R.KEYS)
def test_the_cap_per_case_and_per_lane_form(key):
    c, sel = R.case(key), R.selection(key)
    kept = _kept(key)
    line = ['%s (%s): kept %d of %d' % (key, c.kind, len(kept), len(sel))]
    assert len(sel) - len(kept) <= R.CAP * len(sel)
    for lanes in FORMS:
        sub = c.form(lanes)
        n = sum(1 for k in sub if sel[k][0])
        line.append('%d lanes %d of %d' % (lanes, n, len(sub)))
        assert len(sub) >= 4 and len(sub) - n <= R.CAP * len(sub), (lanes, n, len(sub))
    print('; '.join(line))
    for k, s in enumerate(sel):
        if not s[0]:
            print('   dropped fit %d (n = %d): counts %s, self-difference %.1e, margins accept %.1e pin %.1e clamp %.1e exit %.1e'
                  % ((k, c.batch().n[k], s[4].counts, s[2]) + s[3]))


def test_the_forms_lengths_hold_each_forms_row_edges():
    n = R.case('a_hi3').batch().n
    for lanes, edges in ((16, (16, 17, 31, 33)), (64, (63, 64, 65, 129)), (256, (255, 256, 257, 513))):
        have = set(int(n[k]) for k in R.case('a_hi3').form(lanes))
        assert set(edges) <= have, (lanes, sorted(have))
    assert min(n) >= 16


@pytest.mark.parametrize('key', R.KEYS)
def test_every_start_lies_inside_the_box(key):
    """gfh_fit_batch_bounded refuses a start outside the box before the device is asked for"""
    c = R.case(key)
    lo, hi = c.box()
    st = c.starts()[:, c.active()]
    assert st.shape[0] == len(c.batch().items) and np.all(st >= lo) and np.all(st <= hi)


def test_the_cube_is_kept_within_the_cap():
    sel = R.cube_selection()
    kept = [s for s in sel if s[0]]
    print('cube: kept %d of %d' % (len(kept), len(sel)))
    assert len(sel) - len(kept) <= R.CAP * len(sel)
    assert sum(1 for s in kept if R.COVERS['clamps then pins'](s[4])) * 4 >= len(kept)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', R.KEYS)
def test_each_case_shows_what_it_is_there_for(key):
    c, sel = R.case(key), R.selection(key)
    kept = _kept(key)
    shown = sum(1 for k in kept if c.shown(sel[k][4]))
    print('%s: "%s" on %d of %d kept fits; exits %s, at_bound %s' % (key, c.covers, shown, len(kept), sorted(set(sel[k][4].counts[4] for k in kept)),
                                                                    sorted(set(sel[k][4].at_bound for k in kept))))
    assert 4 * shown >= len(kept) > 0


def test_the_control_is_mostly_untouched_by_its_box():
    sel = R.selection('release')
    quiet = sum(1 for k in _kept('release') if R._ev(sel[k][4], 'first_clamped') + R._ev(sel[k][4], 'retrials_clamped') == 0)
    assert 2 * quiet >= len(_kept('release'))


def test_coverage_over_all_cases():
    fits = [R.selection(key)[k][4] for key in R.KEYS for k in _kept(key)]
    na = {key: len(R.case(key).active()) for key in R.KEYS}
    exits = set(f.counts[4] for f in fits if f.at_bound)
    assert {0, 2, 5, 7} <= exits, exits
    assert any(f.at_bound & 0xff for f in fits) and any(f.at_bound >> 8 for f in fits)
    assert any(R._ev(f, 'retrials_clamped') for f in fits)
    first = middle = last = 0
    for key in R.KEYS:
        for k in _kept(key):
            bits = R._ev(R.selection(key)[k][4], 'pinned_bits')
            first += bits & 1
            middle += 1 if bits & ((1 << (na[key] - 1)) - 2) else 0
            last += bits >> (na[key] - 1) & 1
    print('fits with a pin in position 0: %d, in a middle position: %d, in the last: %d' % (first, middle, last))
    assert first and middle and last


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('change', R.ALTERED)
def test_each_rule_is_noticed(change):
    by_case = []
    for key in R.KEYS:
        c, sel = R.case(key), R.selection(key)
        by_case.append(sum(1 for k in _kept(key) if R.noticed(sel[k][4], R.altered(key, k, change), c.active())))
    print('%s noticed by %d kept fits: %s' % (change, sum(by_case), ' + '.join('%d %s' % (n, key) for n, key in zip(by_case, R.KEYS) if n)))
    assert sum(by_case) >= R.NOTICED_MIN


@pytest.mark.parametrize('key', R.LSQ_KEYS)
def test_an_untouched_change_is_the_unaltered_fit(key):
    """the shortcut of altered(): over the first five fits of the case, every change the unaltered fit did not touch gives its bits"""
    c = R.case(key)
    lo, hi = c.box()
    st = c.starts()
    ran = 0
    for k, (x, y, w) in enumerate(c.batch().items[:5]):
        one = R.selection(key)[k][4]
        for change in R.ALTERED:
            if change in one.touched:
                continue
            f = R.restated_bounded_fit(c.tape(), x, y, w, st[k], c.active(), lo, hi, c.kw, _alter=change)
            assert f.counts == one.counts and f.at_bound == one.at_bound and np.array_equal(f.pars, one.pars) and f.lam == one.lam, (k, change)
            ran += 1
    assert ran > 0


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_an_infinite_box_gives_the_oracles_fit_exactly(name):
    off, kw = SCENARIOS[name]
    batch = BB.exp2_batch(R.LENGTHS)[1]
    st = BB.exp2_starts(off, R.LENGTHS)
    lo, hi = BB.box(4)
    for k in (0, 5, 9, 14, 19, 24):
        x, y, w = batch.items[k]
        for n_images in (1, 3):
            counts, pars, lam, chi2 = BC.oracle_fit(BB.tape2(), x, y, w, st[k], R.ACTIVE, kw, n_images)
            f = R.restated_bounded_fit(BB.tape2(), x, y, w, st[k], R.ACTIVE, lo, hi, kw, n_images)
            assert f.counts == counts and np.array_equal(f.pars, pars) and f.lam == lam and f.chi2 == chi2, (k, n_images)
            assert f.at_bound == 0 and f.events == (0,) * len(R.EVENTS) and f.pin == np.inf and f.clamp == np.inf


def test_the_restated_loop_is_deterministic():
    for key in ('c_two', 'relerr_n', 'huber_hi2', 'poisson_lo02'):
        c = R.case(key)
        lo, hi = c.box()
        x, y, w = c.batch().items[3]
        a, b = (R.restated_bounded_fit(c.tape(), x, y, w, c.starts()[3], c.active(), lo, hi, c.kw, **c.how()) for _ in range(2))
        assert a.counts == b.counts and np.array_equal(a.pars, b.pars) and a.margins() == b.margins() and a.events == b.events
        assert a.chi2 == b.chi2 and a.lam == b.lam and a.at_bound == b.at_bound and a.touched == b.touched


def test_the_estimators_first_deviance_nan_ends_with_reason_8():
    c = R.case('poisson_hi3')
    lo, hi = c.box()
    x, y, w = c.batch().items[2]
    start = c.starts()[2].copy()
    start[2] = -start[2]          # the slow component's amplitude negative: the model is negative in the tail
    f = R.restated_bounded_fit(c.tape(), x, y, w, start, c.active(), lo, hi, c.kw, estimator=1)
    assert f.counts == (0, 0, 1, 0, 8) and np.array_equal(f.pars, start)
