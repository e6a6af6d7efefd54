"""The table of tests/lm_loop_cases.py under its rule, without a GPU: the rule runs over every row, the cap holds, every coverage
condition holds over the KEPT rows alone (asserted from the oracle's counts), and the oracle's new report min_exit_margin is what its
definition says.  tests/test_gpu_lm_loop.py then holds gfh_fit to the kept rows."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as orc
from tests import lm_loop_cases as LC
from tests.batch_common import COUNTS
from tests.parity_common import TOL_LAMBDA


def _all():
    return [LC.selected(k) for k in range(len(LC.TABLE))]


def _kept(where=lambda s: True):
    return [s for s in LC.kept() if where(s)]


def _flag(s, name):
    return bool(s.options.get(name, 0))


def test_the_rule_runs_over_the_whole_table_and_the_cap_holds():
    sel = _all()
    ids = [s.id for s in sel]
    assert len(set(ids)) == len(ids), 'the ids of the table are the test ids: no two rows may share one'
    for s in sel:
        print('%-36s %-4s %s lambda %.3g  1 vs 3 images %.1e  over %s images %.1e  margin %.1e  exit margin %.1e  %s'
              % (s.id, 'kept' if s.kept else 'DROP', LC.counts(s.r), s.r.lambda_, s.diff, LC.IMAGES, LC.spread(s.row), s.margin, s.exit_margin,
                 ', '.join(s.why)))
        assert np.isfinite(s.pars).all() and np.isfinite(s.r.chi2) and s.r.exit_reason >= 0
    dropped = [s.id for s in sel if not s.kept]
    print('%d rows, %d kept, dropped: %s' % (len(sel), len(sel) - len(dropped), dropped))
    assert len(dropped) <= LC.CAP * len(sel), dropped
    assert {s.row[0] for s in sel if s.kept} == set(LC.PROBLEMS)


def test_the_rule_drops_a_fit_that_rounding_decides():
    """the example of the module's docstring: model_exp2 under lam_incs = 1 converges, then leaves with exit 7 on a comparison of two
    chi2 that agree to rounding -- point 3 must see it"""
    s = LC.Selected(('exp2', 0.3, 'converged', dict(lambda_=1e-6, lam_incs=1, lam_up=2.0)))
    assert s.r.exit_reason == 7 and s.r.iterations >= 3 and s.margin < LC.MARGIN and 'margin' in s.why and not s.kept
    # ... and point 4 a threshold set where the value lands (the value itself, read from a fit that max_iter ends)
    r, _ = LC.oracle_fit(('exp2', 0.3, '', dict(lambda_=1.0, max_iter=3)))
    near = float(np.float32(r.chi2 / r.dof * (1 + 1e-5)))
    s = LC.Selected(('exp2', 0.3, 'near', dict(lambda_=1.0, chi2_abs=near, max_iter=30)))
    assert 0 < s.exit_margin < LC.EXIT_MARGIN and s.why == ['exit margin']


def test_every_exit_reason_is_reached_on_a_single_dataset_problem_and_on_a_global_one():
    single = {s.r.exit_reason for s in _kept(lambda s: s.row[0] in LC.SINGLE)}
    glob = {s.r.exit_reason for s in _kept(lambda s: s.row[0] in LC.GLOBAL)}
    assert single == {0, 1, 2, 3, 4, 5, 7}, single          # (reason 6 needs a global parameter)
    assert glob == {0, 1, 2, 3, 4, 5, 6, 7}, glob
    # the exit fired because its own test was the only one enabled beside max_iter: exits 3 and 4 never share a case
    tests = ('chi2_abs', 'chi2_rel', 'grad_chi2', 'cos_phi', 'rel_error', 'rel_error_global')
    for reason, name in ((3, 'grad_chi2'), (4, 'cos_phi')):
        for group in (LC.SINGLE, LC.GLOBAL):
            own = _kept(lambda s: s.row[0] in group and s.r.exit_reason == reason and [t for t in tests if t in s.options] == [name])
            assert own, (reason, group)
            assert all(s.r.iterations < s.options['max_iter'] for s in own)


POLICIES = {
    'plain, lam_up = 3, lam_down = 7': lambda o: (o.get('lam_up'), o.get('lam_down'), o.get('nielsen', 0), o.get('umnigh', 0), o.get('uphill', 0)) == (3.0, 7.0, 0, 0, 0),
    'nielsen': lambda o: (o.get('nielsen', 0), o.get('umnigh', 0), o.get('uphill', 0)) == (1, 0, 0),
    'umnigh': lambda o: (o.get('nielsen', 0), o.get('umnigh', 0), o.get('uphill', 0)) == (0, 1, 0),
    'nielsen + umnigh': lambda o: (o.get('nielsen', 0), o.get('umnigh', 0), o.get('uphill', 0)) == (1, 1, 0),
    'umnigh + uphill = 1': lambda o: (o.get('nielsen', 0), o.get('umnigh', 0), o.get('uphill', 0)) == (0, 1, 1),
    'uphill = 2': lambda o: (o.get('nielsen', 0), o.get('umnigh', 0), o.get('uphill', 0)) == (0, 0, 2),
}


def _both_kinds_of_trial(s):
    """at least two iterations, an accepted and a rejected trial among them"""
    return s.r.iterations >= 2 and s.r.n_chi2 > s.r.iterations + 1


@pytest.mark.parametrize('policy', sorted(POLICIES))
def test_each_lambda_policy_has_a_kept_case_with_an_accepted_and_a_rejected_trial(policy):
    cases = _kept(lambda s: POLICIES[policy](s.options) and _both_kinds_of_trial(s))
    print(policy, [(s.id, LC.counts(s.r)) for s in cases])
    assert cases


def test_the_matrix_core_form_and_the_global_fit_each_have_such_a_policy_case():
    for name in ('gauss8', 'global7'):
        assert _kept(lambda s: s.row[0] == name and any(p(s.options) for p in POLICIES.values()) and _both_kinds_of_trial(s)), name


def test_damp_max_0_has_a_kept_case_and_changes_the_fit():
    cases = _kept(lambda s: s.options.get('damp_max') == 0)
    assert cases
    for s in cases:          # (DTD is this iteration's diagonal, not the running maximum: from the second iteration on the steps differ)
        other, p = LC.oracle_fit(s.row[:3] + ({k: v for k, v in s.row[3].items() if k != 'damp_max'},))
        assert s.r.iterations >= 2 and not np.array_equal(p.pars, s.pars)


def test_dtd_min_binds_for_some_coordinates_and_not_for_others():
    cases = _kept(lambda s: 'DTD_min' in s.options)
    assert {s.row[0] for s in cases} == {'exp2', 'global7'}
    for s in cases:
        dtd, diag = np.array(s.options['DTD_min']), np.diag(s.p.JTJ0)
        assert dtd.size == s.r.dim and len(set(dtd)) > 1
        print(s.id, 'binds for', np.flatnonzero(dtd > diag), 'of', s.r.dim)
        assert (dtd > diag).any() and (dtd < diag).any()
        other, p = LC.oracle_fit(s.row[:3] + ({k: v for k, v in s.row[3].items() if k != 'DTD_min'},))
        assert not np.array_equal(p.pars, s.pars)


def test_accth_has_a_case_that_takes_delta2_and_one_that_zeroes_it():
    cases = _kept(lambda s: 'accth' in s.options)
    taken = [s for s in cases if s.r.n_omega == s.r.n_sweeps and np.any(s.p.delta2_0 != 0.0)]
    zeroed = [s for s in cases if s.r.n_omega == s.r.n_sweeps and not np.any(s.p.delta2_0 != 0.0)]
    assert taken and zeroed, ([s.id for s in taken], [s.id for s in zeroed])
    for s in zeroed:          # acc_ratio > accth at the first iteration: the step is delta1 alone (gadfit.F90:739-743)
        np.testing.assert_array_equal(s.p.delta1_0, orc.potr(s.p.JTJ0 + s.options['lambda_'] * np.diag(np.diag(s.p.JTJ0)), s.p.JTres0))
    assert {s.row[0] for s in cases} >= {'exp2', 'gauss8', 'global7'}


def test_a_fit_without_max_iter_is_ended_by_another_test():
    cases = _kept(lambda s: 'max_iter' not in s.options and s.r.exit_reason in (1, 2, 3, 4, 5, 6))
    assert cases


def test_lam_incs_1_ends_with_exit_7_after_an_accepted_iteration():
    cases = _kept(lambda s: s.options.get('lam_incs') == 1 and s.r.exit_reason == 7 and s.r.iterations >= 1)
    assert cases
    for s in cases:          # two trials, both rejected, in the iteration that ends the fit
        assert s.r.n_sweeps == s.r.iterations + 1 and s.r.n_chi2 >= 1 + s.r.iterations + 2


def test_where_uphill_is_0_the_oracle_returns_the_chi2_of_the_parameters_it_returns():
    """the pair (parameters, chi2) of a result belongs together, exit 7 included, which hands back the last accepted point: the GPU
    module asks the same of gfh_fit, bit for bit"""
    for s in _kept(lambda s: not s.options.get('uphill', 0)):
        p = s.problem.oracle(s.pars)
        assert p.chi2()[0] == s.r.chi2, s.id


def test_an_uphill_case_accepts_a_step_that_goes_uphill():
    """(1 - beta)^uphill new_chi2 < old_chi2 with new_chi2 > old_chi2: the fit then returns the SMALLER chi2 (old_chi2 = min,
    gadfit.F90:829) with the parameters of the larger one.  Shown by ending the same fit after k iterations"""
    s = LC.by_id('global7-0.2-uphill_step_taken')
    uphill = []
    for k in range(1, s.r.iterations + 1):
        r, p = LC.oracle_fit(s.row[:3] + (dict(s.row[3], max_iter=k),))
        assert r.iterations == k
        if p.chi2()[0] > r.chi2:
            uphill.append(k)
    print('iterations that end uphill:', uphill)
    assert uphill


def test_the_umnigh_a_carried_into_a_second_fit_matters():
    """two fits in a row, the second given the first's umnigh_a, against a second fit given 0.5 again: lambda must differ by far more
    than the device's lambda is held to, or the GPU test of the carry-over would show nothing"""
    for cid in LC.CARRY:
        s = LC.by_id(cid)
        assert _flag(s, 'umnigh') and s.umnigh_a != 0.5
        carried, _ = LC.oracle_fit(s.row, umnigh_a=s.umnigh_a, start=LC.carry_start(s))
        fresh, _ = LC.oracle_fit(s.row, umnigh_a=0.5, start=LC.carry_start(s))
        print(cid, s.umnigh_a, carried.lambda_, fresh.lambda_)
        assert abs(carried.lambda_ - fresh.lambda_) > 100 * TOL_LAMBDA * abs(carried.lambda_)
        # the second fit obeys the rule as well: counts at 1 and 3 images, and its chi2 comparisons
        three, _ = LC.oracle_fit(s.row, 3, umnigh_a=s.umnigh_a, start=LC.carry_start(s))
        assert LC.counts(three) == LC.counts(carried) and carried.min_margin > LC.MARGIN and carried.min_exit_margin > LC.EXIT_MARGIN


# ---- the oracle's report min_exit_margin ----------------------------------------------------------------------------------------------
def test_min_exit_margin_is_inf_where_nothing_was_compared():
    for s in _kept(lambda s: set(s.options) <= {'lambda_', 'max_iter', 'lam_incs', 'lam_up', 'lam_down', 'nielsen', 'damp_max', 'DTD_min'}):
        assert s.exit_margin == np.inf, s.id
    assert LC.by_id('exp2-0.3-max_iter').exit_margin == np.inf
    for s in _kept(lambda s: set(s.options) & {'chi2_abs', 'chi2_rel', 'grad_chi2', 'cos_phi', 'rel_error', 'rel_error_global', 'accth', 'uphill'}):
        assert np.isfinite(s.exit_margin), s.id


def test_min_exit_margin_of_a_chi2_abs_case_by_hand():
    """chi2_abs alone: STEP 5 compares old_chi2 / dof with the threshold once per iteration, and old_chi2 after k iterations is what a
    fit ended by max_iter = k returns"""
    s = LC.by_id('exp2-0.3-chi2_abs')
    th = s.options['chi2_abs']
    assert th == float(np.float32(th)) and s.r.exit_reason == 1
    seen = []
    for k in range(1, s.r.iterations + 1):
        r, _ = LC.oracle_fit(s.row[:3] + (dict(lambda_=1.0, max_iter=k),))
        seen.append(abs(r.chi2 / r.dof - th) / abs(th))
        assert (r.chi2 / r.dof < th) == (k == s.r.iterations)
    assert s.exit_margin == min(seen)


def test_a_fit_is_the_same_numbers_whether_or_not_the_caller_reads_the_report():
    """the report is written to the result only: a caller that passes no result gets the same parameters and the same umnigh_a, and
    two callers that do get every field of it equal"""
    for cid in ('exp2-0.3-umnigh_uphill_1', 'global7-0.3-rel_error_global', 'gauss8-0.03-accth'):
        s = LC.by_id(cid)
        again, p = LC.oracle_fit(s.row)
        for f, _ in orc.FitResult._fields_:
            if not f.endswith('0'):          # (the first-iteration snapshots are pointers, chi2_0 a value)
                assert getattr(again, f) == getattr(s.r, f), f
        assert again.chi2_0 == s.r.chi2_0 and np.array_equal(p.pars, s.pars)
        q = s.problem.oracle(s.problem.start(s.row[1]))
        o = orc.FitOptions()
        for k, v in s.options.items():
            name = 'lambda' if k == 'lambda_' else k
            setattr(o, k, v); setattr(o, 'has_' + name, 1)
        o.n_images = 1; o.umnigh_a = 0.5
        assert orc.lib().orc_fit(C.byref(q.c), C.byref(o), None) == 0
        assert np.array_equal(q.pars, s.pars) and o.umnigh_a == s.umnigh_a


def test_a_caller_that_holds_the_shorter_result_is_not_written_past_its_end():
    """orc_fit_result was 8 bytes shorter before min_exit_margin.  A caller that has not said orc_report_exit_margin(1) -- any binding
    written before the field -- gets the fit it got before and the bytes behind min_margin untouched, on a case that does compare"""
    class Shorter(C.Structure):          # the result without the new field, and guard words behind it
        _fields_ = [f for f in orc.FitResult._fields_ if f[0] != 'min_exit_margin'] + [('guard', C.c_uint64 * 4)]
    assert C.sizeof(Shorter) == C.sizeof(orc.FitResult) + 24 and Shorter.guard.offset == orc.FitResult.min_exit_margin.offset
    s = LC.by_id('global7-0.3-rel_error_global')
    assert np.isfinite(s.exit_margin)
    q = s.problem.oracle(s.problem.start(s.row[1]))
    o = orc.FitOptions()
    for k, v in s.options.items():
        setattr(o, k, v); setattr(o, 'has_' + ('lambda' if k == 'lambda_' else k), 1)
    o.n_images = 1; o.umnigh_a = 0.5
    r = Shorter()
    r.guard[:] = [0xA5A5A5A5A5A5A5A5] * 4
    orc.lib().orc_report_exit_margin(0)
    try:
        assert orc.lib().orc_fit(C.byref(q.c), C.byref(o), C.byref(r)) == 0
    finally:
        orc.lib().orc_report_exit_margin(1)
    assert list(r.guard) == [0xA5A5A5A5A5A5A5A5] * 4
    assert np.array_equal(q.pars, s.pars) and r.min_margin == s.margin and r.chi2 == s.r.chi2 and r.iterations == s.r.iterations
    again, _ = LC.oracle_fit(s.row)          # (the binding's own callers have the report back)
    assert again.min_exit_margin == s.exit_margin


# ---- gfh_lm_iterate's starts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,pert,lam', LC.LM_ITERATE, ids=[r[0] for r in LC.LM_ITERATE])
def test_the_starts_of_the_restated_loop_pass_the_rule_and_hold_a_rejection(name, pert, lam):
    prob = LC.problem(name)
    one = LC.lm_iterate_restated(prob, prob.start(pert), LC.LM_ITERATE_N, lam)
    three = LC.lm_iterate_restated(prob, prob.start(pert), LC.LM_ITERATE_N, lam, n_images=3)
    print(name, 'accepted', one[3], 'of', LC.LM_ITERATE_N, 'lambda', one[1], 'margin', one[5])
    assert 0 < one[3] < LC.LM_ITERATE_N, 'the start is meant to hold a rejection'
    assert one[5] > LC.MARGIN and one[3] == three[3] and one[1] == three[1]
    act = prob.active
    assert np.max(np.abs(one[0][:, act] - three[0][:, act]) / np.abs(one[0][:, act])) <= LC.SELF_TOL


def test_the_units_of_the_gpu_module():
    units = LC.units()
    assert len(units) == 2 * len(LC.PROBLEMS)
    assert sorted({(len(a), nd) for _, a, nd, _ in units}) == [(4, 1), (4, 3), (7, 3), (32, 1)]
    assert tuple(COUNTS) == ('iterations', 'n_sweeps', 'n_chi2', 'n_omega', 'exit_reason')
