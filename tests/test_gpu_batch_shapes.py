"""The 64-lane form of the batch kernels (a wave per fit; what a context launches that nobody told anything) under the suite of
tests/batch_form_suite.py, over the input space tests/test_gpu_batch.py leaves out -- the form's row of the table in
tests/batch_form_cases.py: n = 4 ... 20001, cuts that leave 3, 2, 1 live waves in the last workgroup -- and what only this form's
module holds: the context's state from call to call, and the whole operator set (Part 3 of tests/batch_cases.py).  The observed
maxima go under the keys shapes_*."""
import numpy as np
import pytest

pytest.register_assert_rewrite('tests.batch_form_suite')
from tests import batch_cases as BC  # noqa: E402
from tests import batch_form_cases as FC  # noqa: E402
from tests import batch_form_suite as S  # noqa: E402
from tests.batch_common import SCENARIOS, TOL_FIT, TOL_PASS, check_fit, context, fit_worst, observe, pass_worst, same_bits, same_pass  # noqa: E402

pytestmark = pytest.mark.gpu

globals().update(S.tests_of(FC.WAVE))          # F, E and the suite's tests under the names they have had here


# ---- the context's state from call to call -----------------------------------------------------------------------------------------
def test_state_on_one_context(F):
    """batch_pass -> fit_batch -> batch_pass (io and img reallocated in between), a batch of 3 in place of the batch of 108 and
    back, then a plain set_data + fit on the same context (its kernel cache holds the batch unit under a key of its own): every
    result is the bits of the first call on that data, and the plain fit returns what a fresh context returns"""
    off, kw = SCENARIOS['c']
    starts, p5 = F.starts(off), F.starts(0.05)
    k = 5                       # (a spectrum of 1000 points)
    c = context(F.tape, F.batch)
    try:
        pass0 = c.batch_pass(p5, FC.ACTIVE)
        same_pass(pass0, F.one_pass())
        p0, r0, _ = c.fit_batch(starts, FC.ACTIVE, **kw)
        same_bits(p0, r0, *F.fit('c'))
        same_pass(c.batch_pass(p5, FC.ACTIVE), pass0)
        c.set_batch_data(*F.batch.first(3))
        p3, r3, _ = c.fit_batch(starts[:3], FC.ACTIVE, **kw)
        same_bits(p3, r3, p0[:3], r0[:3])
        same_pass(c.batch_pass(p5[:3], FC.ACTIVE), [v[:3] for v in pass0])
        c.set_batch_data(F.batch.off, F.batch.x, F.batch.y, F.batch.w)
        same_pass(c.batch_pass(p5, FC.ACTIVE), pass0)
        p1, r1, _ = c.fit_batch(starts, FC.ACTIVE, **kw)
        same_bits(p1, r1, p0, r0)
        plain = S.plain_fit(c, F.batch.items[k], starts[k], kw)
        p2, r2, _ = c.fit_batch(starts, FC.ACTIVE, **kw)          # ... and the batch is still there after the plain fit
        same_bits(p2, r2, p0, r0)
    finally:
        c.close()
    f = context(F.tape)
    try:
        fresh = S.plain_fit(f, F.batch.items[k], starts[k], kw)
    finally:
        f.close()
    S.same_plain_fit(plain, fresh)


# ---- Part 3: the whole operator set (64 lanes) -----------------------------------------------------------------------------------------
def _operator_pass(seed, c):
    tape, active, starts, batch = BC.part3(seed)
    JTJ, JTr, chi2 = c.batch_pass(starts, active)
    return pass_worst(tape, batch.items, starts, active, JTJ, JTr, chi2)


@pytest.mark.parametrize('seed', BC.OPERATOR_SEEDS)
def test_operator_set_against_the_oracle(seed):
    """p[0] e_0 + ... + p[4] e_4 with random expressions over pow in its four forms, log, sqrt, exp, the trigonometric and hyperbolic
    functions and their inverses, and (seed 32) the written model with erf, a bare abs and unary minus, which the random expressions
    never draw: gfh_point_grad, gfh_point_value and gfh_point_dd_grad inside the batch unit.  Under (i)
    delta2 is always kept, so one iteration is old + delta1 + delta2 / 2 of a well-damped system: STEP 3 without conditioning."""
    tape, active, starts, batch = BC.part3(seed)
    c = context(tape, batch)
    try:
        worst = _operator_pass(seed, c)
        observe(shapes_random_pass=worst)
        assert worst < TOL_PASS
        for name, kw in BC.RANDOM_ARGS.items():
            sel = BC.part3_selection(seed, name)
            pars, res, _ = c.fit_batch(starts, active, **kw)
            passive = [k for k in range(BC.NP_) if k not in active]
            assert np.array_equal(pars[:, passive], starts[:, passive])
            if name == 'i':
                assert np.all(res['n_omega'] == 1) and np.all(res['iterations'] == 1)
            check_fit('shapes', 'random_%s' % name, fit_worst(sel, pars, res, batch.n, len(active)), TOL_FIT, TOL_FIT)
    finally:
        c.close()


def test_operator_set_with_the_librarys_pow_and_divisions(monkeypatch):
    """a model with x ** a on a context created under GADFIT_HIP_FAST_DIV=0 (read when the context is created): the same bound"""
    seed = BC.RANDOM_POW_SEED
    tape, active, starts, batch = BC.part3(seed)
    monkeypatch.setenv('GADFIT_HIP_FAST_DIV', '0')
    c = context(tape, batch)
    try:
        src = c.batch_source(active)
        assert '#define GFH_FAST_DIV 0' in src and 'gfh_pow_ln(' not in src
        worst = _operator_pass(seed, c)
    finally:
        c.close()
    observe(shapes_random_pass_library_pow=worst)
    assert worst < TOL_PASS
