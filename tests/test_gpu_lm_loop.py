"""The plain fit's LM loop (gfh_fit, gfh_lm_iterate: lm.cpp, lm_options.h, normal_eq.cpp) held to the oracle on every exit test and
lambda policy, on the VALU fused form, the matrix-core form and a global fit, over the kept rows of tests/lm_loop_cases.py (the rule
that keeps them is evaluated by the oracle alone: tests/test_cpu_lm_loop_cases.py).  The oracle's fits are made once and shared
(lm_loop_cases.selected); so is each case's fit on the default context, which the schedule variants are compared with bit for bit.

GADFIT_PARITY_DUMP=<file> records the observed maxima (parity_common._observe); DESIGN section 7 quotes them."""
import contextlib
import os

import numpy as np
import pytest

from gadfit_amd import _lib
from tests import lm_loop_cases as LC
from tests.batch_common import COUNTS, TOL_CHI2
from tests.parity_common import TOL_FIT, TOL_LAMBDA, _close

pytestmark = pytest.mark.gpu

KEPT = LC.kept_ids()


@contextlib.contextmanager
def _env(**kw):
    """the switches a context reads when it is created"""
    before = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _default():
    return _lib.Context(0)


def _la0():
    c = _lib.Context(0); c.set_lookahead(0)
    return c


def _keep2():
    c = _lib.Context(0); c.set_keep_jacobian(2)
    return c


def _la0_keep2():
    c = _lib.Context(0); c.set_lookahead(0); c.set_keep_jacobian(2)
    return c


def _defer1():
    with _env(GADFIT_HIP_DEFER_J='1', GADFIT_HIP_DEFER_J_FROM='0'):
        return _lib.Context(0)


def _defer0():
    with _env(GADFIT_HIP_DEFER_J='0'):
        return _lib.Context(0)


def _group():
    return _lib.Context(devices=[0, 0, 0])


def _unfused():
    with _env(GADFIT_HIP_FUSED='0'):
        return _lib.Context(0)


MAKE = dict(default=_default, la0=_la0, keep2=_keep2, la0_keep2=_la0_keep2, defer1=_defer1, defer0=_defer0, group=_group, unfused=_unfused)
SCHEDULES = ('la0', 'keep2', 'la0_keep2', 'defer1', 'defer0')
KEEPS_RESIDUALS = ('default', 'la0', 'defer1', 'defer0')          # keep_jacobian mode 1: residuals() can be read after the fit


class Pool:
    """one context per variant, made when first asked for; each holds one problem at a time (the table is ordered by problem)"""

    def __init__(self):
        self.ctx, self.bound = {}, {}

    def get(self, variant, prob):
        if variant not in self.ctx:
            self.ctx[variant] = MAKE[variant]()
        c = self.ctx[variant]
        if self.bound.get(variant) != prob.name:
            c.set_model(prob.tape)
            c.set_data(prob.x, prob.y, prob.w, prob.pos)
            self.bound[variant] = prob.name
        return c

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope='module')
def pool():
    p = Pool()
    yield p
    p.close()


def _fit(pool, variant, s, umnigh_a=0.5, start=None, residuals=False):
    """the row's fit on a variant's context: (parameters, FitResult, the umnigh_a handed on, residuals() or None)"""
    prob = s.problem
    c = pool.get(variant, prob)
    out, r = c.fit(prob.start(s.row[1]) if start is None else start, prob.active, prob.is_global, umnigh_a=umnigh_a, **s.options)
    return out, r, float(c.umnigh_a), (c.residuals().copy() if residuals else None)


_DEFAULT = {}


def _default_fit(pool, cid):
    if cid not in _DEFAULT:
        _DEFAULT[cid] = _fit(pool, 'default', LC.by_id(cid), residuals=True)
    return _DEFAULT[cid]


def _counts(r):
    return tuple(int(getattr(r, f)) for f in COUNTS)


def _against_the_oracle(s, out, r, umnigh_a, r0=None, pars0=None, umnigh_a0=None):
    """counts, dim and dof equal; the active parameters at TOL_FIT (the passive ones untouched), lambda at TOL_LAMBDA, chi2 at TOL_CHI2,
    umnigh_a to 4 ulp"""
    r0 = s.r if r0 is None else r0
    pars0 = s.pars if pars0 is None else pars0
    umnigh_a0 = s.umnigh_a if umnigh_a0 is None else umnigh_a0
    assert _counts(r) + (r.dim, r.dof) == LC.counts(r0) + (r0.dim, r0.dof), (s.id, _counts(r), LC.counts(r0))
    act = s.problem.active
    passive = [k for k in range(s.problem.n_pars) if k not in act]
    assert np.array_equal(out[:, passive], pars0[:, passive])
    _close('pars', out[:, act], pars0[:, act], TOL_FIT)
    _close('lambda', r.lambda_, r0.lambda_, TOL_LAMBDA)
    _close('chi2', r.chi2, r0.chi2, TOL_CHI2)
    if s.options.get('umnigh'):
        assert abs(umnigh_a - umnigh_a0) <= 4 * np.spacing(umnigh_a0), (umnigh_a, umnigh_a0)
    else:
        assert umnigh_a == umnigh_a0 == 0.5


@pytest.mark.parametrize('cid', KEPT)
def test_fit_against_the_oracle(pool, cid):
    s = LC.by_id(cid)
    out, r, umnigh_a, _ = _default_fit(pool, cid)
    _against_the_oracle(s, out, r, umnigh_a)
    if 'grad_chi2' in s.options or 'cos_phi' in s.options:
        assert r.n_lookahead == 0
    if not s.options.get('uphill', 0):
        # the pair a fit returns belongs together: exit 7 hands back the last accepted point with its chi2
        assert pool.get('default', s.problem).chi2(out) == r.chi2, (s.id, r.exit_reason)


@pytest.mark.parametrize('cid', KEPT)
def test_every_schedule_gives_the_default_contexts_bits(pool, cid):
    """look-ahead, the Jacobian store and its deferral change which kernels run, never a value the loop sees"""
    s = LC.by_id(cid)
    p0, r0, a0, res0 = _default_fit(pool, cid)
    for variant in SCHEDULES:
        p1, r1, a1, res1 = _fit(pool, variant, s, residuals=variant in KEEPS_RESIDUALS)
        assert _counts(r1) + (r1.dim, r1.dof) == _counts(r0) + (r0.dim, r0.dof), (variant, _counts(r1), _counts(r0))
        assert np.array_equal(p1, p0), variant
        assert r1.chi2 == r0.chi2 and r1.lambda_ == r0.lambda_ and a1 == a0, variant
        if variant.startswith('la0') or 'grad_chi2' in s.options or 'cos_phi' in s.options:
            assert r1.n_lookahead == 0, variant
        if res1 is not None:
            assert res1.size == s.problem.x.size and np.array_equal(res1, res0), variant


def _one_per_problem(also=()):
    """the first kept row of every problem, and every kept row of the problems in `also`"""
    seen, out = set(), []
    for s in LC.kept():
        if s.row[0] in also or s.row[0] not in seen:
            out.append(s.id)
        seen.add(s.row[0])
    return out


@pytest.mark.parametrize('cid', _one_per_problem(also=LC.GLOBAL))
def test_fit_on_a_device_group_against_the_oracle(pool, cid):
    """three members on the one card: another order of the point sums, the same decisions"""
    s = LC.by_id(cid)
    out, r, umnigh_a, _ = _fit(pool, 'group', s)
    _against_the_oracle(s, out, r, umnigh_a)


@pytest.mark.parametrize('cid', _one_per_problem())
def test_fit_on_the_unfused_chain_against_the_oracle(pool, cid):
    """GADFIT_HIP_FUSED=0: the plain sweep and the stand-alone Gram kernels under the same loop"""
    s = LC.by_id(cid)
    out, r, umnigh_a, _ = _fit(pool, 'unfused', s)
    _against_the_oracle(s, out, r, umnigh_a)


@pytest.mark.parametrize('cid', LC.CARRY)
def test_umnigh_a_is_carried_from_fit_to_fit(pool, cid):
    """the SAVEd local of gadfit.F90:515: a second fit given the first's umnigh_a, against the oracle doing the same; a third given 0.5
    again lands elsewhere (by how much is judged on the oracle: tests/test_cpu_lm_loop_cases.py)"""
    s = LC.by_id(cid)
    start = LC.carry_start(s)
    _, _, a1, _ = _default_fit(pool, cid)
    r2, p2 = LC.oracle_fit(s.row, umnigh_a=s.umnigh_a, start=start)
    out2, d2, a2, _ = _fit(pool, 'default', s, umnigh_a=a1, start=start)
    _against_the_oracle(s, out2, d2, a2, r0=r2, pars0=p2.pars, umnigh_a0=float(p2.umnigh_a))
    r3, p3 = LC.oracle_fit(s.row, umnigh_a=0.5, start=start)
    out3, d3, a3, _ = _fit(pool, 'default', s, umnigh_a=0.5, start=start)
    _against_the_oracle(s, out3, d3, a3, r0=r3, pars0=p3.pars, umnigh_a0=float(p3.umnigh_a))
    # the value matters: judged on the oracle, whose two lambdas the device's are each held to at TOL_LAMBDA
    assert abs(r2.lambda_ - r3.lambda_) > 100 * TOL_LAMBDA * abs(r2.lambda_)


# ---- gfh_lm_iterate -------------------------------------------------------------------------------------------------------------------
def _iterate(c, prob, start, calls):
    pars = np.ascontiguousarray(start, dtype=np.float64).copy()
    state3 = np.array([calls[0], -1.0, 0.0]); DTD = np.zeros(c.jacobian_indices(prob.active, prob.is_global)[1])
    for n in calls[1:]:
        c.lm_iterate(pars, prob.active, prob.is_global, n, state3, DTD)
    return pars, state3, DTD


@pytest.mark.parametrize('name,pert,lam', LC.LM_ITERATE, ids=[r[0] for r in LC.LM_ITERATE])
@pytest.mark.parametrize('variant', ['default', 'la0'])
def test_lm_iterate_against_its_scheme_restated_over_the_oracle(pool, name, pert, lam, variant):
    prob = LC.problem(name)
    pars0, lam0, chi0, accepted0, DTD0, _ = LC.lm_iterate_restated(prob, prob.start(pert), LC.LM_ITERATE_N, lam)
    c = pool.get(variant, prob)
    pars, state3, DTD = _iterate(c, prob, prob.start(pert), (lam, LC.LM_ITERATE_N))
    assert int(state3[2]) == accepted0 and 0 < accepted0 < LC.LM_ITERATE_N
    act = prob.active
    _close('pars', pars[:, act], pars0[:, act], TOL_FIT)
    _close('lambda', state3[0], lam0, TOL_LAMBDA)
    _close('chi2', state3[1], chi0, TOL_CHI2)
    _close('DTD', DTD, DTD0, TOL_CHI2)
    assert c.chi2(pars) == state3[1]
    # two calls of three iterations that carry state3 and DTD are one call of six
    pars2, state2, DTD2 = _iterate(c, prob, prob.start(pert), (lam, 3, 3))
    assert np.array_equal(pars2, pars) and np.array_equal(state2, state3) and np.array_equal(DTD2, DTD)
