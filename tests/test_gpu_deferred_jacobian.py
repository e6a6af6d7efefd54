"""The deferred Jacobian store of keep_jacobian mode 1 (gfh_set_keep_jacobian): inside gfh_fit only the sweeps that max_iter
guarantees to be the fit's last write J; a fit that ends any other way owes J, and the first reader materialises it.

Every case runs twice in one process -- a context created under GADFIT_HIP_DEFER_J=0 (every sweep stores: the behaviour before the
deferral) and one under GADFIT_HIP_DEFER_J=1 with GADFIT_HIP_DEFER_J_FROM=0 (no size threshold) -- and whatever a caller can read must be
equal BIT FOR BIT between the two; gfh_debug_deferred tells deferral from its absence.

Shapes: model_exp4 with 8 active parameters (the VALU form of the fused kernel) and gauss8 with 32 (the matrix form), each at
5 * 512 + 301 points (several workgroups, a padded last pass) and at 64 points (the single-workgroup tail).

One departure from the issue's wording: after gfh_set_data / gfh_set_keep_jacobian(0) a read-back fails with "no Jacobian on the device
yet" -- the message those calls have always left behind (they clear have_sweep, which gfh_get_jacobian tests first) and the same in both
contexts; "Jacobian was not kept" is what the readers say when a sweep ran without the store.  The tests pin the error, the unchanged
message, that nothing was materialised and that nothing is owed any more."""
import functools

import numpy as np
import pytest

from gadfit_amd import _lib
from gadfit_amd.ad import trace_model
from tests import models as M

pytestmark = pytest.mark.gpu

N_BIG = 5 * 512 + 301
RESULT_FIELDS = ('iterations', 'dim', 'dof', 'exit_reason', 'lambda_', 'chi2', 'n_sweeps', 'n_chi2', 'n_omega', 'n_lookahead')
CASES = [('exp4', N_BIG), ('exp4', 64), ('gauss8', N_BIG), ('gauss8', 64)]
CASE_IDS = ['%s-%d' % c for c in CASES]


@functools.lru_cache(maxsize=None)
def _problem(name, n):
    """(tape, x, y, w, truth, number of parameters): computed once, shared, never written to"""
    if name == 'exp4':
        fn, model, truth = M.exp4_numpy, M.model_exp4, M.EXP4_TRUTH
    else:
        fn, model, truth = M.gauss8_numpy, M.model_gauss8, M.gauss8_truth()
    x, y, s = M.make_single(fn, truth, n, 0.0, 100.0)
    w = 1.0 / s
    for a in (x, y, w):
        a.setflags(write=False)
    return trace_model(model, truth.size), x, y, w, truth, truth.size


def _near(truth):
    return M.start_values(truth).reshape(1, -1)


def _far(truth):
    """the start of bench.py's rejecting leg: 40 % off, alternating sign"""
    return (truth * (1.0 + 0.4 * np.where(np.arange(truth.size) % 2 == 0, 1.0, -1.0))).reshape(1, -1)


class Pair:
    """the same problem on two contexts: [0] stores at every sweep, [1] defers"""

    def __init__(self, monkeypatch, name, n, threshold='0', make=lambda: _lib.Context(0)):
        self.tape, x, y, w, self.truth, self.np_ = _problem(name, n)
        self.act = list(range(self.np_)); self.glob = [0] * self.np_
        self.ctx = []
        for defer in ('0', '1'):
            monkeypatch.setenv('GADFIT_HIP_DEFER_J', defer)
            if threshold is None:
                monkeypatch.delenv('GADFIT_HIP_DEFER_J_FROM', raising=False)
            else:
                monkeypatch.setenv('GADFIT_HIP_DEFER_J_FROM', threshold)
            c = make()
            self.ctx.append(c)
            c.set_model(self.tape)
            c.set_data(x, y, w, [0, x.size])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for c in self.ctx:
            c.close()

    def fit(self, start, **kw):
        """the fit on both contexts; the parameters and every count of the result must agree"""
        out = [c.fit(start, self.act, self.glob, **kw) for c in self.ctx]
        (p0, r0), (p1, r1) = out
        assert np.array_equal(p0, p1)
        for f in RESULT_FIELDS:
            assert getattr(r0, f) == getattr(r1, f), f
        return p0, r0

    def counts(self):
        return [c.debug_deferred() for c in self.ctx]

    def same_jacobian(self):
        J0, J1 = (c.jacobian(len(self.act)) for c in self.ctx)
        assert J0.size and np.array_equal(J0, J1)
        return J0

    def same_residuals(self):
        r0, r1 = (c.residuals() for c in self.ctx)
        assert r0.size and np.array_equal(r0, r1)


@pytest.mark.parametrize('lookahead', [True, False], ids=['lookahead', 'reference-schedule'])
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_max_iter_exit_stores_once(monkeypatch, case, lookahead):
    """a fit that max_iter ends returns with J in HBM, and has paid for it once: five sweeps deferred, the one of the last permitted
    iteration stored, nothing materialised, nothing owed"""
    with Pair(monkeypatch, *case) as P:
        for c in P.ctx:
            c.set_lookahead(lookahead)
        p, r = P.fit(_near(P.truth), lambda_=1.0, max_iter=6)
        assert r.exit_reason == 0 and r.iterations == 6
        eager, deferring = P.counts()
        print('max_iter exit', case, lookahead, 'n_sweeps', r.n_sweeps, 'n_lookahead', r.n_lookahead, eager, deferring)
        # six iterations are six sweeps unless a look-ahead sweep was thrown away at a rejected trial (exp4 at 64 points rejects one):
        # the context that stores at every sweep counts them
        n = eager['stored']
        assert n >= 6 and (lookahead or n == 6)
        assert eager == dict(deferred=0, stored=n, materialised=0, owed=False)
        if n == 6:
            assert deferring == dict(deferred=5, stored=1, materialised=0, owed=False)
        else:          # (only sweeps handed to, or made by, iteration 6 store: one, or two if the one handed over was the rejected one)
            assert deferring['deferred'] + deferring['stored'] == n and 1 <= deferring['stored'] <= 2
            assert deferring['materialised'] == 0 and not deferring['owed']
        P.same_jacobian(); P.same_residuals()
        assert P.counts()[1]['materialised'] == 0


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_chi2_rel_exit_owes_the_jacobian(monkeypatch, case):
    with Pair(monkeypatch, *case) as P:
        p, r = P.fit(_near(P.truth), lambda_=1.0, chi2_rel=1e-3, lam_incs=8)
        assert r.exit_reason == 2 and r.iterations >= 2          # (the iteration the storing context's result names)
        eager, deferring = P.counts()
        print('chi2_rel exit', case, 'iterations', r.iterations, eager, deferring)
        assert eager['deferred'] == 0 and not eager['owed']
        assert deferring['stored'] == 0 and deferring['deferred'] == eager['stored'] and deferring['owed'] and deferring['materialised'] == 0
        P.same_jacobian()
        assert P.counts()[1] == dict(deferring, materialised=1, owed=False)
        P.same_residuals()
        P.same_jacobian()                                          # (a second read-back finds J there)
        assert P.counts()[1]['materialised'] == 1 and P.counts()[0]['materialised'] == 0
    with Pair(monkeypatch, *case) as P:                            # J^T res of the device's J and res, on a fresh pair
        P.fit(_near(P.truth), lambda_=1.0, chi2_rel=1e-3, lam_incs=8)
        g0, g1 = (c.aux(0, dim=P.np_) for c in P.ctx)
        assert np.any(g0 != 0.0) and np.array_equal(g0, g1)
        assert P.counts()[1]['materialised'] == 1
        P.same_residuals()


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_give_up_exit_repeats_the_chi2_pass(monkeypatch, case):
    """exit 7: the last pass of the fit is a chi2() at a rejected trial point, which wrote res after the owed sweep -- materialising J
    rewrites res, so that pass is repeated and the residual read-back returns the bits it returned before"""
    with Pair(monkeypatch, *case) as P:
        p, r = P.fit(_far(P.truth), lambda_=1e-6, lam_incs=1)
        print('give-up exit', case, 'iterations', r.iterations, 'n_sweeps', r.n_sweeps, 'n_chi2', r.n_chi2, P.counts())
        assert r.exit_reason == 7
        assert P.counts()[1]['owed'] and P.counts()[1]['stored'] == 0
        before = P.ctx[1].residuals().copy()                       # (res needs no J: nothing is materialised by reading it)
        assert P.counts()[1]['materialised'] == 0
        P.same_jacobian()
        assert P.counts()[1]['materialised'] == 1
        P.same_residuals()
        assert np.array_equal(P.ctx[1].residuals(), before)


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_rejected_lookahead_sweep(monkeypatch, case):
    """the start and lambda of bench.py's rejecting leg: J is that of the most recent sweep, whichever point that was"""
    with Pair(monkeypatch, *case) as P:
        p, r = P.fit(_far(P.truth), lambda_=1e-6, lam_incs=8, max_iter=4)
        print('rejecting fit', case, 'exit', r.exit_reason, 'iterations', r.iterations, 'n_sweeps', r.n_sweeps, 'n_chi2', r.n_chi2,
              'n_lookahead', r.n_lookahead, P.counts())
        assert r.n_chi2 > r.n_lookahead                            # (trials were rejected)
        P.same_jacobian(); P.same_residuals()


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_options_that_read_the_jacobian(monkeypatch, case):
    with Pair(monkeypatch, *case) as P:
        for kw in (dict(cos_phi=1e-30), dict(grad_chi2=1e-30)):
            P.fit(_near(P.truth), lambda_=1.0, max_iter=4, **kw)
            assert P.counts()[1]['deferred'] == 0 and not P.counts()[1]['owed']
            P.same_jacobian(); P.same_residuals()
        if case[0] == 'exp4':          # STEP 3 recomputes its rows (gfh_k_omega_jt): the accelerated fit does not read J
            p, r = P.fit(_near(P.truth), lambda_=1.0, accth=0.9, max_iter=4)
            assert r.n_omega > 0 and P.counts()[1]['deferred'] > 0
            P.same_jacobian(); P.same_residuals()
            p, r = P.fit(_near(P.truth), lambda_=1.0, accth=0.9, chi2_rel=1e-3, lam_incs=8)
            assert r.n_omega > 0 and P.counts()[1]['owed']
            P.same_jacobian(); P.same_residuals()


def test_global_fit(monkeypatch):
    """3 datasets x 700 points, four local and three shared parameters"""
    xs, ys, ss, truths = M.make_global7(3, 700)
    tape = trace_model(M.model_global7, 7)
    act = list(range(7)); glob = [0, 0, 0, 0, 1, 1, 1]
    start = truths * np.where(np.arange(7) % 2 == 0, 1.05, 0.95)[None, :]
    start[:, 4:] = start[0, 4:]
    got = []
    for defer in ('0', '1'):
        monkeypatch.setenv('GADFIT_HIP_DEFER_J', defer); monkeypatch.setenv('GADFIT_HIP_DEFER_J_FROM', '0')
        c = _lib.Context(0)
        try:
            c.set_model(tape)
            c.set_data(np.concatenate(xs), np.concatenate(ys), 1.0 / np.concatenate(ss), [0, 700, 1400, 2100])
            p, r = c.fit(start, act, glob, lambda_=1.0, chi2_rel=1e-3, lam_incs=8)
            d = c.debug_deferred()
            got.append((p, r.chi2, r.iterations, r.exit_reason, d, c.jacobian(7), c.residuals(), c.debug_deferred()))
        finally:
            c.close()
    e, f = got
    assert e[3] == 2 and np.array_equal(e[0], f[0]) and e[1:4] == f[1:4]
    assert e[4]['deferred'] == 0 and f[4]['deferred'] > 0 and f[4]['owed'] and f[7]['materialised'] == 1
    assert np.array_equal(e[5], f[5]) and np.any(e[5] != 0.0) and np.array_equal(e[6], f[6])


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_state_changes_drop_an_owed_jacobian(monkeypatch, case):
    tape, x, y, w, truth, np_ = _problem(*case)
    for change in ('set_data', 'keep_0', 'sweep'):
        with Pair(monkeypatch, *case) as P:
            p, r = P.fit(_near(P.truth), lambda_=1.0, chi2_rel=1e-3, lam_incs=8)
            assert P.counts()[1]['owed']
            if change == 'sweep':
                jac, dim = P.ctx[0].jacobian_indices(P.act, P.glob)
                s0, s1 = (c.sweep(_near(P.truth), P.act, jac, dim) for c in P.ctx)      # a direct sweep stores as always
                assert np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1]) and s0[2] == s1[2]
                assert not P.counts()[1]['owed']
                P.same_jacobian(); P.same_residuals()
            else:
                for c in P.ctx:
                    if change == 'set_data':
                        c.set_data(x, y, w, [0, x.size])
                    else:
                        c.set_keep_jacobian(0)
                    assert not c.debug_deferred()['owed']
                    # (see the module's docstring: the message both calls have always left behind)
                    with pytest.raises(_lib.GadfitHipError, match='no Jacobian on the device yet'):
                        c.jacobian(np_)
            assert P.counts()[1]['materialised'] == 0 and not P.counts()[1]['owed']


def test_never_owed_jacobian_fails_with_the_usual_message(monkeypatch):
    """keep_jacobian mode 2 gives J up: its read-back fails as before, in both contexts, and materialises nothing"""
    with Pair(monkeypatch, 'exp4', N_BIG) as P:
        for c in P.ctx:
            c.set_keep_jacobian(2)
        P.fit(_near(P.truth), lambda_=1.0, chi2_rel=1e-3, lam_incs=8)
        for c in P.ctx:
            with pytest.raises(_lib.GadfitHipError, match='Jacobian was not kept'):
                c.jacobian(P.np_)
            assert c.debug_deferred() == dict(deferred=0, stored=0, materialised=0, owed=False)


def test_threshold_default_defers_nothing_small(monkeypatch):
    """GADFIT_HIP_DEFER_J_FROM at its default (the size from which a Jacobian buffer is placed): the same small fit stores at every sweep"""
    with Pair(monkeypatch, 'gauss8', N_BIG, threshold=None) as P:
        p, r = P.fit(_near(P.truth), lambda_=1.0, chi2_rel=1e-3, lam_incs=8)
        assert r.exit_reason == 2
        eager, deferring = P.counts()
        assert eager == deferring and deferring['deferred'] == 0 and deferring['stored'] > 0 and not deferring['owed']
        P.same_jacobian()


def test_two_member_device_group(monkeypatch):
    """two members on one card, their sums added on the host in rank order: the fit is the same with and without deferral, and every
    member materialises its own share on a read-back (no collective)"""
    monkeypatch.setenv('GADFIT_HIP_GROUP_REDUCE', 'host')
    with Pair(monkeypatch, 'exp4', N_BIG, make=lambda: _lib.Context(devices=[0, 0])) as P:
        p, r = P.fit(_near(P.truth), lambda_=1.0, chi2_rel=1e-3, lam_incs=8)
        assert r.exit_reason == 2
        eager, deferring = P.counts()
        assert eager['deferred'] == 0 and deferring['deferred'] > 0 and deferring['owed']
        P.same_jacobian(); P.same_residuals()
        assert P.counts()[1]['materialised'] == 1
