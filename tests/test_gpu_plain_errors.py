"""The errors and the curves of a plain fit on the device (gfh_covariance, gfh_fit_errors, gfh_eval; Context.covariance, Context.eval,
gadf_errors, gadf_curves; the kernels of device/eval.hip).  Inputs, rule and yardstick: tests/plain_errors_cases.py
(tests/test_cpu_plain_errors.py runs them without a GPU and shows that the rule keeps every case: none is left out here).

Bounds -- the batch's, carried over (tests/test_gpu_batch_cov.py, tests/test_gpu_batch_eval.py), with r_host the yardstick of the
library's own host algebra (tests/test_cpu_plain_errors.py: observed 1.47), eps = 2^-52, TOL_PASS = 2e-13 the project's per-pass
bound and kappa = kappa_2 of the ORACLE's J^T J scaled to unit diagonal:
  covariance, algebra alone, against the longdouble inverse of the device's OWN sweep matrix: err <= 10 r_host eps kappa, and
      || C~ A~ - I || <= that times || A~ || || C~ ||; cov symmetric and sigma = sqrt(diag) bit for bit
  covariance against the oracle's matrix: err <= (na TOL_PASS + 10 r_host eps) kappa
  scale=True: scale=False times chi2() / dof, bit for bit
  |model - f0| <= TOL_PASS |f0|
  |residual - res0| <= TOL_PASS (|y| + |f0|) w
  |band^2 - g0^T C g0| <= (2 TOL_PASS + (na^2 + na) eps) sum_ab |g0_a| |C_ab| |g0_b| in longdouble, C the dataset's block of the
      covariance that was passed in
f0, g0: oracle.binding.eval_reverse point by point (the plain models); for the branching and the auxiliary-column model, which
eval_reverse does not take, OracleProblem.sweep's stored Jacobian and residuals (plain_errors_cases.oracle_points).
Under use_ad = 0 the gradient is the forward difference, rounding noise of f over the step: entry by entry it lies within D_a =
FD_DEVICE_FACTOR FD_C_REF eps S / |step_a| of the longdouble forward difference g0 of the closed form (tests/gram_option_cases.py:
S the sum of the model's positive terms, the factor 4 x 1.96 derived and measured there), and through the quadratic form
  |band^2 - g0^T C g0| <= 2 sum_ab D_a |C_ab| |g0_b| + sum_ab D_a |C_ab| D_b + (na^2 + na) eps sum_ab |g0_a| |C_ab| |g0_b|.
The observed maxima go where the batch modules' go (GADFIT_BATCH_OBSERVE), under plain_*; profiles/plain_eval.json holds a run's:
covariance 0.27 eps kappa against the device's own matrix and 8e-4 of the bound against the oracle's, model 3.6e-3, residual 1.8e-3
and band 1.5e-3 of their bounds (3.0e-3 and 2.2e-4 on a grid), the band under finite differences 0.079 of its allowance."""
import itertools

import numpy as np
import pytest

from gadfit_amd import _lib
from gadfit_amd import tape as T
from oracle import binding as orc
from tests import batch_cov_cases as CV
from tests import branching as B
from tests import gram_option_cases as GO
from tests import models as M
from tests import plain_errors_cases as PC
from tests.batch_common import TOL_PASS, observe

pytestmark = pytest.mark.gpu

EPS = PC.EPS
LD = np.longdouble
_CTX = {}
_COV = {}
CASES = [c.name for c in PC.all_cases()]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def case_of(name):
    return {c.name: c for c in PC.all_cases()}[name]


def ctx_of(case):
    if case.name not in _CTX:
        _CTX[case.name] = case.context()
    return _CTX[case.name]


def cov_of(case):
    """(cov, sigma, info) of the case on its context, unscaled, once"""
    if case.name not in _COV:
        _COV[case.name] = ctx_of(case).covariance(case.pars, case.active, case.is_global)
    return _COV[case.name]


@pytest.fixture(scope='module', autouse=True)
def _contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear(); _COV.clear()


def reference_points(case, xs=None):
    """(f0, g0 [n][na] in the caller's order) of a case on its own abscissas or, per dataset, on the grid xs"""
    if case.name in ('piecewise2', 'aux'):
        assert xs is None
        f0, g0, _ = PC.oracle_points(case)
        return f0, g0
    f0, g0 = [], []
    for d in range(len(case.xs)):
        for xv in (case.xs[d] if xs is None else xs):
            f, g = orc.eval_reverse(case.tape, float(xv), case.pars[d], [1] * case.n_pars)
            f0.append(f); g0.append(g[case.active])
    return np.array(f0), np.array(g0)


def blocks(case, cov):
    """the datasets' na x na blocks of a dim x dim covariance, gathered through Jacobian_indices"""
    jac = case.oracle().jac
    return [cov[np.ix_(jac[d], jac[d])] for d in range(len(case.xs))]


def band_check(band, g, Cf, extra=None):
    """a band against g^T C g in longdouble; `extra` a further allowance per point (finite differences); returns the worst
    |band^2 - s2_ref| / bound"""
    na = g.shape[1]
    gl, Cl = g.astype(LD), Cf.astype(LD)
    s2 = np.einsum('ia,ab,ib->i', gl, Cl, gl)
    A = np.einsum('ia,ab,ib->i', np.abs(gl), np.abs(Cl), np.abs(gl))
    bound = (2 * TOL_PASS + (na * na + na) * EPS) * A if extra is None else (na * na + na) * EPS * A + extra
    err = np.abs(band.astype(LD) ** 2 - s2)
    worst = float(np.max(err / bound))
    print('band: max |band^2 - s2_ref| / bound = %.3e' % worst)
    assert np.all(err <= bound)
    return worst


def curves_check(case, got, f0, g0, cov, res0=None):
    """model, residual (where res0 is given) and band (where got holds one) of the data's own points against the references; returns
    the worst ratios to the bounds"""
    model, residual, band, _ = got
    worst = {}
    e = np.abs(model - f0) / np.abs(f0)
    assert np.all(e <= TOL_PASS), (case.name, e.max())
    worst['model'] = float(e.max() / TOL_PASS)
    if res0 is not None:
        er = np.abs(residual - res0) / ((np.abs(case.y()) + np.abs(f0)) * case.w())
        assert np.all(er <= TOL_PASS), (case.name, er.max())
        worst['residual'] = float(er.max() / TOL_PASS)
    if band is not None:
        worst['band'] = 0.0
        for d, Cd in enumerate(blocks(case, cov)):
            s = slice(case.pos[d], case.pos[d + 1])
            worst['band'] = max(worst['band'], band_check(band[s], g0[s], Cd))
    return worst


# ---- 1: the covariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_covariance_against_the_oracle(name):
    case = case_of(name)
    c = ctx_of(case)
    r_host = PC.r_host()
    A0, _, kap, jac, dim = PC.oracle_pass(name)
    assert kap <= PC.KAPPA_MAX
    na = len(case.active)
    JTJ = c.sweep(case.pars, case.active, jac, dim)[0]
    cov, sigma, info = cov_of(case)
    assert info == 0 and cov.shape == (dim, dim)
    assert np.array_equal(_bits(cov), _bits(cov.T)) and np.array_equal(_bits(sigma), _bits(np.sqrt(np.diag(cov))))
    d = CV.scale_of(JTJ)
    bound = 10.0 * r_host * EPS * kap
    err = CV.scaled_error(cov, CV.longdouble_inverse(JTJ), d)
    res, na_, nc_ = CV.residual(cov, JTJ, d)
    assert err <= bound and res <= bound * na_ * nc_, (name, err, res, bound)
    err0 = CV.scaled_error(cov, CV.longdouble_inverse(A0), CV.scale_of(A0))
    bound0 = (na * TOL_PASS + 10.0 * r_host * EPS) * kap
    assert err0 <= bound0, (name, err0, bound0)
    # scale=True: every entry times chi2() / dof -- the sweep's own sum, which is chi2() bit for bit -- with gfh_fit's dof
    chi2 = c.chi2(case.pars)
    n = int(case.pos[-1])
    dof = float(max(n - dim, 1)) if n != dim else 1.0
    cov1, sigma1, info1 = c.covariance(case.pars, case.active, case.is_global, scale=True)
    assert info1 == 0 and np.array_equal(_bits(cov1), _bits(cov * (chi2 / dof))) and np.array_equal(_bits(sigma1), _bits(np.sqrt(np.diag(cov1))))
    observe(**{'plain_cov_algebra_over_eps_kappa': err / (EPS * kap), 'plain_cov_oracle_over_bound': err0 / bound0, 'plain_cov_r_host': r_host})


def test_the_callers_order_gives_the_permuted_matrix():
    """[6, 1, 4] against [1, 4, 6]: the sums are the same bits in another place, the factorisation walks them in another order, so
    the two covariances are each other's permutation within twice the algebra's bound -- and so are the bands, each formed in its
    own order of the same terms"""
    ca, cb = PC.exp4(0), PC.exp4(1)
    a, b = PC.PERMUTED
    perm = [a.index(v) for v in b]
    ja, da = ctx_of(ca).jacobian_indices(a, ca.is_global)
    JA = ctx_of(ca).sweep(ca.pars, a, ja, da)[0]
    JB = ctx_of(cb).sweep(cb.pars, b, ja, da)[0]
    same(np.ascontiguousarray(JA[perm][:, perm]), JB)
    (CA, sa, _), (CB, sb, _) = cov_of(ca), cov_of(cb)
    kap = PC.oracle_pass(cb.name)[2]
    assert CV.scaled_error(CA[perm][:, perm], CB, CV.scale_of(JB)) <= 2 * 10.0 * PC.r_host() * EPS * kap
    assert not np.array_equal(sa, sb)          # (the order does reach the outputs)
    ba = ctx_of(ca).eval(ca.pars, a, ca.is_global, cov=CA)[2]
    bb = ctx_of(cb).eval(cb.pars, b, cb.is_global, cov=CB)[2]
    _, g0 = reference_points(cb)
    A = np.einsum('ia,ab,ib->i', np.abs(g0), np.abs(CB), np.abs(g0))
    assert np.all(np.abs(ba ** 2 - bb ** 2) <= 2 * (2 * TOL_PASS + 12 * EPS) * A + 2 * 2 * 10.0 * PC.r_host() * EPS * kap * A)


# ---- 2: the curves on the data's own points -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_model_residual_and_band_against_the_oracle(name):
    case = case_of(name)
    c = ctx_of(case)
    cov = cov_of(case)[0]
    f0, g0 = reference_points(case)
    res0 = case.oracle().sweep()[2]
    full = c.eval(case.pars, case.active, case.is_global, cov=cov, residuals=True)
    plain = c.eval(case.pars, case.active, case.is_global, residuals=True)
    assert plain[2] is None and full[3] > 0.0 and all(v.shape == (int(case.pos[-1]),) for v in full[:3])
    w_full = curves_check(case, full, f0, g0, cov, res0)
    w_plain = curves_check(case, plain, f0, g0, cov, res0)
    observe(**{'plain_eval_model_over_bound': max(w_full['model'], w_plain['model']), 'plain_eval_residual_over_bound': max(w_full['residual'], w_plain['residual']),
               'plain_eval_band_over_bound': w_full['band']})


def test_every_subset_of_null_outputs():
    """the outputs of a call do not depend on which others are asked for, with a band (gfh_point_grad) and without one (gfh_point_value)"""
    case = PC.exp2(257)
    c = ctx_of(case)
    cov = cov_of(case)[0]
    args = (case.pars, case.active, case.is_global)
    full = c.eval(*args, cov=cov, residuals=True)
    plain = c.eval(*args, residuals=True)
    for m, r, b in itertools.product((False, True), repeat=3):
        if not (m or r or b):
            continue
        got = c.eval(*args, cov=cov if b else None, residuals=r, model=m)
        want = full if b else plain
        for j, asked in enumerate((m, r, b)):
            if asked:
                same(got[j], want[j])
            else:
                assert got[j] is None


def test_bits_of_the_residual_and_a_nan_covariance():
    for case in (PC.exp2(1000), PC.global7()):
        c = ctx_of(case)
        args = (case.pars, case.active, case.is_global)
        r = c.eval(*args, residuals=True, model=False)[1]
        c.chi2(case.pars)
        same(r, c.residuals())          # without a band: chi2()'s residual vector, bit for bit
        dim = cov_of(case)[0].shape[0]
        m, r2, b, _ = c.eval(*args, cov=np.full((dim, dim), np.nan), residuals=True)
        assert np.all(np.isnan(b)) and np.all(np.isfinite(m)) and np.all(np.isfinite(r2))


def test_an_unseen_path_is_recorded_and_the_pass_repeated():
    """the branching model recorded at its first abscissa alone: the points behind the break leave the recorded tree, the handler
    records their path and the call returns what the fully recorded model returns"""
    case = PC.piecewise2()
    want = ctx_of(case).eval(case.pars, case.active, case.is_global, cov=cov_of(case)[0], residuals=True)
    V = T.Variants(B.model_piecewise2, 4)
    V.explore([case.xs[0][0]], B.PIECEWISE2_TRUTH)
    assert len(V) == 1
    c = _lib.Context(0)
    try:
        c.set_model(V)
        c.set_data(case.x(), case.y(), case.w(), case.pos)
        got = c.eval(case.pars, case.active, case.is_global, cov=cov_of(case)[0], residuals=True)
        assert c.n_variants() == 2 and c.unseen_log
        for u, v in zip(got[:3], want[:3]):
            same(u, v)
    finally:
        c.close()


# ---- 3: a caller's grid ----------------------------------------------------------------------------------------------------------------
def test_a_callers_grid_of_a_global_fit_against_the_oracle():
    case = PC.global7()
    c = ctx_of(case)
    cov = cov_of(case)[0]
    worst = dict(model=0.0, band=0.0)
    for n in PC.GRIDS:
        xe = np.linspace(0.0, 75.0, n) if n > 1 else np.array([0.25])
        m, r, b, sec = c.eval(case.pars, case.active, case.is_global, cov=cov, x_eval=xe)
        m0 = c.eval(case.pars, case.active, case.is_global, x_eval=xe)[0]
        assert r is None and m.shape == b.shape == m0.shape == (3, n) and sec > 0.0
        f0, g0 = reference_points(case, xe)
        for d, Cd in enumerate(blocks(case, cov)):
            s = slice(d * n, (d + 1) * n)
            for out in (m, m0):
                e = np.abs(out[d] - f0[s]) / np.abs(f0[s])
                assert np.all(e <= TOL_PASS), (n, d, e.max())
                worst['model'] = max(worst['model'], float(e.max() / TOL_PASS))
            worst['band'] = max(worst['band'], band_check(b[d], g0[s], Cd))
    observe(plain_eval_grid_model_over_bound=worst['model'], plain_eval_grid_band_over_bound=worst['band'])


def test_a_grid_equal_to_the_datas_abscissas_returns_the_data_modes_bits():
    case = PC.exp2(513)
    c = ctx_of(case)
    cov = cov_of(case)[0]
    args = (case.pars, case.active, case.is_global)
    m, _, b, _ = c.eval(*args, cov=cov)
    mg, _, bg, _ = c.eval(*args, cov=cov, x_eval=case.xs[0])
    same(mg[0], m); same(bg[0], b)
    same(c.eval(*args, x_eval=case.xs[0])[0][0], c.eval(*args)[0])


# ---- 4: the robust loss and finite differences ---------------------------------------------------------------------------------------
def test_under_a_robust_loss():
    """cov against the inverse of the oracle's loss-scaled J^T J (the reference's getInvJTJ under a loss); the residual is chi2()'s
    plain one; scale=True takes chi2() from a chi2 pass in front of the sweep and leaves the sweep's residual vector on the device"""
    case = PC.exp2(257)
    A0 = case.oracle(loss=1).sweep()[0]
    kap = CV.kappa(A0)
    assert kap <= PC.KAPPA_MAX
    c = case.context()
    try:
        c.set_loss(1)
        args = (case.pars, case.active, case.is_global)
        cov, sigma, info = c.covariance(*args)
        assert info == 0
        bound0 = (4 * TOL_PASS + 10.0 * PC.r_host() * EPS) * kap
        assert CV.scaled_error(cov, CV.longdouble_inverse(A0), CV.scale_of(A0)) <= bound0
        swept = c.residuals()                         # the scaled residuals the sweep stores
        chi0, res_plain = case.oracle().chi2()
        cov1 = c.covariance(*args, scale=True)[0]
        same(c.residuals(), swept)
        chi2 = c.chi2(case.pars)
        assert abs(chi2 - chi0) <= TOL_PASS * chi0
        same(cov1, cov * (chi2 / float(257 - 4)))
        f0, g0 = reference_points(case)
        got = c.eval(*args, cov=cov, residuals=True)
        curves_check(case, got, f0, g0, cov, res_plain)
        r = c.eval(*args, residuals=True, model=False)[1]
        c.chi2(case.pars)
        same(r, c.residuals())
        assert not np.array_equal(r, swept)
    finally:
        c.close()


def test_under_finite_differences():
    case = PC.exp2(257)
    x, w, p = case.xs[0], case.ws[0], case.pars[0]
    c = case.context()
    try:
        c.set_use_ad(False)
        args = (case.pars, case.active, case.is_global)
        jac, dim = c.jacobian_indices(case.active, case.is_global)
        JTJ = c.sweep(case.pars, case.active, jac, dim)[0]
        cov, sigma, info = c.covariance(*args)
        assert info == 0
        kap = CV.kappa(JTJ)
        assert kap <= PC.KAPPA_MAX
        assert CV.scaled_error(cov, CV.longdouble_inverse(JTJ), CV.scale_of(JTJ)) <= 10.0 * PC.r_host() * EPS * kap
        m, r, b, _ = c.eval(*args, cov=cov, residuals=True)
        f0 = M.exp2_numpy(p.astype(LD), x.astype(LD))
        assert np.all(np.abs(m - f0) <= TOL_PASS * np.abs(f0))
        res0 = case.oracle().chi2()[1]
        assert np.all(np.abs(r - res0) <= TOL_PASS * (np.abs(case.y()) + np.abs(f0)) * w)
        # the longdouble forward difference of the closed form, divided by the double step (fitfunction.F90:164-169)
        step = GO.fd_steps(p)
        g0 = np.empty((x.size, 4), dtype=LD)
        for j in range(4):
            q = p.copy(); q[j] = p[j] + GO.FD_STEP * p[j]
            g0[:, j] = (M.exp2_numpy(q.astype(LD), x.astype(LD)) - f0) / LD(step[j])
        S = np.abs(p[0]) * np.exp(-x / p[1]) + np.abs(p[2]) * np.exp(-x / p[3])
        D = GO.FD_DEVICE_FACTOR * GO.FD_C_REF * EPS * S[:, None] / np.abs(step)[None, :]
        aC = np.abs(cov)
        extra = 2 * np.einsum('ia,ab,ib->i', D, aC, np.abs(g0).astype(np.float64)) + np.einsum('ia,ab,ib->i', D, aC, D)
        observe(plain_eval_fd_band_over_bound=band_check(b, g0, cov, extra=extra))
    finally:
        c.close()


# ---- 5: state ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', (1, 2))
def test_fit_covariance_eval_fit_on_one_context_returns_the_bits_of_fresh_contexts(mode):
    case = PC.global7()
    start = case.pars * np.where(np.arange(7) % 2 == 0, 1.05, 0.95)
    kw = dict(lambda_=1.0, max_iter=6, chi2_rel=1e-8)
    args = (case.active, case.is_global)

    def fresh(call):
        c = case.context()
        try:
            c.set_keep_jacobian(mode)
            return call(c)
        finally:
            c.close()

    def fit(c):
        p, r = c.fit(start, *args, **kw)
        return p, (r.iterations, r.exit_reason, r.n_sweeps, r.n_chi2), np.array([r.lambda_, r.chi2])
    p0 = fresh(fit)[0]
    calls = (fit, lambda c: c.covariance(p0, *args, scale=True), lambda c: c.eval(p0, *args, cov=fresh_cov, residuals=True)[:3], fit)
    fresh_cov = fresh(lambda c: c.covariance(p0, *args))[0]
    want = [fresh(call) for call in calls]
    c = case.context()
    try:
        c.set_keep_jacobian(mode)
        before = c.device_memory()['workspace_pool']
        got = [call(c) for call in calls]
        # the two blocks of the call -- three datasets' 7 x 7 blocks down, three padded outputs back -- are counted
        assert c.device_memory()['workspace_pool'] - before == 8 * 3 * 7 * 7 + 3 * 8 * c.debug_layout()['n_slots']
        # fit_errors is fit, then covariance at the fitted parameters
        p, r, (cov, sigma, info) = c.fit_errors(start, *args, scale=True, **kw)
        same(p, got[0][0]); same(cov, got[1][0]); same(sigma, got[1][1])
        assert info == 0 and r.iterations == got[0][1][0]
    finally:
        c.close()
    for k in (0, 3):
        same(got[k][0], want[k][0]); same(got[k][2], want[k][2])
        assert got[k][1] == want[k][1]
    same(got[0][0], got[3][0])
    for u, v in zip(got[1][:2], want[1][:2]):
        same(u, v)
    for u, v in zip(got[2], want[2]):
        same(u, v)


# ---- 6: end to end -----------------------------------------------------------------------------------------------------------------------
def test_gadf_fit_then_gadf_errors_and_gadf_curves():
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp

    class global7(gf.fitfunc):
        def init(self):
            self.allocate(7)

        def eval(self, x):
            A, Bq, Cc, bgr, t1, t2, t3 = self.pars
            return A * exp(-(x / t1)) + Bq * exp(-(x / t2)) + Cc * x * exp(-(x / t3)) + bgr

    case = PC.global7()
    gf.gadf_close()
    gf.gadf_init(global7(), 3)
    try:
        for d in range(3):
            gf.gadf_add_dataset(case.xs[d], case.ys[d], 1.0 / case.ws[d])
            for j in range(4):
                gf.gadf_set(d + 1, j + 1, float(case.pars[d, j] * 1.03), True)
        for j in range(4, 7):
            gf.gadf_set(j + 1, float(case.pars[0, j] * 0.97), True)
        gf.gadf_set_errors(gf.USER)
        gf.gadf_fit(lambda_=1.0, max_iter=20, chi2_rel=1e-8)
        e = gf.gadf_errors(scaled=True)
        assert e['info'] == 0 and e['cov'].shape == (15, 15) and np.all(e['sigma'] > 0.0)
        assert e['columns'][:7] == [(1, 1), (1, 2), (1, 3), (1, 4), (0, 5), (0, 6), (0, 7)] and e['columns'][7:11] == [(2, 1), (2, 2), (2, 3), (2, 4)]
        out = gf.gadf_curves(cov=e['cov'], residuals=True)
        pars = np.array([[q.val for q in g.pars] for g in gf.fitfuncs])
        for d in range(3):
            assert out['model'][d].shape == out['residual'][d].shape == out['band'][d].shape == case.xs[d].shape
            f0 = M.global7_numpy(pars[d].astype(LD), case.xs[d].astype(LD))
            assert np.all(np.abs(out['model'][d] - f0) <= TOL_PASS * np.abs(f0))
            assert np.all(np.abs(out['residual'][d] - (case.ys[d] - f0) * case.ws[d]) <= TOL_PASS * (np.abs(case.ys[d]) + np.abs(f0)) * case.ws[d])
            assert np.all(out['band'][d] > 0.0) and np.all(out['band'][d] < 0.1 * np.abs(f0))
        xe = np.linspace(0.0, 70.0, 9)
        g = gf.gadf_curves(cov=e['cov'], x=xe)
        assert len(g['model']) == 3 and g['model'][2].shape == g['band'][2].shape == (9,) and g['residual'] is None
        with pytest.raises(gf.GadfitError, match="a residual on a caller's grid has no meaning"):
            gf.gadf_curves(x=xe, residuals=True)
    finally:
        gf.gadf_close()
