"""The errors of a batch on the device (gfh_batch_covariance, gfh_fit_batch_errors; the kernel gfh_k_batch_cov) in the three lane
forms.  Inputs, reference, rule and yardstick: tests/batch_cov_cases.py (tests/test_cpu_batch_cov.py runs them without a GPU).
Every translation unit asked for is one the build has compiled for the batch forms' and the cube's modules.

Bounds, with r_host the host yardstick (the kernel's algebra in plain doubles against the longdouble inverse, <= 2.5 by reasoning),
eps = 2^-52 and kappa = kappa_2 of the ORACLE's J^T J scaled to unit diagonal:
 1. algebra, against the longdouble inverse of the device's OWN batch_pass matrix: err <= 10 r_host eps kappa on the kept fits (10 x
    for another order of operations than the host's: the project's 10 x convention); on every fit || C~ A~ - I || <= that times
    || A~ || || C~ ||; cov symmetric and sigma = sqrt(diag) bit for bit.
 2. end to end against the oracle's matrix on the kept fits: err <= (na TOL_PASS + 10 r_host eps) kappa -- the per-pass bound through
    the inverse.  scale=True: the same plus TOL_PASS against that reference times the oracle's chi2 / dof, and BIT FOR BIT cov(scale=False)
    times batch_pass's chi2 / dof (one IEEE division and one multiplication per entry, which numpy repeats).
The observed maxima go where the other batch modules' go (GADFIT_BATCH_OBSERVE), under cov_*."""
import numpy as np
import pytest

from gadfit_amd import _lib
from tests import batch_cases as BC
from tests import batch_cov_cases as CV
from tests import batch_cube_cases as CC
from tests.batch_common import SCENARIOS, TOL_PASS, context, observe, same_bits

pytestmark = pytest.mark.gpu

FORMS = (64, 16, 256)          # the one table of lane forms
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same_cov(a, b):
    """two results (cov, sigma, info) bit for bit (NaN included)"""
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))


class Part:
    """a part's batch on one context in one lane form, with pass and covariances per active list cached"""

    def __init__(self, part, lanes):
        self.part, self.lanes = part, lanes
        if part == 1:
            self.tape, _, self._starts, self.batch = CV.part1()
        else:
            self.tape, _, self.batch = BC.part2()
        self.ctx = context(self.tape, self.batch)
        self.got = {}

    def starts(self, active):
        return self._starts if self.part == 1 else CV.part2_starts(active)

    def at(self, active):
        key = tuple(active)
        if key not in self.got:
            st = self.starts(active)
            ps = self.ctx.batch_pass(st, active, lanes_per_fit=self.lanes)
            c0 = self.ctx.batch_covariance(st, active, scale=False, lanes_per_fit=self.lanes)
            assert self.ctx.batch_lanes_used() == self.lanes and self.ctx.batch_form_used() == 'ragged'
            c1 = self.ctx.batch_covariance(st, active, scale=True, lanes_per_fit=self.lanes)
            self.got[key] = (ps, c0, c1)
        return self.got[key]


def part(k, lanes):
    if (k, lanes) not in _CACHE:
        _CACHE[(k, lanes)] = Part(k, lanes)
    return _CACHE[(k, lanes)]


@pytest.fixture(scope='module', autouse=True)
def _contexts():
    yield
    for p in _CACHE.values():
        p.ctx.close()
    _CACHE.clear()


def _sets(k):
    return [list(a) for p, a in CV.all_sets() if p == k]


# ---- 1: the algebra, free of the pass's error ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_algebra_against_the_inverse_of_the_devices_own_pass(lanes):
    r_host = CV.r_host()
    worst = dict(err=0.0, res=0.0)
    for k in (1, 2):
        P = part(k, lanes)
        for active in _sets(k):
            (JTJ, _, _), (cov, sigma, info), _ = P.at(active)
            keep = CV.kept(k, active)
            kap = [m[2] for m in CV.oracle_matrices(k, tuple(active))]
            assert np.all(info == 0), (k, active, np.nonzero(info)[0])
            assert np.array_equal(_bits(cov), _bits(np.ascontiguousarray(np.transpose(cov, (0, 2, 1)))))
            assert np.array_equal(_bits(sigma), _bits(np.sqrt(np.diagonal(cov, axis1=1, axis2=2))))
            for f in range(len(kap)):
                d = CV.scale_of(JTJ[f])
                bound = 10.0 * r_host * CV.EPS * kap[f]
                res, na_, nc_ = CV.residual(cov[f], JTJ[f], d)
                assert res <= bound * na_ * nc_, (k, active, f, res, bound * na_ * nc_)
                worst['res'] = max(worst['res'], res / (CV.EPS * kap[f] * na_ * nc_))
                if keep[f]:
                    err = CV.scaled_error(cov[f], CV.longdouble_inverse(JTJ[f]), d)
                    assert err <= bound, (k, active, f, err, bound)
                    worst['err'] = max(worst['err'], err / (CV.EPS * kap[f]))
    observe(**{'cov_%d_algebra_over_eps_kappa' % lanes: worst['err'], 'cov_%d_residual_over_eps_kappa_norms' % lanes: worst['res'],
               'cov_r_host': r_host})


# ---- 2: end to end against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_end_to_end_against_the_oracle(lanes):
    r_host = CV.r_host()
    worst = dict(unscaled=0.0, scaled=0.0)
    for k in (1, 2):
        P = part(k, lanes)
        for active in _sets(k):
            (_, _, chi2), (cov, sigma, info), (cov1, sigma1, info1) = P.at(active)
            na = len(active)
            dof = np.maximum(P.batch.n - na, 1).astype(np.float64)
            dof[P.batch.n - na == 0] = 1.0                                      # n = na: dof 0 is taken as 1
            # scale=True is scale=False times the pass's chi2 / dof, bit for bit, on EVERY fit (n = na and the dropped ones included)
            assert np.array_equal(_bits(cov1), _bits(cov * (chi2 / dof)[:, None, None]))
            assert np.array_equal(_bits(sigma1), _bits(np.sqrt(np.diagonal(cov1, axis1=1, axis2=2)))) and np.array_equal(info1, info)
            keep = CV.kept(k, active)
            for f, (A, chi0, kap) in enumerate(CV.oracle_matrices(k, tuple(active))):
                if not keep[f]:
                    continue
                d = CV.scale_of(A)
                ref = CV.longdouble_inverse(A)
                bound = (na * TOL_PASS + 10.0 * r_host * CV.EPS) * kap
                err = CV.scaled_error(cov[f], ref, d)
                assert err <= bound, (k, active, f, err, bound)
                err1 = CV.scaled_error(cov1[f], ref * np.longdouble(chi0 / dof[f]), d)
                assert err1 <= bound + TOL_PASS, (k, active, f, err1, bound + TOL_PASS)
                worst['unscaled'] = max(worst['unscaled'], err / bound); worst['scaled'] = max(worst['scaled'], err1 / (bound + TOL_PASS))
    observe(**{'cov_%d_oracle_over_bound' % lanes: worst['unscaled'], 'cov_%d_oracle_scaled_over_bound' % lanes: worst['scaled']})


# ---- 3: shapes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_the_callers_order_gives_the_permuted_matrix(lanes):
    """[6, 1, 4] against [1, 4, 6]: the sums are the same bits in another place (G[a] G[b] commutes), the factorisation walks them in
    another order, so the two covariances are each other's permutation within twice the algebra's bound"""
    P = part(2, lanes)
    a, b = CV.PERMUTED
    (JA, _, _), (ca, sa, _), _ = P.at(a)
    (JB, _, _), (cb, sb, _), _ = P.at(b)
    perm = [a.index(v) for v in b]
    assert np.array_equal(_bits(JA[:, perm][:, :, perm]), _bits(JB))
    r_host = CV.r_host()
    for f, (A, _, kap) in enumerate(CV.oracle_matrices(2, tuple(b))):
        err = CV.scaled_error(ca[f][perm][:, perm], cb[f], CV.scale_of(JB[f]))
        assert err <= 2 * 10.0 * r_host * CV.EPS * kap, (f, err)
    assert not np.array_equal(sa, sb)          # (the order does reach the outputs)


@pytest.mark.parametrize('lanes', FORMS)
def test_a_fit_does_not_depend_on_its_batch(lanes):
    """the batch cut to its first 7, 5, 3, 2 and 1 fits, every fit alone, and the batch reversed: every fit's bits are those it has in
    the whole batch (short spectra beside long ones, rows, waves and workgroups left without a fit)"""
    P = part(1, lanes)
    full = {s: P.at(CV.ACTIVE)[1 + s] for s in (0, 1)}
    st = P.starts(CV.ACTIVE)
    total = len(P.batch.n)
    c = context(P.tape)
    try:
        def same(idx, scales=(0, 1)):
            sub = BC.Batch([P.batch.items[k] for k in idx])
            c.set_batch_data(sub.off, sub.x, sub.y, sub.w)
            for s in scales:
                got = c.batch_covariance(st[idx], CV.ACTIVE, scale=bool(s), lanes_per_fit=lanes)
                assert c.batch_lanes_used() == lanes
                same_cov(got, [v[idx] for v in full[s]])
        for k in CV.CUTS:
            same(list(range(k)))
        for k in range(total):
            same([k], scales=(k % 2,))
        same(list(range(total - 1, -1, -1)))
    finally:
        c.close()


def test_the_workgroup_form_returns_the_wave_forms_bits_up_to_64_points():
    """waves 1 ... 3 add exact zeros (tests/batch_form_suite.py, same_bits_as_the_wave_form): the same sums, then the same algebra"""
    wave, wg = part(1, 64), part(1, 256)
    short = wave.batch.n <= 64
    assert set(wave.batch.n[short]) == {4, 5, 6, 8, 16, 17, 63, 64}
    for active in (CV.ACTIVE, CV.ONE_ACTIVE):
        for s in (1, 2):
            same_cov([v[short] for v in wg.at(active)[s]], [v[short] for v in wave.at(active)[s]])
    assert not np.array_equal(wg.at(CV.ACTIVE)[1][0][~short], wave.at(CV.ACTIVE)[1][0][~short])          # (beyond that the sums differ)


# ---- 4: a singular fit ends alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_a_singular_fit_and_a_nan_fit_end_alone(lanes):
    """[good, singular, good, NaN, good]: the singular spectrum (every abscissa 0: an exact zero pivot, tests/batch_cov_cases.py) gets
    info 2, the NaN one info 1, both NaN throughout under both scalings; the good ones return their bits"""
    P = part(1, lanes)
    g = list(CV.SINGULAR_NEIGHBOURS)
    items = [P.batch.items[g[0]], CV.singular_item(), P.batch.items[g[1]], CV.nan_item(), P.batch.items[g[2]]]
    st = P.starts(CV.ACTIVE)
    starts = st[[g[0], 0, g[1], 0, g[2]]]
    sub = BC.Batch(items)
    c = context(P.tape, sub)
    try:
        for s in (0, 1):
            cov, sigma, info = c.batch_covariance(starts, CV.ACTIVE, scale=bool(s), lanes_per_fit=lanes)
            assert c.batch_lanes_used() == lanes
            assert info.tolist() == [0, 2, 0, 1, 0]
            assert np.all(np.isnan(cov[[1, 3]])) and np.all(np.isnan(sigma[[1, 3]]))
            same_cov([v[[0, 2, 4]] for v in (cov, sigma, info)], [v[g] for v in P.at(CV.ACTIVE)[1 + s]])
    finally:
        c.close()


# ---- 5: data forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_cubes_and_frames_return_the_ragged_forms_bits(lanes):
    """a uint16 cube under SQRT_Y, a float32 cube under USER and that cube put as frames in two pieces, against the ragged call on the
    doubles they stand for with the weights gfh_init_weights establishes"""
    n, nf = 65, 7
    x = CC.grid(n)
    pick = CC.pick(nf)
    starts = CC.starts(n, 0.05)[pick]
    tape = CC.tape()
    plain = context(tape)
    c = context(tape)
    try:
        for dtype, et in ((np.uint16, CC.SQRT_Y), (np.float32, CC.USER)):
            Y = np.ascontiguousarray(CC.cube(n, dtype)[pick])
            w = np.ascontiguousarray(CC.user_weights(n)[pick]) if et == CC.USER else None
            W = CC.established_weights(plain, x, Y, et, w)
            c.set_batch_data(np.arange(nf + 1, dtype=np.int64) * n, np.tile(x, nf), Y.astype(np.float64).ravel(), W.ravel())
            want = {s: c.batch_covariance(starts, CC.ACTIVE, scale=bool(s), lanes_per_fit=lanes) for s in (0, 1)}
            assert c.batch_form_used() == 'ragged' and np.all(want[0][2] == 0)
            routes = [lambda: c.set_batch_cube(x, Y, et, w)]
            if et == CC.USER:
                def frames():
                    F, Fw = np.ascontiguousarray(Y.T), np.ascontiguousarray(w.T)
                    c.batch_frames_begin(x, nf, dtype, et)
                    c.batch_frames_put(30, F[30:], Fw[30:])
                    c.batch_frames_put(0, F[:30], Fw[:30])
                routes.append(frames)
            for put in routes:
                put()
                for s in (0, 1):
                    same_cov(c.batch_covariance(starts, CC.ACTIVE, scale=bool(s), lanes_per_fit=lanes), want[s])
                    assert c.batch_form_used() == CC.form_of(dtype, et) and c.batch_lanes_used() == lanes
    finally:
        c.close(); plain.close()


# ---- 6: fit_batch_errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_fit_batch_errors_is_fit_batch_then_batch_covariance(lanes):
    P = part(1, lanes)
    off, kw = SCENARIOS['a']
    _, order, _, _ = CV.part1()
    from tests.batch_common import start_of
    starts = np.array([start_of(BC.spectrum_n(n, s)[0], off) for n, s in order])
    p0, r0, _ = P.ctx.fit_batch(starts, CV.ACTIVE, lanes_per_fit=lanes, **kw)
    for s in (False, True):
        p, r, errs, sec = P.ctx.fit_batch_errors(starts, CV.ACTIVE, scale=s, lanes_per_fit=lanes, **kw)
        assert P.ctx.batch_lanes_used() == lanes and sec > 0.0
        same_bits(p, r, p0, r0)
        same_cov(errs, P.ctx.batch_covariance(p, CV.ACTIVE, scale=s, lanes_per_fit=lanes))
    # at the fitted parameters scale=True is chi2 / dof of the fit's own record, bit for bit (the sweep at the exit parameters is
    # the last chi2() of an accepted step only up to the order of its sums, so the pass's chi2 is used, as above)
    chi2 = P.ctx.batch_pass(p0, CV.ACTIVE, lanes_per_fit=lanes)[2]
    unscaled = P.ctx.batch_covariance(p0, CV.ACTIVE, lanes_per_fit=lanes)[0]
    assert np.array_equal(_bits(errs[0]), _bits(unscaled * (chi2 / r0['dof'])[:, None, None]))


def test_gadf_fit_cube_with_errors():
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    n, nf = 65, 5
    x, Y, starts = CC.grid(n), np.ascontiguousarray(CC.cube(n, np.uint16)[CC.pick(nf)]), CC.starts(n, 0.05)[CC.pick(nf)]
    off, kw = SCENARIOS['a']
    gf.gadf_close()
    gf.gadf_init(exp2())
    try:
        for k in range(4):
            gf.gadf_set(k + 1, float(starts[0][k]), True)
        gf.gadf_set_errors(gf.SQRT_Y)
        plain = gf.gadf_fit_cube(x, Y, starts, **kw)
        assert len(plain) == 2
        for name, s in (('scaled', True), ('unscaled', False)):
            p, r, e = gf.gadf_fit_cube(x, Y, starts, errors=name, **kw)
            same_bits(p, r, *plain)
            assert sorted(e) == ['cov', 'info', 'sigma'] and np.all(e['info'] == 0) and np.all(e['sigma'] > 0.0)
            same_cov((e['cov'], e['sigma'], e['info']), gf._S.ctx.batch_covariance(p, CV.ACTIVE, scale=s))
        pf, rf, ef = gf.gadf_fit_frames(x, np.ascontiguousarray(Y.T), starts, errors='unscaled', **kw)
        same_bits(pf, rf, *plain)
        same_cov((ef['cov'], ef['sigma'], ef['info']), (e['cov'], e['sigma'], e['info']))
    finally:
        gf.gadf_close()


def test_one_context_through_every_call():
    """batch_pass -> fit_batch_errors -> batch_covariance -> a plain fit on one context: the bits of fresh contexts"""
    from tests.batch_form_suite import plain_fit, same_plain_fit
    tape, _, st, batch = CV.part1()
    idx = list(range(9))
    sub = BC.Batch([batch.items[k] for k in idx])
    off, kw = SCENARIOS['a']
    starts = st[idx] * np.where(np.arange(4) % 2 == 0, 1.0 + off, 1.0 - off)

    def fresh(call):
        c = context(tape, sub)
        try:
            return call(c)
        finally:
            c.close()
    calls = (lambda c: c.batch_pass(st[idx], CV.ACTIVE), lambda c: c.fit_batch_errors(starts, CV.ACTIVE, scale=True, **kw)[:3],
             lambda c: c.batch_covariance(st[idx], CV.ACTIVE), lambda c: plain_fit(c, batch.items[7], starts[7], kw))
    want = [fresh(call) for call in calls]
    c = context(tape, sub)
    try:
        got = [call(c) for call in calls]
    finally:
        c.close()
    for u, v in zip(got[0], want[0]):
        assert np.array_equal(_bits(u), _bits(v))
    same_bits(got[1][0], got[1][1], want[1][0], want[1][1]); same_cov(got[1][2], want[1][2])
    same_cov(got[2], want[2])
    same_plain_fit(got[3], want[3])
