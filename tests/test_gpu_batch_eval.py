"""The curves of a batch on the device (gfh_batch_eval, Context.batch_eval, gadf_batch_curves; the kernel gfh_k_batch_eval) in the
three lane forms and on every data form.  tests/test_cpu_batch_eval.py holds the source, the refusals and the record without a GPU.

The batches: 19 ragged spectra of model_exp2 (the first 19 of tests/batch_cov_cases.part1: every length of LENGTHS, 4 ... 257 and
1000, so every row edge of the 16-, 64- and 256-lane walks is met; 19 is no multiple of 4 or 16) and the first 19 spectra of
model_exp4 (tests/batch_cases.part2) under all eight parameters and under the two orders of PERMUTED, with five passive ones.  The
parameters are the spectra's truths, cov is the device's own batch_covariance (unscaled).

Bounds (TOL_PASS = 2e-13 is the project's asserted per-pass bound and covers the value and each entry of the gradient; eps = 2^-52):
    |model - f0| <= TOL_PASS |f0|                     f0, g0: oracle.binding.eval_reverse at every point
    |residual - res0| <= TOL_PASS (|y| + |f0|) w      res0: OracleProblem.sweep
    |band^2 - s2_ref| <= (2 TOL_PASS + (na^2 + na) eps) A,   s2_ref = g0^T C g0,  A = sum_ab |g0_a| |C_ab| |g0_b|
both in numpy.longdouble with the device's own C: 2 TOL_PASS for the two factors g, the rest the rounding of the stated summation
order (na^2 products and additions of t, na + na of s2, the root).  The models are sums of positive terms, so f has no cancellation
and a relative bound on it is meaningful; the oracle's f0 is itself held to the closed form in longdouble within TOL_PASS / 10, so the
bounds test the device, not the inputs.
Against the device's own Gram (cov unscaled): sum_i w_i^2 band_i^2 = sum_ab C_ab JTJ_ab of batch_pass within
(n + 2 na^2 + 8) eps sum_ab |C_ab| sqrt(JTJ_aa JTJ_bb) -- Cauchy-Schwarz on sum_i w_i^2 |g_ia| |g_ib| and the number of additions on
either side -- and sum residual^2 in longdouble = batch_pass's chi2 within n eps chi2.
The observed maxima go where the other batch modules' go (GADFIT_BATCH_OBSERVE), under eval_*."""
import functools

import numpy as np
import pytest

from gadfit_amd import _lib
from oracle import binding as orc
from tests import batch_cases as BC
from tests import batch_cov_cases as CV
from tests import batch_cube_cases as CC
from tests import models as M
from tests.batch_common import SCENARIOS, TOL_PASS, context, observe

pytestmark = pytest.mark.gpu

FORMS = (64, 16, 256)
N_FITS = 19
EPS = CV.EPS
LD = np.longdouble
EXP4_SETS = (list(range(8)),) + tuple(CV.PERMUTED)
GRIDS = (1, 15, 17, 65, 257)
RANGES = ((0, 1), (7, 12))          # [0, 1) and [7, 19); the whole batch is the third
_CTX = {}
_GOT = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- the batches and their oracle ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def part(k):
    """(tape, Batch of 19, pars [19][n_pars], closed form)"""
    if k == 1:
        tape, _, starts, batch = CV.part1()
        return tape, BC.Batch(batch.items[:N_FITS]), starts[:N_FITS].copy(), M.exp2_numpy
    tape, truths, batch = BC.part2()
    return tape, BC.Batch(batch.items[:N_FITS]), truths[:N_FITS].copy(), M.exp4_numpy


@functools.lru_cache(maxsize=None)
def oracle_points(k, grid=None):
    """per fit (f0 [n], g0 [n][n_pars]) of the oracle at the fit's own abscissas or on `grid` (a tuple), every parameter active: the
    derivative by a parameter does not depend on which others are active.  f0 is held to the closed form here, on the CPU"""
    tape, batch, pars, closed = part(k)
    mask = [1] * tape.n_pars
    out = []
    for f, item in enumerate(batch.items):
        xs = item[0] if grid is None else np.array(grid)
        f0 = np.empty(xs.size); g0 = np.empty((xs.size, tape.n_pars))
        for i, xv in enumerate(xs):
            f0[i], g0[i] = orc.eval_reverse(tape, float(xv), pars[f], mask)
        ref = closed(pars[f].astype(LD), xs.astype(LD))
        assert np.all(np.abs(f0 - ref) <= (TOL_PASS / 10) * np.abs(ref)), (k, f)
        out.append((f0, g0))
    return out


@functools.lru_cache(maxsize=None)
def oracle_residuals(k, active):
    tape, batch, pars, _ = part(k)
    return [orc.OracleProblem(tape, [x], [y], [w], [pars[f]], list(active), [0] * tape.n_pars).sweep()[2] for f, (x, y, w) in enumerate(batch.items)]


def ctx(k):
    if k not in _CTX:
        tape, batch, _, _ = part(k)
        _CTX[k] = context(tape, batch)
    return _CTX[k]


def got(k, active, lanes):
    """the device's outputs for a part under an active list in a lane form, once: the pass, the call with a band and the one without;
    and cov, which is the 64-lane form's in every form (the lane forms sum J^T J in different orders, and the same C goes into each)"""
    key = (k, tuple(active), lanes)
    if key not in _GOT:
        c, pars = ctx(k), part(k)[2]
        cov, _, info = c.batch_covariance(pars, active, scale=False, lanes_per_fit=64)
        assert np.all(info == 0)
        ps = c.batch_pass(pars, active, lanes_per_fit=lanes)
        full = c.batch_eval(pars, active, cov=cov, residuals=True, lanes_per_fit=lanes)
        assert c.batch_lanes_used() == lanes and c.batch_form_used() == 'ragged' and full[4] > 0.0
        plain = c.batch_eval(pars, active, residuals=True, lanes_per_fit=lanes)
        assert plain[2] is None and np.array_equal(full[3], part(k)[1].off) and np.array_equal(plain[3], full[3])
        _GOT[key] = dict(cov=cov, ps=ps, full=full, plain=plain)
    return _GOT[key]


@pytest.fixture(scope='module', autouse=True)
def _contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear(); _GOT.clear()


def _cases():
    return [(1, CV.ACTIVE)] + [(2, a) for a in EXP4_SETS]


def band_check(band, g, Cf, na):
    """the band of one fit against s2_ref = g^T C g in longdouble; returns the worst |band^2 - s2_ref| / bound"""
    gl, Cl = g.astype(LD), Cf.astype(LD)
    s2 = np.einsum('ia,ab,ib->i', gl, Cl, gl)
    A = np.einsum('ia,ab,ib->i', np.abs(gl), np.abs(Cl), np.abs(gl))
    bound = (2 * TOL_PASS + (na * na + na) * EPS) * A
    err = np.abs(band.astype(LD) ** 2 - s2)
    print('band: max |band^2 - s2_ref| / bound = %.3e' % float(np.max(err / bound)))
    assert np.all(err <= bound)
    return float(np.max(err / bound))


# ---- 1: against the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_model_residual_and_band_against_the_oracle(lanes):
    worst = dict(model=0.0, model_plain=0.0, residual=0.0, band=0.0)
    for k, active in _cases():
        _, batch, _, _ = part(k)
        g = got(k, active, lanes)
        pts, res0 = oracle_points(k), oracle_residuals(k, tuple(active))
        na = len(active)
        for f, (x, y, w) in enumerate(batch.items):
            s = slice(batch.off[f], batch.off[f + 1])
            f0, g0 = pts[f]
            for name, out in (('model', g['full']), ('model_plain', g['plain'])):          # with a band (gfh_point_grad) and without
                e = np.abs(out[0][s] - f0) / np.abs(f0)
                worst[name] = max(worst[name], e.max())
                assert np.all(e <= TOL_PASS), (k, active, f, name, e.max())
                er = np.abs(out[1][s] - res0[f]) / ((np.abs(y) + np.abs(f0)) * w)
                worst['residual'] = max(worst['residual'], er.max())
                assert np.all(er <= TOL_PASS), (k, active, f, name, er.max())
            worst['band'] = max(worst['band'], band_check(g['full'][2][s], g0[:, active], g['cov'][f], na))
    print(worst)
    observe(**{'eval_%d_%s_over_bound' % (lanes, n): (v if n == 'band' else v / TOL_PASS) for n, v in worst.items()})


# ---- 2: against the device's own Gram ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_bands_and_residuals_against_the_devices_own_pass(lanes):
    worst = dict(gram=0.0, chi2=0.0)
    for k, active in _cases():
        _, batch, _, _ = part(k)
        g = got(k, active, lanes)
        JTJ, _, chi2 = g['ps']
        na = len(active)
        for f, (x, y, w) in enumerate(batch.items):
            s = slice(batch.off[f], batch.off[f + 1])
            n = x.size
            Cf = g['cov'][f].astype(LD)
            lhs = np.sum(w.astype(LD) ** 2 * g['full'][2][s].astype(LD) ** 2)
            rhs = np.sum(Cf * JTJ[f].astype(LD))
            d = np.sqrt(np.diag(JTJ[f]))
            tol = (n + 2 * na * na + 8) * EPS * np.sum(np.abs(Cf) * np.outer(d, d))
            assert abs(lhs - rhs) <= tol, (k, active, f, float(lhs), float(rhs), float(tol))
            worst['gram'] = max(worst['gram'], float(abs(lhs - rhs) / tol))
            for out in (g['full'], g['plain']):
                c2 = np.sum(out[1][s].astype(LD) ** 2)
                assert abs(c2 - chi2[f]) <= n * EPS * chi2[f], (k, active, f, float(c2), chi2[f])
                worst['chi2'] = max(worst['chi2'], float(abs(c2 - chi2[f]) / (n * EPS * chi2[f])))
    # (a covariance indexed in another order than the caller's does not pass: [6, 1, 4] is held above beside [1, 4, 6])
    assert not np.array_equal(got(2, CV.PERMUTED[0], lanes)['cov'], got(2, CV.PERMUTED[1], lanes)['cov'])
    observe(**{'eval_%d_gram_over_bound' % lanes: worst['gram'], 'eval_%d_chi2_over_bound' % lanes: worst['chi2']})


# ---- 3: bits ---------------------------------------------------------------------------------------------------------------------------
def test_the_three_lane_forms_return_the_same_bits():
    """no reduction: every point is one lane's own, whichever lane"""
    for k, active in _cases():
        ref = got(k, active, FORMS[0])
        for lanes in FORMS[1:]:
            g = got(k, active, lanes)
            for which in ('full', 'plain'):
                for u, v in zip(g[which][:3], ref[which][:3]):
                    if u is not None:
                        same(u, v)


@pytest.mark.parametrize('lanes', FORMS)
def test_a_fit_does_not_depend_on_its_range(lanes):
    """as a range of one, inside [7, 19) and inside the whole batch: the same bits, with and without a band"""
    c, (_, batch, pars, _) = ctx(1), part(1)
    g = got(1, CV.ACTIVE, lanes)
    ranges = [(f, 1) for f in range(N_FITS)] + [RANGES[1], (3, 4)]
    for first, n in ranges:
        s = slice(batch.off[first], batch.off[first + n])
        for cov, want in ((g['cov'][first:first + n], g['full']), (None, g['plain'])):
            m, r, b, off, _ = c.batch_eval(pars[first:first + n], CV.ACTIVE, cov=cov, residuals=True, first_fit=first, n_fits=n, lanes_per_fit=lanes)
            assert c.batch_lanes_used() == lanes and np.array_equal(off, batch.off[first:first + n + 1] - batch.off[first])
            same(m, want[0][s]); same(r, want[1][s])
            if cov is not None:
                same(b, want[2][s])
    # n_fits None: to the end of the batch
    m = c.batch_eval(pars[7:], CV.ACTIVE, first_fit=7, lanes_per_fit=lanes)[0]
    same(m, g['plain'][0][batch.off[7]:])


@pytest.mark.parametrize('lanes', FORMS)
def test_cubes_frames_and_the_grid_return_the_ragged_forms_bits(lanes):
    """a float64 cube under USER, that cube put as frames in two pieces and a uint16 cube under SQRT_Y against the ragged call on the
    doubles they stand for with oracle.init_weights' weights; and the cube's own abscissas given as a grid against its own points"""
    n, nf = 65, 7
    x, pick = CC.grid(n), CC.pick(nf)
    pars = CC.starts(n, 0.0)[pick]
    c = context(CC.tape())
    try:
        for dtype, et in ((np.float64, CC.USER), (np.uint16, CC.SQRT_Y)):
            Y = np.ascontiguousarray(CC.cube(n, dtype)[pick])
            w = np.ascontiguousarray(CC.user_weights(n)[pick]) if et == CC.USER else None
            Yd = Y.astype(np.float64)
            W = w if et == CC.USER else orc.init_weights(et, Yd.ravel()).reshape(Yd.shape)
            c.set_batch_data(np.arange(nf + 1, dtype=np.int64) * n, np.tile(x, nf), Yd.ravel(), W.ravel())
            cov, _, info = c.batch_covariance(pars, CC.ACTIVE, lanes_per_fit=lanes)
            assert np.all(info == 0)
            want = c.batch_eval(pars, CC.ACTIVE, cov=cov, residuals=True, lanes_per_fit=lanes)
            want_plain = c.batch_eval(pars, CC.ACTIVE, residuals=True, lanes_per_fit=lanes)
            assert c.batch_form_used() == 'ragged' and want[0].shape == (nf * n,)
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
                m, r, b, off, _ = c.batch_eval(pars, CC.ACTIVE, cov=cov, residuals=True, lanes_per_fit=lanes)
                assert c.batch_form_used() == CC.form_of(dtype, et) and c.batch_lanes_used() == lanes
                assert m.shape == r.shape == b.shape == (nf, n) and np.array_equal(off, np.arange(nf + 1) * n)
                same(m.ravel(), want[0]); same(r.ravel(), want[1]); same(b.ravel(), want[2])
                m0, r0 = c.batch_eval(pars, CC.ACTIVE, residuals=True, lanes_per_fit=lanes)[:2]
                same(m0.ravel(), want_plain[0]); same(r0.ravel(), want_plain[1])
                # a range of the cube: rows [2, 5)
                ms, rs, bs = c.batch_eval(pars[2:5], CC.ACTIVE, cov=cov[2:5], residuals=True, first_fit=2, n_fits=3, lanes_per_fit=lanes)[:3]
                same(ms, m[2:5]); same(rs, r[2:5]); same(bs, b[2:5])
                # the data's own abscissas as a grid
                mg, rg, bg, _, _ = c.batch_eval(pars, CC.ACTIVE, cov=cov, x_eval=x, lanes_per_fit=lanes)
                assert rg is None
                same(mg, m); same(bg, b)
                same(c.batch_eval(pars, CC.ACTIVE, x_eval=x, lanes_per_fit=lanes)[0], m0)
    finally:
        c.close()


# ---- 4: nothing strays --------------------------------------------------------------------------------------------------------------
GUARD = 67
PATTERN = np.uint64(0x7ff8dead0000beef)          # a NaN no computation returns


def _guarded(n):
    buf = np.full(n + 2 * GUARD, PATTERN, dtype=np.uint64).view(np.float64)
    return buf, buf[GUARD:GUARD + n]


def _guards_untouched(buf, n):
    b = buf.view(np.uint64)
    assert np.all(b[:GUARD] == PATTERN) and np.all(b[GUARD + n:] == PATTERN)


@pytest.mark.parametrize('lanes', FORMS)
def test_nothing_is_written_outside_the_range(lanes):
    """through the C entry: guard bands of a NaN pattern before and after each output stay what they were for [0, 1), [7, 19) and the
    whole batch, on the fits' own points and on a grid; what lies between is what Context.batch_eval returns"""
    c, (_, batch, pars, _) = ctx(1), part(1)
    g = got(1, CV.ACTIVE, lanes)
    a = np.array(CV.ACTIVE, dtype=np.int32)
    grid = np.linspace(-3.0, 130.0, 17)
    c.set_batch_lanes(lanes)
    for first, n in RANGES + ((0, N_FITS),):
        p = np.ascontiguousarray(pars[first:first + n]); cov = np.ascontiguousarray(g['cov'][first:first + n])
        s = slice(batch.off[first], batch.off[first + n])
        for xe in (None, grid):
            tot = int(batch.off[first + n] - batch.off[first]) if xe is None else n * grid.size
            bufs = [_guarded(tot) for _ in range(3)]
            outs = [_lib.dp(v[1]) for v in bufs]
            if xe is not None:
                outs[1] = None
            c._chk(_lib.lib().gfh_batch_eval(c._h, _lib.dp(p), 4, _lib.ip(a), _lib.dp(cov), None if xe is None else _lib.dp(xe),
                                             0 if xe is None else xe.size, first, n, *outs, None))
            assert c.batch_lanes_used() == lanes
            for buf, _ in bufs:
                _guards_untouched(buf, tot)
            if xe is None:
                for j in range(3):
                    same(bufs[j][1], g['full'][j][s])
            else:
                assert np.all(bufs[1][1].view(np.uint64) == PATTERN)          # the residual that was not asked for
                want = c.batch_eval(p, CV.ACTIVE, cov=cov, x_eval=xe, first_fit=first, n_fits=n)
                same(bufs[0][1], want[0].ravel()); same(bufs[2][1], want[2].ravel())
                assert np.all(np.isfinite(bufs[0][1])) and np.all(np.isfinite(bufs[2][1]))
            # one output alone: the others' pointers are null and nothing else is written
            buf, view = _guarded(tot)
            only = [None, None, _lib.dp(view)]
            c._chk(_lib.lib().gfh_batch_eval(c._h, _lib.dp(p), 4, _lib.ip(a), _lib.dp(cov), None if xe is None else _lib.dp(xe),
                                             0 if xe is None else xe.size, first, n, *only, None))
            _guards_untouched(buf, tot)
            same(view, bufs[2][1])


@pytest.mark.parametrize('lanes', FORMS)
def test_a_fit_with_a_nan_covariance_gets_nan_bands_alone(lanes):
    """[good, singular, good, good]: the singular spectrum (every abscissa 0, tests/batch_cov_cases.py) has info 2 and a NaN
    covariance; its band is NaN throughout, its model and residuals are finite, and its neighbours keep the bits they have in the
    batch of 19"""
    tape, batch, pars, _ = part(1)
    nb = list(CV.SINGULAR_NEIGHBOURS)
    assert max(nb) < N_FITS
    sub = BC.Batch([batch.items[nb[0]], CV.singular_item(), batch.items[nb[1]], batch.items[nb[2]]])
    p = pars[[nb[0], 0, nb[1], nb[2]]]
    g = got(1, CV.ACTIVE, lanes)
    c = context(tape, sub)
    try:
        cov, _, info = c.batch_covariance(p, CV.ACTIVE, lanes_per_fit=64)          # (the form of got()'s cov)
        assert info.tolist() == [0, 2, 0, 0] and np.all(np.isnan(cov[1]))
        m, r, b, off, _ = c.batch_eval(p, CV.ACTIVE, cov=cov, residuals=True, lanes_per_fit=lanes)
        s1 = slice(off[1], off[2])
        assert np.all(np.isnan(b[s1])) and np.all(np.isfinite(m[s1])) and np.all(np.isfinite(r[s1]))
        for j, f in ((0, nb[0]), (2, nb[1]), (3, nb[2])):
            s, s0 = slice(off[j], off[j + 1]), slice(batch.off[f], batch.off[f + 1])
            same(m[s], g['full'][0][s0]); same(r[s], g['full'][1][s0]); same(b[s], g['full'][2][s0])
        assert not np.any(np.isnan(np.delete(b, np.arange(off[1], off[2]))))
    finally:
        c.close()


# ---- 5: a caller's grid -------------------------------------------------------------------------------------------------------------
def _grid(n):
    """n abscissas from below the data's range (0.5 ... 100) to beyond it"""
    return tuple(np.linspace(-3.0, 130.0, n)) if n > 1 else (0.25,)


@pytest.mark.parametrize('lanes', FORMS)
def test_a_callers_grid_against_the_oracle(lanes):
    c, (_, batch, pars, _) = ctx(1), part(1)
    g = got(1, CV.ACTIVE, lanes)
    worst = dict(model=0.0, band=0.0)
    for n in GRIDS:
        xe = np.array(_grid(n))
        m, r, b, off, _ = c.batch_eval(pars, CV.ACTIVE, cov=g['cov'], x_eval=xe, lanes_per_fit=lanes)
        m0 = c.batch_eval(pars, CV.ACTIVE, x_eval=xe, lanes_per_fit=lanes)[0]
        assert c.batch_lanes_used() == lanes and r is None and m.shape == b.shape == m0.shape == (N_FITS, n)
        assert np.array_equal(off, np.arange(N_FITS + 1) * n)
        for f, (f0, g0) in enumerate(oracle_points(1, _grid(n))):
            for out in (m, m0):
                e = np.abs(out[f] - f0) / np.abs(f0)
                worst['model'] = max(worst['model'], e.max())
                assert np.all(e <= TOL_PASS), (n, f, e.max())
            worst['band'] = max(worst['band'], band_check(b[f], g0[:, CV.ACTIVE], g['cov'][f], 4))
        # a range of the batch on the grid
        ms, _, bs, _, _ = c.batch_eval(pars[7:], CV.ACTIVE, cov=g['cov'][7:], x_eval=xe, first_fit=7, lanes_per_fit=lanes)
        same(ms, m[7:]); same(bs, b[7:])
    observe(**{'eval_%d_grid_model_over_bound' % lanes: worst['model'] / TOL_PASS, 'eval_%d_grid_band_over_bound' % lanes: worst['band']})


# ---- 6: end to end -----------------------------------------------------------------------------------------------------------------
def test_gadf_fit_cube_then_gadf_batch_curves():
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    tape = CC.tape()
    _, kw = SCENARIOS['a']
    gf.gadf_close()
    gf.gadf_init(exp2())
    try:
        gf.gadf_set_errors(gf.SQRT_Y)
        for n, nf in ((65, 5), (33, 3)):          # the second fit is of another shape: the curves follow the batch held
            x, Y, starts = CC.grid(n), np.ascontiguousarray(CC.cube(n, np.uint16)[CC.pick(nf)]), CC.starts(n, 0.05)[CC.pick(nf)]
            for j in range(4):
                gf.gadf_set(j + 1, float(starts[0][j]), True)
            pars, rec, e = gf.gadf_fit_cube(x, Y, starts, errors='scaled', **kw)
            assert np.all(e['info'] == 0)
            out = gf.gadf_batch_curves(pars, e['cov'], residuals=True)
            assert gf._S.ctx.batch_lanes_used() == 64 and gf._S.ctx.batch_form_used() == CC.form_of(np.uint16, CC.SQRT_Y)
            assert out['model'].shape == out['residual'].shape == out['band'].shape == (nf, n)
            assert np.array_equal(out['offsets'], np.arange(nf + 1) * n)
            Yd = Y.astype(np.float64)
            W = CC.reference_weights(Yd, CC.SQRT_Y)
            for f in range(nf):
                f0 = np.empty(n); g0 = np.empty((n, 4))
                for i, xv in enumerate(x):
                    f0[i], g0[i] = orc.eval_reverse(tape, float(xv), pars[f], [1] * 4)
                res0 = orc.OracleProblem(tape, [x], [Yd[f]], [W[f]], [pars[f]], CC.ACTIVE, [0] * 4).sweep()[2]
                assert np.all(np.abs(out['model'][f] - f0) <= TOL_PASS * np.abs(f0))
                assert np.all(np.abs(out['residual'][f] - res0) <= TOL_PASS * (np.abs(Yd[f]) + np.abs(f0)) * W[f])
                band_check(out['band'][f], g0, e['cov'][f], 4)
            # the last fits alone, on a grid, without residuals
            xe = np.linspace(0.0, 120.0, 9)
            tail = gf.gadf_batch_curves(pars[1:], e['cov'][1:], x=xe, first_fit=1)
            assert tail['model'].shape == tail['band'].shape == (nf - 1, 9) and tail['residual'] is None
            with pytest.raises(gf.GadfitError, match="a residual on a caller's grid has no meaning"):
                gf.gadf_batch_curves(pars, e['cov'], x=xe, residuals=True)
    finally:
        gf.gadf_close()
