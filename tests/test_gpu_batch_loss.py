"""Batched fits under a robust loss with a residual scale on the device (gfh_set_batch_loss; the loss units of the batch kernels).
Inputs, the reference for a scale c (the oracle at the weights w / c) and the selection rule: tests/batch_loss_cases.py;
tests/test_cpu_batch_loss.py runs the rule over the same cases without a GPU.  Every unit asked for is one the build has compiled.

1. batch_pass against the oracle's loss-scaled sweep() and its plain chi2(): J^T J and J^T r within parity_common.TOL_LOSS (the project's
   bound for loss-scaled passes), chi2 within TOL_PASS.
2. Fits against the oracle's: counts and dof equal, lambda within TOL_LAMBDA, parameters and chi2 within TOL_FIT = 1e-10.
3. Bit for bit on the device: (a) loss 0 with any scale is the linear fit; (b) c = 8 and c = 1/4 against c = 1 with the weights times 1 / c:
   the same parameters, counts and lambda, chi2 and every pass sum exactly c^2 times; (c) Huber at c = 2^10, where no |u| reaches 1, is
   the linear fit, omega pass included; (d) fit_batch_errors is fit_batch under the loss; (e) so is fit_batch_bounded under infinite bounds.
4. A parameter pinned throughout under Cauchy against the oracle's reduced fit with loss = 1.
5. batch_covariance against the longdouble inverse of the oracle's loss-scaled J^T J (times the plain chi2 / dof under scale=True), and
   against Context.covariance of the plain path under set_loss.
6. A uint16 cube under SQRT_Y with cosmic-ray-sized steps, Cauchy at c = 2: the bits of the ragged form with the weights formed on the host.
7. batch_eval's residuals: the same bytes whatever the batch loss.
The observed maxima go where the other batch modules' go (GADFIT_BATCH_OBSERVE), under loss_*."""
import numpy as np
import pytest

from gadfit_amd import _lib
from tests import batch_bounds_cases as BB
from tests import batch_cases as BC
from tests import batch_cov_cases as CV
from tests import batch_cube_cases as CC
from tests import batch_form_cases as FC
from tests import batch_loss_cases as LC
from tests.batch_common import (COUNTS, SCENARIOS, TOL_CHI2, TOL_FIT, TOL_PARS, TOL_PASS, check_fit, context, fit_worst, observe, same_bits,
                                same_pass)
from tests.parity_common import TOL_LOSS

pytestmark = pytest.mark.gpu

FORMS = (64, 16, 256)
INF = float('inf')
_CTX = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def part_a_context(key='a', scale_weights=1.0):
    """Part A on a context of its own per key, its weights multiplied by scale_weights"""
    if key not in _CTX:
        tape, b = LC.part_a()
        c = context(tape)
        c.set_batch_data(b.off, b.x, b.y, b.w * scale_weights)
        _CTX[key] = c
    return _CTX[key]


@pytest.fixture(scope='module', autouse=True)
def _contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _tag(loss, c):
    return '%s_c%g' % (LC.LOSS_NAMES[loss], c)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_one_pass_against_the_oracle(lanes):
    tape, batch = LC.part_a()
    c = part_a_context()
    worst = dict(sums=0.0, chi2=0.0)
    for active, loss, scale in LC.pass_cases(lanes):
        st = LC.starts_a(active, 'conv')
        JTJ, JTr, chi2 = c.batch_pass(st, active, lanes_per_fit=lanes, loss=loss, loss_scale=scale)
        assert c.batch_lanes_used() == lanes and c.batch_loss_used() == (loss, scale)
        w, wc = LC.pass_worst(tape, batch.items, st, active, loss, scale, JTJ, JTr, chi2)
        print('pass %d lanes %s na=%d: sums %.3e chi2 %.3e' % (lanes, _tag(loss, scale), len(active), w, wc))
        worst['sums'] = max(worst['sums'], w); worst['chi2'] = max(worst['chi2'], wc)
    observe(**{'loss_pass_lanes%d_sums' % lanes: worst['sums'], 'loss_pass_lanes%d_chi2' % lanes: worst['chi2']})
    assert worst['sums'] < TOL_LOSS and worst['chi2'] < TOL_PASS


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def _fit_params():
    out = []
    for lanes in FORMS:
        for name, loss, scale in dict.fromkeys((k[0], k[2], k[3]) for k in LC.fit_cases(lanes)):
            out.append(pytest.param(lanes, name, loss, scale, id='%d-%s-%s' % (lanes, name, _tag(loss, scale))))
    return out


@pytest.mark.parametrize('lanes,name,loss,scale', _fit_params())
def test_fits_against_the_oracle(lanes, name, loss, scale):
    _, batch = LC.part_a()
    c = part_a_context()
    kw = LC.ARGS[name][1]
    for _, active, _, _ in [k for k in LC.fit_cases(lanes) if (k[0], k[2], k[3]) == (name, loss, scale)]:
        pars, res, _ = c.fit_batch(LC.starts_a(active, name), active, lanes_per_fit=lanes, loss=loss, loss_scale=scale, **kw)
        assert c.batch_lanes_used() == lanes and c.batch_loss_used() == (loss, scale)
        sel = LC.selection_a(active, name, loss, scale)
        assert sum(1 for s in sel if not s[0]) <= LC.CAP_A[name]
        worst = fit_worst(sel, pars, res, batch.n, len(active))
        check_fit('loss_lanes%d_%s_%s' % (lanes, name, _tag(loss, scale)), 'na%d' % len(active), worst, TOL_FIT, TOL_FIT)
        if name != 'conv':
            assert np.all(res['n_omega'] == res['n_sweeps']) and np.all(res['n_omega'] > 0)          # the omega pass is in it


@pytest.mark.parametrize('loss', LC.LOSSES)
@pytest.mark.parametrize('form', FC.FORMS, ids=lambda f: str(f.lanes))
def test_fits_at_the_forms_edge_lengths(form, loss):
    tape, _, st, batch = LC.part_b(form)
    c = context(tape, batch)
    try:
        pars, res, _ = c.fit_batch(st, LC.ACTIVE2, lanes_per_fit=form.lanes, loss=loss, **LC.ARGS['conv'][1])
        assert c.batch_lanes_used() == form.lanes and c.batch_loss_used() == (loss, 1.0)
    finally:
        c.close()
    sel = LC.selection_b(form, loss)
    assert sum(1 for s in sel if not s[0]) <= BC.RANDOM_CAP * len(sel)
    check_fit('loss_edges_lanes%d' % form.lanes, LC.LOSS_NAMES[loss], fit_worst(sel, pars, res, batch.n, 4), TOL_FIT, TOL_FIT)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_loss_zero_with_any_scale_is_the_linear_fit(lanes):
    tape, batch = LC.part_a()
    plain = context(tape, batch)          # a context whose batch loss was never set
    try:
        c = part_a_context()
        for name, active in (('conv', LC.SETS[3]), ('conv_acc', LC.SETS[7])):
            st = LC.starts_a(active, name)
            p0, r0, _ = plain.fit_batch(st, active, lanes_per_fit=lanes, **LC.ARGS[name][1])
            ps0 = plain.batch_pass(st, active, lanes_per_fit=lanes)
            c.set_batch_loss(1, 3.0)          # (and coming back from a loss leaves nothing behind)
            for scale in (7.0, 1e-3):
                p, r, _ = c.fit_batch(st, active, lanes_per_fit=lanes, loss=0, loss_scale=scale, **LC.ARGS[name][1])
                same_bits(p, r, p0, r0)
                assert np.array_equal(_bits(p), _bits(p0))
                same_pass(c.batch_pass(st, active, lanes_per_fit=lanes), ps0)
                assert c.batch_loss_used() == (0, scale)
    finally:
        plain.close()


@pytest.mark.parametrize('loss', LC.LOSSES)
@pytest.mark.parametrize('lanes', FORMS)
def test_a_power_of_two_scale_is_the_same_fit_at_scaled_weights(lanes, loss):
    """c = 8 and c = 1/4 on the weights w against c = 1 on the weights w / c: every sum exactly c^2 times, everything else the same bits"""
    c = part_a_context()
    active = LC.SETS[7]
    name = 'conv_acc'
    st = LC.starts_a(active, name)
    for scale in (8.0, 0.25):
        ref = part_a_context('w/%g' % scale, 1.0 / scale)
        p0, r0, _ = ref.fit_batch(st, active, lanes_per_fit=lanes, loss=loss, loss_scale=1.0, **LC.ARGS[name][1])
        ps0 = ref.batch_pass(st, active, lanes_per_fit=lanes)
        p, r, _ = c.fit_batch(st, active, lanes_per_fit=lanes, loss=loss, loss_scale=scale, **LC.ARGS[name][1])
        ps = c.batch_pass(st, active, lanes_per_fit=lanes)
        assert np.array_equal(_bits(p), _bits(p0))
        for f in COUNTS + ('dof',):
            assert np.array_equal(r[f], r0[f]), f
        assert np.array_equal(_bits(r['lambda_']), _bits(r0['lambda_']))
        assert np.array_equal(_bits(r['chi2']), _bits(r0['chi2'] * (scale * scale)))
        for u, v in zip(ps, ps0):
            assert np.array_equal(_bits(u), _bits(v * (scale * scale)))
        assert np.all(r['n_omega'] > 0) and np.all(r['iterations'] >= 2)


@pytest.mark.parametrize('lanes', FORMS)
def test_huber_beyond_every_residual_is_the_linear_fit(lanes):
    c = part_a_context()
    for active in LC.EDGE_SETS:
        st = LC.starts_a(active, 'conv_acc')
        kw = LC.ARGS['conv_acc'][1]
        p0, r0, _ = c.fit_batch(st, active, lanes_per_fit=lanes, loss=0, loss_scale=1.0, **kw)
        ps0 = c.batch_pass(st, active, lanes_per_fit=lanes)
        p, r, _ = c.fit_batch(st, active, lanes_per_fit=lanes, loss=LC.HUBER, loss_scale=2.0 ** 10, **kw)
        assert c.batch_loss_used() == (LC.HUBER, 1024.0)
        same_bits(p, r, p0, r0)
        assert np.array_equal(_bits(p), _bits(p0)) and np.all(r['n_omega'] > 0)
        same_pass(c.batch_pass(st, active, lanes_per_fit=lanes), ps0)


@pytest.mark.parametrize('loss', LC.LOSSES)
@pytest.mark.parametrize('lanes', FORMS)
def test_errors_and_infinite_bounds_return_fit_batchs_bits_under_the_loss(lanes, loss):
    c = part_a_context()
    active = LC.SETS[7]
    st = LC.starts_a(active, 'conv_acc')
    kw = LC.ARGS['conv_acc'][1]
    p0, r0, _ = c.fit_batch(st, active, lanes_per_fit=lanes, loss=loss, loss_scale=1.345, **kw)
    for scale in (False, True):
        p, r, (cov, sigma, info), _ = c.fit_batch_errors(st, active, scale=scale, lanes_per_fit=lanes, **kw)
        same_bits(p, r, p0, r0)
        assert np.array_equal(_bits(p), _bits(p0)) and c.batch_loss_used() == (loss, 1.345)
        cov1 = c.batch_covariance(p0, active, scale=scale, lanes_per_fit=lanes)
        for u, v in zip((cov, sigma), cov1[:2]):
            assert np.array_equal(_bits(u), _bits(v))
        assert np.array_equal(info, cov1[2]) and np.all(info == 0)
    p, r, at, _ = c.fit_batch_bounded(st, active, [-INF] * 8, [INF] * 8, lanes_per_fit=lanes, **kw)
    same_bits(p, r, p0, r0)
    assert np.array_equal(_bits(p), _bits(p0)) and np.all(at == 0) and c.batch_loss_used() == (loss, 1.345)
    assert np.all(r0['n_omega'] > 0)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_pinned_throughout_under_cauchy_equals_the_reduced_fit(lanes):
    case = LC.PINNED
    off, kw = SCENARIOS[LC.PINNED_SCENARIO]
    c = context(case.tape(), case.batch())
    try:
        lo, hi = case.box()
        pars, res, at, _ = c.fit_batch_bounded(case.starts(off), case.active, lo, hi, lanes_per_fit=lanes, loss=LC.CAUCHY, **kw)
        assert c.batch_lanes_used() == lanes and c.batch_loss_used() == (LC.CAUCHY, 1.0)
    finally:
        c.close()
    sel = LC.pinned_selection()
    kept = [b for b, s in enumerate(sel) if s[0]]
    assert len(kept) >= BB.CAP
    worst = fit_worst(sel, pars, res, case.batch().n, len(case.active))
    wall = np.float64(case.value)
    for b in kept:
        assert pars[b, case.active[case.j]].view(np.uint64) == wall.view(np.uint64), b
        assert int(at[b]) == case.bit(), (b, int(at[b]))
    check_fit('loss_pinned_lanes%d' % lanes, 'cauchy', worst, TOL_PARS, TOL_CHI2)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', LC.LOSSES)
@pytest.mark.parametrize('lanes', FORMS)
def test_covariance_against_the_inverse_of_the_oracles_scaled_matrix(lanes, loss):
    """tests/test_gpu_batch_cov.py's end-to-end bound, the per-pass bound through the inverse: err <= (na TOL_PASS + 10 r_host eps) kappa,
    under scale=True the same plus TOL_PASS against that reference times the oracle's PLAIN chi2 / dof"""
    tape, batch = LC.part_a()
    c = part_a_context()
    r_host = CV.r_host()
    worst = 0.0
    for active in LC.EDGE_SETS:
        na = len(active)
        st = LC.starts_a(active, 'conv')
        for scale_c in LC.PASS_SCALES:
            cov0, sig0, info0 = c.batch_covariance(st, active, scale=False, lanes_per_fit=lanes, loss=loss, loss_scale=scale_c)
            cov1, sig1, info1 = c.batch_covariance(st, active, scale=True, lanes_per_fit=lanes)
            assert c.batch_loss_used() == (loss, scale_c) and np.all(info0 == 0) and np.all(info1 == 0)
            for b, (x, y, w) in enumerate(batch.items):
                A, _, chi2 = LC.oracle_pass(tape, x, y, w, st[b], active, loss, scale_c)
                kap = CV.kappa(A)
                assert kap <= CV.KAPPA_MAX
                d = CV.scale_of(A)
                ref = CV.longdouble_inverse(A)
                bound = (na * TOL_PASS + 10.0 * r_host * CV.EPS) * kap
                err = CV.scaled_error(cov0[b], ref, d)
                assert err <= bound, (active, scale_c, b, err, bound)
                q = np.longdouble(chi2) / np.longdouble(max(batch.n[b] - na, 1))
                err1 = CV.scaled_error(cov1[b], ref * q, d)
                assert err1 <= bound + TOL_PASS, (active, scale_c, b, err1, bound)
                worst = max(worst, err / (CV.EPS * kap), err1 / (CV.EPS * kap))
                assert np.array_equal(_bits(sig1[b]), _bits(np.sqrt(np.diag(cov1[b]))))
    observe(**{'loss_cov_lanes%d_%s_over_eps_kappa' % (lanes, LC.LOSS_NAMES[loss]): worst})


@pytest.mark.parametrize('loss', LC.LOSSES)
def test_covariance_against_the_plain_paths_under_set_loss(loss):
    """three spectra of 5, 64 and 65 points at c = 1: Context.covariance (gfh_covariance) under set_loss inverts the same loss-scaled
    J^T J and multiplies by the same plain chi2 / dof, in another order of sums; the bound is the one above"""
    spectra = [BC.spectrum_n(n, 1) for n in (5, 64, 65)]
    items = [(x, LC.displaced(y, w, 3, 11), w) for _, x, y, w, _ in spectra]
    starts = np.array([t * np.where(np.arange(4) % 2 == 0, 1.05, 0.95) for t, _, _, _, _ in spectra])
    batch = BC.Batch(items)
    tape = LC.part_b(FC.WAVE)[0]
    r_host = CV.r_host()
    c = context(tape, batch)
    plain = _lib.Context(0)
    try:
        plain.set_model(tape)
        plain.set_loss(loss)
        for scale in (False, True):
            cov, sigma, info = c.batch_covariance(starts, LC.ACTIVE2, scale=scale, lanes_per_fit=64, loss=loss, loss_scale=1.0)
            assert np.all(info == 0)
            for b, (x, y, w) in enumerate(items):
                plain.set_data(x, y, 1.0 / w, [0, x.size])
                plain.init_weights(4)
                cov0, sig0, info0 = plain.covariance([starts[b]], LC.ACTIVE2, [0] * 4, scale=scale)
                assert info0 == 0
                A = LC.oracle_pass(tape, x, y, w, starts[b], LC.ACTIVE2, loss)[0]
                kap = CV.kappa(A)
                bound = (4 * TOL_PASS + 10.0 * r_host * CV.EPS) * kap + (TOL_PASS if scale else 0.0)
                err = CV.scaled_error(cov[b], cov0, CV.scale_of(A))
                print('n = %d, %s, scale=%s: kappa %.2e, difference %.3e (bound %.3e)' % (x.size, LC.LOSS_NAMES[loss], scale, kap, err, bound))
                assert err <= bound, (b, err, bound)
    finally:
        plain.close()
        c.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lanes', FORMS)
def test_a_uint16_cube_with_steps_returns_the_ragged_forms_bits(lanes):
    x, Y, starts = LC.cube()
    n, nf = LC.CUBE_N, LC.CUBE_FITS
    plain = _lib.Context(0)
    c = context(CC.tape())
    try:
        plain.set_model(CC.tape())
        W = CC.established_weights(plain, x, Y, LC.CUBE_ERROR, None)          # the device's own gfh_init_weights on a plain context
        kw = LC.ARGS['conv_acc'][1]
        c.set_batch_loss(LC.CUBE_LOSS, LC.CUBE_SCALE)
        c.set_batch_lanes(lanes)
        c.set_batch_cube(x, Y, LC.CUBE_ERROR)
        got = (c.batch_pass(starts, LC.ACTIVE2), c.fit_batch(starts, LC.ACTIVE2, **kw)[:2])
        assert c.batch_form_used() == ('cube', 2, LC.CUBE_ERROR) and c.batch_loss_used() == (LC.CUBE_LOSS, LC.CUBE_SCALE)
        c.set_batch_data(n * np.arange(nf + 1, dtype=np.int64), np.tile(x, nf), Y.astype(np.float64).ravel(), np.ascontiguousarray(W).ravel())
        ref = (c.batch_pass(starts, LC.ACTIVE2), c.fit_batch(starts, LC.ACTIVE2, **kw)[:2])
        assert c.batch_form_used() == 'ragged' and c.batch_lanes_used() == lanes
        same_pass(got[0], ref[0])
        same_bits(got[1][0], got[1][1], ref[1][0], ref[1][1])
        assert np.array_equal(_bits(got[1][0]), _bits(ref[1][0]))
        # the loss is at work: the linear fit of the same cube ends elsewhere
        lin = c.fit_batch(starts, LC.ACTIVE2, loss=0, **kw)[0]
        assert np.max(np.abs(lin - ref[1][0]) / np.abs(ref[1][0])) > 100.0 * TOL_FIT
    finally:
        plain.close()
        c.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_the_residuals_of_batch_eval_do_not_see_the_loss():
    c = part_a_context()
    active = LC.SETS[3]
    st = LC.starts_a(active, 'conv')
    c.set_batch_loss(0, 1.0)
    m0, r0, _, off0, _ = c.batch_eval(st, active, residuals=True, lanes_per_fit=64)
    for loss, scale in ((1, 1.0), (2, 1.345), (1, 8.0)):
        c.set_batch_loss(loss, scale)
        m, r, _, off, _ = c.batch_eval(st, active, residuals=True, lanes_per_fit=64)
        assert np.array_equal(_bits(m), _bits(m0)) and np.array_equal(_bits(r), _bits(r0)) and np.array_equal(off, off0)
    # ... and they are the plain (y - f) w: their squares sum to batch_pass's chi2 under any loss
    chi2 = c.batch_pass(st, active, lanes_per_fit=64)[2]
    for b in range(3):
        assert abs(np.sum(r0[off0[b]:off0[b + 1]] ** 2) - chi2[b]) <= TOL_PASS * chi2[b]


# ---- the session calls -------------------------------------------------------------------------------------------------------------------
def test_the_session_calls_set_the_loss_themselves():
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    tape, _, st, batch = LC.part_b(FC.WAVE)
    items = batch.items[:6]
    kw = dict(lambda_=1.0, max_iter=50, chi2_rel=2.0 ** -20)          # (exact in real32, as the session passes them)
    c = context(tape, BC.Batch(items))
    gf.gadf_close()
    gf.gadf_init(exp2())
    try:
        for k in range(4):
            gf.gadf_set(k + 1, 1.0, True)
        xs, ys, ws = zip(*items)
        ref = {loss: c.fit_batch(st[:6], LC.ACTIVE2, loss=loss, loss_scale=scale, **kw)[:2]
               for loss, scale in ((0, 1.0), (2, 1.345))}
        out = gf.gadf_fit_batch(xs, ys, ws, st[:6], loss=gf.LOSS_HUBER, loss_scale=1.345, **kw)
        same_bits(out[0], out[1], *ref[2])
        out = gf.gadf_fit_batch(xs, ys, ws, st[:6], **kw)          # None is the linear loss: nothing stays behind from the call before
        same_bits(out[0], out[1], *ref[0])
        assert not np.array_equal(ref[0][0], ref[2][0])
        gf.gadf_set_loss(gf.LOSS_CAUCHY)                           # the session's own loss is the plain fit's and stays refused in a batch
        with pytest.raises(gf.GadfitError, match=r'a robust loss \(gfh_set_loss\) is not carried by the batch kernels'):
            gf.gadf_fit_batch(xs, ys, ws, st[:6], loss=gf.LOSS_HUBER, **kw)
        gf.gadf_set_loss(gf.LOSS_LINEAR)
    finally:
        gf.gadf_close()
        c.close()
