"""The options that change what the kernels compute per point -- the robust losses and use_ad = .false. -- on every form of the fused
sweep + Gram kernel (tests/gram_option_cases.py: the cases; tests/test_cpu_gram_option_cases.py: why the oracle is a sound reference
on them).  Under a loss every case is one full pass against the oracle at the unchanged tolerances of tests/parity_common.py:
_device_vs_oracle(loss=) on the dispatch the case expects, and then, on the same data,
 - the device's J^T J, J^T r and sum of squares against the same sums of the device's OWN jacobian() and residuals() in
   numpy.longdouble: a form that stages another row than it stores, or scales one of them only, fails here whatever its Jacobian is,
 - fused forms: the kernel without the Jacobian store returns bitwise the storing kernel's three, and omega() then fails with
   'Jacobian was not kept' (under a loss STEP 3 reads the stored, scaled Jacobian),
 - where the in-kernel tail served the case, a second context under GADFIT_HIP_TAIL=0 returns bitwise the same three; the
   pattern-only cases the same under GADFIT_HIP_SPARSE=0.
Under finite differences the Jacobian is rounding noise of f over the step, so it is held entry by entry to the longdouble forward
difference under the derived bound of GO.expK_fd_bound, and the Gram stage by the self-consistency check.  D4 fits under a loss on
the matrix-core forms against the oracle's fits and over the keep_jacobian modes."""
import numpy as np
import pytest

from gadfit_amd import _lib
from oracle import binding as orc
from tests import gram_layout_cases as GL
from tests import gram_option_cases as GO
from tests.parity_common import _close, _device_vs_oracle, _observe, rel

pytestmark = pytest.mark.gpu

SELF_TOL = 1e-13          # _device_vs_oracle's tol: looser than needed, no Jacobian error enters [J^T J 4.1e-15, J^T r 2.8e-16, chi2 1.8e-16]


class _KeepsModel:
    """a context whose set_model is skipped while the tape is the one it holds: the kernels loaded for it stay (set_data alone between
    the sizes of a form)"""

    def __init__(self, ctx):
        self._ctx, self._held = ctx, None

    def set_model(self, tape):
        if tape is not self._held:
            self._ctx.set_model(tape)
            self._held = tape

    def __getattr__(self, name):
        return getattr(self._ctx, name)


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield _KeepsModel(c)
    c.close()


@pytest.fixture
def options(ctx):
    """sets the case's loss and use_ad on the module's context and takes them back afterwards"""
    def set_(o):
        ctx.set_loss(o.loss); ctx.set_use_ad(o.use_ad)
    yield set_
    ctx.set_loss(0); ctx.set_use_ad(True); ctx.set_keep_jacobian(1)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _second_context(o, pars, jac, dim, monkeypatch, switch):
    """(the sweep, debug_layout()) of a fresh context created with the environment switch off, under the case's options"""
    c = o.case
    xs, ys, ws, _ = c.data()
    monkeypatch.setenv(switch, '0')
    k = _lib.Context(0)
    try:
        k.set_loss(o.loss); k.set_use_ad(o.use_ad)
        k.set_model(c.tape())
        k.set_data(np.concatenate(xs), np.concatenate(ys), np.concatenate(ws), np.concatenate([[0], np.cumsum(c.sizes)]))
        return k.sweep(pars, c.active, jac, dim), k.debug_layout()
    finally:
        k.close()
        monkeypatch.delenv(switch)


def _self_consistent(ctx, o, p, stored):
    """the sums of the Gram stage against the sums of the rows and residuals the same sweep stored, in longdouble"""
    J = ctx.jacobian(o.case.na); res = ctx.residuals()
    want = GO.longdouble_sums(J, res, p.dp, p.jac, p.dim)
    e = GO.sum_errors(stored[0], stored[1], stored[2], want)
    print('%s: device sums against its own rows in longdouble: J^T J %.2e, J^T r %.2e, chi2 %.2e' % ((o.id,) + e))
    _observe(self_JTJ=e[0], self_JTres=e[1], self_chi2=e[2])
    assert e[0] < SELF_TOL, (o.id, 'J^T J is not the Gram matrix of the stored rows', e)
    assert e[1] < SELF_TOL and e[2] <= SELF_TOL, (o.id, e)


def _without_the_store(ctx, o, p, stored, want):
    ctx.set_keep_jacobian(0)
    try:
        assert _same(ctx.sweep(p.pars, o.case.active, p.jac, p.dim), stored), o.id
        assert ctx.debug_layout() == want, o.id
        with pytest.raises(_lib.GadfitHipError, match='Jacobian was not kept'):          # STEP 3 needs J under a loss and under finite differences
            ctx.omega(p.pars, np.ones(p.dim))
    finally:
        ctx.set_keep_jacobian(1)


def _pass(ctx, o, monkeypatch):
    """one case under a loss: the pass against the oracle, the dispatch, and the bitwise identities between the kernel's variants"""
    c = o.case
    xs, ys, ws, start = c.data()
    p = _device_vs_oracle(ctx, c.tape(), xs, ys, ws, start, c.active, c.is_global, loss=o.loss)
    want = c.expect()
    assert ctx.debug_layout() == want, o.id
    assert p.dim == c.dim
    stored = ctx.sweep(p.pars, c.active, p.jac, p.dim)
    _self_consistent(ctx, o, p, stored)
    if o.loss == GO.HUBER and p.N >= 65:
        plain = p.chi2()[1]
        assert np.any(np.abs(plain) > 1.0) and np.any(np.abs(plain) < 1.0), o.id
    if c.fused:
        _without_the_store(ctx, o, p, stored, want)
    if want['tail_mode']:
        a, lay = _second_context(o, p.pars, p.jac, p.dim, monkeypatch, 'GADFIT_HIP_TAIL')
        assert lay == c.expect(tail_on=False) and lay['tail_mode'] == 0, o.id
        assert _same(a, stored), o.id
    if want['sparse']:
        a, lay = _second_context(o, p.pars, p.jac, p.dim, monkeypatch, 'GADFIT_HIP_SPARSE')
        assert lay == c.expect(sparse_ok=False) and lay['sparse'] == 0, o.id
        assert _same(a, stored), o.id
    return p, stored


@pytest.mark.parametrize('o', GO.d1(), ids=repr)
def test_loss_on_every_form(ctx, options, o, monkeypatch):
    """D1: Cauchy and Huber x 16, 32, 48 (full stage), 80 (half stage), 96, 128 (cooperative), 130 (plain sweep + blocked Gram) active
    parameters x 1, 65 and 2049 points"""
    options(o)
    _pass(ctx, o, monkeypatch)


@pytest.mark.parametrize('o', GO.d2(), ids=repr)
def test_loss_over_several_datasets(ctx, options, o, monkeypatch):
    """D2: Cauchy on B2 (tail, inv[] scatter) and B3 (chain, pattern-only image, parameter block by pointer) at 32 and 96 active"""
    options(o)
    want = o.case.expect()
    assert (want['tail_mode'], want['sparse']) == ((2, 0) if o.case.part == 'B2' else (0, 1)) and want['kernarg'] == 0
    _pass(ctx, o, monkeypatch)


@pytest.mark.parametrize('o', GO.d3(), ids=repr)
def test_finite_differences_on_every_fused_form(ctx, options, o):
    """D3: use_ad = .false. at 17 (full stage), 65 (half stage) and 81 (cooperative) active parameters x 65 and 2049 points.  The
    residuals against the oracle (no differencing: 1e-10, as tests/test_gpu_parity.py has it); J^T J is the finite-difference one
    (1e-10 ... 1e-5 from the AD oracle's); the Jacobian against the longdouble forward difference within 4 C_ref bounds
    (GO.expK_fd_bound); the Gram stage against the stored rows; STEP 3 through gfh_k_omega (central difference) and k_jtv"""
    options(o)
    c = o.case
    xs, ys, ws, start = c.data()
    x, y, w = xs[0], ys[0], ws[0]
    p = orc.OracleProblem(c.tape(), xs, ys, ws, start, c.active, c.is_global, use_ad=False)
    JTJ0, JTr0, res0, JT0 = p.sweep(want_J=True)
    JTJa = orc.OracleProblem(c.tape(), xs, ys, ws, start, c.active, c.is_global).sweep()[0]
    ctx.set_model(c.tape())
    ctx.set_data(x, y, w, p.dp)
    jac, dim = ctx.jacobian_indices(c.active, c.is_global)
    stored = ctx.sweep(p.pars, c.active, jac, dim)
    want = c.expect()
    assert ctx.debug_layout() == want, o.id
    res = ctx.residuals(); J = ctx.jacobian(c.na)
    assert rel(res, res0) < 1e-10
    sc = np.sqrt(np.outer(np.diag(JTJ0), np.diag(JTJ0)))
    d_ad = float(np.max(np.abs(stored[0] - JTJa) / sc))
    assert 1e-10 < d_ad < 1e-5, (o.id, d_ad)
    _, g = GO.expK_fd_rows(c.K, start[0], x, c.active)
    bound = GO.expK_fd_bound(c.K, start[0], x, w, c.active)
    ratio = float(np.max(np.abs(J - g * w.astype(np.longdouble)[:, None]) / bound))
    print('%s: J^T J against the AD oracle %.2e; Jacobian against the longdouble forward difference: %.3f bounds (allowed %.3f), against the oracle %.2e of max |J|'
          % (o.id, d_ad, ratio, GO.FD_DEVICE_FACTOR * GO.FD_C_REF, np.max(np.abs(J - JT0)) / np.max(np.abs(JT0))))
    _observe(fd_ratio=ratio, res=rel(res, res0))
    assert ratio <= GO.FD_DEVICE_FACTOR * GO.FD_C_REF, (o.id, ratio)
    _self_consistent(ctx, o, p, stored)
    d1 = _lib.potr(JTJ0 + np.diag(np.diag(JTJ0)), JTr0)
    om0, JTom0 = p.omega(d1, JT0)
    JTom = ctx.omega(p.pars, d1)
    e_om = float(np.max(np.abs(ctx.omega_vector() - om0)) / np.max(np.abs(w * GL.expK_numpy(c.K)(start[0], x))))
    e_jto = float(np.max(np.abs(JTom - JTom0)) / np.max(np.abs(JTom0)))
    print('%s: omega %.2e of max |f| w, J^T omega %.2e' % (o.id, e_om, e_jto))
    _observe(omega=e_om, JTomega=e_jto)
    assert e_om < 1e-6 and e_jto < 1e-3, (o.id, e_om, e_jto)
    if c.na in GO.D3_NO_STORE:
        _without_the_store(ctx, o, p, stored, want)


@pytest.mark.parametrize('o', GO.d4(), ids=repr)
def test_fits_under_a_loss_and_the_keep_jacobian_modes(ctx, options, o, monkeypatch):
    """D4: gaussK(8) (32 active per dataset, tail) and gaussK(24) (96, cooperative, chain) under Cauchy: the pass; 4-iteration fits with
    and without geodesic acceleration against the oracle's (the same iterations, chi2() and omega() calls, no look-ahead, parameters at
    TOL_FIT, at 96 active at TOL_FIT_LOSS_96: tests/parity_common.py); and what test_keep_jacobian_modes cannot reach at 8 active parameters under AD, where STEP 3 never needs J: with accth,
    mode 2 stores (jacobian() succeeds afterwards) and equals mode 1 bitwise, mode 0 refuses; without, all three are bitwise equal
    and mode 2 has not stored"""
    options(o)
    c = o.case
    xs, ys, ws, start = c.data()
    _pass(ctx, o, monkeypatch)
    N = sum(c.sizes)
    for fit in o.fits:
        acc = 'accth' in fit
        q = orc.OracleProblem(c.tape(), xs, ys, ws, start, c.active, c.is_global, loss=o.loss)
        r0 = q.fit(**fit)
        got = {}
        for mode in (1, 2, 0):
            ctx.set_keep_jacobian(mode)
            if mode == 0 and acc:
                with pytest.raises(_lib.GadfitHipError, match='Jacobian was not kept'):
                    ctx.fit(start.copy(), c.active, c.is_global, **fit)
                continue
            out, r = ctx.fit(start.copy(), c.active, c.is_global, **fit)
            got[mode] = (out, r.chi2)
            assert (r.iterations, r.n_chi2, r.n_omega) == (r0.iterations, r0.n_chi2, r0.n_omega), (o.id, mode, acc)
            assert r.n_lookahead == 0 and (r.n_omega > 0) == acc
            if mode == 2 and acc:
                assert ctx.jacobian(c.na).shape == (N, c.na)
            elif mode == 2:
                with pytest.raises(_lib.GadfitHipError, match='Jacobian was not kept'):
                    ctx.jacobian(c.na)
        ctx.set_keep_jacobian(1)
        for mode in got:
            assert np.array_equal(got[mode][0], got[1][0]) and got[mode][1] == got[1][1], (o.id, mode, acc)
        assert sorted(got) == ([1, 2] if acc else [0, 1, 2])
        print('%s %s: chi2 %.17g after %d iterations, oracle %.17g' % (o.id, 'accelerated' if acc else 'plain', got[1][1], r0.iterations, r0.chi2))
        _close('pars_fit', got[1][0], q.pars, o.fit_tol)
