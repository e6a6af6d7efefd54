"""What tests/test_gpu_gram_options.py rests on, shown without a GPU: under every case's loss the oracle's residuals, Jacobian rows and
sums equal a numpy.longdouble closed form to a tenth of the Jacobian tolerance and half of the tolerance of the sums; both Huber
branches are taken and no residual sits where device and oracle could choose different ones; the oracle's forward differences are
the forward differences of the closed form up to C_ref rounding errors of f; the cases cover every form under both losses on the
dispatch they are there for; and every translation unit the GPU file asks for compiles for gfx950 on a compile-only context."""
import time

import numpy as np

from gadfit_amd import _lib
from oracle import binding as orc
from tests import gram_layout_cases as GL
from tests import gram_option_cases as GO

JTOL = 7e-13          # tests/parity_common.py: _device_vs_oracle's jtol


def _problem(o):
    xs, ys, ws, start = o.case.data()
    return orc.OracleProblem(o.case.tape(), xs, ys, ws, start, o.case.active, o.case.is_global, loss=o.loss, use_ad=o.use_ad)


def test_the_oracle_is_a_sound_reference_under_every_loss():
    """D1, D2 and D4: the oracle's scaled residuals and Jacobian rows against the closed form in longdouble under _device_vs_oracle's
    per-entry metric (a tenth of jtol), its J^T J, J^T r and robust sum of squares against the longdouble sums (ORACLE_SUM_TOL), chi2()
    plain and larger; from 65 points on both Huber branches occur; no |r| within 1e-6 of 1, where Huber's branches meet"""
    cases = GO.d1() + GO.d2() + GO.d4()
    worst = dict(J=0.0, res=0.0, JTJ=0.0, JTr=0.0, chi2=0.0, gap=1.0)
    for o in cases:
        c = o.case
        p = _problem(o)
        JTJ, JTr, res, JT = p.sweep(want_J=True)
        chi_plain, res_plain = p.chi2()
        assert np.all(np.isfinite(JT)) and np.all(np.isfinite(res)) and np.all(np.isfinite(JTJ)), o.id
        errJ = errR = 0.0
        rows = []; rr = []
        for d in range(c.nd):
            sl = slice(p.dp[d], p.dp[d + 1])
            plain, r, want = GO.longdouble_rows(o, d)
            got = JT[sl][:, p.jac[d]]
            scale = np.maximum(np.abs(want), 1e-6 * np.max(np.abs(want), axis=0, keepdims=True) + 1e-300)
            errJ = max(errJ, float(np.max(np.abs(got - want) / scale)))
            errR = max(errR, float(np.max(np.abs(res[sl] - r)) / max(1.0, float(np.max(np.abs(r))))))
            assert float(np.max(np.abs(res_plain[sl] - plain))) <= 0.1 * JTOL * max(1.0, float(np.max(np.abs(plain)))), o.id
            rows.append(want); rr.append(r)
        gap = float(np.min(np.abs(np.abs(res_plain) - 1.0)))
        assert gap > 1e-6, (o.id, gap)
        n_hi, n_lo = int(np.sum(np.abs(res_plain) > 1.0)), int(np.sum(np.abs(res_plain) < 1.0))
        if o.loss == GO.HUBER and p.N >= 65:
            assert n_hi > 0 and n_lo > 0, (o.id, n_hi, n_lo)
        want = GO.longdouble_sums(np.concatenate(rows), np.concatenate(rr), p.dp, p.jac, p.dim)
        chi_robust = float(np.sum(res * res))
        e = GO.sum_errors(JTJ, JTr, chi_robust, want)
        assert chi_plain > chi_robust, o.id
        print('%-28s na %3d dim %3d, |r| > 1 at %4d points and < 1 at %4d, nearest to 1 by %.1e; oracle against longdouble: Jacobian %.2e, residuals %.2e, '
              'J^T J %.2e, J^T r %.2e, chi2 %.2e' % (o.id, c.na, c.dim, n_hi, n_lo, gap, errJ, errR, e[0], e[1], e[2]))
        assert errJ <= 0.1 * JTOL and errR <= 0.1 * JTOL, (o.id, errJ, errR)
        assert max(e) <= GL.ORACLE_SUM_TOL, (o.id, e)
        worst = dict(J=max(worst['J'], errJ), res=max(worst['res'], errR), JTJ=max(worst['JTJ'], e[0]), JTr=max(worst['JTr'], e[1]),
                     chi2=max(worst['chi2'], e[2]), gap=min(worst['gap'], gap))
    print('worst over %d cases: Jacobian %.2e, residuals %.2e, J^T J %.2e, J^T r %.2e, chi2 %.2e; nearest |r| to 1: %.1e'
          % (len(cases), worst['J'], worst['res'], worst['JTJ'], worst['JTr'], worst['chi2'], worst['gap']))
    assert len(cases) == 40 + 4 + 2


def test_fd_oracle_against_longdouble_forward_differences():
    """D3: the oracle's forward-difference Jacobian against the same difference, with the same double step, of the closed form in
    longdouble, in units of eps S_i w_i / |step_j| (GO.expK_fd_bound): C_ref, the constant the device is held to four times of.  It IS
    a finite difference (differs from the AD oracle's J^T J by 1e-10 ... 1e-5), its residuals are the AD oracle's, and no active start
    parameter is small enough for 'Absolute value of parameter ... is too small'"""
    c_ref = 0.0
    for o in GO.d3():
        c = o.case
        xs, ys, ws, start = c.data()
        assert c.active == list(range(c.na)) and c.K == (c.na + 1) // 2 and c.nd == 1 and not o.use_ad and o.loss == 0
        assert np.all(np.abs(GO.fd_steps(start[0])[c.active]) > 1e-10)          # (the error is raised below DBL_MIN = 2.2e-308)
        p = _problem(o)
        JTJ, JTr, res, JT = p.sweep(want_J=True)
        pa = orc.OracleProblem(c.tape(), xs, ys, ws, start, c.active, c.is_global)
        JTJa, _, resa, JTa = pa.sweep(want_J=True)
        sc = np.sqrt(np.outer(np.diag(JTJa), np.diag(JTJa)))
        d_ad = float(np.max(np.abs(JTJ - JTJa) / sc))
        assert 1e-10 < d_ad < 1e-5, (o.id, d_ad)
        assert np.array_equal(res, resa), o.id
        f, g = GO.expK_fd_rows(c.K, start[0], xs[0], c.active)
        want = g * ws[0].astype(np.longdouble)[:, None]
        bound = GO.expK_fd_bound(c.K, start[0], xs[0], ws[0], c.active)
        ratio = float(np.max(np.abs(JT - want) / bound))
        of_max = float(np.max(np.abs(JT - want)) / np.max(np.abs(JT)))
        print('%-20s FD oracle against the longdouble forward difference: %.3f bounds (%.2e of max |J|); J^T J against the AD oracle: %.2e'
              % (o.id, ratio, of_max, d_ad))
        c_ref = max(c_ref, ratio)
    print('C_ref = %.4f' % c_ref)
    assert 0.9 * GO.FD_C_REF <= c_ref <= GO.FD_C_REF, c_ref
    assert GO.FD_DEVICE_FACTOR == 4.0 and len(GO.d3()) == 6


def test_option_cases_by_hand():
    """D1 covers every form under both losses; each case expects the dispatch it is there for"""
    d1 = GO.d1()
    forms = set(GL.form_of(na) for na in range(9, 200))
    assert forms == {'full', 'half', 'coop', 'unfused'}
    assert set((GL.form_of(o.case.na), o.loss) for o in d1) == set((f, l) for f in forms for l in (1, 2))
    assert len(d1) == 2 * (6 * 3 + 2) and [o.case.na for o in d1[:20]] == [16] * 3 + [32] * 3 + [48] * 3 + [80] * 3 + [96] * 3 + [128] * 3 + [130] * 2
    lay = {1: (512, 1), 65: (512, 1), 2049: (2560, 5)}
    waves = {16: 8, 32: 8, 48: 4, 80: 4, 96: 4, 128: 4, 130: 0}
    for o in d1:
        c = o.case; e = c.expect()
        assert e == dict(n_slots=lay[c.sizes[0]][0], n_gb=lay[c.sizes[0]][1], datasets_with_blocks=1, fused=int(c.na <= 128), waves=waves[c.na],
                         tail_mode=2 if c.na <= 128 else 0, sparse=0, kernarg=c.n_pars), o.id
        assert c.n_pars == (161 if c.na <= 80 else 241)
    d2 = GO.d2()
    assert [o.id for o in d2] == ['D2-cauchy-B2-32', 'D2-cauchy-B2-96', 'D2-cauchy-B3-32', 'D2-cauchy-B3-96'] and all(o.loss == 1 for o in d2)
    assert d2[0].case.expect() == dict(n_slots=2048, n_gb=3, datasets_with_blocks=3, fused=1, waves=8, tail_mode=2, sparse=0, kernarg=0)
    assert d2[1].case.expect() == dict(n_slots=1536, n_gb=2, datasets_with_blocks=2, fused=1, waves=4, tail_mode=2, sparse=0, kernarg=0)
    for o, fw in zip(d2[2:], (8, 4)):
        assert o.case.expect() == dict(n_slots=7168, n_gb=14, datasets_with_blocks=8, fused=1, waves=fw, tail_mode=0, sparse=1, kernarg=0)
    d3 = GO.d3()
    assert [(o.case.na, o.case.K, o.case.n_pars, o.case.sizes[0]) for o in d3] == [(17, 9, 19, 65), (17, 9, 19, 2049), (65, 33, 67, 65), (65, 33, 67, 2049),
                                                                                   (81, 41, 83, 65), (81, 41, 83, 2049)]
    assert [GL.form_of(o.case.na) for o in d3[::2]] == ['full', 'half', 'coop']
    for o in d3:
        e = o.case.expect()
        assert (e['fused'], e['tail_mode'], e['sparse'], e['kernarg'], e['n_gb']) == (1, 2, 0, o.case.n_pars, 1 if o.case.sizes[0] == 65 else 5)
    d4 = GO.d4()
    assert [(o.case.na, o.loss, o.fits) for o in d4] == [(32, 1, (GO.D4_FIT_ACC, GO.D4_FIT_PLAIN)), (96, 1, (GO.D4_FIT_ACC, GO.D4_FIT_PLAIN))]
    assert d4[0].case.expect() == dict(n_slots=4096, n_gb=8, datasets_with_blocks=3, fused=1, waves=8, tail_mode=2, sparse=0, kernarg=96)
    assert d4[1].case.expect() == dict(n_slots=4096, n_gb=8, datasets_with_blocks=3, fused=1, waves=4, tail_mode=0, sparse=1, kernarg=288)
    assert 'accth' in GO.D4_FIT_ACC and 'accth' not in GO.D4_FIT_PLAIN
    assert len(GO.all_cases()) == 40 + 4 + 6 + 2 and len(set(o.id for o in GO.all_cases())) == 52


def test_the_oracles_own_fit_moves_with_the_rounding_of_its_sums():
    """D4: the oracle's fits with its sums cut into 2, 3, 8 and 64 images.  J^T J moves by less than 1e-14 -- a tenth of the 1e-13 the
    device's is held to -- and the parameters fitted in 4 iterations move by less than TOL_FIT at 32 active per dataset, but by
    more than ten times TOL_FIT at 96 (the skew parameters, which lie near zero, in 240 columns): there the device cannot be held to
    TOL_FIT against a reference that does not keep it against itself, and TOL_FIT_LOSS_96 is ten times what the device showed"""
    from tests.parity_common import TOL_FIT, TOL_FIT_LOSS_96
    moved = {}
    for o in GO.d4():
        p = _problem(o)
        JTJ1 = p.sweep()[0]
        dg = np.sqrt(np.outer(np.diag(JTJ1), np.diag(JTJ1)))
        for fit in o.fits:
            q = _problem(o); r = q.fit(**fit); base = q.pars.copy()
            for k in GO.D4_IMAGES:
                dJ = float(np.max(np.abs(p.sweep(n_images=k)[0] - JTJ1) / dg))
                q = _problem(o); rk = q.fit(n_images=k, **fit)
                dp = float(np.max(np.abs(q.pars - base) / np.abs(base)))
                print('%s %s on %2d images: J^T J moves by %.2e, the fitted parameters by %.2e, chi2 by %.2e'
                      % (o.id, 'accelerated' if 'accth' in fit else 'plain', k, dJ, dp, abs(rk.chi2 - r.chi2) / r.chi2))
                assert dJ < 1e-14 and rk.iterations == r.iterations == 4 and abs(rk.chi2 - r.chi2) <= 1e-12 * r.chi2
                moved[o.case.na] = max(moved.get(o.case.na, 0.0), dp)
    print('the oracle against itself: %.2e at 32 active, %.2e at 96' % (moved[32], moved[96]))
    assert moved[32] < TOL_FIT and 10 * TOL_FIT < moved[96] < TOL_FIT_LOSS_96
    assert [o.fit_tol for o in GO.d4()] == [TOL_FIT, TOL_FIT_LOSS_96]


N_UNITS = 38


def test_every_option_unit_compiles_for_gfx950():
    """2 losses x (6 fused forms x 2 + 1) units of D1, 2 x 2 of D2, 3 + 1 of D3, 2 x 2 of D4: each compiled alone on a compile-only
    context whose loss and use_ad are set before the form is prepared (both are part of the generated source), the seconds printed"""
    units = GO.units()
    print('%d translation units' % len(units))
    assert len(units) == N_UNITS == 2 * 13 + 4 + 4 + 4
    c = _lib.Context(-1)
    try:
        t0 = time.perf_counter()
        for tape, active, nd, store, loss, use_ad in units:
            t1 = time.perf_counter()
            c.set_loss(loss); c.set_use_ad(use_ad)
            c.set_model(tape)
            c.model_prepare_form(active, nd, store)
            print('  %3d active of %3d parameters, %d dataset(s), loss %d, %s, %s: %.1f s' % (len(active), tape.n_pars, nd, loss, 'AD' if use_ad else 'finite differences',
                                                                                        'stores J' if store else 'no store', time.perf_counter() - t1))
        print('compiled (or found in the cache) in %.1f s' % (time.perf_counter() - t0))
        c.set_loss(GO.HUBER); c.set_use_ad(True)
        c.set_model(units[0][0])
        src = c.model_source(units[0][1])
        assert '#define GFH_NA 16\n' in src and 'GFH_ROBUST' in src
    finally:
        c.close()
