"""What the GPU parity files share: the tolerances, the error metrics and _device_vs_oracle, one full pass of the device against the
CPU oracle on identical inputs (tests/test_gpu_parity.py, tests/test_gpu_gram_layouts.py, tests/test_gpu_gram_options.py).  Importable without a GPU."""
import numpy as np

from oracle import binding as orc

# Asserted tolerances = about 10 x the maxima OBSERVED on MI355X (run with GADFIT_PARITY_DUMP=<file> to re-record them; the
# numbers in brackets are those maxima).  All relative.
TOL_FIT = 1e-12                # fitted parameters against the oracle after 3-20 LM iterations of the small test problems [7e-14]
# ... of gaussK(24)'s three datasets (96 active each, 240 columns) under the Cauchy loss after 4 iterations (tests/gram_option_cases.py: D4)
# [2.4e-11 plain, 1.6e-11 accelerated, both on the skew parameters, which lie near zero; against the largest parameter of each kind
# 5e-13].  Every per-pass check of that case holds at the tolerances below.  The oracle's own fitted parameters move by 1.8e-11 when its
# sums are cut into 2 ... 64 images, which moves its J^T J by 2.4e-15, a fortieth of the 1e-13 the device's is held to
# (tests/test_cpu_gram_option_cases.py: test_the_oracles_own_fit_moves_with_the_rounding_of_its_sums), so TOL_FIT cannot hold there.
TOL_FIT_LOSS_96 = 2.4e-10
TOL_LAMBDA = 3e-11             # final lambda under Nielsen's update: a function of a chi2 DIFFERENCE [2.6e-12]
# the reference's golden fits (its own tolerances: 1e-13, 1e-11, 1e-9, 1e-13 absolute): [1.1e-15, 2.7e-13, 3.6e-11, 4.1e-16].
# Test 3 (nested quadrature to rel 1e-5 / 1e-6) is pinned by the reference itself only to 1e-9 absolute: the value depends on
# the compiler's libm through the adaptive mesh (flang reproduces the gfortran golden to 3e-10).
TOL_GOLDEN_1, TOL_GOLDEN_2, TOL_GOLDEN_3, TOL_GOLDEN_4 = 2e-14, 3e-12, 4e-10, 1e-14
TOL_PASS = 2e-13               # one pass (JTJ, JTres, chi2, res, omega, J^T omega) outside _device_vs_oracle [1.3e-14]
TOL_LOSS = 3e-11               # the same under a robust loss: res and J carry sqrt(rho'), which the C++ side forms as sqrt(1 / (1 + r^2)) [2.6e-12]
TOL_CXX, TOL_CXX_SUMS, TOL_CXX_INTEGRAL, TOL_CXX_NESTED = 1e-13, 1e-13, 2e-14, 2e-13      # the C++ side's known answers [8.9e-15, 9.9e-15, 8.9e-16, 1.3e-14]


def rel(a, b):
    a = np.asarray(a, dtype=float); b = np.asarray(b, dtype=float)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300 + 1e-3 * np.max(np.abs(b))))


_OBSERVED = {}      # GADFIT_PARITY_DUMP=<file>: the maxima actually seen, per test (tolerances below = these x 10, profiles/parity_r02.json)


def _observe(**kw):
    import os
    key = os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]
    d = _OBSERVED.setdefault(key, {})
    for k, v in kw.items():
        d[k] = max(d.get(k, 0.0), float(v))
    dst = os.environ.get('GADFIT_PARITY_DUMP')
    if dst:
        import json
        json.dump(_OBSERVED, open(dst, 'w'), indent=1)


def _close(label, got, want, tol, scale=None):
    """max |got - want| / scale <= tol (scale: |want| entry by entry unless given); the maximum seen is recorded (_observe)"""
    got = np.asarray(got, dtype=float); want = np.asarray(want, dtype=float)
    sc = np.abs(want) if scale is None else scale
    err = float(np.max(np.abs(got - want) / sc)) if want.size else 0.0
    _observe(**{label: err})
    assert err <= tol, (label, err, tol, got, want)


def _device_vs_oracle(ctx, tape, xs, ys, ws, pars, active, is_global, tol=1e-13, with_omega=True, jtol=7e-13, otol=1.5e-13, loss=0, use_ad=True):
    """tol: JTJ / JTres / chi2 [observed over all callers: 7e-15, 2.2e-15, 4.6e-15]; jtol: Jacobian entries -- relative to the
    entry, floored at 1e-6 of the column maximum, so cancellation in small entries shows -- and residuals [7.1e-14, 4.4e-15];
    otol: omega, J^T omega and the convergence reductions J^T res, cos(phi) sums [3e-15, 1.3e-15, 1.3e-14, 1.5e-15].
    See also profiles/parity_r02.json (the BASELINE configurations at N = 2e4).
    loss, use_ad: the oracle's; the caller has set the same on the context (set_loss, set_use_ad).  Under a loss the sweep's residuals,
    Jacobian and sum of squares are the robust ones (scaled by sqrt(rho')), chi2() and the residuals it leaves stay plain
    (lm_solver.cpp:303-317, 513-529): the sweep's chi2 is held to sum(res0^2), chi2() to the oracle's, plain > robust, and the
    convergence sums pair the scaled Jacobian with chi2()'s plain residuals, as the fit has them at that point."""
    p = orc.OracleProblem(tape, xs, ys, ws, pars, active, is_global, loss=loss, use_ad=use_ad)
    JTJ0, JTr0, res0, JT0 = p.sweep(want_J=True)
    chi0, res_c = p.chi2()          # chi0: what chi2() returns; chi_s: what the sweep returns; res_c: the residuals chi2() leaves
    chi_s = chi0
    if loss:
        chi_s = float(np.sum(res0 * res0))
        assert chi0 > chi_s, 'the plain sum of squares exceeds the robust one'
    else:
        res_c = res0
    ctx.set_model(tape)
    ctx.set_data(np.concatenate(xs), np.concatenate(ys), np.concatenate(ws), p.dp)
    jac, dim = ctx.jacobian_indices(active, is_global)
    assert dim == p.dim and np.array_equal(jac, p.jac)
    JTJ, JTr, chi2 = ctx.sweep(p.pars, active, jac, dim)
    res = ctx.residuals()
    J = ctx.jacobian(len(active))
    # per-point quantities
    Jd = np.zeros_like(JT0)
    for d in range(p.nd):
        sl = slice(p.dp[d], p.dp[d + 1])
        Jd[sl][:, jac[d]] = J[sl]
    scale = np.maximum(np.abs(JT0), 1e-6 * np.max(np.abs(JT0), axis=0, keepdims=True) + 1e-300)
    dscale = np.sqrt(np.outer(np.diag(JTJ0), np.diag(JTJ0))) + 1e-300
    chi_k = ctx.chi2(p.pars)
    _observe(J=np.max(np.abs(Jd - JT0) / scale), res=np.max(np.abs(res - res0)) / max(1.0, np.max(np.abs(res0))),
             JTJ=np.max(np.abs(JTJ - JTJ0) / dscale), JTres=np.max(np.abs(JTr - JTr0) / (np.sqrt(np.diag(JTJ0) * chi_s) + 1e-300)),
             chi2=max(abs(chi2 - chi_s) / chi_s, abs(chi_k - chi0) / chi0))
    assert np.max(np.abs(Jd - JT0) / scale) < jtol, 'Jacobian entries'
    assert np.max(np.abs(res - res0)) <= jtol * max(1.0, np.max(np.abs(res0)))
    assert np.max(np.abs(JTJ - JTJ0) / dscale) < tol, 'JTJ'
    assert np.allclose(JTJ, JTJ.T, rtol=0, atol=0), 'JTJ must come back exactly symmetric'
    assert np.max(np.abs(JTr - JTr0) / (np.sqrt(np.diag(JTJ0) * chi_s) + 1e-300)) < tol, 'JTres'
    assert abs(chi2 - chi_s) <= tol * chi_s
    assert not loss or chi_k > chi2, 'chi2() stays plain under a loss'
    assert abs(chi_k - chi0) <= tol * chi0
    if not with_omega:
        return p
    # STEP 3
    delta1 = orc.potr(JTJ0 + np.diag(np.diag(JTJ0)), JTr0)
    om0, jto0 = p.omega(delta1, JT0)
    jto = ctx.omega(p.pars, delta1)
    om = ctx.omega_vector()
    # convergence reductions (gadfit.F90:849, 865-873) with res from chi2 at shifted parameters
    g = ctx.aux(0, dim=dim)
    s3 = ctx.aux(1, delta1=delta1)
    jd = JT0 @ delta1
    _observe(omega=np.max(np.abs(om - om0)) / max(1e-300, np.max(np.abs(om0))), JTomega=np.max(np.abs(jto - jto0)) / np.max(np.abs(jto0)),
             grad=np.max(np.abs(g - JT0.T @ res_c)) / np.max(np.abs(JTr0)), cosphi=rel(s3, [res_c @ jd, res_c @ res_c, jd @ jd]))
    assert np.max(np.abs(om - om0)) <= otol * max(1e-300, np.max(np.abs(om0)))
    assert np.max(np.abs(jto - jto0)) <= otol * np.max(np.abs(jto0))
    assert np.max(np.abs(g - JT0.T @ res_c)) <= otol * np.max(np.abs(JTr0))
    assert rel(s3, [res_c @ jd, res_c @ res_c, jd @ jd]) < otol
    return p
