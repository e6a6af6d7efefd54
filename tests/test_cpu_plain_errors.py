"""CPU tests of the errors and the curves of a plain fit (gfh_covariance, gfh_fit_errors, gfh_invert_normal, gfh_eval; the kernels of
device/eval.hip): the host algebra against the longdouble inverse, dense and block-arrow, and as a stand-alone program under
AddressSanitizer and UBSan; the generated source of the eval translation unit and its compilation for gfx950 on compile-only
contexts; every refusal by its message; and -- without a GPU -- the rule that selects what tests/test_gpu_plain_errors.py holds
against the oracle and the host yardstick of the algebra (tests/plain_errors_cases.py).

oracle/binding.py exposes the reference's potr (dpotrf + dpotrs) alone, not its packed dpptrf / dpptri: nothing here is compared with
those."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gadfit_amd import _lib
from gadfit_amd.ad import trace_model
from tests import batch_cov_cases as CV
from tests import models as M
from tests import plain_errors_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin', 'clang++')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1: the algebra ------------------------------------------------------------------------------------------------------------------
def test_the_rule_keeps_every_case():
    """kappa_2 of the oracle's J^T J scaled to unit diagonal, per case; printed, and every case is kept -- the GPU module leaves out
    none of them"""
    for c in PC.all_cases():
        _, _, k, _, dim = PC.oracle_pass(c.name)
        print('%s: dim %d, kappa %.3g' % (c.name, dim, k))
        assert k <= PC.KAPPA_MAX, (c.name, k)
    assert PC.oracle_pass('exp2_4')[2] <= 30.0 and 1e7 < PC.oracle_pass('gauss8')[2] < 1e8


def test_the_host_yardstick_of_the_algebra():
    """r_host of the library's own host code: err(gfh_invert_normal, longdouble inverse) / (eps kappa_2) over the synthetic matrices
    and the cases' oracle matrices, dense and with the structure on.  Observed 1.47 (model_global7's pattern over 40 datasets taken
    densely, dim 163; at most 0.55 elsewhere).  The bound here is reasoning, not observation: the inverse through a Cholesky factor
    has an error of c n eps kappa_2 with a modest c (Higham, Accuracy and Stability, 14.3), so no ratio may exceed its matrix's dim."""
    dims = {label: dim for label, _, dim, _ in PC.synthetic()}
    dims.update({c.name: PC.oracle_pass(c.name)[4] for c in PC.all_cases()})
    for (label, s), r in PC.host_ratios().items():
        print('%s %s: err / (eps kappa) = %.3f' % (label, 'structure' if s else 'dense', r))
        assert 0.0 <= r <= dims[label], (label, s, r)
    print('r_host = %.4f' % PC.r_host())
    assert PC.r_host() > 0.0


def test_dense_and_arrow_against_the_longdouble_inverse():
    r_host = PC.r_host()
    for label, jac, dim, A in PC.synthetic():
        k = CV.kappa(A)
        assert k <= PC.KAPPA_MAX
        d = CV.scale_of(A)
        ref = CV.longdouble_inverse(A)
        bound = 10.0 * r_host * PC.EPS * k
        got = {}
        for s in (False, True):
            cov, sigma, info, form = _lib.invert_normal(jac, dim, A, s)
            assert info == 0
            # the arrow form where it applies -- several datasets, dim above 16, half the columns local -- and only when asked for
            assert form == (1 if s and label == 'global7x40' else 0), (label, s, form)
            assert np.array_equal(_bits(cov), _bits(cov.T)) and np.array_equal(_bits(sigma), _bits(np.sqrt(np.diag(cov))))
            err = CV.scaled_error(cov, ref, d)
            res, na_, nc_ = CV.residual(cov, A, d)
            print('%s %s: err %.2e, bound %.2e, residual %.2e' % (label, 'arrow' if form else 'dense', err, bound, res))
            assert err <= bound and res <= bound * na_ * nc_, (label, s)
            got[s] = cov
        assert CV.scaled_error(got[True], got[False], d) <= bound          # the two forms of one matrix, within the bound of each other
    assert not np.array_equal(*[_lib.invert_normal(*PC.global7_pattern(40)[:3], s)[0] for s in (False, True)])      # (they are two forms)


def test_singular_and_nan_matrices_give_info_and_nan_throughout():
    tape, _, starts, _ = CV.part1()
    A, _ = CV.oracle_pass(tape, CV.singular_item(), starts[0], CV.ACTIVE)          # an exact zero on the diagonal: pivot 1
    jac = np.arange(4, dtype=np.int32)[None, :]
    cov, sigma, info, _ = _lib.invert_normal(jac, 4, A)
    assert info == 2 and np.all(np.isnan(cov)) and np.all(np.isnan(sigma))
    A, _ = CV.oracle_pass(tape, CV.nan_item(), starts[0], CV.ACTIVE)
    cov, sigma, info, _ = _lib.invert_normal(jac, 4, A)
    assert info == 1 and np.all(np.isnan(cov)) and np.all(np.isnan(sigma))
    B = np.diag([1.0, np.inf, 1.0])                                                 # a pivot that is positive but not finite
    assert _lib.invert_normal(np.arange(3, dtype=np.int32)[None, :], 3, B)[2] == 2
    # both forms of a global fit: a local column of dataset 5 zeroed, and a global one
    jac, dim, A = PC.global7_pattern(40)
    for col in (int(jac[5, 1]), int(jac[0, 6])):
        bad = A.copy(); bad[col, :] = 0.0; bad[:, col] = 0.0
        for s in (False, True):
            cov, sigma, info, form = _lib.invert_normal(jac, dim, bad, s)
            assert form == int(s) and info == col + 1 and np.all(np.isnan(cov)) and np.all(np.isnan(sigma)), (col, s, info)


def test_the_factor_multiplies_every_entry_bit_for_bit():
    for label, jac, dim, A in PC.synthetic():
        for s in (False, True):
            c0, s0, _, _ = _lib.invert_normal(jac, dim, A, s)
            f = 886.4 / 796.0                                                       # a chi2 / dof
            c1, s1, info, _ = _lib.invert_normal(jac, dim, A, s, factor=f)
            assert info == 0 and np.array_equal(_bits(c1), _bits(c0 * f)) and np.array_equal(_bits(s1), _bits(np.sqrt(np.diag(c1))))
    with pytest.raises(_lib.GadfitHipError, match='gfh_invert_normal: Jacobian index out of range'):
        _lib.invert_normal(np.array([[0, 4]], dtype=np.int32), 4, np.eye(4))
    with pytest.raises(_lib.GadfitHipError, match='invert_normal: jac_idx must be'):
        _lib.invert_normal(np.array([[0, 1]], dtype=np.int32), 4, np.eye(3))


@pytest.mark.skipif(not os.path.exists(CLANG), reason='no ROCm clang')
def test_the_inverse_as_a_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    csrc = os.path.join(ROOT, 'gadfit_amd', 'csrc')
    exe = str(tmp_path / 'normal_eq_invert_main')
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-I' + csrc,
                    os.path.join(ROOT, 'tests', 'host', 'normal_eq_invert_main.cpp'), os.path.join(csrc, 'normal_eq.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == ''


# ---- 2: the translation unit ---------------------------------------------------------------------------------------------------------
def _units():
    """(label, tape, active, use_ad) of every unit compiled here: the cases of the GPU module and the active counts beyond them"""
    out = [('exp2', PC.exp2(4).tape, [0, 1, 2, 3], True), ('exp4', trace_model(M.model_exp4, 8), list(range(8)), True),
           ('exp4_6_1_4', trace_model(M.model_exp4, 8), [6, 1, 4], True), ('exp4_1_4_6', trace_model(M.model_exp4, 8), [1, 4, 6], True),
           ('gauss3', trace_model(M.make_model_gaussK(3), 12), list(range(12)), True), ('gauss8', PC.gauss8().tape, list(range(32)), True),
           ('gauss9', trace_model(M.make_model_gaussK(9), 36), list(range(36)), True), ('global7', PC.global7().tape, PC.GLOBAL7_ACTIVE, True),
           ('piecewise2', PC.piecewise2().tape, [0, 1, 2, 3], True), ('aux', PC.auxiliary().tape, [0, 1, 2], True)]
    return out + [(label + '_fd', tape, active, False) for label, tape, active, _ in out if label in ('exp2', 'piecewise2', 'aux')]


@pytest.mark.parametrize('label,tape,active,use_ad', _units(), ids=[u[0] for u in _units()])
def test_the_eval_unit_compiles_for_gfx950_and_the_default_unit_is_unchanged(label, tape, active, use_ad):
    c = _lib.Context(-1)
    try:
        c.set_model(tape)
        c.set_use_ad(use_ad)
        plain = c.model_source(active)
        src = c.eval_source(active)
        assert 'gfh_k_eval' not in plain and 'GFH_EVAL' not in plain
        for k in ('gfh_k_eval', 'gfh_k_eval_band'):
            assert src.count('void %s(' % k) == 1
        grid = label.split('_')[0] not in ('piecewise2', 'aux')          # a grid carries one recorded path and no auxiliary columns
        assert ('#define GFH_EVAL_GRID %d' % grid) in src
        assert '#define GFH_NA %d' % len(active) in src
        for k in ('gfh_k_sweep', 'gfh_k_sweep_gram', 'gfh_k_chi2', 'gfh_k_omega'):          # the kernels of a fit are not in it
            assert 'void %s(' % k not in src
        tail = re.sub(r'//[^\n]*', '', src[src.index('#define GFH_EVAL 1'):])                 # (the code, not what its comments say)
        assert 'atomic' not in tail and 'asm' not in tail and '__shared__' not in tail and '__syncthreads' not in tail
        c.eval_prepare(active)                           # hiprtc compile for gfx950
        assert c.model_source(active) == plain           # the default translation unit is what it was
    finally:
        c.close()


def test_the_compilers_figures_no_scratch_and_no_lds():
    """the four kernels of the headline unit (model_gauss8, 32 active) and of model_exp2 as hipcc compiles them for gfx950: no scratch
    (a parameter block or a covariance block copied to the stack would show here) and no LDS; the figures themselves are recorded in
    profiles/plain_eval.json by tools/bench_eval.py --registers"""
    from tools import bench_eval as BE
    c = _lib.Context(-1)
    try:
        for tape, active in ((PC.exp2(4).tape, [0, 1, 2, 3]), (PC.gauss8().tape, list(range(32)))):
            c.set_model(tape)
            figs = BE.kernel_registers(c.eval_source(active))
            assert sorted(figs) == ['gfh_k_eval', 'gfh_k_eval_band', 'gfh_k_eval_grid', 'gfh_k_eval_grid_band']
            for name, f in figs.items():
                print(len(active), name, f)
                assert f['scratch_bytes_per_lane'] == 0 and f['lds_bytes_per_block'] == 0 and f['vgprs'] <= 128, (name, f)
    finally:
        c.close()
    rec = BE.load_record()
    assert sorted(rec['registers']) == sorted(BE.REGISTER_UNITS)


# ---- 3: refusals ---------------------------------------------------------------------------------------------------------------------
def _ctx(tape=None, n=4):
    c = _lib.Context(-1)
    c.set_model(tape if tape is not None else trace_model(M.model_exp2, n))
    c.nd = 1
    return c


def test_covariance_refusals_and_the_missing_gpu():
    c = _ctx()
    try:
        p = np.array([M.EXP2_TRUTH])
        with pytest.raises(_lib.GadfitHipError, match='covariance: pars must hold n_datasets x n_pars = 1 x 4'):
            c.covariance(np.ones((1, 3)), [0, 1], [0] * 4)
        with pytest.raises(_lib.GadfitHipError, match='covariance: is_global must hold one flag per parameter'):
            c.covariance(p, [0, 1], [0] * 3)
        with pytest.raises(_lib.GadfitHipError, match='covariance: active parameter indices'):
            c.covariance(p, [0, 4], [0] * 4)
        for bad in (2, -1):
            with pytest.raises(_lib.GadfitHipError, match=r'gfh_covariance: scale is 0 .* or 1 .*, got %d' % bad):
                c.covariance(p, [0, 1], [0] * 4, scale=bad)
            with pytest.raises(_lib.GadfitHipError, match=r'gfh_fit_errors: scale is 0 .* or 1 .*, got %d' % bad):
                c.fit_errors(p, [0, 1], [0] * 4, scale=bad, max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='gfh_covariance: an active parameter is listed twice'):
            c.covariance(p, [1, 1], [0] * 4)
        # a null output, each in turn: the C entries directly
        a = np.array([0, 1], dtype=np.int32); g = np.zeros(4, dtype=np.int32)
        cov = np.zeros((2, 2)); sig = np.zeros(2); info = np.zeros(1, dtype=np.int32)
        outs = (_lib.dp(cov), _lib.dp(sig), _lib.ip(info))
        for k in range(3):
            args = [None if j == k else v for j, v in enumerate(outs)]
            with pytest.raises(_lib.GadfitHipError, match='gfh_covariance: null argument'):
                c._chk(_lib.lib().gfh_covariance(c._h, _lib.dp(p), 2, _lib.ip(a), _lib.ip(g), 0, *args))
            with pytest.raises(_lib.GadfitHipError, match='gfh_fit_errors: null argument'):
                c._chk(_lib.lib().gfh_fit_errors(c._h, _lib.dp(p), 2, _lib.ip(a), _lib.ip(g), None, None, 0, *args))
        with pytest.raises(_lib.GadfitHipError, match='There are no active parameters'):
            c._chk(_lib.lib().gfh_covariance(c._h, _lib.dp(p), 0, _lib.ip(a), _lib.ip(g), 0, *outs))
        for scale in (False, True):                      # a well-formed call gets as far as the device
            with pytest.raises(_lib.GadfitHipError, match='no GPU bound'):
                c.covariance(p, [0, 1, 2, 3], [0] * 4, scale=scale)
            with pytest.raises(_lib.GadfitHipError, match='no GPU bound'):
                c.fit_errors(p, [0, 1, 2, 3], [0] * 4, scale=scale, max_iter=1)
    finally:
        c.close()
    c = _lib.Context(-1)
    try:
        c.n_pars, c.nd = 4, 1
        with pytest.raises(_lib.GadfitHipError, match='gfh_covariance: no model set'):
            c.covariance(np.ones((1, 4)), [0], [0] * 4)
    finally:
        c.close()


def test_eval_refusals_and_the_missing_gpu():
    c = _ctx()
    try:
        p = np.array([M.EXP2_TRUTH]); act = [0, 1, 2, 3]; g = [0] * 4
        cov = np.eye(4)
        with pytest.raises(_lib.GadfitHipError, match='eval: pars must hold n_datasets x n_pars = 1 x 4'):
            c.eval(np.ones((1, 5)), act, g)
        with pytest.raises(_lib.GadfitHipError, match='eval: cov must hold dim x dim = 4 x 4'):
            c.eval(p, act, g, cov=np.eye(3))
        with pytest.raises(_lib.GadfitHipError, match='gfh_eval: no output requested'):
            c.eval(p, act, g, model=False)
        with pytest.raises(_lib.GadfitHipError, match="gfh_eval: a residual on a caller's grid has no meaning"):
            c.eval(p, act, g, x_eval=[1.0, 2.0], residuals=True)
        with pytest.raises(_lib.GadfitHipError, match='gfh_eval: an active parameter is listed twice'):
            c.eval(p, [2, 2], g)
        # through the C entry: what the Python layer cannot express
        a = np.array(act, dtype=np.int32); jac = np.arange(4, dtype=np.int32); out = np.zeros(8); xe = np.ones(2)
        L = _lib.lib()

        def call(pars=_lib.dp(p), jac_=_lib.ip(jac), dim=4, cov_=None, x=None, n=0, m=_lib.dp(out), r=None, b=None):
            c._chk(L.gfh_eval(c._h, pars, 4, _lib.ip(a), jac_, dim, cov_, x, n, m, r, b, None))
        with pytest.raises(_lib.GadfitHipError, match=r'gfh_eval: null argument \(pars is required\)'):
            call(pars=None)
        with pytest.raises(_lib.GadfitHipError, match="gfh_eval: a band needs the fit's covariance"):
            call(b=_lib.dp(out))
        with pytest.raises(_lib.GadfitHipError, match='gfh_eval: a band needs the column map'):
            call(b=_lib.dp(out), cov_=_lib.dp(cov), jac_=None)
        with pytest.raises(_lib.GadfitHipError, match=r'gfh_eval: a grid holds at least one point \(x_eval given with n_eval = 0\)'):
            call(x=_lib.dp(xe), n=0)
        with pytest.raises(_lib.GadfitHipError, match='gfh_eval: n_eval = 2 without x_eval'):
            call(n=2)
        for kw in (dict(), dict(cov=cov), dict(residuals=True), dict(cov=cov, x_eval=[1.0, 2.0, 3.0])):      # well-formed calls reach the device
            with pytest.raises(_lib.GadfitHipError, match='no GPU bound'):
                c.eval(p, act, g, **kw)
    finally:
        c.close()
    # what no eval unit exists for, under the three names
    from gadfit_amd.ad import integrate
    t = trace_model(lambda q, x: integrate(lambda u, r: r[0] * u, [q[0]], 0.0, x), 1)
    c = _ctx(t)
    try:
        for name, call in (('gfh_eval', lambda: c.eval(np.ones((1, 1)), [0], [0])), ('gfh_eval_source', lambda: c.eval_source([0])),
                           ('gfh_eval_prepare', lambda: c.eval_prepare([0]))):
            with pytest.raises(_lib.GadfitHipError, match=name + r': models with integrate\(\) are not carried'):
                call()
    finally:
        c.close()
    for case, what in ((PC.piecewise2(), 'variant tapes'), (PC.auxiliary(), 'auxiliary per-point columns')):
        c = _ctx(case.tape)
        try:
            with pytest.raises(_lib.GadfitHipError, match='gfh_eval: on a grid, models .*' + what):
                c.eval(case.pars, case.active, case.is_global, x_eval=[1.0, 2.0])
            with pytest.raises(_lib.GadfitHipError, match='no GPU bound'):          # on the data's own points they are carried
                c.eval(case.pars, case.active, case.is_global)
        finally:
            c.close()
    # a band beyond 64 active parameters is refused with the count; the model alone is not
    t = trace_model(M.make_model_gaussK(17), 68)
    c = _ctx(t)
    try:
        p = np.ones((1, 68)); act = list(range(68))
        with pytest.raises(_lib.GadfitHipError, match='gfh_eval: a band is carried up to 64 active parameters per dataset, got 68'):
            c.eval(p, act, [0] * 68, cov=np.eye(68))
        with pytest.raises(_lib.GadfitHipError, match='no GPU bound'):
            c.eval(p, act, [0] * 68)
    finally:
        c.close()
    # group handles and contexts that are one of several ranks
    grp = _lib.Context(devices=[-1, -1])
    try:
        grp.set_model(trace_model(M.model_exp2, 4)); grp.nd = 1
        with pytest.raises(_lib.GadfitHipError, match='gfh_eval is not available on a device-group handle'):
            grp.eval(np.array([M.EXP2_TRUTH]), [0, 1], [0] * 4)
        with pytest.raises(_lib.GadfitHipError, match='gfh_eval_prepare is not available on a device-group handle'):
            grp.eval_prepare([0, 1])
    finally:
        grp.close()
    c = _ctx()
    try:
        c.debug_set_rank(2, 1)
        with pytest.raises(_lib.GadfitHipError, match='gfh_eval: a context that is one of 2 ranks is not carried'):
            c.eval(np.array([M.EXP2_TRUTH]), [0, 1], [0] * 4)
    finally:
        c.close()


def test_the_session_calls_check_their_session():
    import gadfit_amd
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp
    assert gadfit_amd.gadf_errors is gf.gadf_errors and gadfit_amd.gadf_curves is gf.gadf_curves

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    gf.gadf_close()
    for call in (gf.gadf_errors, gf.gadf_curves):
        with pytest.raises(gf.GadfitError, match='Call gadf_init first'):
            call()
    gf.gadf_init(exp2(), 2)
    try:
        for call in (gf.gadf_errors, gf.gadf_curves):
            with pytest.raises(gf.GadfitError, match='There are no active parameters'):
                call()
        gf.gadf_set(1, 1.0, True)
        for call in (gf.gadf_errors, gf.gadf_curves):
            with pytest.raises(gf.GadfitError, match='Some datasets are missing'):
                call()
    finally:
        gf.gadf_close()
