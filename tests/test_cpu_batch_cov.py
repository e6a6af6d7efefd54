"""CPU tests of the errors of a batch (gfh_batch_covariance, gfh_fit_batch_errors; the kernel gfh_k_batch_cov): the generated source
and its compilation for gfx950 on compile-only contexts, every refusal by its message, and -- without a GPU -- the reference of
tests/test_gpu_batch_cov.py, the rule that selects what is held against it and the host yardstick of the kernel's algebra
(tests/batch_cov_cases.py)."""
import ctypes as C
import re

import numpy as np
import pytest

from gadfit_amd import _lib
from gadfit_amd.ad import trace_model
from tests import batch_cov_cases as CV
from tests import models as M


@pytest.mark.parametrize('lanes', (64, 16, 256))
@pytest.mark.parametrize('model,n', [(M.model_exp2, 4), (M.model_exp4, 8)])
def test_the_kernel_is_in_every_batch_unit_and_in_no_other(model, n, lanes):
    c = _lib.Context(-1)
    try:
        c.set_model(trace_model(model, n))
        c.set_batch_lanes(lanes)
        active = list(range(n))
        plain = c.model_source(active)
        src = c.batch_source(active)
        assert src.count('void gfh_k_batch_cov(') == 1 and 'gfh_k_batch_cov' not in plain
        assert src.index('void gfh_k_batch_pass(') < src.index('void gfh_k_batch_cov(')          # behind batch_fit.hip
        tail = re.sub(r'//[^\n]*', '', src[src.index('void gfh_k_batch_cov('):])                  # (the code, not what its comments say)
        assert 'atomic' not in tail and 'asm' not in tail and '__shared__' not in tail and '__syncthreads' not in tail
        assert tail.count('gfh_b_sweep(') == 1          # the one call: the 256-lane form's one barrier
        if lanes != 256:
            whole = re.sub(r'//[^\n]*', '', src[src.index('#define GFH_BATCH 1'):])
            assert '__syncthreads' not in whole and '__shared__' not in whole and 'atomic' not in whole and 'asm' not in whole
        c.batch_prepare(active)                          # hiprtc compile for gfx950
        assert c.model_source(active) == plain           # the default translation unit is what it was
    finally:
        c.close()


def test_a_cube_form_compiles_with_the_kernel():
    c = _lib.Context(-1)
    try:
        c.set_model(trace_model(M.model_exp2, 4))
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_cube(np.arange(1.0, 9.0), np.ones((3, 8), dtype=np.uint16), 1)
        src = c.batch_source(CV.ACTIVE)
        assert '#define GFH_BCUBE 1' in src and src.count('void gfh_k_batch_cov(') == 1
        c.batch_prepare(CV.ACTIVE)
    finally:
        c.close()


def _ctx(model=M.model_exp2, n=4):
    c = _lib.Context(-1)
    c.set_model(trace_model(model, n))
    return c


def _data(c, sizes=(10, 12, 9)):
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    with pytest.raises(_lib.GadfitHipError, match='no GPU'):
        c.set_batch_data(off, np.linspace(0.5, 9.5, n), np.ones(n), np.ones(n))
    return len(sizes)


def test_valid_calls_end_at_the_missing_gpu():
    c = _ctx()
    try:
        start = np.tile(M.EXP2_TRUTH, (_data(c), 1))
        for scale in (False, True):
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                c.batch_covariance(start, CV.ACTIVE, scale=scale)
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                c.fit_batch_errors(start, CV.ACTIVE, scale=scale, lambda_=1.0, max_iter=5, chi2_rel=1e-6, accth=0.9, DTD_min=[1.0] * 4)
    finally:
        c.close()


def test_scale_nulls_and_the_shared_refusals_under_the_new_names():
    c = _ctx()
    try:
        start3 = np.tile(M.EXP2_TRUTH, (3, 1))
        with pytest.raises(_lib.GadfitHipError, match='batch_covariance: no batch data'):
            c.batch_covariance(start3, [0, 1])
        _data(c)
        for bad in (2, -1):
            with pytest.raises(_lib.GadfitHipError, match=r'gfh_batch_covariance: scale is 0 .* or 1 .*, got %d' % bad):
                c.batch_covariance(start3, CV.ACTIVE, scale=bad)
            with pytest.raises(_lib.GadfitHipError, match=r'gfh_fit_batch_errors: scale is 0 .* or 1 .*, got %d' % bad):
                c.fit_batch_errors(start3, CV.ACTIVE, scale=bad, max_iter=1)
        # a null output, each in turn: the C entries directly
        p = start3.copy(); a = np.array(CV.ACTIVE, dtype=np.int32)
        cov = np.zeros((3, 4, 4)); sig = np.zeros((3, 4)); info = np.zeros(3, dtype=np.int32)
        res = np.zeros(3, dtype=_lib.BATCH_RESULT_DTYPE)
        o = _lib.FitOptions(); o.max_iter = 1; o.has_max_iter = 1
        outs = (_lib.dp(cov), _lib.dp(sig), _lib.ip(info))
        for k in range(3):
            args = [None if j == k else v for j, v in enumerate(outs)]
            with pytest.raises(_lib.GadfitHipError, match='gfh_batch_covariance: null argument'):
                c._chk(_lib.lib().gfh_batch_covariance(c._h, _lib.dp(p), 4, _lib.ip(a), 0, *args))
            with pytest.raises(_lib.GadfitHipError, match='gfh_fit_batch_errors: null argument'):
                c._chk(_lib.lib().gfh_fit_batch_errors(c._h, _lib.dp(p), 4, _lib.ip(a), C.byref(o), res.ctypes.data_as(C.POINTER(_lib.BatchResult)),
                                                       0, *args, None))
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_covariance: null argument'):
            c._chk(_lib.lib().gfh_batch_covariance(c._h, None, 4, _lib.ip(a), 0, *outs))
        # the checks gfh_batch_pass and gfh_fit_batch make, with their wording
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_covariance: an active parameter is listed twice'):
            c.batch_covariance(start3, [1, 1])
        with pytest.raises(_lib.GadfitHipError, match='active parameter indices'):
            c.batch_covariance(start3, [0, 4])
        with pytest.raises(_lib.GadfitHipError, match='n_fits x n_pars = 3 x 4'):
            c.fit_batch_errors(np.ones((2, 4)), [0, 1], max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='gfh_fit_batch_errors: max_iter is required'):
            c.fit_batch_errors(start3, CV.ACTIVE, chi2_rel=1e-6)
        with pytest.raises(_lib.GadfitHipError, match='gfh_fit_batch_errors: uphill'):
            c.fit_batch_errors(start3, CV.ACTIVE, max_iter=1, uphill=1)
        with pytest.raises(_lib.GadfitHipError, match="fit_batch_errors: unknown fit argument 'max_iters'"):
            c.fit_batch_errors(start3, [0, 1], max_iters=1)
        with pytest.raises(_lib.GadfitHipError, match='fit_batch_errors: DTD_min must hold one value per active parameter'):
            c.fit_batch_errors(start3, [0, 1], DTD_min=[1.0], max_iter=1)
        _data(c, sizes=(10, 3, 9))
        for call in (lambda: c.batch_covariance(start3, CV.ACTIVE), lambda: c.fit_batch_errors(start3, CV.ACTIVE, max_iter=1)):
            with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
                call()
        c.set_loss(1)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_covariance: a robust loss'):
            c.batch_covariance(start3, [0, 1, 2])
        with pytest.raises(_lib.GadfitHipError, match='gfh_fit_batch_errors: a robust loss'):
            c.fit_batch_errors(start3, [0, 1, 2], max_iter=1)
    finally:
        c.close()
    c = _ctx(M.model_gauss8, 32)
    try:
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_covariance: more than 8 active parameters'):
            c.batch_covariance(np.ones((3, 32)), list(range(9)))
    finally:
        c.close()
    # frames that have not been put
    c = _ctx()
    try:
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.batch_frames_begin(np.arange(1.0, 9.0), 3, np.uint16, 1)
        with pytest.raises(_lib.GadfitHipError, match=r'gfh_batch_covariance: 8 of 8 frames of the batch begun by gfh_batch_frames_begin have not been put'):
            c.batch_covariance(np.tile(M.EXP2_TRUTH, (3, 1)), CV.ACTIVE)
    finally:
        c.close()


def test_the_errors_argument_of_the_session_calls():
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    x = np.linspace(0.5, 9.5, 10)
    gf.gadf_close()
    gf.gadf_init(exp2())
    try:
        for k in range(4):
            gf.gadf_set(k + 1, float(M.EXP2_TRUTH[k]), True)
        for bad in ('x', 'Scaled', True, 1):
            with pytest.raises(gf.GadfitError, match=r"gadf_fit_batch: errors must be None, 'unscaled' .* or 'scaled'"):
                gf.gadf_fit_batch([x], [x], None, [M.EXP2_TRUTH], max_iter=1, errors=bad)
        with pytest.raises(gf.GadfitError, match='gadf_fit_cube: errors must be None'):
            gf.gadf_fit_cube(x, np.ones((1, 10)), [M.EXP2_TRUTH], max_iter=1, errors='x')
        with pytest.raises(gf.GadfitError, match='gadf_fit_frames: errors must be None'):
            gf.gadf_fit_frames(x, np.ones((10, 1)), [M.EXP2_TRUTH], max_iter=1, errors='x')
    finally:
        gf.gadf_close()


def test_the_rule_keeps_and_drops_what_the_cases_say():
    """kappa_2 of the oracle's J^T J scaled to unit diagonal, per comparison; printed, and the counts held"""
    n = CV.part1()[3].n
    for part, active in CV.all_sets():
        k = np.array([m[2] for m in CV.oracle_matrices(part, active)])
        keep = CV.kept(part, active)
        print('part %d %s: kept %d, dropped %d, kappa of the kept <= %.3g' % (part, list(active), keep.sum(), (~keep).sum(), k[keep].max()))
        if (part, list(active)) == (1, CV.ACTIVE):
            assert {int(L): int(np.sum(~keep & (n == L))) for L in CV.LENGTHS if np.any(~keep & (n == L))} == CV.DROPPED
            assert k[keep & (n == 8)].max() <= 1.8e7 and k[keep & (n >= 16) & (n <= 17)].max() <= 1.8e3 and k[n >= 63].max() <= 30.0
            assert 2.7e9 < k[~keep & (n == 6)].max() < 2.9e9 and 1.7e14 < k.max() < 1.9e14
        else:
            assert keep.all()
            assert k.max() <= 3.6e3
    # the short rows stay covered: one-parameter fits of 4, 5 and 6 points are kept
    one = CV.kept(1, CV.ONE_ACTIVE)
    assert all(np.sum(one & (n == L)) == CV.SAMPLES for L in (4, 5, 6))


def test_the_host_yardstick_of_the_algebra():
    """r_host: the kernel's algebra in plain doubles against the longdouble inverse, over the kept matrices, in units of eps kappa_2.
    Its bound here is reasoning, not observation: in the 1 x 1 case C = (1 / sqrt(a))^2 makes three roundings of relative size
    eps / 2 each, of which the first two are doubled by the square: (2 + 2 + 1) eps / 2 = 2.5 eps at kappa_2 = 1, and the 1 x 1 fits
    are where the ratio is largest (observed 1.63 there, at most 0.63 on the larger matrices, whose errors are far from the
    worst case eps kappa_2 allows)."""
    for key, r in CV.host_ratios().items():
        print('%s: max err / (eps kappa) = %.3f over %d kept fits' % (key, max(r), len(r)))
    print('r_host = %.4f' % CV.r_host())
    assert 0.0 < CV.r_host() <= 2.5
    # the longdouble inverse is one: A C_ref - I at the longdouble's own rounding level, scaled by the condition
    for part, active in ((1, tuple(CV.ACTIVE)), (2, tuple(range(8)))):
        for A, _, k in CV.oracle_matrices(part, active):
            if k <= CV.KAPPA_MAX:
                d = CV.scale_of(A)
                R = (np.asarray(A, dtype=np.longdouble) @ CV.longdouble_inverse(A)) - np.eye(A.shape[0], dtype=np.longdouble)
                assert CV.norm2(R) <= 64 * float(np.finfo(np.longdouble).eps) * k * A.shape[0] * CV.norm2(CV.scaled(A, d)) * (d.max() / d.min())


def test_the_singular_spectrum_is_one_for_the_oracle():
    tape, _, starts, _ = CV.part1()
    A, _ = CV.oracle_pass(tape, CV.singular_item(), starts[0], CV.ACTIVE)
    assert np.linalg.matrix_rank(A) == 1 and A[1, 1] == 0.0 and A[3, 3] == 0.0 and A[0, 0] > 0.0
    C_, info = CV.host_cholesky_inverse(A)
    assert C_ is None and info == 2 and CV.kappa(A) == float('inf')
    A, _ = CV.oracle_pass(tape, CV.nan_item(), starts[0], CV.ACTIVE)
    assert CV.host_cholesky_inverse(A) == (None, 1)
