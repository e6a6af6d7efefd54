"""CPU tests of batched independent fits (gfh_set_batch_data, gfh_fit_batch, gfh_batch_pass): the generated source and its
compilation for gfx950 on compile-only contexts, and every refusal -- arguments, options and the model are checked before the device
is asked for, so each message can be provoked without a GPU; a well-formed call gets as far as the device and ends in `no GPU`."""
import ctypes as C

import numpy as np
import pytest

from gadfit_amd import _lib, ad
from gadfit_amd import tape as T
from gadfit_amd.ad import trace_model
from tests import branching as B
from tests import models as M
from tests.golden import goldens as G


@pytest.mark.parametrize('model,n', [(M.model_exp2, 4), (M.model_exp4, 8)])
def test_batch_kernels_are_a_translation_unit_of_their_own(model, n):
    c = _lib.Context(-1)
    try:
        c.set_model(trace_model(model, n))
        active = list(range(n))
        plain = c.model_source(active)
        src = c.batch_source(active)
        assert 'gfh_k_fit_batch' in src and 'gfh_k_batch_pass' in src
        assert 'gfh_k_fit_batch' not in plain and 'gfh_k_batch_pass' not in plain and 'GFH_BATCH' not in plain
        # the two kernels sit BEHIND the model's point functions: no second lowering of the tape
        for fn in ('gfh_point_grad', 'gfh_point_value', 'gfh_point_dd_grad'):
            assert src.count('static __device__ __forceinline__ double ' + fn + '(') + \
                src.count('static __device__ __forceinline__ void ' + fn + '(') == 1
        # waves of a workgroup never talk to each other
        import re
        tail = re.sub(r'//[^\n]*', '', src[src.index('#define GFH_BATCH 1'):])          # (the code, not what its comments say)
        assert '__syncthreads' not in tail and '__shared__' not in tail and 'atomic' not in tail and 'asm' not in tail
        c.batch_prepare(active)                     # hiprtc compile for gfx950
        assert c.model_source(active) == plain      # ... and the default translation unit is what it was
    finally:
        c.close()


def test_a_subset_of_the_parameters_can_be_active():
    c = _lib.Context(-1)
    try:
        c.set_model(trace_model(M.model_exp4, 8))
        src = c.batch_source([1, 4, 6])
        assert '#define GFH_BACT {1, 4, 6}' in src and '#define GFH_NA 3' in src
        c.batch_prepare([1, 4, 6])
    finally:
        c.close()


def _ctx(model=M.model_exp2, n=4):
    c = _lib.Context(-1)
    c.set_model(trace_model(model, n))
    return c


def _data(c, sizes=(10, 12, 9)):
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    with pytest.raises(_lib.GadfitHipError, match='no GPU'):       # a well-formed batch gets as far as the device; its geometry is kept
        c.set_batch_data(off, np.linspace(0.5, 9.5, n), np.ones(n), np.ones(n))
    return len(sizes)


def test_valid_calls_end_at_the_missing_gpu():
    c = _ctx()
    try:
        nf = _data(c)
        start = np.tile(M.EXP2_TRUTH, (nf, 1))
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.fit_batch(start, [0, 1, 2, 3], lambda_=1.0, max_iter=5, chi2_rel=1e-6, accth=0.9)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.batch_pass(start, [0, 1, 2, 3])
    finally:
        c.close()


def test_data_and_argument_refusals():
    c = _ctx()
    try:
        start3 = np.tile(M.EXP2_TRUTH, (3, 1))
        with pytest.raises(_lib.GadfitHipError, match='no batch data'):
            c.fit_batch(start3, [0, 1], max_iter=1)
        x = np.linspace(0.5, 9.5, 20)
        with pytest.raises(_lib.GadfitHipError, match='offsets must ascend'):
            c.set_batch_data([0, 12, 8, 20], x, x, x)
        with pytest.raises(_lib.GadfitHipError, match='offsets must begin at 0'):
            c.set_batch_data([2, 12, 20], x, x, x)
        with pytest.raises(_lib.GadfitHipError, match=r'offsets\[-1\] = 20 values each'):
            c.set_batch_data([0, 12, 20], x, x, x[:19])
        with pytest.raises(_lib.GadfitHipError, match='at least one fit'):      # (the binding refuses an empty batch itself: the C entry directly)
            off0 = np.zeros(1, dtype=np.int64)
            c._chk(_lib.lib().gfh_set_batch_data(c._h, 0, off0.ctypes.data_as(C.POINTER(C.c_int64)), _lib.dp(x), _lib.dp(x), _lib.dp(x)))
        # a fit with fewer points than active parameters: per fit, as gadfit.F90:648-657 per problem
        _data(c, sizes=(10, 3, 9))
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.fit_batch(start3, [0, 1, 2, 3], max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.batch_pass(start3, [0, 1, 2, 3])
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):          # three active parameters fit three points
            c.fit_batch(start3, [0, 1, 2], max_iter=1)
        # lengths and ranges, before the call
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match='n_fits x n_pars = 3 x 4'):
            c.fit_batch(np.ones((2, 4)), [0, 1], max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='active parameter indices'):
            c.fit_batch(start3, [0, 4], max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='active parameter indices'):
            c.batch_pass(start3, [-1])
        with pytest.raises(_lib.GadfitHipError, match='listed twice'):
            c.fit_batch(start3, [1, 1], max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='one value per active parameter'):
            c.fit_batch(start3, [0, 1], DTD_min=[1.0], max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match="unknown fit argument 'max_iters'"):
            c.fit_batch(start3, [0, 1], max_iters=1)
    finally:
        c.close()


@pytest.mark.parametrize('kw,msg', [
    (dict(uphill=1), 'uphill'), (dict(nielsen=1), 'nielsen'), (dict(umnigh=1), 'umnigh'), (dict(grad_chi2=1e-3), 'grad_chi2'),
    (dict(cos_phi=1e-3), 'cos_phi'), (dict(rel_error_global=1e-3), 'rel_error_global'), (dict(lam_incs=0), 'lam_incs must be at least 1')])
def test_options_the_device_loop_does_not_carry_are_refused(kw, msg):
    c = _ctx()
    try:
        nf = _data(c)
        with pytest.raises(_lib.GadfitHipError, match=msg):
            c.fit_batch(np.tile(M.EXP2_TRUTH, (nf, 1)), [0, 1, 2, 3], max_iter=3, **kw)
    finally:
        c.close()


def test_the_device_loop_must_be_bounded():
    c = _ctx()
    try:
        nf = _data(c)
        with pytest.raises(_lib.GadfitHipError, match='max_iter is required'):
            c.fit_batch(np.tile(M.EXP2_TRUTH, (nf, 1)), [0, 1, 2, 3], chi2_rel=1e-6)
        # the options that ARE carried pass the checks (uphill = 0, nielsen / umnigh switched off explicitly)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.fit_batch(np.tile(M.EXP2_TRUTH, (nf, 1)), [0, 1, 2, 3], max_iter=3, uphill=0, nielsen=0, umnigh=0, lam_incs=3, lam_up=5.0,
                        lam_down=7.0, damp_max=0, chi2_abs=1e-3, rel_error=1e-6, DTD_min=[1.0] * 4)
    finally:
        c.close()


def test_models_and_contexts_a_batch_cannot_have():
    start = np.ones((3, 8))
    # more than 8 active parameters
    c = _lib.Context(-1)
    try:
        c.set_model(trace_model(M.model_gauss8, 32))
        with pytest.raises(_lib.GadfitHipError, match='more than 8 active parameters'):
            c.batch_source(list(range(9)))
        with pytest.raises(_lib.GadfitHipError, match='more than 8 active parameters'):
            c.batch_prepare(list(range(9)))
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match='more than 8 active parameters'):
            c.fit_batch(np.ones((3, 32)), list(range(9)), max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='There are no active parameters'):
            c.batch_source([])
    finally:
        c.close()
    # integrate()
    c = _lib.Context(-1)
    try:
        t = trace_model(G.model_integral_single, 2)
        t.set_integration(rel_error=1e-12)
        c.set_model(t)
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match=r'integrate\(\)'):
            c.fit_batch(np.ones((3, 2)), [0, 1], max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match=r'integrate\(\)'):
            c.batch_source([0, 1])
    finally:
        c.close()
    # variant tapes
    c = _lib.Context(-1)
    try:
        V = T.Variants(B.model_piecewise2, 4)
        V.explore([1.0, 36.0, 38.0, 99.0], B.PIECEWISE2_TRUTH)
        c.set_model(V)
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match='variant tapes'):
            c.fit_batch(np.ones((3, 4)), [0, 1], max_iter=1)
    finally:
        c.close()
    # auxiliary columns
    c = _lib.Context(-1)
    try:
        c.set_model(trace_model(lambda p, x: p[0] * ad.aux(0) + p[1], 2))
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match='auxiliary per-point columns'):
            c.batch_pass(np.ones((3, 2)), [0, 1])
    finally:
        c.close()
    # a pars hook, a robust loss, use_ad = 0, a communicator of several ranks
    hook = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double))(lambda user, target, pars: 0)
    for setup, msg in ((lambda c: c._chk(_lib.lib().gfh_set_pars_hook(c._h, C.cast(hook, C.c_void_p), None)), 'pars hook'),
                       (lambda c: c.set_loss(1), 'robust loss'), (lambda c: c.set_use_ad(False), 'use_ad = 0'),
                       (lambda c: c.debug_set_rank(2, 0), 'more than one rank')):
        c = _ctx(M.model_exp4, 8)
        try:
            _data(c)
            setup(c)
            with pytest.raises(_lib.GadfitHipError, match=msg):
                c.fit_batch(start, list(range(8)), max_iter=1)
            with pytest.raises(_lib.GadfitHipError, match=msg):
                c.batch_pass(start, list(range(8)))
        finally:
            c.close()


def _held_nothing(c):
    pass


def _held_short(c):
    _data(c, sizes=(10, 3, 9))


def _held_begun(c):          # three spectra of six frames, none of them put
    x = np.linspace(0.5, 9.5, 6)
    with pytest.raises(_lib.GadfitHipError, match='no GPU'):
        c._chk(_lib.lib().gfh_batch_frames_begin(c._h, 3, 6, _lib.dp(x), 0, 0))


def test_of_two_refusals_the_first_in_order_wins():
    """calls that are wrong in two ways at once, as (name, the batch held, the C call, the refusal that wins): the order of the
    refusals of every entry point is part of what it promises"""
    L = _lib.lib()
    p = np.tile(M.EXP2_TRUTH, (3, 1)); P = _lib.dp(p)
    a4 = np.arange(4, dtype=np.int32); A4 = _lib.ip(a4)
    twice = np.array([1, 1], dtype=np.int32)
    res = np.zeros(3, dtype=_lib.BATCH_RESULT_DTYPE); R = res.ctypes.data_as(C.POINTER(_lib.BatchResult))
    cov = np.zeros((3, 4, 4)); sig = np.zeros((3, 4)); info = np.zeros(3, dtype=np.int32)
    E = (_lib.dp(cov), _lib.dp(sig), _lib.ip(info))
    img = np.zeros(3 * 21); I = _lib.dp(img)
    x = np.linspace(0.5, 9.5, 6); X = _lib.dp(x)

    def opts(**kw):
        o = _lib.FitOptions()
        for k, v in kw.items():
            setattr(o, k, v); setattr(o, 'has_' + k, 1)
        return C.byref(o)
    bounded = opts(max_iter=1)
    cases = [
        # null pars and no batch held: the null argument wins over `no batch data`, under every launching call
        ('fit_null_pars', _held_nothing, lambda c: L.gfh_fit_batch(c, None, 4, A4, bounded, R, None), 'gfh_fit_batch: null argument'),
        ('fit_errors_null_pars', _held_nothing, lambda c: L.gfh_fit_batch_errors(c, None, 4, A4, bounded, R, 0, *E, None),
         'gfh_fit_batch_errors: null argument'),
        ('covariance_null_pars', _held_nothing, lambda c: L.gfh_batch_covariance(c, None, 4, A4, 0, *E), 'gfh_batch_covariance: null argument'),
        ('pass_null_pars', _held_nothing, lambda c: L.gfh_batch_pass(c, None, 4, A4, I, I, I), 'gfh_batch_pass: null argument'),
        ('eval_null_pars', _held_nothing, lambda c: L.gfh_batch_eval(c, None, 4, A4, None, None, 0, 0, 3, I, None, None, None),
         'gfh_batch_eval: null argument (pars is required)'),
        # the active set is looked at before the call's own pointers
        ('pass_twice_null_out', _data, lambda c: L.gfh_batch_pass(c, P, 2, _lib.ip(twice), None, I, I),
         'gfh_batch_pass: an active parameter is listed twice'),
        ('fit_twice_null_out', _data, lambda c: L.gfh_fit_batch(c, P, 2, _lib.ip(twice), bounded, None, None),
         'gfh_fit_batch: an active parameter is listed twice'),
        # the options: what the loop does not carry, then the reference's own refusal, then the bound, then the geometry
        ('fit_uphill_unbounded', _data, lambda c: L.gfh_fit_batch(c, P, 4, A4, opts(uphill=1), R, None),
         'gfh_fit_batch: uphill != 0 is not carried by the batch kernel'),
        ('fit_lam_incs_short', _held_short, lambda c: L.gfh_fit_batch(c, P, 4, A4, opts(lam_incs=0, max_iter=1), R, None),
         'Input parameter lam_incs must be at least 1.'),
        ('fit_lam_incs_unbounded', _data, lambda c: L.gfh_fit_batch(c, P, 4, A4, opts(lam_incs=0), R, None),
         'Input parameter lam_incs must be at least 1.'),
        ('fit_unbounded_short', _held_short, lambda c: L.gfh_fit_batch(c, P, 4, A4, opts(chi2_rel=1e-6), R, None),
         'gfh_fit_batch: max_iter is required'),
        # scale before the geometry, under both calls that take one
        ('covariance_scale_short', _held_short, lambda c: L.gfh_batch_covariance(c, P, 4, A4, 2, *E),
         'gfh_batch_covariance: scale is 0 (the inverse of J^T J) or 1 (that times chi2 / dof), got 2'),
        ('fit_errors_scale_short', _held_short, lambda c: L.gfh_fit_batch_errors(c, P, 4, A4, bounded, R, 2, *E, None),
         'gfh_fit_batch_errors: scale is 0 (the inverse of J^T J) or 1 (that times chi2 / dof), got 2'),
        # a batch begun and not put: the call's own arguments first
        ('pass_begun_null_pars', _held_begun, lambda c: L.gfh_batch_pass(c, None, 4, A4, I, I, I), 'gfh_batch_pass: null argument'),
        ('eval_begun_null_pars', _held_begun, lambda c: L.gfh_batch_eval(c, None, 4, A4, None, None, 0, 0, 3, I, None, None, None),
         'gfh_batch_eval: null argument (pars is required)'),
        ('eval_begun_bad_range', _held_begun, lambda c: L.gfh_batch_eval(c, P, 4, A4, None, None, 0, 2, 3, I, None, None, None),
         'gfh_batch_eval: 6 of 6 frames of the batch begun by gfh_batch_frames_begin have not been put'),
        # the calls that set a batch
        ('cube_null_y_no_fits', _data, lambda c: L.gfh_set_batch_cube(c, 0, 6, X, None, 0, 0, None),
         'gfh_set_batch_cube: null argument (x and y are required)'),
        ('put_negative_null_y', _held_begun, lambda c: L.gfh_batch_frames_put(c, -1, 1, None, None),
         'gfh_batch_frames_put: first_frame is negative (-1)'),
        ('put_not_begun_null_y', _data, lambda c: L.gfh_batch_frames_put(c, -1, 1, None, None),
         'gfh_batch_frames_put: no batch has been begun'),
        ('frames_y_type_per_put', _data, lambda c: L.gfh_set_batch_frames(c, 3, 6, X, X, 3, 0, None, -1),
         'gfh_set_batch_frames: unknown y_type 3 (0 double, 1 float, 2 uint16_t)'),
        ('frames_per_put_kept', _data, lambda c: L.gfh_set_batch_frames(c, 3, 6, X, X, 0, 0, None, -1),
         'gfh_set_batch_frames: frames_per_put is negative'),
    ]
    wrong = []
    for name, held, call, wins in cases:
        c = _ctx()
        try:
            held(c)
            rc = call(c._h)
            said = L.gfh_last_error(c._h).decode()
            if rc == 0 or not said.startswith(wins):
                wrong.append((name, rc, said))
            if name == 'frames_per_put_kept':          # refused before the batch held was replaced: it is still the ragged one
                assert L.gfh_debug_batch_frames_missing(c._h) == -1
                with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                    c.batch_pass(p, [0, 1, 2, 3])
        finally:
            c.close()
    assert not wrong, wrong


def test_python_api_checks_its_session():
    import gadfit_amd
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp
    assert gadfit_amd.gadf_fit_batch is gf.gadf_fit_batch

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    gf.gadf_close()
    x = np.linspace(0.5, 9.5, 10)
    with pytest.raises(gf.GadfitError, match='Call gadf_init first'):
        gf.gadf_fit_batch([x], [x], None, [M.EXP2_TRUTH], max_iter=1)
    gf.gadf_init(exp2(), 2)
    gf.gadf_set(1, 1.0, True)
    with pytest.raises(gf.GadfitError, match='one dataset slot'):
        gf.gadf_fit_batch([x], [x], None, [M.EXP2_TRUTH], max_iter=1)
    gf.gadf_close()
    gf.gadf_init(exp2())
    with pytest.raises(gf.GadfitError, match='There are no active parameters'):
        gf.gadf_fit_batch([x], [x], None, [M.EXP2_TRUTH], max_iter=1)
    for k in range(4):
        gf.gadf_set(k + 1, float(M.EXP2_TRUTH[k]), True)
    with pytest.raises(gf.GadfitError, match='one array per spectrum'):
        gf.gadf_fit_batch([x, x], [x], None, [M.EXP2_TRUTH] * 2, max_iter=1)
    with pytest.raises(gf.GadfitError, match=r'\[n_fits\]\[n_pars\] = \[2\]\[4\]'):
        gf.gadf_fit_batch([x, x], [x, x], None, [M.EXP2_TRUTH], max_iter=1)
    gf.gadf_close()
