"""CPU tests of batched fits inside a box (gfh_fit_batch_bounded, Context.fit_batch_bounded, the bounds= argument of gadf_fit_batch,
gadf_fit_cube and gadf_fit_frames; the kernel gfh_k_fit_batch_bounded): every refusal by its message and the order of simultaneous
ones on a compile-only context, the bounded unit as a translation unit of its own that leaves the four kernels' unit untouched, and
its compilation for gfx950.  tests/test_gpu_batch_bounds.py holds the values."""
import ctypes as C

import numpy as np
import pytest

from gadfit_amd import _lib
from gadfit_amd.ad import trace_model
from tests import batch_bounds_cases as BB
from tests import models as M

INF = float('inf')
NAN = float('nan')
ACTIVE = [0, 1, 2, 3]
HEAD = 'void gfh_k_fit_batch_bounded('


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


def _raw(c, pars, active, lower, upper, max_iter=3, results=True, at_bound=True):
    """gfh_fit_batch_bounded itself: None passes NULL"""
    n = max(getattr(c, 'n_fits', 0), 1)
    a = np.ascontiguousarray(active, dtype=np.int32)
    o = _lib.FitOptions()
    o.max_iter, o.has_max_iter = max_iter, 1
    res = np.zeros(n, dtype=_lib.BATCH_RESULT_DTYPE); at = np.zeros(n, dtype=np.int32)
    keep = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (pars, lower, upper)]
    q = [None if v is None else _lib.dp(v) for v in keep]
    c._chk(_lib.lib().gfh_fit_batch_bounded(c._h, q[0], a.size, _lib.ip(a), q[1], q[2], C.byref(o),
                                            res.ctypes.data_as(C.POINTER(_lib.BatchResult)) if results else None,
                                            _lib.ip(at) if at_bound else None, None))


def test_a_well_formed_call_ends_at_the_missing_gpu():
    c = _ctx()
    try:
        nf = _data(c)
        start = np.tile(M.EXP2_TRUTH, (nf, 1))
        for lo, hi in (([-INF] * 4, [INF] * 4), ([0.0, 0.1, 0.0, 0.1], [INF, 100.0, INF, 100.0]), ([5.0, -INF, -INF, 30.0], [6.0, 2.0, INF, INF])):
            for lanes in (64, 16, 256):          # (a start ON a bound is inside the box)
                with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                    c.fit_batch_bounded(start, ACTIVE, lo, hi, lanes_per_fit=lanes, lambda_=1.0, max_iter=5, chi2_rel=1e-6, accth=0.9)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.fit_batch_bounded(start, [3, 1], [20.0, -INF], [INF, 2.5], max_iter=5, DTD_min=[1.0, 2.0])
    finally:
        c.close()


def test_every_refusal_has_its_message():
    c = _ctx()
    try:
        start3 = np.tile(M.EXP2_TRUTH, (3, 1))
        lo, hi = [-INF] * 4, [INF] * 4
        who = 'gfh_fit_batch_bounded: '
        with pytest.raises(_lib.GadfitHipError, match=who + 'no batch data'):
            _raw(c, start3, ACTIVE, lo, hi)
        with pytest.raises(_lib.GadfitHipError, match='fit_batch_bounded: no batch data'):
            c.fit_batch_bounded(start3, ACTIVE, lo, hi, max_iter=1)
        _data(c)
        # the model and the active set, as gfh_fit_batch refuses them, under this call's name
        with pytest.raises(_lib.GadfitHipError, match=who + 'an active parameter is listed twice'):
            c.fit_batch_bounded(start3, [1, 1], lo[:2], hi[:2], max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='There are no active parameters'):
            _raw(c, start3, [], lo[:0], hi[:0])
        # null arguments
        for kw in (dict(pars=None), dict(lower=None), dict(upper=None), dict(results=False), dict(at_bound=False)):
            args = dict(pars=start3, lower=lo, upper=hi)
            args.update({k: v for k, v in kw.items() if k in args})
            with pytest.raises(_lib.GadfitHipError, match=who + 'null argument'):
                _raw(c, args['pars'], ACTIVE, args['lower'], args['upper'], results=kw.get('results', True), at_bound=kw.get('at_bound', True))
        # the box
        with pytest.raises(_lib.GadfitHipError, match=who + r'a bound of active parameter 2 is NaN'):
            c.fit_batch_bounded(start3, ACTIVE, [0.0, 0.0, NAN, 0.0], hi, max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match=who + r'a bound of active parameter 0 is NaN'):
            c.fit_batch_bounded(start3, ACTIVE, lo, [NAN, 1.0, 1.0, 1.0], max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match=who + r'the lower bound of active parameter 1 is \+inf'):
            c.fit_batch_bounded(start3, ACTIVE, [0.0, INF, 0.0, 0.0], hi, max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match=who + r'the upper bound of active parameter 3 is -inf'):
            c.fit_batch_bounded(start3, ACTIVE, lo, [INF, INF, INF, -INF], max_iter=1)
        for l1, h1 in ((2.0, 2.0), (2.5, 2.0)):
            with pytest.raises(_lib.GadfitHipError, match=who + r'the box of active parameter 1 is empty or a single value .*make that parameter passive instead'):
                c.fit_batch_bounded(start3, ACTIVE, [0.0, l1, 0.0, 0.0], [INF, h1, INF, INF], max_iter=1)
        # the options, as gfh_fit_batch checks them
        with pytest.raises(_lib.GadfitHipError, match=who + 'max_iter is required'):
            c.fit_batch_bounded(start3, ACTIVE, lo, hi)
        for kw, msg in ((dict(uphill=1), 'uphill'), (dict(nielsen=1), 'nielsen'), (dict(umnigh=1), 'umnigh'), (dict(grad_chi2=1e-3), 'grad_chi2'),
                        (dict(cos_phi=1e-3), 'cos_phi'), (dict(rel_error_global=1e-3), 'rel_error_global')):
            with pytest.raises(_lib.GadfitHipError, match=who + '.*' + msg):
                c.fit_batch_bounded(start3, ACTIVE, lo, hi, max_iter=3, **kw)
        with pytest.raises(_lib.GadfitHipError, match='lam_incs must be at least 1'):
            c.fit_batch_bounded(start3, ACTIVE, lo, hi, max_iter=3, lam_incs=0)
        # the starts: the fit and the parameter are named; a start ON a bound is inside
        bad = start3.copy(); bad[2, 1] = 0.05
        with pytest.raises(_lib.GadfitHipError, match=who + r'the start of fit 2 lies outside the box at active parameter 1 \(parameter 1\)'):
            c.fit_batch_bounded(bad, ACTIVE, [0.0, 0.1, 0.0, 0.1], [INF, 100.0, INF, 100.0], max_iter=1)
        bad = start3.copy(); bad[1, 3] = 100.5
        with pytest.raises(_lib.GadfitHipError, match=who + r'the start of fit 1 lies outside the box at active parameter 0 \(parameter 3\)'):
            c.fit_batch_bounded(bad, [3, 1], [0.1, 0.1], [100.0, 100.0], max_iter=1)
        # the short spectrum
        _data(c, sizes=(10, 3, 9))
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.fit_batch_bounded(start3, ACTIVE, lo, hi, max_iter=1)
        # lengths, before the call
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match=r'fit_batch_bounded: lower must hold one value per active parameter \(4\), got 3'):
            c.fit_batch_bounded(start3, ACTIVE, lo[:3], hi, max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match=r'fit_batch_bounded: upper must hold one value per active parameter \(2\), got 4'):
            c.fit_batch_bounded(start3, [0, 1], lo[:2], hi, max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='n_fits x n_pars = 3 x 4'):
            c.fit_batch_bounded(np.ones((2, 4)), ACTIVE, lo, hi, max_iter=1)
    finally:
        c.close()


def test_what_the_batch_kernels_do_not_carry_is_refused_under_this_name():
    c = _lib.Context(-1)
    try:
        with pytest.raises(_lib.GadfitHipError, match='gfh_fit_batch_bounded: no model set'):
            _raw(c, np.ones((1, 4)), ACTIVE, [-INF] * 4, [INF] * 4)
        c.set_model(trace_model(M.model_exp4, 8))
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_source_bounded: more than 8 active parameters per fit'):
            c.batch_source(list(range(8)) + [0], bounded=True)
        c.set_loss(1)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_prepare_bounded: a robust loss'):
            c.batch_prepare([0, 1], bounded=True)
        c.set_loss(0)
        c.set_use_ad(False)
        with pytest.raises(_lib.GadfitHipError, match='gfh_fit_batch_bounded: use_ad = 0'):
            _raw(c, np.ones((1, 8)), [0, 1], [-INF] * 2, [INF] * 2)
    finally:
        c.close()


def test_the_order_of_simultaneous_refusals():
    """check_batchable; null arguments; the box; the options; check_held; the starts"""
    c = _ctx()
    try:
        start3 = np.tile(M.EXP2_TRUTH, (3, 1))
        lo, hi = [-INF] * 4, [INF] * 4
        # a twice-listed active set and a null lower: the active set
        with pytest.raises(_lib.GadfitHipError, match='listed twice'):
            _raw(c, start3, [0, 1, 1, 2], None, hi)
        # a null upper and a NaN bound: the null argument
        with pytest.raises(_lib.GadfitHipError, match='null argument'):
            _raw(c, start3, ACTIVE, [NAN] * 4, None)
        # a NaN bound and no batch held: the bound
        with pytest.raises(_lib.GadfitHipError, match='is NaN'):
            _raw(c, start3, ACTIVE, [0.0, NAN, 0.0, 0.0], hi)
        # an option that is not carried and no batch held: the option
        with pytest.raises(_lib.GadfitHipError, match='max_iter is required'):
            _raw(c, start3, ACTIVE, lo, hi, max_iter=-1)
        # an empty box and an option that is not carried: the box
        _data(c, sizes=(10, 3, 9))
        with pytest.raises(_lib.GadfitHipError, match='make that parameter passive instead'):
            c.fit_batch_bounded(start3, ACTIVE, [0.0, 3.0, 0.0, 0.0], [INF, 2.0, INF, INF], max_iter=1, uphill=1)
        # an option that is not carried and a short spectrum: the option
        with pytest.raises(_lib.GadfitHipError, match='uphill'):
            c.fit_batch_bounded(start3, ACTIVE, lo, hi, max_iter=1, uphill=1)
        # a start outside and a short spectrum: the spectrum
        bad = start3.copy(); bad[0, 0] = -1.0
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.fit_batch_bounded(bad, ACTIVE, [0.0] * 4, hi, max_iter=1)
        # a start outside and nothing else: refused before the device is asked for
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match='the start of fit 0 lies outside the box at active parameter 0'):
            c.fit_batch_bounded(bad, ACTIVE, [0.0] * 4, hi, max_iter=1)
    finally:
        c.close()


@pytest.mark.parametrize('model,n,active', [(M.model_exp2, 4, [0, 1, 2, 3]), (M.model_exp2, 4, [3, 1]), (M.model_exp4, 8, list(range(8)))])
def test_the_bounded_kernel_is_a_translation_unit_of_its_own(model, n, active):
    c = _ctx(model, n)
    try:
        for lanes in (64, 16, 256):
            c.set_batch_lanes(lanes)
            src = c.batch_source(active)
            assert c.batch_source(active, bounded=False) == src and 'gfh_k_fit_batch_bounded' not in src and 'gfh_b_solve_pinned' not in src
            b = c.batch_source(active, bounded=True)
            assert b.count(HEAD) == 1 and 'void gfh_k_fit_batch(' not in b and 'gfh_k_batch_cov' not in b and 'gfh_k_batch_eval(' not in b
            # the two units share everything in front of their kernels: the point functions, the data form, the passes, the solve
            at = src.index('\n// The whole fit of each spectrum')
            assert b[:at] == src[:at] and b[at:].lstrip().startswith('// ---- Batched fits inside a box')
            assert '#define GFH_BLANES %d\n' % lanes in b
            assert c.batch_source(active) == src          # ... and asking for the bounded unit leaves the other what it was
    finally:
        c.close()


@pytest.mark.parametrize('lanes', [64, 16, 256])
def test_the_bounded_unit_compiles_for_gfx950(lanes):
    """1, 4 and 8 active parameters on each lane form (hiprtc, compile-only context)"""
    for tape, active in ((BB.tape2(), [0]), (BB.tape2(), [0, 1, 2, 3]), (BB.tape4(), list(range(8)))):
        c = _lib.Context(-1)
        try:
            c.set_model(tape)
            c.set_batch_lanes(lanes)
            c.batch_prepare(active, bounded=True)
        finally:
            c.close()


def test_the_bounded_unit_of_a_uint16_cube_compiles():
    c = _lib.Context(-1)
    try:
        c.set_model(BB.tape2())
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_cube(np.linspace(0.5, 99.5, 20), np.ones((3, 20), dtype=np.uint16), 1)
        ragged = _ctx()
        try:
            b = c.batch_source(ACTIVE, bounded=True)
            assert '#define GFH_BCUBE 1' in b and '#define GFH_BYTYPE 2' in b and b.count(HEAD) == 1
            assert '#define GFH_BCUBE' not in ragged.batch_source(ACTIVE, bounded=True)
        finally:
            ragged.close()
        c.batch_prepare(ACTIVE, bounded=True)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.fit_batch_bounded(np.tile(M.EXP2_TRUTH, (3, 1)), ACTIVE, [0.0] * 4, [INF] * 4, max_iter=2)
    finally:
        c.close()


def test_every_unit_the_gpu_tests_ask_for_compiles():
    """... into the in-tree cache, where the GPU tests find them (build() compiles the same list)"""
    c = _lib.Context(-1)
    try:
        BB.prepare_units(c)
    finally:
        c.close()


def test_the_bounds_argument_of_the_session_calls():
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
            gf.gadf_set(k + 1, float(M.EXP2_TRUTH[k]), k != 2)          # three active parameters: 0, 1, 3
        box = ([0.0, None, 0.1], [None, 100.0, INF])
        calls = (('gadf_fit_batch', lambda **kw: gf.gadf_fit_batch([x], [x], None, [M.EXP2_TRUTH], max_iter=1, **kw)),
                 ('gadf_fit_cube', lambda **kw: gf.gadf_fit_cube(x, np.ones((1, 10)), [M.EXP2_TRUTH], max_iter=1, **kw)),
                 ('gadf_fit_frames', lambda **kw: gf.gadf_fit_frames(x, np.ones((10, 1)), [M.EXP2_TRUTH], max_iter=1, **kw)))
        for who, call in calls:
            with pytest.raises(gf.GadfitError, match=who + ': bounds together with errors= is not carried in this version'):
                call(bounds=box, errors='scaled')
            with pytest.raises(gf.GadfitError, match=who + r': bounds must hold one lower and one upper value per active parameter \(3\), got 4 and 3'):
                call(bounds=([0.0] * 4, [1.0] * 3))
            with pytest.raises(gf.GadfitError, match=who + r': bounds must hold one lower and one upper value per active parameter \(3\), got 3 and 2'):
                call(bounds=([0.0] * 3, [1.0] * 2))
            with pytest.raises(gf.GadfitError, match=who + r': bounds must be \(lower, upper\)'):
                call(bounds=5.0)
            with pytest.raises(gf.GadfitError, match=who + r': bounds must be \(lower, upper\)'):
                call(bounds=([0.0] * 3,))
    finally:
        gf.gadf_close()
