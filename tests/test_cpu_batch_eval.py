"""CPU tests of the curves of a batch (gfh_batch_eval, Context.batch_eval, gadf_batch_curves; the kernel gfh_k_batch_eval): the
generated source and its compilation for gfx950 on compile-only contexts, every refusal by its message, the session call's checks
and the structure of profiles/batch_eval.json.  tests/test_gpu_batch_eval.py holds the values."""
import json
import os
import re

import numpy as np
import pytest

from gadfit_amd import _lib
from gadfit_amd.ad import trace_model
from tests import batch_cov_cases as CV
from tests import models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = 'void gfh_k_batch_eval('


def _code(text):
    """the code, not what its comments say"""
    return re.sub(r'//[^\n]*', '', text)


@pytest.mark.parametrize('lanes', (64, 16, 256))
@pytest.mark.parametrize('model,n', [(M.model_exp2, 4), (M.model_exp4, 8)])
def test_the_kernel_is_in_every_batch_unit_once_behind_the_covariance_and_in_no_other(model, n, lanes):
    c = _lib.Context(-1)
    try:
        c.set_model(trace_model(model, n))
        c.set_batch_lanes(lanes)
        active = list(range(n))
        plain = c.model_source(active)
        src = c.batch_source(active)
        assert src.count(HEAD) == 1 and 'gfh_k_batch_eval' not in plain and 'gfh_b_band' not in plain
        assert src.index('void gfh_k_batch_cov(') < src.index(HEAD)          # behind batch_cov.hip
        # everything batch_eval.hip adds: from its first definition to the end of the unit
        tail = _code(src[src.index('#ifdef GFH_BCUBE\n#define GFH_BOUT(k)', src.index('void gfh_k_batch_cov(')):])
        assert HEAD in tail
        for word in ('__shared__', '__syncthreads', 'atomic', 'asm', 'gfh_b_sweep('):
            assert word not in tail, word
        assert 'gfh_point_grad(' in tail and 'gfh_point_value(' in tail and 'GFH_BLOAD(' in tail
        c.batch_prepare(active)                          # hiprtc compile for gfx950
        assert c.model_source(active) == plain           # the default translation unit is what it was
    finally:
        c.close()


def test_a_cube_form_holds_the_kernel_once_and_compiles():
    c = _lib.Context(-1)
    try:
        c.set_model(trace_model(M.model_exp2, 4))
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_cube(np.arange(1.0, 9.0), np.ones((3, 8), dtype=np.uint16), 1)
        src = c.batch_source(CV.ACTIVE)
        assert '#define GFH_BCUBE 1' in src and src.count(HEAD) == 1 and src.index('void gfh_k_batch_cov(') < src.index(HEAD)
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


def _cube(c, nf=3, n=8, dtype=np.uint16, et=1):
    with pytest.raises(_lib.GadfitHipError, match='no GPU'):
        c.set_batch_cube(np.arange(1.0, n + 1.0), np.ones((nf, n), dtype=dtype), et)
    return nf


def test_well_formed_calls_end_at_the_missing_gpu():
    c = _ctx()
    try:
        nf = _data(c)
        p = np.tile(M.EXP2_TRUTH, (nf, 1))
        cov = np.tile(np.eye(4), (nf, 1, 1))
        grid = np.linspace(-1.0, 20.0, 17)
        calls = (dict(), dict(cov=cov), dict(cov=cov, residuals=True), dict(residuals=True, model=False), dict(x_eval=grid),
                 dict(x_eval=grid, cov=cov), dict(x_eval=grid[:1], cov=cov, model=False))
        for kw in calls:
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                c.batch_eval(p, CV.ACTIVE, **kw)
        for first, n in ((0, 1), (1, 2), (2, 1), (2, None), (0, 3)):
            m = nf - first if n is None else n
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                c.batch_eval(p[first:first + m], CV.ACTIVE, cov=cov[first:first + m], first_fit=first, n_fits=n, lanes_per_fit=16)
        _cube(c)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.batch_eval(p[1:], [1, 3], cov=cov[1:, :2, :2], residuals=True, first_fit=1)
    finally:
        c.close()


def test_the_calls_own_refusals():
    c = _ctx()
    try:
        p3 = np.tile(M.EXP2_TRUTH, (3, 1))
        cov3 = np.tile(np.eye(4), (3, 1, 1))
        with pytest.raises(_lib.GadfitHipError, match='batch_eval: no batch data'):
            c.batch_eval(p3, CV.ACTIVE)
        a = np.array(CV.ACTIVE, dtype=np.int32)
        out = np.zeros(64)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_eval: no batch data'):
            c._chk(_lib.lib().gfh_batch_eval(c._h, _lib.dp(p3), 4, _lib.ip(a), None, None, 0, 0, 3, _lib.dp(out), None, None, None))
        _data(c)
        grid = np.linspace(0.0, 1.0, 5)

        def call(pars=p3, cov=None, x=None, n_eval=0, first=0, n=3, model=out, residual=None, band=None):
            q = lambda v: None if v is None else _lib.dp(v)          # noqa: E731
            c._chk(_lib.lib().gfh_batch_eval(c._h, q(pars), 4, _lib.ip(a), q(cov), q(x), n_eval, first, n, q(model), q(residual), q(band), None))
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            call()
        with pytest.raises(_lib.GadfitHipError, match=r'gfh_batch_eval: null argument \(pars is required\)'):
            call(pars=None)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_eval: no output requested'):
            call(model=None)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_eval: no output requested'):
            c.batch_eval(p3, CV.ACTIVE, model=False)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_eval: a band needs the fits. covariances'):
            call(band=out)
        with pytest.raises(_lib.GadfitHipError, match="gfh_batch_eval: a residual on a caller's grid has no meaning"):
            call(x=grid, n_eval=5, residual=out)
        with pytest.raises(_lib.GadfitHipError, match="gfh_batch_eval: a residual on a caller's grid has no meaning"):
            c.batch_eval(p3, CV.ACTIVE, x_eval=grid, residuals=True)
        for bad in (0, -1):
            with pytest.raises(_lib.GadfitHipError, match=r'gfh_batch_eval: a grid holds at least one point \(x_eval given with n_eval = %d\)' % bad):
                call(x=grid, n_eval=bad)
        with pytest.raises(_lib.GadfitHipError, match=r'gfh_batch_eval: n_eval = 5 without x_eval'):
            call(n_eval=5)
        for first, n in ((0, 0), (0, -1), (-1, 1), (3, 1), (2, 2), (0, 4), (2 ** 62, 2 ** 62)):
            with pytest.raises(_lib.GadfitHipError, match=r'gfh_batch_eval: fits \[%d, %d \+ %d\) are empty or reach past the 3 fits of the batch' % (first, first, n)):
                call(first=first, n=n)
        with pytest.raises(_lib.GadfitHipError, match='are empty or reach past the 3 fits'):
            c.batch_eval(p3[:1], CV.ACTIVE, first_fit=3, n_fits=1)
        with pytest.raises(_lib.GadfitHipError, match='are empty or reach past the 3 fits'):
            c.batch_eval(p3[:1], CV.ACTIVE, first_fit=3)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_eval: the size of the outputs overflows'):
            call(x=grid, n_eval=2 ** 60, cov=cov3, band=out)
        # the object's own checks of what it sizes the call by
        with pytest.raises(_lib.GadfitHipError, match=r'batch_eval: pars must hold the rows of the evaluated fits, n_fits x n_pars = 2 x 4 values, got 12'):
            c.batch_eval(p3, CV.ACTIVE, first_fit=1)
        with pytest.raises(_lib.GadfitHipError, match=r'batch_eval: cov must hold the rows of the evaluated fits, n_fits x na x na = 2 x 4 x 4 values, got 48'):
            c.batch_eval(p3[1:], CV.ACTIVE, cov=cov3, first_fit=1)
        with pytest.raises(_lib.GadfitHipError, match='batch_eval: active parameter indices'):
            c.batch_eval(p3, [0, 4])
    finally:
        c.close()


def test_the_shared_refusals_under_the_new_name():
    c = _ctx()
    try:
        p3 = np.tile(M.EXP2_TRUTH, (3, 1))
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_eval: an active parameter is listed twice'):
            c.batch_eval(p3, [1, 1])
        _data(c, sizes=(10, 3, 9))
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.batch_eval(p3, CV.ACTIVE)
        c.set_use_ad(False)
        with pytest.raises(_lib.GadfitHipError, match=r'gfh_batch_eval: use_ad = 0 \(finite differences\) is not carried by the batch kernels'):
            c.batch_eval(p3, [0, 1, 2])
        c.set_use_ad(True)
        c.set_loss(1)
        with pytest.raises(_lib.GadfitHipError, match=r'gfh_batch_eval: a robust loss \(gfh_set_loss\) is not carried by the batch kernels'):
            c.batch_eval(p3, [0, 1, 2])
    finally:
        c.close()
    c = _ctx(M.model_gauss8, 32)
    try:
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_eval: more than 8 active parameters'):
            c.batch_eval(np.ones((3, 32)), list(range(9)))
    finally:
        c.close()
    # a model recorded as variant tapes
    from gadfit_amd import tape as T
    from tests import branching as B
    c = _lib.Context(-1)
    try:
        V = T.Variants(B.model_piecewise2, 4)
        V.explore([1.0, 36.0, 38.0, 99.0], B.PIECEWISE2_TRUTH)
        c.set_model(V)
        _data(c)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_eval: models recorded as variant tapes'):
            c.batch_eval(np.ones((3, 4)), [0, 1])
    finally:
        c.close()
    # frames that have not been put
    c = _ctx()
    try:
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.batch_frames_begin(np.arange(1.0, 9.0), 3, np.uint16, 1)
        with pytest.raises(_lib.GadfitHipError, match=r'gfh_batch_eval: 8 of 8 frames of the batch begun by gfh_batch_frames_begin have not been put'):
            c.batch_eval(np.tile(M.EXP2_TRUTH, (3, 1)), CV.ACTIVE)
    finally:
        c.close()


def test_gadf_batch_curves_checks_its_session():
    import gadfit_amd
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp
    assert gadfit_amd.gadf_batch_curves is gf.gadf_batch_curves

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    gf.gadf_close()
    with pytest.raises(gf.GadfitError):
        gf.gadf_batch_curves([M.EXP2_TRUTH])          # no session
    gf.gadf_init(exp2())
    try:
        for k in range(4):
            gf.gadf_set(k + 1, float(M.EXP2_TRUTH[k]), True)
        with pytest.raises(gf.GadfitError, match='gadf_batch_curves: the session holds no batch'):
            gf.gadf_batch_curves([M.EXP2_TRUTH])
    finally:
        gf.gadf_close()


def test_the_record_holds_the_compilers_figures_and_the_measurement():
    """profiles/batch_eval.json (tools/bench_batch.py --eval [--registers]): gfh_k_batch_eval's figures for model_exp2 and model_exp4 at
    the three lane forms -- no scratch, no LDS --; the four cells of the cube table, each with 'model' and 'all' on the ragged and the
    uint16 / SQRT_Y forms, device times with their spread, the wall time and the two yardsticks"""
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'batch_eval.json')))
    reg = rec['registers']
    assert sorted(reg) == sorted('%s_lanes%d' % (m, l) for m in ('exp2', 'exp4') for l in (64, 16, 256))
    for name, k in reg.items():
        assert {'vgprs', 'agprs', 'sgprs', 'scratch_bytes_per_lane', 'waves_per_simd', 'lds_bytes_per_block'} <= set(k)
        assert k['scratch_bytes_per_lane'] == 0 and k['lds_bytes_per_block'] == 0, name
    cells = [(m['model'], m['lanes'], m['fits'], m['points']) for m in rec['measurements']]
    assert cells == [('gauss4', 64, 16384, 1000), ('gauss4', 64, 131072, 1000), ('gauss4', 16, 131072, 64), ('gauss4', 256, 256, 65536)]
    for m in rec['measurements']:
        assert sorted(m['forms']) == ['ragged', 'uint16_sqrt_y']
        for form, e in m['forms'].items():
            assert e['pass_device_ms']['min'] <= e['pass_device_ms']['median'] <= e['pass_device_ms']['max']
            assert sorted(e['outputs']) == ['all', 'model']
            for what, o in e['outputs'].items():
                assert 0.0 < o['device_ms']['min'] <= o['device_ms']['median'] <= o['device_ms']['max'] <= o['wall_ms']['max']
                n_out = 1 if what == 'model' else 3
                read = {'ragged': 24, 'uint16_sqrt_y': 2}[form]          # what the form's load reads per point (a cube's grid is shared)
                assert o['bytes_per_point'] == read + 8 * n_out
                assert o['bytes_moved'] == o['bytes_per_point'] * m['fits'] * m['points']
                assert o['fraction_of_8TBps'] == pytest.approx(o['bytes_moved'] / (1e-3 * o['device_ms']['median']) / 8e12, rel=1e-9)
                assert o['over_batch_pass_device_time'] == pytest.approx(o['device_ms']['median'] / e['pass_device_ms']['median'], rel=1e-9)
    if 'observed' in rec:
        assert all(k.startswith('eval_') for k in rec['observed'])
