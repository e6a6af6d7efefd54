"""CPU tests of batches as data cubes (gfh_set_batch_cube, Context.set_batch_cube, gadf_fit_cube): every refusal by its message, the
geometry and the form kept on a compile-only context, the generated source and its compilation for gfx950 in all 15 loads, the
inputs of tests/batch_cube_cases.py and the selection rule of the oracle check -- evaluated by the oracle alone, with the reference's
weight formulas in numpy -- and gadf_fit_cube's argument checks.  None of this needs a GPU."""
import ctypes as C
import re

import numpy as np
import pytest

from gadfit_amd import _lib
from gadfit_amd.ad import trace_model
from tests import batch_cube_cases as CC
from tests import models as M


def _ctx():
    c = _lib.Context(-1)
    c.set_model(trace_model(M.model_exp2, 4))
    return c


def _raw(c, n_fits, n_points, x, y, y_type, error_type, w):
    as_p = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
    c._chk(_lib.lib().gfh_set_batch_cube(c._h, n_fits, n_points, as_p(x, C.POINTER(C.c_double)), as_p(y, C.c_void_p), y_type, error_type,
                                         as_p(w, C.POINTER(C.c_double))))


def test_every_refusal_has_its_message():
    c = _ctx()
    try:
        x = CC.grid(8); y = np.ones((3, 8)); w = np.ones((3, 8))
        for args, msg in (((3, 8, None, y, 0, 0, None), 'null argument'), ((3, 8, x, None, 0, 0, None), 'null argument'),
                          ((0, 8, x, y, 0, 0, None), 'at least one fit'), ((3, 0, x, y, 0, 0, None), 'at least one point'),
                          ((2 ** 31 - 3, 8, x, y, 0, 0, None), r'more fits than one launch takes \(2\^31 - 4\)'),
                          ((3, 8, x, y, 3, 0, None), 'unknown y_type 3'), ((3, 8, x, y, -1, 0, None), 'unknown y_type -1'),
                          ((3, 8, x, y, 0, 5, None), 'unknown error_type 5'), ((3, 8, x, y, 0, -1, None), 'unknown error_type -1'),
                          ((3, 8, x, y, 0, 4, None), 'USER needs the weights w'),
                          ((3, 8, x, y, 0, 1, w), 'w is taken under error_type USER alone')):
            with pytest.raises(_lib.GadfitHipError, match='gfh_set_batch_cube: .*' + msg):
                _raw(c, *args)
        # nothing was kept of a refused call
        with pytest.raises(_lib.GadfitHipError, match='no batch data'):
            c.batch_pass(np.ones((3, 4)), CC.ACTIVE)
        c.debug_set_rank(2, 0)
        with pytest.raises(_lib.GadfitHipError, match='gfh_set_batch_cube is not available on a context with a communicator of more than one rank'):
            c.set_batch_cube(x, y)
    finally:
        c.close()
    g = _lib.Context(devices=[-1, -1])                       # a group of compile-only members
    try:
        g.set_model(trace_model(M.model_exp2, 4))
        with pytest.raises(_lib.GadfitHipError, match='gfh_set_batch_cube is not available on a device-group handle'):
            g.set_batch_cube(x, y)
    finally:
        g.close()


def test_the_binding_takes_three_dtypes_and_converts_nothing():
    c = _ctx()
    try:
        x = CC.grid(8)
        for Y, msg in ((np.ones((3, 8), dtype=np.int16), 'float64, float32 or uint16'), (np.ones((3, 8), dtype=np.int64), 'float64, float32 or uint16'),
                       ([[1.0] * 8] * 3, 'float64, float32 or uint16'), (np.ones(8), '2-D'), (np.ones((8, 3)).T, 'C-contiguous'),
                       (np.ones((3, 7)), 'one abscissa per column')):
            with pytest.raises(_lib.GadfitHipError, match=msg):
                c.set_batch_cube(x, Y)
        with pytest.raises(_lib.GadfitHipError, match='shape of Y'):
            c.set_batch_cube(x, np.ones((3, 8)), CC.USER, np.ones((3, 7)))
    finally:
        c.close()


def test_a_compile_only_context_keeps_geometry_and_form():
    c = _ctx()
    try:
        x = CC.grid(200)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_cube(x, np.ones((3, 200), dtype=np.uint16), CC.SQRT_Y)
        assert c.n_fits == 3
        src = c.batch_source(CC.ACTIVE)
        assert '#define GFH_BCUBE 1\n#define GFH_BYTYPE 2\n#define GFH_BERR 1\n' in src and '#define GFH_BLANES 64\n' in src
        # the argument checks of the launches know the geometry: a well-formed call gets as far as the device
        start = np.tile(CC.CUBE_TRUTH, (3, 1))
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.fit_batch(start, CC.ACTIVE, max_iter=3)
        with pytest.raises(_lib.GadfitHipError, match='n_fits x n_pars = 3 x 4'):
            c.batch_pass(np.ones((2, 4)), CC.ACTIVE)
        # the auto rule reads n_points as the longest spectrum
        c.set_batch_lanes(0)
        assert '#define GFH_BLANES 64\n' in c.batch_source(CC.ACTIVE)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_cube(x[:100], np.ones((3, 100), dtype=np.float32), CC.USER, np.ones((3, 100)))
        src = c.batch_source(CC.ACTIVE)
        assert '#define GFH_BLANES 16\n' in src and '#define GFH_BYTYPE 1\n#define GFH_BERR 4\n' in src
        c.set_batch_lanes(64)
        # fewer points than active parameters: the ragged call's refusal, per fit
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_cube(x[:3], np.ones((2, 3)), CC.NONE)
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.fit_batch(np.ones((2, 4)), CC.ACTIVE, max_iter=1)
        # the ragged call replaces a cube: its source carries none of the three macros again
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_data([0, 10], x[:10], x[:10], x[:10])
        assert 'GFH_BYTYPE' not in c.batch_source(CC.ACTIVE)
        assert c.batch_form_used() is None                   # no launch yet
    finally:
        c.close()


def _code(src):
    return re.sub(r'//[^\n]*', '', src)                      # the code, not what its comments say


@pytest.mark.parametrize('y_type', range(3))
@pytest.mark.parametrize('error_type', CC.ERROR_TYPES)
def test_every_load_is_a_translation_unit_of_its_own_and_compiles(y_type, error_type):
    c = _ctx()
    try:
        ragged = c.batch_source(CC.ACTIVE)
        for macro in ('#define GFH_BCUBE', '#define GFH_BYTYPE', '#define GFH_BERR', 'gfh_by_t', 'GFH_BWEIGHT'):
            assert macro not in ragged
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_cube(CC.grid(8), np.ones((2, 8), dtype=CC.Y_TYPES[y_type]), error_type, np.ones((2, 8)) if error_type == CC.USER else None)
        src = c.batch_source(CC.ACTIVE)
        assert '#define GFH_BCUBE 1\n#define GFH_BYTYPE %d\n#define GFH_BERR %d\n' % (y_type, error_type) in src
        # one text of the LM loop: the cube unit is the ragged one with the three macros and batch_cube.hip in front of batch_fit.hip
        head, tail = src.index('#define GFH_BCUBE 1'), src.index('// ---- Batched independent fits')
        assert src[:head] + '\n' + src[tail:] == ragged
        assert src.count('void gfh_k_fit_batch(') == 1 and src.count('void gfh_k_batch_pass(') == 1
        added = _code(src[head:tail])
        assert '__syncthreads' not in added and '__shared__' not in added and 'atomic' not in added and 'asm' not in added
        c.batch_prepare(CC.ACTIVE)                            # hiprtc for gfx950
        assert c.model_source(CC.ACTIVE) == _ctx_plain_source()
    finally:
        c.close()


def _ctx_plain_source():
    c = _ctx()
    try:
        return c.model_source(CC.ACTIVE)
    finally:
        c.close()


def test_the_units_of_the_gpu_tests_compile():
    """every unit of batch_cube_cases.cube_units(), the 16- and 256-lane ones included (build() compiles the same list)"""
    assert len(CC.cube_units()) == 45 and len(set(CC.cube_units())) == 45
    c = _lib.Context(-1)
    try:
        CC.prepare_units(c)
    finally:
        c.close()


def test_the_barrier_invariant_names_the_cube_load():
    c = _ctx()
    try:
        c.set_batch_lanes(256)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_cube(CC.grid(8), np.ones((2, 8), dtype=np.uint16), CC.SQRT_Y)
        src = c.batch_source(CC.ACTIVE)
        inv = src[src.index('BARRIER INVARIANT (GFH_BLANES 256'):src.index('void gfh_k_fit_batch(')]
        assert 'adds only per-lane values' in inv and 'none of them enters a branch that encloses a barrier' in inv
        # the load itself holds no barrier and nothing but selects
        load = _code(src[src.index('#define GFH_BCUBE 1'):src.index('// ---- The cross-wave reducer')])
        assert '__syncthreads' not in load and not re.search(r'\bif\b', re.sub(r'#(if|elif|endif|else)[^\n]*', '', load))
    finally:
        c.close()


def test_the_inputs_are_what_the_module_says():
    zeros = 0
    for lanes, lengths in CC.LENGTHS.items():
        for n in lengths:
            c = CC.counts(n)
            assert c.dtype == np.uint16 and c.shape == (6, n) and c.max() < 65535
            zeros += int(np.sum(c == 0))
            f32, f64 = CC.cube(n, np.float32), CC.cube(n, np.float64)
            assert f32.dtype == np.float32 and f64.dtype == np.float64 and f32.flags['C_CONTIGUOUS'] and f64.flags['C_CONTIGUOUS']
            assert np.array_equal(np.floor(f32), c) and np.array_equal(np.floor(f64), c)
            assert np.array_equal(f32 == 0, c == 0) and np.array_equal(f64 == 0, c == 0)
            assert np.any(f32 != c) and np.any(f64 != f32)
    long = CC.counts(1000)
    assert long.max() > 1500 and np.median(long[:, -100:]) < 10 and np.sum(long == 0) > 0      # a few thousand down to a few, and zeros
    assert zeros > 20
    # the reference's formulas, the 0.0 arm included
    y = np.array([0.0, 4.0, 1e-307, 0.25])
    assert np.array_equal(CC.reference_weights(y, CC.SQRT_Y), [0.0, 0.5, 0.0, 2.0])
    assert np.array_equal(CC.reference_weights(y, CC.PROPTO_Y), [0.0, 0.25, 0.0, 4.0])
    assert np.array_equal(CC.reference_weights(y, CC.INVERSE_Y), y) and np.array_equal(CC.reference_weights(y, CC.NONE), np.ones(4))


@pytest.mark.parametrize('k', range(len(CC.ORACLE_FORMS)))
def test_the_selection_rule_keeps_enough_of_the_oracle_check(k):
    """check 2's rule, by the oracle alone: at most 5 % of a form's fits dropped, every length keeps at least four of its six"""
    y_type, error_type = CC.ORACLE_FORMS[k]
    dropped = total = 0
    for name in CC.FIT_SCENARIOS:
        sel = CC.oracle_selection(CC.Y_TYPES.index(y_type), error_type, name)
        for n, rows in sel.items():
            kept = sum(1 for r in rows if r[0])
            print('%s %s scenario %s n = %d: kept %d of %d, exits %s' % (np.dtype(y_type).name, error_type, name, n, kept, len(rows),
                                                                        sorted(set(r[1][0][4] for r in rows))))
            assert kept >= CC.ORACLE_KEEP, (name, n, kept)
            dropped += len(rows) - kept; total += len(rows)
    print('dropped %d of %d' % (dropped, total))
    assert dropped <= CC.ORACLE_CAP * total


def test_gadf_fit_cube_checks_its_arguments():
    import gadfit_amd
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp
    assert gadfit_amd.gadf_fit_cube is gf.gadf_fit_cube

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    gf.gadf_close()
    x = CC.grid(10); Y = np.ones((2, 10))
    p = [CC.CUBE_TRUTH] * 2
    with pytest.raises(gf.GadfitError, match='Call gadf_init first'):
        gf.gadf_fit_cube(x, Y, p, max_iter=1)
    gf.gadf_init(exp2(), 2)
    gf.gadf_set(1, 1.0, True)
    with pytest.raises(gf.GadfitError, match='one dataset slot'):
        gf.gadf_fit_cube(x, Y, p, max_iter=1)
    gf.gadf_close()
    gf.gadf_init(exp2())
    try:
        with pytest.raises(gf.GadfitError, match='There are no active parameters'):
            gf.gadf_fit_cube(x, Y, p, max_iter=1)
        for k in range(4):
            gf.gadf_set(k + 1, float(CC.CUBE_TRUTH[k]), True)
        with pytest.raises(gf.GadfitError, match=r'one column per abscissa of x \(10\)'):
            gf.gadf_fit_cube(x, np.ones((2, 9)), p, max_iter=1)
        with pytest.raises(gf.GadfitError, match=r'\[n_fits\]\[n_pars\] = \[2\]\[4\]'):
            gf.gadf_fit_cube(x, Y, p[:1], max_iter=1)
        with pytest.raises(gf.GadfitError, match='sigma is taken under USER errors alone'):
            gf.gadf_fit_cube(x, Y, p, sigma=Y, max_iter=1)
        gf.gadf_set_errors(gf.USER)
        with pytest.raises(gf.GadfitError, match='USER errors requested but no sigma was given'):
            gf.gadf_fit_cube(x, Y, p, max_iter=1)
        with pytest.raises(gf.GadfitError, match='sigma must have the shape of Y'):
            gf.gadf_fit_cube(x, Y, p, sigma=np.ones((2, 9)), max_iter=1)
    finally:
        gf.gadf_close()


def test_the_record_holds_the_compilers_figures_and_the_measurement():
    """profiles/batch_cube.json (tools/bench_batch.py --cube [--registers]): the two units of model_exp2 and model_exp4 at the three
    lane forms, no scratch in model_exp2's; the five cells with their five forms, the yardstick among them"""
    import json
    import os
    rec = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'batch_cube.json')))
    reg = rec['registers']
    assert sorted(reg) == sorted('%s_lanes%d_%s' % (m, l, f) for m in ('exp2', 'exp4') for l in (64, 16, 256) for f in ('uint16_sqrt_y', 'float64_user'))
    for name, kernels in reg.items():
        assert sorted(kernels) == ['gfh_k_batch_pass', 'gfh_k_fit_batch']
        for k in kernels.values():
            assert {'vgprs', 'agprs', 'scratch_bytes_per_lane', 'waves_per_simd'} <= set(k)
            if name.startswith('exp2'):
                assert k['scratch_bytes_per_lane'] == 0
    cells = [(m['model'], m['lanes'], m['fits'], m['points']) for m in rec['measurements']]
    assert cells == [('gauss4', 64, 16384, 1000), ('gauss4', 64, 131072, 1000), ('gauss4', 16, 131072, 64), ('gauss4', 256, 256, 65536),
                     ('exp4', 64, 16384, 1000)]
    for m in rec['measurements']:
        assert sorted(m['forms']) == ['float32_sqrt_y', 'float64_sqrt_y', 'float64_user', 'ragged', 'uint16_sqrt_y'] and m['finite']
