"""CPU tests of batches that arrive as stacks of frames (gfh_batch_frames_begin, gfh_batch_frames_put, gfh_set_batch_frames,
Context.batch_frames_begin / batch_frames_put / set_batch_frames, gadf_fit_frames): every refusal by its message -- through the C
entries where the binding would catch it first, through the binding and gadf_fit_frames for their own checks --, what a compile-only
context keeps, that the generated sources are untouched by where a cube comes from, and the inputs of tests/batch_frames_cases.py.
None of this needs a GPU."""
import ctypes as C

import numpy as np
import pytest

from gadfit_amd import _lib
from gadfit_amd.ad import trace_model
from tests import batch_cube_cases as CC
from tests import batch_frames_cases as FR
from tests import models as M

_DP = C.POINTER(C.c_double)


def _ctx():
    c = _lib.Context(-1)
    c.set_model(trace_model(M.model_exp2, 4))
    return c


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _begin(c, n_fits, n_points, x, y_type, error_type):
    c._chk(_lib.lib().gfh_batch_frames_begin(c._h, n_fits, n_points, _p(x, _DP), y_type, error_type))


def _put(c, first, n, y, w):
    c._chk(_lib.lib().gfh_batch_frames_put(c._h, first, n, _p(y, C.c_void_p), _p(w, _DP)))


def _set(c, n_fits, n_points, x, y, y_type, error_type, w, per=0):
    c._chk(_lib.lib().gfh_set_batch_frames(c._h, n_fits, n_points, _p(x, _DP), _p(y, C.c_void_p), y_type, error_type, _p(w, _DP), per))


def _begun(c, n_fits=3, n_points=8, y_type=0, error_type=0):
    with pytest.raises(_lib.GadfitHipError, match='no GPU'):
        _begin(c, n_fits, n_points, CC.grid(n_points), y_type, error_type)


def test_begin_takes_the_cube_calls_checks_under_its_own_name():
    c = _ctx()
    try:
        x = CC.grid(8)
        for args, msg in (((3, 8, None, 0, 0), r'null argument \(x is required\)'), ((0, 8, x, 0, 0), 'at least one fit'),
                          ((3, 0, x, 0, 0), 'at least one point'), ((2 ** 31 - 3, 8, x, 0, 0), r'more fits than one launch takes \(2\^31 - 4\)'),
                          ((3, 8, x, 3, 0), 'unknown y_type 3'), ((3, 8, x, -1, 0), 'unknown y_type -1'),
                          ((3, 8, x, 0, 5), 'unknown error_type 5'), ((3, 8, x, 0, -1), 'unknown error_type -1'),
                          ((2 ** 31 - 4, 2 ** 60, x, 0, 0), 'n_fits x n_points overflows')):
            with pytest.raises(_lib.GadfitHipError, match='gfh_batch_frames_begin: .*' + msg):
                _begin(c, *args)
        # the order is the cube call's: the first failing check speaks
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_frames_begin: .*at least one fit'):
            _begin(c, 0, 0, x, 7, 7)
        # nothing was kept of a refused call
        assert c.batch_frames_missing() == -1
        with pytest.raises(_lib.GadfitHipError, match='no batch data'):
            c.batch_pass(np.ones((3, 4)), CC.ACTIVE)
        c.debug_set_rank(2, 0)
        for call, name in ((lambda: _begin(c, 3, 8, x, 0, 0), 'gfh_batch_frames_begin'), (lambda: _put(c, 0, 1, x, None), 'gfh_batch_frames_put'),
                           (lambda: _set(c, 1, 8, x, x, 0, 0, None), 'gfh_set_batch_frames')):
            with pytest.raises(_lib.GadfitHipError, match=name + ' is not available on a context with a communicator of more than one rank'):
                call()
    finally:
        c.close()
    g = _lib.Context(devices=[-1, -1])
    try:
        g.set_model(trace_model(M.model_exp2, 4))
        with pytest.raises(_lib.GadfitHipError, match='gfh_set_batch_frames is not available on a device-group handle'):
            g.set_batch_frames(x, np.ones((8, 3)))
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_frames_begin is not available on a device-group handle'):
            g.batch_frames_begin(x, 3, np.float64)
    finally:
        g.close()


def test_set_batch_frames_refuses_what_the_cube_call_refuses_and_negative_pieces():
    c = _ctx()
    try:
        x = CC.grid(8); y = np.ones((8, 3)); w = np.ones((8, 3))
        for args, msg in (((3, 8, None, y, 0, 0, None), r'null argument \(x and y are required\)'), ((3, 8, x, None, 0, 0, None), 'null argument'),
                          ((0, 8, x, y, 0, 0, None), 'at least one fit'), ((3, 0, x, y, 0, 0, None), 'at least one point'),
                          ((2 ** 31 - 3, 8, x, y, 0, 0, None), r'more fits than one launch takes \(2\^31 - 4\)'),
                          ((3, 8, x, y, 3, 0, None), 'unknown y_type 3'), ((3, 8, x, y, 0, 5, None), 'unknown error_type 5'),
                          ((3, 8, x, y, 0, 4, None), 'USER needs the weights w'),
                          ((3, 8, x, y, 0, 1, w), 'w is taken under error_type USER alone'),
                          ((3, 8, x, y, 0, 0, None, -1), 'frames_per_put is negative')):
            with pytest.raises(_lib.GadfitHipError, match='gfh_set_batch_frames: .*' + msg):
                _set(c, *args)
        assert c.batch_frames_missing() == -1
    finally:
        c.close()


def test_every_refusal_of_put_has_its_message():
    c = _ctx()
    try:
        y = np.ones((2, 3)); w = np.ones((2, 3))
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_frames_put: no batch has been begun'):
            _put(c, 0, 2, y, None)
        _begun(c, 3, 8, 0, CC.SQRT_Y)
        assert c.batch_frames_missing() == 8
        for args, msg in (((-1, 2, y, None), r'first_frame is negative \(-1\)'), ((0, 0, y, None), 'at least one frame'), ((0, -3, y, None), 'at least one frame'),
                          ((7, 2, y, None), r'frames \[7, 7 \+ 2\) reach past the 8 frames'), ((8, 1, y, None), 'reach past the 8 frames'),
                          ((0, 2 ** 62, y, None), 'reach past the 8 frames'), ((2 ** 62, 2 ** 62, y, None), 'reach past the 8 frames'),
                          ((0, 2, None, None), r'null argument \(y is required\)'),
                          ((0, 2, y, w), 'w is taken under error_type USER alone')):
            with pytest.raises(_lib.GadfitHipError, match='gfh_batch_frames_put: .*' + msg):
                _put(c, *args)
        _begun(c, 3, 8, 2, CC.USER)
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_frames_put: error_type USER needs the weights w'):
            _put(c, 0, 2, y, None)
        # a well-formed put gets as far as the device, and nothing was counted
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            _put(c, 6, 2, y, w)
        assert c.batch_frames_missing() == 8
        # the ragged call and the cube call replace a begun batch: nothing is begun any more
        for replace in (lambda: c.set_batch_cube(CC.grid(8), np.ones((3, 8))), lambda: c.set_batch_data([0, 8], CC.grid(8), CC.grid(8), CC.grid(8))):
            _begun(c)
            assert c.batch_frames_missing() == 8
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                replace()
            assert c.batch_frames_missing() == -1
            with pytest.raises(_lib.GadfitHipError, match='gfh_batch_frames_put: no batch has been begun'):
                _put(c, 0, 2, y, None)
            with pytest.raises(_lib.GadfitHipError, match='no batch has been begun'):
                c.batch_frames_put(0, y)
    finally:
        c.close()


def test_a_compile_only_context_keeps_geometry_form_and_the_missing_frames():
    c = _ctx()
    try:
        x = CC.grid(200)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.batch_frames_begin(x, 3, np.uint16, CC.SQRT_Y)
        assert c.n_fits == 3 and c.batch_frames_missing() == 200
        src = c.batch_source(CC.ACTIVE)
        assert '#define GFH_BCUBE 1\n#define GFH_BYTYPE 2\n#define GFH_BERR 1\n' in src and '#define GFH_BLANES 64\n' in src
        c.batch_prepare(CC.ACTIVE)                            # needs no data: unaffected by the missing frames
        c.set_batch_lanes(0)                                  # the auto rule reads n_points as the longest spectrum
        assert '#define GFH_BLANES 64\n' in c.batch_source(CC.ACTIVE)
        c.set_batch_lanes(64)
        start = np.tile(CC.CUBE_TRUTH, (3, 1))
        # fewer active parameters than points: the frames are what is missing
        for call, name in ((lambda: c.fit_batch(start, CC.ACTIVE, max_iter=3), 'gfh_fit_batch'), (lambda: c.batch_pass(start, CC.ACTIVE), 'gfh_batch_pass')):
            with pytest.raises(_lib.GadfitHipError, match=name + ': 200 of 200 frames of the batch begun by gfh_batch_frames_begin have not been put'):
                call()
        with pytest.raises(_lib.GadfitHipError, match='n_fits x n_pars = 3 x 4'):
            c.batch_pass(np.ones((2, 4)), CC.ACTIVE)
        # a well-formed put ends at the device and counts nothing
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.batch_frames_put(10, np.ones((5, 3), dtype=np.uint16))
        assert c.batch_frames_missing() == 200
        # more active parameters than points: the reference's message comes first
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_frames(x[:3], np.ones((3, 2), dtype=np.float32), CC.USER, np.ones((3, 2)))
        assert c.n_fits == 2 and c.batch_frames_missing() == 3
        src = c.batch_source(CC.ACTIVE)
        assert '#define GFH_BYTYPE 1\n#define GFH_BERR 4\n' in src
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.fit_batch(np.ones((2, 4)), CC.ACTIVE, max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.batch_pass(np.ones((2, 4)), CC.ACTIVE)
        # after a set_batch_cube the next put is refused: no batch has been begun
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_cube(x, np.ones((3, 200)))
        with pytest.raises(_lib.GadfitHipError, match='no batch has been begun'):
            c.batch_frames_put(0, np.ones((1, 3)))
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):      # ... and the launches are the cube's again
            c.fit_batch(start, CC.ACTIVE, max_iter=3)
        assert c.batch_form_used() is None
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.debug_batch_read(0, 0, 4)
        with pytest.raises(_lib.GadfitHipError, match='reach past the cube'):
            c.debug_batch_read(0, 599, 2)
        with pytest.raises(_lib.GadfitHipError, match='weights under error_type USER alone'):
            c.debug_batch_read(1, 0, 2)
    finally:
        c.close()


def test_the_binding_takes_three_dtypes_and_converts_nothing():
    c = _ctx()
    try:
        x = CC.grid(8)
        for F, msg in ((np.ones((8, 3), dtype=np.int16), 'float64, float32 or uint16'), ([[1.0] * 3] * 8, 'float64, float32 or uint16'),
                       (np.ones(8), '2-D'), (np.ones((3, 8)).T, 'C-contiguous'), (np.ones((7, 3)), 'one abscissa per frame')):
            with pytest.raises(_lib.GadfitHipError, match='set_batch_frames: .*' + msg):
                c.set_batch_frames(x, F)
        with pytest.raises(_lib.GadfitHipError, match='set_batch_frames: w must have the shape of F'):
            c.set_batch_frames(x, np.ones((8, 3)), CC.USER, np.ones((8, 2)))
        with pytest.raises(_lib.GadfitHipError, match='gfh_set_batch_frames: frames_per_put is negative'):
            c.set_batch_frames(x, np.ones((8, 3)), frames_per_put=-2)
        for dtype in (np.int16, np.float16, 'no such type'):
            with pytest.raises(_lib.GadfitHipError, match='batch_frames_begin: dtype must be float64, float32 or uint16'):
                c.batch_frames_begin(x, 3, dtype)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.batch_frames_begin(x, 3, np.float32, CC.USER)
        for F, msg in ((np.ones((2, 3)), 'numpy array of float32'), (np.ones((2, 3), dtype=np.uint16), 'numpy array of float32'),
                       (np.ones(3, dtype=np.float32), '2-D'), (np.ones((3, 2), dtype=np.float32).T, 'C-contiguous'),
                       (np.ones((2, 4), dtype=np.float32), r'one sample per fit of the batch in every frame \(3\), got 4')):
            with pytest.raises(_lib.GadfitHipError, match='batch_frames_put: .*' + msg):
                c.batch_frames_put(0, F, np.ones((2, 3)))
        with pytest.raises(_lib.GadfitHipError, match='batch_frames_put: w_piece must have the shape of F_piece'):
            c.batch_frames_put(0, np.ones((2, 3), dtype=np.float32), np.ones((2, 2)))
        with pytest.raises(_lib.GadfitHipError, match='gfh_batch_frames_put: error_type USER needs the weights w'):
            c.batch_frames_put(0, np.ones((2, 3), dtype=np.float32))
        assert c.batch_frames_missing() == 8
    finally:
        c.close()


def test_where_a_cube_comes_from_is_no_part_of_the_generated_source():
    """batch_source after batch_frames_begin is batch_source after set_batch_cube of the type and rule, text for text; model_source is
    untouched by either"""
    for yt, et in ((2, CC.SQRT_Y), (0, CC.USER), (1, CC.NONE)):
        a, b = _ctx(), _ctx()
        try:
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                a.batch_frames_begin(CC.grid(8), 2, CC.Y_TYPES[yt], et)
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                b.set_batch_cube(CC.grid(8), np.ones((2, 8), dtype=CC.Y_TYPES[yt]), et, np.ones((2, 8)) if et == CC.USER else None)
            assert a.batch_source(CC.ACTIVE) == b.batch_source(CC.ACTIVE)
            assert a.model_source(CC.ACTIVE) == b.model_source(CC.ACTIVE)
        finally:
            a.close(); b.close()


def test_the_inputs_are_what_the_module_says():
    seen = {np.dtype(np.float32): set(), np.dtype(np.float64): set()}
    for dtype in CC.Y_TYPES:
        dtype = np.dtype(dtype)
        for nf in FR.BYTE_FITS:
            for n in FR.BYTE_POINTS:
                F = FR.stack(n, nf, dtype, 17)
                assert F.dtype == dtype and F.shape == (n, nf) and F.flags['C_CONTIGUOUS'] and not F.flags['WRITEABLE']
                bits = FR.as_bits(F).ravel()
                want = M.splitmix64(n * nf, M.SEED + FR.FRAMES_SEED + 17).astype(bits.dtype)
                at = 3 + 11 * np.arange(8)
                at = at[at < n * nf]
                if dtype in FR.SPECIALS:
                    want[at] = FR.SPECIALS[dtype][:at.size]
                    seen[dtype] |= set(bits[at].tolist())
                assert np.array_equal(bits, want)
                assert np.array_equal(FR.as_bits(FR.cube_of(F)), FR.as_bits(F).T) and FR.cube_of(F).flags['C_CONTIGUOUS']
    big = FR.as_bits(FR.stack(129, 257, np.uint16)).ravel()
    assert np.unique(big).size > 0.7 * 65536 * (1 - np.exp(-big.size / 65536.0))        # bits, not a ramp: close to all the values 33153 draws can hit
    for dtype, bits in FR.SPECIALS.items():
        assert seen[dtype] == set(bits.tolist())                                          # each special value occurs
        v = bits.view(dtype)
        assert np.all(np.isnan(v[:3])) and v[3] == np.inf and v[4] == -np.inf and v[5] == 0 and np.signbit(v[5])
        tiny = np.finfo(dtype).tiny
        assert 0 < v[6] < tiny and -tiny < v[7] < 0
        assert np.signbit(v[2]) and len(set(bits[:3].tolist())) == 3                      # three NaNs that differ in sign and payload
    assert FR.stack(4, 4, np.float64, 1).tobytes() != FR.stack(4, 4, np.float64, 2).tobytes()
    # the forms of the fit check: all 15 loads at 64 lanes, the three oracle forms and uint16 / USER at 16 and at 256
    assert [(l, n, len(f)) for l, n, f in FR.FIT_FORMS] == [(64, (5, 65), 15), (16, (17,), 4), (256, (257,), 4)]
    assert all(set(f) <= {(yt, et) for _, yt, et in CC.cube_units()} for _, _, f in FR.FIT_FORMS)
    Y = CC.cube(65, np.float32)
    assert np.array_equal(FR.frames_of(Y), Y.T) and FR.frames_of(Y).flags['C_CONTIGUOUS'] and FR.frames_of(Y).shape == (65, 6)


def test_the_record_holds_the_five_shapes_and_the_one_condition():
    """profiles/batch_frames.json (tools/bench_batch.py --frames): the shapes of the cube table, the routes with their spreads, the
    fits equal from every route, and at 131072 x 1000 the frames route ahead of the host transpose by tests/batch_records.row_wins"""
    import json
    import os
    from tests import batch_records as RC
    rec = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'batch_frames.json')))
    cells = [(m['sample_type'], m['error_type'], m['fits'], m['points']) for m in rec['measurements']]
    assert cells == [('uint16', 1, 131072, 1000), ('uint16', 1, 131072, 64), ('uint16', 1, 256, 65536), ('float32', 1, 16384, 1000), ('float64', 4, 16384, 1000)]
    for m in rec['measurements']:
        assert {'cube', 'host_transpose', 'frames', 'frames_one_put'} <= set(m['routes']) and m['fits_equal'] and m['finite']
        for r in m['routes'].values():
            assert r['wall_ms_min'] <= r['wall_ms'] <= r['wall_ms_max']
        for name in ('frames', 'frames_one_put'):
            assert m['routes'][name]['kernel_ms'] > 0 and m['routes'][name]['kernel_GB_per_s'] > 0
        # (what the device holds after the last route is the cube: grid + samples + USER weights, and the parameter / result block of the fit)
        assert m['device_bytes_held'] >= 8 * m['points'] + m['fits'] * m['points'] * (np.dtype(m['sample_type']).itemsize + (8 if m['error_type'] == 4 else 0))
    row = lambda e: dict(device_ms=e['wall_ms'], device_ms_min=e['wall_ms_min'], device_ms_max=e['wall_ms_max'])      # noqa: E731
    head = rec['measurements'][0]['routes']
    assert RC.row_wins(row(head['frames']), row(head['host_transpose'])) and head['frames']['wins']


def test_gadf_fit_frames_checks_its_arguments():
    import gadfit_amd
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp
    assert gadfit_amd.gadf_fit_frames is gf.gadf_fit_frames

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    gf.gadf_close()
    x = CC.grid(10); F = np.ones((10, 2))
    p = [CC.CUBE_TRUTH] * 2
    with pytest.raises(gf.GadfitError, match='Call gadf_init first'):
        gf.gadf_fit_frames(x, F, p, max_iter=1)
    gf.gadf_init(exp2(), 2)
    gf.gadf_set(1, 1.0, True)
    with pytest.raises(gf.GadfitError, match='gadf_fit_frames needs a session with one dataset slot'):
        gf.gadf_fit_frames(x, F, p, max_iter=1)
    gf.gadf_close()
    gf.gadf_init(exp2())
    try:
        with pytest.raises(gf.GadfitError, match='There are no active parameters'):
            gf.gadf_fit_frames(x, F, p, max_iter=1)
        for k in range(4):
            gf.gadf_set(k + 1, float(CC.CUBE_TRUTH[k]), True)
        with pytest.raises(gf.GadfitError, match=r'gadf_fit_frames: F must be a numpy array \[n_points\]\[n_fits\] with one row \(a frame\) per abscissa of x \(10\)'):
            gf.gadf_fit_frames(x, np.ones((2, 10)), p, max_iter=1)
        with pytest.raises(gf.GadfitError, match=r'\[n_fits\]\[n_pars\] = \[2\]\[4\]'):
            gf.gadf_fit_frames(x, F, p[:1], max_iter=1)
        with pytest.raises(gf.GadfitError, match='gadf_fit_frames: sigma is taken under USER errors alone'):
            gf.gadf_fit_frames(x, F, p, sigma=F, max_iter=1)
        gf.gadf_set_errors(gf.USER)
        with pytest.raises(gf.GadfitError, match='gadf_fit_frames: USER errors requested but no sigma was given'):
            gf.gadf_fit_frames(x, F, p, max_iter=1)
        with pytest.raises(gf.GadfitError, match='gadf_fit_frames: sigma must have the shape of F'):
            gf.gadf_fit_frames(x, F, p, sigma=np.ones((2, 10)), max_iter=1)
    finally:
        gf.gadf_close()
