"""Batches that arrive as stacks of frames, on the device (gfh_batch_frames_begin, gfh_batch_frames_put, gfh_set_batch_frames): the
frames are uploaded as stored, F [n_points][n_fits], and k_frames_to_cube transposes them into the cube the batch kernels read.
Inputs: tests/batch_frames_cases.py.  Nothing here has a tolerance: the cube's bytes, and from them the bits of fit_batch and
batch_pass, are those of set_batch_cube(np.ascontiguousarray(F.T)).

1. THE BYTES: for each sample type and for the USER weights of a uint16 cube, over n_fits x n_points on both sides of a 32- and of a
   64-wide tile with odd row alignments, the whole cube read back equals F.T as bytes (NaN payloads, +-inf, -0.0, denormals included).
2. PIECES: one stack put whole, frame by frame in reverse, in uneven pieces from an odd frame on, and through frames_per_put 1, 3, 64
   and 0 gives the same bytes; the missing count runs down as expected and the launches are refused until it is 0.
3. NEIGHBOURS: a piece put again over [p0, p1) of a complete cube changes those columns and nothing else.
4. 64-BIT ROWS: the last two frames of a 65537 x 32769 uint16 cube land in rows 0, 1, 65535 and 65536 where f * n_points says,
   which passes 2**31 from row 65536 on.  (p * n_fits on the staged side would pass it for a piece of more than 2**31 samples,
   which no test uploads: frames.hip forms both products from i64 operands, held by reading the code.)
5. THE BITS OF THE FITS: fit_batch under scenario a and batch_pass after set_batch_frames equal, bit for bit, the same calls after
   set_batch_cube, in all 15 loads at 64 lanes and in four at 16 and at 256 lanes; the dispatch probe reports the cube's form.
6. LIFE CYCLE on one context.
7. gadf_fit_frames returns what gadf_fit_cube returns on the transposed arrays."""
import numpy as np
import pytest

from gadfit_amd import _lib
from tests import batch_cube_cases as CC
from tests import batch_frames_cases as FR
from tests.batch_common import COUNTS, SCENARIOS, context, same_pass

pytestmark = pytest.mark.gpu

KINDS = ('float64', 'float32', 'uint16', 'uint16_user_weights')


def _stacks(kind, n_points, n_fits, seed=0):
    """(F, error type, w) of a kind: the USER weights of a uint16 stack are a float64 stack of another seed"""
    if kind == 'uint16_user_weights':
        return FR.stack(n_points, n_fits, np.uint16, seed), CC.USER, FR.stack(n_points, n_fits, np.float64, seed + 100)
    return FR.stack(n_points, n_fits, kind, seed), CC.NONE, None


def _holds(c, F, w):
    """the cube held is F.T, and under USER its weights are w.T, byte for byte"""
    n_points, n_fits = F.shape
    FR.same_bytes(FR.read_cube(c, n_fits, n_points), FR.cube_of(F))
    if w is not None:
        FR.same_bytes(FR.read_cube(c, n_fits, n_points, 1), FR.cube_of(w))


# ---- 1: the bytes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_the_cube_holds_the_bytes_of_the_transposed_stack(kind):
    c = context(CC.tape())
    try:
        for nf in FR.BYTE_FITS:
            for n in FR.BYTE_POINTS:
                F, et, w = _stacks(kind, n, nf, seed=nf * 1000 + n)
                c.set_batch_frames(CC.grid(n), F, et, w)
                assert c.batch_frames_missing() == 0
                _holds(c, F, w)
    finally:
        c.close()


# ---- 2: pieces -------------------------------------------------------------------------------------------------------------------------
def test_pieces_in_any_order_and_size_give_the_same_bytes():
    """130 frames x 67 fits of uint16 with USER weights (both kernels' widths).  The uneven pieces start at frame 1: 1, 3 and 64 frames
    reach frame 69, the piece of 65 is [65, 130) -- 1 + 3 + 64 + 65 exceed 130, so it puts four frames again, with the same data --
    and the rest is frame 0."""
    n, nf = FR.PIECE_POINTS, FR.PIECE_FITS
    F, et, w = _stacks('uint16_user_weights', n, nf, seed=7)
    x = CC.grid(n)
    start = CC.starts(n, 0.05)[CC.pick(nf)]
    c = context(CC.tape())
    try:
        def begin():
            c.batch_frames_begin(x, nf, np.uint16, et)
            assert c.batch_frames_missing() == n

        def put(lo, hi, missing):
            for call in (lambda: c.fit_batch(start, CC.ACTIVE, max_iter=2), lambda: c.batch_pass(start, CC.ACTIVE)):
                with pytest.raises(_lib.GadfitHipError, match=r'%d of %d frames of the batch begun by gfh_batch_frames_begin have not been put'
                                   % (c.batch_frames_missing(), n)):
                    call()
            c.batch_frames_put(lo, np.ascontiguousarray(F[lo:hi]), np.ascontiguousarray(w[lo:hi]))
            assert c.batch_frames_missing() == missing

        begin()                                                # whole
        put(0, n, 0)
        _holds(c, F, w)
        c.batch_pass(start, CC.ACTIVE)                         # complete: the launches run
        assert c.batch_form_used() == ('cube', 2, CC.USER)
        begin()                                                # frame by frame in reverse
        for p in range(n - 1, -1, -1):
            c.batch_frames_put(p, F[p:p + 1], w[p:p + 1])
            assert c.batch_frames_missing() == p
        _holds(c, F, w)
        begin()                                                # uneven pieces from an odd frame on
        for lo, hi, missing in ((1, 2, 129), (2, 5, 126), (5, 69, 62), (65, 130, 1), (0, 1, 0)):
            put(lo, hi, missing)
        _holds(c, F, w)
        c.fit_batch(start, CC.ACTIVE, max_iter=2)
        for per in (1, 3, 64, 0):
            c.set_batch_frames(x, F, et, w, frames_per_put=per)
            assert c.batch_frames_missing() == 0
            _holds(c, F, w)
    finally:
        c.close()


# ---- 3: neighbours ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ('uint16_user_weights', 'float32'))
@pytest.mark.parametrize('nf', FR.EDGE_FITS)
def test_a_piece_put_again_changes_its_columns_and_nothing_else(nf, kind):
    """complete with pattern A, put pattern B over [p0, p1): B inside, A everywhere else -- a tile that writes past its piece or past
    the last fit lands in a neighbour and shows; then A goes back over the range for the next pair"""
    n = FR.EDGES[-1]
    A, et, wA = _stacks(kind, n, nf, seed=1)
    B, _, wB = _stacks(kind, n, nf, seed=2)
    piece = lambda S, lo, hi: None if S is None else np.ascontiguousarray(S[lo:hi])      # noqa: E731
    c = context(CC.tape())
    try:
        c.set_batch_frames(CC.grid(n), A, et, wA)
        _holds(c, A, wA)
        for i, p0 in enumerate(FR.EDGES):
            for p1 in FR.EDGES[i + 1:]:
                c.batch_frames_put(p0, piece(B, p0, p1), piece(wB, p0, p1))
                assert c.batch_frames_missing() == 0
                want = A.copy(); want[p0:p1] = B[p0:p1]
                ww = None
                if wA is not None:
                    ww = wA.copy(); ww[p0:p1] = wB[p0:p1]
                _holds(c, want, ww)
                c.batch_frames_put(p0, piece(A, p0, p1), piece(wA, p0, p1))
        _holds(c, A, wA)
    finally:
        c.close()


# ---- 4: 64-bit rows, without a large host array ----------------------------------------------------------------------------------------
def test_rows_past_2_31_elements_land_where_a_64_bit_product_says():
    nf, n = CC.HUGE_FITS, CC.HUGE_N
    assert 65536 * n > 2 ** 31
    F2 = FR.stack(2, nf, np.uint16, seed=9)
    c = context(CC.tape())
    try:
        c.batch_frames_begin(CC.grid(n), nf, np.uint16, CC.SQRT_Y)
        assert c.device_memory()['workspace_pool'] >= 2 * nf * n + 8 * n
        c.batch_frames_put(n - 2, F2)
        assert c.batch_frames_missing() == n - 2
        for f in (0, 1, 65535, 65536):
            got = c.debug_batch_read(0, f * n + n - 2, 2)
            assert got.dtype == np.uint16 and np.array_equal(got, F2[:, f]), f
        assert len({(int(F2[0, f]), int(F2[1, f])) for f in (0, 1, 65535, 65536)}) == 4      # four different pairs: a row that lands on another one shows
    finally:
        c.close()


# ---- 5: the bits of the fits -----------------------------------------------------------------------------------------------------------
def _run(c, n, idx, form):
    out = [c.batch_pass(CC.starts(n, 0.05)[idx], CC.ACTIVE)]
    assert c.batch_form_used() == form
    off, kw = SCENARIOS['a']
    out.append(c.fit_batch(CC.starts(n, off)[idx], CC.ACTIVE, **kw)[:2])
    assert c.batch_form_used() == form
    return out


def _same_run(a, b):
    same_pass(a[0], b[0])
    FR.same_fit(*a[1], *b[1])


@pytest.mark.parametrize('lanes,yt,et', [(lanes, yt, et) for lanes, _, forms in FR.FIT_FORMS for yt, et in forms])
def test_the_fits_of_a_stack_are_the_fits_of_its_cube(lanes, yt, et):
    lengths = {l: ns for l, ns, _ in FR.FIT_FORMS}[lanes]
    form = CC.form_of(CC.Y_TYPES[yt], et)
    c = context(CC.tape())
    c.set_batch_lanes(lanes)
    try:
        for n in lengths:
            x = CC.grid(n)
            for nf in CC.FIT_COUNTS:
                idx = CC.pick(nf)
                Y = np.ascontiguousarray(CC.cube(n, CC.Y_TYPES[yt])[idx])
                w = np.ascontiguousarray(CC.user_weights(n)[idx]) if et == CC.USER else None
                c.set_batch_cube(x, Y, et, w)
                want = _run(c, n, idx, form)
                c.set_batch_frames(x, FR.frames_of(Y), et, None if w is None else FR.frames_of(w))
                got = _run(c, n, idx, form)
                assert c.batch_lanes_used() == lanes
                _same_run(got, want)
    finally:
        c.close()


# ---- 6: life cycle on one context ------------------------------------------------------------------------------------------------------
def test_life_cycle_on_one_context():
    """frames (uint16, SQRT_Y) -> ragged -> frames of another type and length (float32, PROPTO_Y, in pieces of 7) -> set_batch_cube of
    that cube -> a plain fit -> the first stack again: each step returns the bits of its first call and of a fresh context, and after
    each completed frames batch gfh_device_memory reports what set_batch_cube of the shape leaves"""
    n1, n2, nf = 129, 65, 5
    idx = CC.pick(nf)
    off, kw = SCENARIOS['a']
    x1, x2 = CC.grid(n1), CC.grid(n2)
    Y1 = np.ascontiguousarray(CC.cube(n1, np.uint16)[idx]); Y2 = np.ascontiguousarray(CC.cube(n2, np.float32)[idx])
    F1, F2 = FR.frames_of(Y1), FR.frames_of(Y2)
    W1 = CC.reference_weights(Y1, CC.SQRT_Y)             # (the ragged step needs weights of its own: not compared with the cube's)
    sigma = 1.0 / CC.user_weights(n1)[0]
    mem = lambda c: c.device_memory()['workspace_pool']      # noqa: E731

    def steps(c, which):
        out = {}
        base = mem(c)
        if 'frames1' in which:
            c.set_batch_frames(x1, F1, CC.SQRT_Y)
            out['mem1'] = mem(c) - base
            out['frames1'] = c.fit_batch(CC.starts(n1, off)[idx], CC.ACTIVE, **kw)[:2]
            assert c.batch_form_used() == ('cube', 2, CC.SQRT_Y)
        if 'ragged' in which:
            c.set_batch_data(n1 * np.arange(nf + 1, dtype=np.int64), np.tile(x1, nf), Y1.astype(np.float64).ravel(), W1.ravel())
            assert c.batch_frames_missing() == -1
            out['ragged'] = c.fit_batch(CC.starts(n1, off)[idx], CC.ACTIVE, **kw)[:2]
            assert c.batch_form_used() == 'ragged'
        if 'frames2' in which:
            c.set_batch_frames(x2, F2, CC.PROPTO_Y, frames_per_put=7)
            out['mem2'] = mem(c) - base
            out['frames2'] = c.fit_batch(CC.starts(n2, off)[idx], CC.ACTIVE, **kw)[:2]
            assert c.batch_form_used() == ('cube', 1, CC.PROPTO_Y)
            out['pass2'] = c.batch_pass(CC.starts(n2, 0.05)[idx], CC.ACTIVE)
        if 'cube2' in which:
            c.set_batch_cube(x2, Y2, CC.PROPTO_Y)
            out['mem_cube2'] = mem(c) - base
            assert c.batch_frames_missing() == -1
            out['cube2'] = c.fit_batch(CC.starts(n2, off)[idx], CC.ACTIVE, **kw)[:2]
        if 'plain' in which:
            c.set_data(x1, Y1[0].astype(np.float64), sigma, [0, n1])
            c.init_weights(4)
            p, r = c.fit([CC.starts(n1, off)[0]], CC.ACTIVE, [0] * 4, **kw)
            out['plain'] = (p, tuple(int(getattr(r, v)) for v in COUNTS), r.chi2, r.lambda_)
        if 'again' in which:
            c.set_batch_frames(x1, F1, CC.SQRT_Y)
            held = mem(c)
            out['again'] = c.fit_batch(CC.starts(n1, off)[idx], CC.ACTIVE, **kw)[:2]
            assert c.batch_form_used() == ('cube', 2, CC.SQRT_Y)
            c.set_batch_cube(x1, Y1, CC.SQRT_Y)
            assert mem(c) == held                          # (beside the plain fit's blocks: what the cube call leaves)
        return out

    c = context(CC.tape())
    try:
        one = steps(c, ('frames1', 'ragged', 'frames2', 'cube2', 'plain', 'again'))
    finally:
        c.close()
    FR.same_fit(*one['again'], *one['frames1'])
    FR.same_fit(*one['cube2'], *one['frames2'])
    assert one['mem1'] == 8 * n1 + 2 * nf * n1 and one['mem2'] == 8 * n2 + 4 * nf * n2 == one['mem_cube2']
    for which in (('frames1',), ('ragged',), ('frames2',), ('cube2',), ('plain',)):
        f = context(CC.tape())
        try:
            fresh = steps(f, which)
        finally:
            f.close()
        for key, v in fresh.items():
            if key.startswith('mem'):
                assert v == one[key], key
            elif key == 'pass2':
                same_pass(v, one[key])
            elif key == 'plain':
                assert np.array_equal(v[0], one[key][0]) and v[1:] == one[key][1:]
            else:
                FR.same_fit(*v, *one[key])


# ---- 7: the session front end ----------------------------------------------------------------------------------------------------------
def test_gadf_fit_frames_returns_what_gadf_fit_cube_returns():
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    n = 129
    x, Y = CC.grid(n), CC.cube(n, np.uint16)
    st = CC.starts(n, 0.05)
    sigma = np.sqrt(CC.counts(n).astype(np.float64) + 1.0)
    kw = dict(lambda_=1.0, max_iter=50, chi2_rel=1e-6)
    gf.gadf_init(exp2())
    try:
        for j in range(4):
            gf.gadf_set(j + 1, float(CC.CUBE_TRUTH[j]), True)
        out = {}
        for errors, s, et in ((gf.SQRT_Y, None, CC.SQRT_Y), (gf.USER, sigma, CC.USER)):
            gf.gadf_set_errors(errors)
            want = gf.gadf_fit_cube(x, Y, st, sigma=s, **kw)
            assert gf._S.ctx.batch_form_used() == ('cube', 2, et) and gf._S.ctx.batch_frames_missing() == -1
            got = gf.gadf_fit_frames(x, FR.frames_of(Y), st, sigma=None if s is None else FR.frames_of(s), **kw)
            assert gf._S.ctx.batch_form_used() == ('cube', 2, et) and gf._S.ctx.batch_frames_missing() == 0
            FR.same_fit(*got, *want)
            got = gf.gadf_fit_frames(x, FR.frames_of(Y), st, sigma=None if s is None else FR.frames_of(s), frames_per_put=10, **kw)
            FR.same_fit(*got, *want)
            out[et] = want
    finally:
        gf.gadf_close()
    assert not np.array_equal(out[CC.SQRT_Y][0], out[CC.USER][0])
