"""Batches as data cubes on the device (gfh_set_batch_cube): one shared grid, samples in float64, float32 or uint16, the weights
formed in the kernels' load.  Inputs and rules: tests/batch_cube_cases.py.

1. THE SAME BITS AS THE RAGGED FORM, for each of the 3 sample types x 5 weight rules at each lane form: fit_batch under scenarios a
   and c (parameters, lambda, chi2, the five counts) and batch_pass (J^T J, J^T r, chi2) equal the ragged form on the same context fed
   x tiled, Y.astype(float64) and the weights the device's own gfh_init_weights establishes on a plain context.  The lanes hold the
   same values and add them in the same order, the conversions are exact, and 1.0 / sqrt(y) and 1.0 / y are correctly rounded IEEE
   operations in both compilations (neither is built with fast-math), so no tolerance is involved.
2. Against the oracle directly, with the reference's weight formulas in numpy: SQRT_Y on uint16, PROPTO_Y on float32, INVERSE_Y on
   float64 at 64 lanes; bounds and selection rule of tests/batch_cases.py.
3. Isolation and indexing: cuts, the reverse, NaN neighbours, 2**17 + 3 fits, and one pass over more than 2**31 samples.
4. Life cycle on one context.
The dispatch probe (Context.batch_form_used) is asserted after every launch."""
import time

import numpy as np
import pytest

from gadfit_amd import _lib
from oracle import binding as orc
from tests import batch_cube_cases as CC
from tests.batch_common import COUNTS, SCENARIOS, TOL_FIT, TOL_LAMBDA, TOL_PASS, context, same_pass

pytestmark = pytest.mark.gpu


def _context(lanes=64):
    c = context(CC.tape())
    c.set_batch_lanes(lanes)
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_fit(p, r, p0, r0):
    """as batch_common.same_bits, and the parameters bit for bit too (same_bits compares their values: +0.0 equals -0.0 there)"""
    assert np.array_equal(_bits(p), _bits(p0))
    for f in COUNTS + ('dof',):
        assert np.array_equal(r[f], r0[f]), f
    assert np.array_equal(_bits(r['lambda_']), _bits(r0['lambda_'])) and np.array_equal(_bits(r['chi2']), _bits(r0['chi2']))


@pytest.fixture(scope='module')
def established():
    """(n, y_type number, error_type) -> the weights [6][n] the device's own gfh_init_weights gives the six spectra, on a plain context"""
    c = _lib.Context(0)
    c.set_model(CC.tape())
    cache = {}

    def get(n, yt, et, n_spectra=CC.N_SPECTRA):
        key = (n, yt, et, n_spectra)
        if key not in cache:
            cache[key] = CC.established_weights(c, CC.grid(n), CC.cube(n, CC.Y_TYPES[yt], n_spectra), et, CC.user_weights(n, n_spectra))
        return cache[key]
    yield get
    c.close()


def _run(c, n, idx, form):
    """one pass at the 5 %-off starts and the fits under a and c of the batch held; the dispatch asserted after every launch"""
    out = [c.batch_pass(CC.starts(n, 0.05)[idx], CC.ACTIVE)]
    assert c.batch_form_used() == form
    for name in CC.FIT_SCENARIOS:
        off, kw = SCENARIOS[name]
        out.append(c.fit_batch(CC.starts(n, off)[idx], CC.ACTIVE, **kw)[:2])
        assert c.batch_form_used() == form
    return out


def _same_run(a, b):
    """two results of _run: the passes by same_pass, each scenario's fit by _same_fit"""
    same_pass(a[0], b[0])
    for (p, r), (p0, r0) in zip(a[1:], b[1:]):
        _same_fit(p, r, p0, r0)


def _set_cube(c, n, yt, et, idx, Y=None, w=None):
    Y = np.ascontiguousarray(CC.cube(n, CC.Y_TYPES[yt])[idx]) if Y is None else Y
    if et == CC.USER and w is None:
        w = CC.user_weights(n)[idx]
    c.set_batch_cube(CC.grid(n), Y, et, w if et == CC.USER else None)


def _set_ragged(c, n, Y, W):
    nf = Y.shape[0]
    c.set_batch_data(n * np.arange(nf + 1, dtype=np.int64), np.tile(CC.grid(n), nf), Y.astype(np.float64).ravel(), np.ascontiguousarray(W).ravel())


# ---- 1: the same bits as the ragged form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('error_type', CC.ERROR_TYPES)
@pytest.mark.parametrize('yt', range(3))
@pytest.mark.parametrize('lanes', (64, 16, 256))
def test_same_bits_as_the_ragged_form(established, lanes, yt, error_type):
    c = _context(lanes)
    exits = set()
    try:
        for n in CC.LENGTHS[lanes]:
            Y6 = CC.cube(n, CC.Y_TYPES[yt])
            W6 = established(n, yt, error_type)
            if error_type in (CC.SQRT_Y, CC.PROPTO_Y):
                assert np.array_equal(W6 == 0.0, Y6 == 0)               # the 0.0 arm, where a zero occurs
            for nf in CC.FIT_COUNTS:
                idx = CC.pick(nf)
                _set_cube(c, n, yt, error_type, idx)
                got = _run(c, n, idx, ('cube', yt, error_type))
                assert c.batch_lanes_used() == lanes
                _set_ragged(c, n, Y6[idx], W6[idx])
                want = _run(c, n, idx, 'ragged')
                _same_run(got, want)
                exits |= set(got[1][1]['exit_reason'].tolist()) | set(got[2][1]['exit_reason'].tolist())
    finally:
        c.close()
    print('lanes %d, %s, error type %d: exits %s' % (lanes, np.dtype(CC.Y_TYPES[yt]).name, error_type, sorted(exits)))


# ---- 2: against the oracle directly --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(CC.ORACLE_FORMS)))
def test_against_the_oracle(k):
    """the six spectra of every 64-lane length as one cube each: one pass to 2e-13 for every fit, the fits the rule keeps under a and c
    with the counts equal, lambda to 1e-14, parameters and chi2 to 1e-10.  The oracle's weights are the reference's formulas in numpy."""
    y_type, error_type = CC.ORACLE_FORMS[k]
    yt = CC.Y_TYPES.index(y_type)
    t = CC.tape()
    c = _context(64)
    worst = dict(JTJ=0.0, JTres=0.0, chi2_pass=0.0, lam=0.0, pars=0.0, chi2=0.0)
    mismatches, kept = [], 0
    try:
        for n in CC.LENGTHS[64]:
            x = CC.grid(n)
            Y = CC.cube(n, y_type)
            Yd = Y.astype(np.float64)
            W = CC.reference_weights(Yd, error_type)
            c.set_batch_cube(x, Y, error_type)
            p5 = CC.starts(n, 0.05)
            JTJ, JTr, chi2 = c.batch_pass(p5, CC.ACTIVE)
            assert c.batch_form_used() == ('cube', yt, error_type) and c.batch_lanes_used() == 64
            for s in range(CC.N_SPECTRA):
                p = orc.OracleProblem(t, [x], [Yd[s].copy()], [W[s].copy()], [p5[s]], CC.ACTIVE, [0] * 4)
                JTJ0, JTr0, _, _ = p.sweep()
                chi0, _ = p.chi2()
                sc = np.sqrt(np.outer(np.diag(JTJ0), np.diag(JTJ0))) + 1e-300
                worst['JTJ'] = max(worst['JTJ'], np.max(np.abs(JTJ[s] - JTJ0) / sc))
                worst['JTres'] = max(worst['JTres'], np.max(np.abs(JTr[s] - JTr0) / (np.sqrt(np.diag(JTJ0) * chi0) + 1e-300)))
                worst['chi2_pass'] = max(worst['chi2_pass'], abs(chi2[s] - chi0) / chi0)
            for name in CC.FIT_SCENARIOS:
                off, kw = SCENARIOS[name]
                pars, res, _ = c.fit_batch(CC.starts(n, off), CC.ACTIVE, **kw)
                assert c.batch_form_used() == ('cube', yt, error_type)
                for s, (keep, one, _, _) in enumerate(CC.oracle_selection(yt, error_type, name)[n]):
                    if not keep:
                        continue
                    kept += 1
                    counts0, pars0, lam0, chi0 = one
                    got = tuple(int(res[f][s]) for f in COUNTS)
                    if got != counts0:
                        mismatches.append((name, n, s, got, counts0))
                        continue
                    worst['lam'] = max(worst['lam'], abs(res['lambda_'][s] - lam0) / lam0)
                    worst['pars'] = max(worst['pars'], np.max(np.abs(pars[s] - pars0) / np.abs(pars0)))
                    worst['chi2'] = max(worst['chi2'], abs(res['chi2'][s] - chi0) / chi0 if chi0 else abs(res['chi2'][s]))
    finally:
        c.close()
    print('%s, error type %d: %d fits held against the oracle; observed %s' % (np.dtype(y_type).name, error_type, kept,
                                                                             ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))
    assert not mismatches, mismatches[:8]
    assert worst['JTJ'] < TOL_PASS and worst['JTres'] < TOL_PASS and worst['chi2_pass'] <= TOL_PASS
    assert worst['lam'] <= TOL_LAMBDA and worst['pars'] < TOL_FIT and worst['chi2'] < TOL_FIT


# ---- 3: isolation and indexing -------------------------------------------------------------------------------------------------------
ISOLATION = ((64, 129), (16, 33), (256, 513))           # (lanes, length): more than one row of points per fit in each form


@pytest.mark.parametrize('lanes,n', ISOLATION)
def test_a_fit_does_not_depend_on_its_batch(lanes, n):
    """17 fits of uint16 / SQRT_Y; the batch cut to 5, 2 and 1 fits and the batch reversed return each fit's bits"""
    c = _context(lanes)
    try:
        idx = CC.pick(17)
        _set_cube(c, n, 2, CC.SQRT_Y, idx)
        full = _run(c, n, idx, ('cube', 2, CC.SQRT_Y))
        for sel in (np.arange(5), np.arange(2), np.arange(1), np.arange(16, -1, -1)):
            _set_cube(c, n, 2, CC.SQRT_Y, idx[sel])
            part = _run(c, n, idx[sel], ('cube', 2, CC.SQRT_Y))
            _same_run(part, [[v[sel] for v in full[0]]] + [(p[sel], r[sel]) for p, r in full[1:]])
    finally:
        c.close()


@pytest.mark.parametrize('yt', range(3))
@pytest.mark.parametrize('lanes,n', ISOLATION)
def test_a_fit_reads_no_point_of_its_neighbours(lanes, n, yt):
    """every other spectrum's row set to NaN (both parities) -- the samples of a float64 and a float32 cube under SQRT_Y, the USER
    weights of a uint16 cube: the clean fits return the bits of the undisturbed batch from both kernels, the poisoned ones end with
    reason 8 and their start values"""
    et = CC.USER if yt == 2 else CC.SQRT_Y
    form = ('cube', yt, et)
    idx = CC.pick(17)
    f = np.arange(17)
    c = _context(lanes)
    try:
        _set_cube(c, n, yt, et, idx)
        full = _run(c, n, idx, form)
        for clean in (f % 2 == 0, f % 2 == 1):
            Y = np.ascontiguousarray(CC.cube(n, CC.Y_TYPES[yt])[idx])
            w = CC.user_weights(n)[idx].copy()
            if yt == 2:
                w[~clean] = np.nan
            else:
                Y[~clean] = np.nan
            _set_cube(c, n, yt, et, idx, Y, w)
            got = _run(c, n, idx, form)
            same_pass([v[clean] for v in got[0]], [v[clean] for v in full[0]])
            for (p1, r1), (p0, r0), name in zip(got[1:], full[1:], CC.FIT_SCENARIOS):
                _same_fit(p1[clean], r1[clean], p0[clean], r0[clean])
                bad = ~clean
                assert np.all(r1['exit_reason'][bad] == 8) and np.all(r1['iterations'][bad] == 0)
                assert np.all(r1['n_sweeps'][bad] == 1) and np.all(r1['n_chi2'][bad] == 1)
                assert np.array_equal(p1[bad], CC.starts(n, SCENARIOS[name][0])[idx][bad])
    finally:
        c.close()


def test_a_large_batch_of_short_rows():
    """2**17 + 3 fits of 33 uint16 points at 16 lanes, tiled from 66 spectra (odd rows: every other one starts on an odd 2-byte
    boundary): every copy returns the bits of its first occurrence, from the pass and from the fit under c"""
    nf, n = CC.LARGE_FITS, CC.LARGE_N
    idx = np.arange(nf) % 66
    Y = np.ascontiguousarray(CC.counts(n, 66)[idx])
    off, kw = SCENARIOS['c']
    st = CC.starts(n, off, 66)[idx]
    c = _context(16)
    try:
        c.set_batch_cube(CC.grid(n), Y, CC.SQRT_Y)
        one = c.batch_pass(CC.starts(n, 0.05, 66)[idx], CC.ACTIVE)
        pars, res, _ = c.fit_batch(st, CC.ACTIVE, **kw)
        assert c.batch_form_used() == ('cube', 2, CC.SQRT_Y) and c.batch_lanes_used() == 16
        # ... and the first 66 are what a batch of those alone returns
        c.set_batch_cube(CC.grid(n), np.ascontiguousarray(Y[:66]), CC.SQRT_Y)
        p66, r66, _ = c.fit_batch(st[:66], CC.ACTIVE, **kw)
    finally:
        c.close()
    same_pass(one, [v[idx] for v in one])
    _same_fit(pars, res, pars[idx], res[idx])
    _same_fit(pars[:66], res[:66], p66, r66)
    assert len(set(res['exit_reason'][:66].tolist()) - {8}) > 0


def test_one_pass_over_more_than_2_31_samples():
    """65537 fits x 32769 uint16 points at 256 lanes, tiled from three spectra: f * n_points passes 2**31, where a 32-bit product
    lands on another spectrum (rows 65536 would read row 0's samples shifted: copies of one spectrum would then differ); every copy
    returns the bits of its first occurrence, which are those of a batch of the three alone"""
    nf, n = CC.HUGE_FITS, CC.HUGE_N
    assert nf * n > 2 ** 31
    idx = np.arange(nf) % 3
    t0 = time.time()
    Y = np.ascontiguousarray(CC.counts(n, 3)[idx])
    p5 = CC.starts(n, 0.05, 3)[idx]
    c = _context(256)
    try:
        c.set_batch_cube(CC.grid(n), Y, CC.SQRT_Y)
        assert c.device_memory()['workspace_pool'] >= 2 * nf * n + 8 * n
        one = c.batch_pass(p5, CC.ACTIVE)
        assert c.batch_form_used() == ('cube', 2, CC.SQRT_Y) and c.batch_lanes_used() == 256
        c.set_batch_cube(CC.grid(n), np.ascontiguousarray(Y[:3]), CC.SQRT_Y)
        three = c.batch_pass(p5[:3], CC.ACTIVE)
    finally:
        c.close()
    print('more than 2**31 samples: %.1f s' % (time.time() - t0))
    same_pass(one, [v[idx] for v in three])
    assert len({three[2][k] for k in range(3)}) == 3          # three different spectra: a row that lands on another one shows


# ---- 4: life cycle on one context ------------------------------------------------------------------------------------------------------
def test_life_cycle_on_one_context(established):
    """cube (uint16, SQRT_Y) -> ragged -> cube of another type (float32, PROPTO_Y, another length) -> batch_pass -> a plain fit ->
    the first cube again: each step returns the bits of its first call and of a fresh context; gfh_device_memory shows the cube's
    bytes and none of the replaced batch's"""
    n1, n2, nf = 129, 65, 5
    idx = CC.pick(nf)
    off, kw = SCENARIOS['c']
    x1, x2 = CC.grid(n1), CC.grid(n2)
    W1 = established(n1, 2, CC.SQRT_Y)
    sigma = 1.0 / CC.user_weights(n1)[0]

    def steps(c, which):
        out = {}
        base = c.device_memory()['workspace_pool']
        if 'cube1' in which:
            _set_cube(c, n1, 2, CC.SQRT_Y, idx)
            out['mem1'] = c.device_memory()['workspace_pool'] - base
            out['cube1'] = c.fit_batch(CC.starts(n1, off)[idx], CC.ACTIVE, **kw)[:2]
            assert c.batch_form_used() == ('cube', 2, CC.SQRT_Y)
        if 'ragged' in which:
            _set_ragged(c, n1, CC.counts(n1)[idx], W1[idx])
            out['mem_ragged'] = c.device_memory()['workspace_pool'] - base
            out['ragged'] = c.fit_batch(CC.starts(n1, off)[idx], CC.ACTIVE, **kw)[:2]
            assert c.batch_form_used() == 'ragged'
        if 'cube2' in which:
            _set_cube(c, n2, 1, CC.PROPTO_Y, idx)
            out['mem2'] = c.device_memory()['workspace_pool'] - base
            out['cube2'] = c.fit_batch(CC.starts(n2, off)[idx], CC.ACTIVE, **kw)[:2]
            assert c.batch_form_used() == ('cube', 1, CC.PROPTO_Y)
            out['pass2'] = c.batch_pass(CC.starts(n2, 0.05)[idx], CC.ACTIVE)
            assert c.batch_form_used() == ('cube', 1, CC.PROPTO_Y)
        if 'plain' in which:
            c.set_data(x1, CC.counts(n1)[0].astype(np.float64), sigma, [0, n1])
            c.init_weights(4)
            p, r = c.fit([CC.starts(n1, off)[0]], CC.ACTIVE, [0] * 4, **kw)
            out['plain'] = (p, tuple(int(getattr(r, v)) for v in COUNTS), r.chi2, r.lambda_)
        if 'again' in which:
            if 'cube2' in which:                          # the batch and its form are still there after the plain fit
                p, r, _ = c.fit_batch(CC.starts(n2, off)[idx], CC.ACTIVE, **kw)
                assert c.batch_form_used() == ('cube', 1, CC.PROPTO_Y)
                _same_fit(p, r, *out['cube2'])
            _set_cube(c, n1, 2, CC.SQRT_Y, idx)
            out['again'] = c.fit_batch(CC.starts(n1, off)[idx], CC.ACTIVE, **kw)[:2]
            assert c.batch_form_used() == ('cube', 2, CC.SQRT_Y)
        return out

    c = _context(64)
    try:
        one = steps(c, ('cube1', 'ragged', 'cube2', 'plain', 'again'))
    finally:
        c.close()
    _same_fit(*one['again'], *one['cube1'])
    _same_fit(*one['ragged'], *one['cube1'])              # (check 1 once more)
    # what the device holds: the grid and the narrow samples, and nothing of the batch they replaced
    assert one['mem1'] == 8 * n1 + 2 * nf * n1
    assert one['mem_ragged'] == 3 * 8 * nf * n1 + 8 * (nf + 1)
    assert one['mem2'] == 8 * n2 + 4 * nf * n2
    for which in (('cube1',), ('ragged',), ('cube2',), ('plain',)):
        f = _context(64)
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
                _same_fit(*v, *one[key])


def test_gadf_fit_cube_returns_what_fit_batch_returns(established):
    """the session front end: the session's gadf_set_errors type reaches the load, and under USER 1 / sigma is passed"""
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
    kw = dict(lambda_=1.0, max_iter=50, chi2_rel=float(np.float32(1e-6)))
    sigma = np.sqrt(CC.counts(n).astype(np.float64) + 1.0)
    c = _context(64)
    try:
        want = {}
        for et in (CC.SQRT_Y, CC.USER):
            c.set_batch_cube(x, Y, et, 1.0 / sigma if et == CC.USER else None)
            want[et] = c.fit_batch(st, CC.ACTIVE, **kw)[:2]
    finally:
        c.close()
    gf.gadf_init(exp2())
    try:
        for j in range(4):
            gf.gadf_set(j + 1, float(CC.CUBE_TRUTH[j]), True)
        gf.gadf_set_errors(gf.SQRT_Y)
        p, r = gf.gadf_fit_cube(x, Y, st, lambda_=1.0, max_iter=50, chi2_rel=1e-6)
        assert gf._S.ctx.batch_form_used() == ('cube', 2, CC.SQRT_Y)
        _same_fit(p, r, *want[CC.SQRT_Y])
        gf.gadf_set_errors(gf.USER)
        p, r = gf.gadf_fit_cube(x, Y, st, sigma=sigma, lambda_=1.0, max_iter=50, chi2_rel=1e-6)
        assert gf._S.ctx.batch_form_used() == ('cube', 2, CC.USER)
        _same_fit(p, r, *want[CC.USER])
    finally:
        gf.gadf_close()
    assert not np.array_equal(want[CC.SQRT_Y][0], want[CC.USER][0])
