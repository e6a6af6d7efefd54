"""The batch kernels (gfh_k_fit_batch, gfh_k_batch_pass) over the input space tests/test_gpu_batch.py leaves out: spectrum lengths at
the edges of a wave (n = na, n < 64, 64 k - 1 / 64 k / 64 k + 1, rows enough that the row loop dominates), batch sizes that leave waves of
the last workgroup without a fit, neighbours filled with NaN, every active count 1 ... 8 in the caller's order, the whole operator
set, a batch of 2^17 + 3 fits, and the context's state from call to call.

The inputs and the rule that selects which fits may be held against the oracle are in tests/batch_cases.py; tests/test_cpu_batch_cases.py
shows without a GPU that the rule's caps hold.  The rule is the oracle's alone: nothing the device returns enters it.
Bounds (the project's own): one pass TOL_PASS = 2e-13 scaled as in test_one_pass_against_the_oracle, the counts equal, lambda
TOL_LAMBDA = 1e-14, fitted parameters and chi2 north_star's 1e-10.  The observed maxima go where test_gpu_batch.py's go
(GADFIT_BATCH_OBSERVE, profiles/batch_fits.json) under the keys shapes_*."""
import numpy as np
import pytest

from gadfit_amd import _lib
from oracle import binding as orc
from tests import batch_cases as BC
from tests.test_gpu_batch import COUNTS, SCENARIOS, TOL_LAMBDA, TOL_PASS, _observe, _same_bits

pytestmark = pytest.mark.gpu

TOL_FIT = 1e-10          # north_star's bound on fitted parameters and chi2


def _context(tape, batch=None):
    c = _lib.Context(0)
    c.set_model(tape)
    if batch is not None:
        c.set_batch_data(batch.off, batch.x, batch.y, batch.w)
    return c


def _pass_worst(tape, items, starts, active, JTJ, JTr, chi2):
    """a batch_pass against OracleProblem.sweep, fit by fit, scaled as test_one_pass_against_the_oracle scales it"""
    worst = 0.0
    for b, (x, y, w) in enumerate(items):
        p = orc.OracleProblem(tape, [x], [y], [w], [starts[b]], active, [0] * tape.n_pars)
        JTJ0, JTr0, _, _ = p.sweep()
        chi0, _ = p.chi2()
        d = np.diag(JTJ0)
        worst = max(worst, np.max(np.abs(JTJ[b] - JTJ0) / (np.sqrt(np.outer(d, d)) + 1e-300)),
                    np.max(np.abs(JTr[b] - JTr0) / (np.sqrt(d * chi0) + 1e-300)), abs(chi2[b] - chi0) / chi0)
        assert np.array_equal(JTJ[b], JTJ[b].T), b
    assert np.isfinite(worst)
    return worst


def _fit_worst(sel, pars, res, n_points, na):
    """fit_batch against the oracle's fits of the selection (kept cases): the counts and dof equal; returns the worst relative
    differences of lambda, the parameters and chi2"""
    worst = dict(lam=0.0, pars=0.0, chi2=0.0)
    mismatches, kept = [], 0
    for b, (ok, (counts, p0, lam0, chi0), _, _) in enumerate(sel):
        assert int(res['dof'][b]) == max(int(n_points[b]) - na, 1), b          # n = na: dof 0 is reported as 1 (gadfit.F90:648-657)
        if not ok:
            continue
        kept += 1
        got = tuple(int(res[f][b]) for f in COUNTS)
        if got != counts:
            mismatches.append((b, got, counts))
            continue
        worst['lam'] = max(worst['lam'], abs(res['lambda_'][b] - lam0) / lam0)
        worst['pars'] = max(worst['pars'], np.max(np.abs(pars[b] - p0) / np.abs(p0)))
        worst['chi2'] = max(worst['chi2'], abs(res['chi2'][b] - chi0) / chi0)
    assert kept > 0, 'the rule kept no fit of this batch: nothing was compared'
    assert not mismatches, '%d of %d kept fits differ in (iterations, n_sweeps, n_chi2, n_omega, exit_reason): %s' % (len(mismatches), kept, mismatches[:8])
    assert all(np.isfinite(v) for v in worst.values())
    return worst


def _check_fit(key, worst):
    _observe(**{'shapes_%s_lambda' % key: worst['lam'], 'shapes_%s_pars' % key: worst['pars'], 'shapes_%s_chi2' % key: worst['chi2']})
    assert worst['lam'] <= TOL_LAMBDA and worst['pars'] < TOL_FIT and worst['chi2'] < TOL_FIT


# ---- Part 1: lengths at the wave's edges, batch sizes at the workgroup's edges, isolation ----------------------------------------
class Lengths:
    def __init__(self):
        self.tape, self.order, self.truths, self.batch = BC.part1()
        self.n = self.batch.n
        self.ctx = _context(self.tape, self.batch)
        self._fits, self._pass = {}, None

    def fit(self, name):
        """the batch of 108 under a scenario (cached: later tests compare other batches with it bit for bit)"""
        if name not in self._fits:
            off, kw = SCENARIOS[name]
            self._fits[name] = self.ctx.fit_batch(BC.part1_starts(off), BC.PART1_ACTIVE, **kw)[:2]
        return self._fits[name]

    def one_pass(self):
        if self._pass is None:
            self._pass = self.ctx.batch_pass(BC.part1_starts(0.05), BC.PART1_ACTIVE)
        return self._pass


@pytest.fixture(scope='module')
def L():
    s = Lengths()
    yield s
    s.ctx.close()


def _same_pass(a, b):
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))


def test_lengths_one_pass_against_the_oracle(L):
    """n = 4 ... 20001: the first row is also the last (n < 64), the last row is full (64 k), has one live lane (64 k + 1) or one
    masked lane (64 k - 1), and 313 rows per pass (n = 20001)"""
    JTJ, JTr, chi2 = L.one_pass()
    worst = _pass_worst(L.tape, L.batch.items, BC.part1_starts(0.05), BC.PART1_ACTIVE, JTJ, JTr, chi2)
    _observe(shapes_lengths_pass=worst)
    assert worst < TOL_PASS


@pytest.mark.parametrize('name', BC.PART1_SCENARIOS)
def test_lengths_fits_against_the_oracle(L, name):
    """all 108 fits are kept by the rule (tests/test_cpu_batch_cases.py); dof = max(n - 4, 1), the n = 4 fits being the dof = 0 case"""
    sel = BC.part1_selection(name)
    assert all(s[0] for s in sel)
    pars, res = L.fit(name)
    print('lengths (%s): iterations %s, exits %s' % (name, sorted(set(res['iterations'].tolist())), sorted(set(res['exit_reason'].tolist()))))
    _check_fit('lengths_%s' % name, _fit_worst(sel, pars, res, L.n, 4))


def test_batch_sizes_that_leave_waves_without_a_fit(L):
    """the batch cut to its first 107, 106, 105 fits (3, 2, 1 live waves in the last workgroup) and to 7, 5, 3, 2: every fit returns
    the bits it returned in the batch of 108, from batch_pass and from fit_batch under (a) and (c)"""
    p5 = BC.part1_starts(0.05)
    c = _context(L.tape)
    try:
        for k in (107, 106, 105, 7, 5, 3, 2):
            c.set_batch_data(*L.batch.first(k))
            _same_pass(c.batch_pass(p5[:k], BC.PART1_ACTIVE), [v[:k] for v in L.one_pass()])
            for name in ('a', 'c'):
                off, kw = SCENARIOS[name]
                pars, res = L.fit(name)
                p1, r1, _ = c.fit_batch(BC.part1_starts(off)[:k], BC.PART1_ACTIVE, **kw)
                _same_bits(p1, r1, pars[:k], res[:k])
    finally:
        c.close()


def test_a_fit_reads_no_point_of_its_neighbours(L):
    """Every other spectrum's x, y and w are NaN: fit k returns the bits of the undisturbed batch from batch_pass and from fit_batch
    under (c) (STEP 1 + 2, chi2 and STEP 3 all read the points).  A NaN that came through a w = 0 mask would show (NaN * 0 = NaN); a
    finite stray value does not.  The poisoned fits end at their first solve (exit 8: 'ajj > 0' is false for a NaN) with their start
    parameters."""
    n = L.n.tolist()
    short_between_long = next(k for k in range(1, 107) if n[k - 1] > 4096 and n[k] < 64 and n[k + 1] > 4096)
    long_between_short = next(k for k in range(1, 107) if n[k - 1] < 64 and n[k] > 4096 and n[k + 1] < 64)
    exact_rows = [k for k in range(108) if n[k] in (64, 128, 192)][:3]            # spectra that end with a full row
    off, kw = SCENARIOS['c']
    starts, p5 = BC.part1_starts(off), BC.part1_starts(0.05)
    pars, res = L.fit('c')
    c = _context(L.tape)
    try:
        for k in [0, 107, short_between_long, long_between_short, 53, 54] + exact_rows:
            x = np.full_like(L.batch.x, np.nan); y = x.copy(); w = x.copy()
            lo, hi = L.batch.off[k], L.batch.off[k + 1]
            x[lo:hi] = L.batch.x[lo:hi]; y[lo:hi] = L.batch.y[lo:hi]; w[lo:hi] = L.batch.w[lo:hi]
            c.set_batch_data(L.batch.off, x, y, w)
            _same_pass([v[k:k + 1] for v in c.batch_pass(p5, BC.PART1_ACTIVE)], [v[k:k + 1] for v in L.one_pass()])
            p1, r1, _ = c.fit_batch(starts, BC.PART1_ACTIVE, **kw)
            _same_bits(p1[k:k + 1], r1[k:k + 1], pars[k:k + 1], res[k:k + 1])
            others = np.arange(108) != k
            assert np.all(r1['exit_reason'][others] == 8) and np.all(r1['iterations'][others] == 0), k
            assert np.all(r1['n_sweeps'][others] == 1) and np.all(r1['n_chi2'][others] == 1), k
            assert np.array_equal(p1[others], starts[others]), k
    finally:
        c.close()


@pytest.mark.parametrize('name', BC.PART1_ONE_SCENARIOS)
def test_lengths_with_one_active_parameter(L, name):
    """the same 108 spectra with active = [1]: the 1 x 1 instance of the solve, the packed triangle and the accumulators (the fits the
    rule keeps: every length stays covered, tests/test_cpu_batch_cases.py)"""
    sel = BC.part1_selection(name, True)
    off, kw = SCENARIOS[name]
    starts = BC.part1_starts(off, BC.PART1_ONE_ACTIVE)
    pars, res, _ = L.ctx.fit_batch(starts, BC.PART1_ONE_ACTIVE, **kw)
    assert np.array_equal(pars[:, [0, 2, 3]], starts[:, [0, 2, 3]])          # the passive parameters come back bit for bit
    _check_fit('one_active_%s' % name, _fit_worst(sel, pars, res, L.n, 1))
    if name == 'a':
        JTJ, JTr, chi2 = L.ctx.batch_pass(starts, BC.PART1_ONE_ACTIVE)
        worst = _pass_worst(L.tape, L.batch.items, starts, BC.PART1_ONE_ACTIVE, JTJ, JTr, chi2)
        _observe(shapes_one_active_pass=worst)
        assert worst < TOL_PASS


# ---- Part 4: a batch of the size the README quotes ---------------------------------------------------------------------------------
def test_a_batch_of_131075_fits(L):
    """the 90 spectra of up to 193 points tiled to 2^17 + 3 fits (1.07e7 points) under (b): every copy returns the bits of its first
    occurrence, and the first 90 are held against the oracle"""
    short = [k for k in range(108) if L.n[k] <= BC.PART1_LARGE_MAX_N]
    assert len(short) == 90
    nf = BC.PART1_LARGE_FITS
    reps = -(-nf // 90)
    seg = [(L.batch.off[k], L.batch.off[k + 1]) for k in short]
    x90, y90, w90 = (np.concatenate([v[lo:hi] for lo, hi in seg]) for v in (L.batch.x, L.batch.y, L.batch.w))
    n_all = np.tile(L.n[short], reps)[:nf]
    off_all = np.concatenate([[0], np.cumsum(n_all)]).astype(np.int64)
    cut = int(off_all[-1])
    off_b, kw = SCENARIOS['b']
    starts90 = BC.part1_starts(off_b)[short]
    starts = np.tile(starts90, (reps, 1))[:nf]
    c = _context(L.tape)
    try:
        c.set_batch_data(off_all, np.tile(x90, reps)[:cut], np.tile(y90, reps)[:cut], np.tile(w90, reps)[:cut])
        pars, res, _ = c.fit_batch(starts, BC.PART1_ACTIVE, **kw)
    finally:
        c.close()
    first = np.arange(nf) % 90
    _same_bits(pars, res, pars[first], res[first])
    sel = [BC.part1_selection('b')[k] for k in short]
    _check_fit('large_batch', _fit_worst(sel, pars[:90], res[:90], L.n[short], 4))
    # the same spectra in the batch of 108 lie at other offsets, beside other neighbours: the same bits again
    p108, r108 = L.fit('b')
    _same_bits(pars[:90], res[:90], p108[short], r108[short])


# ---- Part 5: the context's state from call to call ----------------------------------------------------------------------------------
def test_state_on_one_context(L):
    """batch_pass -> fit_batch -> batch_pass (io and img reallocated in between), a batch of 3 in place of the batch of 108 and back,
    then a plain set_data + fit on the same context (its kernel cache holds the batch unit under a key of its own): every result is
    the bits of the first call on that data, and the plain fit returns what a fresh context returns"""
    off, kw = SCENARIOS['c']
    starts, p5 = BC.part1_starts(off), BC.part1_starts(0.05)
    k = 5                       # (a spectrum of 1000 points)
    x, y, w = L.batch.items[k]
    sigma = 1.0 / w

    def plain(ctx):
        ctx.set_data(x, y, sigma, [0, x.size])
        ctx.init_weights(4)
        return ctx.fit([starts[k]], BC.PART1_ACTIVE, [0] * 4, **kw)
    c = _context(L.tape, L.batch)
    try:
        pass0 = c.batch_pass(p5, BC.PART1_ACTIVE)
        _same_pass(pass0, L.one_pass())
        p0, r0, _ = c.fit_batch(starts, BC.PART1_ACTIVE, **kw)
        _same_bits(p0, r0, *L.fit('c'))
        _same_pass(c.batch_pass(p5, BC.PART1_ACTIVE), pass0)
        c.set_batch_data(*L.batch.first(3))
        p3, r3, _ = c.fit_batch(starts[:3], BC.PART1_ACTIVE, **kw)
        _same_bits(p3, r3, p0[:3], r0[:3])
        _same_pass(c.batch_pass(p5[:3], BC.PART1_ACTIVE), [v[:3] for v in pass0])
        c.set_batch_data(L.batch.off, L.batch.x, L.batch.y, L.batch.w)
        _same_pass(c.batch_pass(p5, BC.PART1_ACTIVE), pass0)
        p1, r1, _ = c.fit_batch(starts, BC.PART1_ACTIVE, **kw)
        _same_bits(p1, r1, p0, r0)
        out, r = plain(c)
        p2, r2, _ = c.fit_batch(starts, BC.PART1_ACTIVE, **kw)          # ... and the batch is still there after the plain fit
        _same_bits(p2, r2, p0, r0)
    finally:
        c.close()
    f = _context(L.tape)
    try:
        out0, rf = plain(f)
    finally:
        f.close()
    assert np.array_equal(out, out0)
    assert tuple(int(getattr(r, v)) for v in COUNTS) == tuple(int(getattr(rf, v)) for v in COUNTS)
    assert r.chi2 == rf.chi2 and r.lambda_ == rf.lambda_


# ---- Part 2: every active count, in the caller's order ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def E():
    tape, truths, batch = BC.part2()
    c = _context(tape, batch)
    yield tape, batch, c
    c.close()


@pytest.mark.parametrize('idx', range(8))
@pytest.mark.parametrize('name', sorted(BC.EXP4_ARGS))
def test_every_active_count_against_the_oracle(E, name, idx):
    """1 ... 8 active parameters of model_exp4, the lists as the caller orders them: the oracle is given the same list in the same order"""
    tape, batch, c = E
    off, kw = BC.EXP4_ARGS[name]
    active = BC.exp4_sets(name)[idx]
    sel = BC.part2_select(active, off, kw)
    assert all(s[0] for s in sel)
    starts = BC.part2_starts(active, off)
    pars, res, _ = c.fit_batch(starts, active, **kw)
    passive = [k for k in range(8) if k not in active]
    assert np.array_equal(pars[:, passive], starts[:, passive])
    print('exp4 %s %s: iterations %s, exits %s' % (name, active, sorted(set(res['iterations'].tolist())), sorted(set(res['exit_reason'].tolist()))))
    _check_fit('exp4_%s_na%d' % (name, len(active)), _fit_worst(sel, pars, res, batch.n, len(active)))
    if name == 'conv':
        JTJ, JTr, chi2 = c.batch_pass(starts, active)
        worst = _pass_worst(tape, batch.items, starts, active, JTJ, JTr, chi2)
        _observe(**{'shapes_exp4_pass_na%d' % len(active): worst})
        assert worst < TOL_PASS


@pytest.mark.parametrize('which', sorted(BC.EXP4_ORDER))
def test_the_callers_order_reaches_every_column(E, which):
    """[6, 1, 4] and [1, 4, 6] with DTD_min permuted alike: each against the oracle given the same list and values, and the two device
    results against each other.  'binding': values that exceed J^T J's diagonal for parameters 6 and 4, so a value on the wrong column
    is another fit."""
    tape, batch, c = E
    off, kw = BC.EXP4_ORDER_ARGS
    got = []
    for active, dtd in BC.EXP4_ORDER[which]:
        sel = BC.part2_select(active, off, kw, dtd)
        assert all(s[0] for s in sel)
        starts = BC.part2_starts(active, off)
        pars, res, _ = c.fit_batch(starts, active, DTD_min=dtd, **kw)
        _check_fit('order_%s_%s' % (which, ''.join(str(a) for a in active)), _fit_worst(sel, pars, res, batch.n, 3))
        got.append((pars, res))
        JTJ, JTr, chi2 = c.batch_pass(starts, active)
        assert _pass_worst(tape, batch.items, starts, active, JTJ, JTr, chi2) < TOL_PASS
    (pa, ra), (pb, rb) = got
    for f in COUNTS:
        assert np.array_equal(ra[f], rb[f]), f
    between = float(np.max(np.abs(pa - pb) / np.abs(pa)))
    _observe(**{'shapes_order_%s_between' % which: between})
    assert between < TOL_FIT


# ---- Part 3: the whole operator set --------------------------------------------------------------------------------------------------
def _operator_pass(seed, c):
    tape, active, starts, batch = BC.part3(seed)
    JTJ, JTr, chi2 = c.batch_pass(starts, active)
    return _pass_worst(tape, batch.items, starts, active, JTJ, JTr, chi2)


@pytest.mark.parametrize('seed', BC.OPERATOR_SEEDS)
def test_operator_set_against_the_oracle(seed):
    """p[0] e_0 + ... + p[4] e_4 with random expressions over pow in its four forms, log, sqrt, exp, the trigonometric and hyperbolic
    functions and their inverses, and (seed 32) the written model with erf, a bare abs and unary minus, which the random expressions
    never draw: gfh_point_grad, gfh_point_value and gfh_point_dd_grad inside the batch unit.  Under (i)
    delta2 is always kept, so one iteration is old + delta1 + delta2 / 2 of a well-damped system: STEP 3 without conditioning."""
    tape, active, starts, batch = BC.part3(seed)
    c = _context(tape, batch)
    try:
        worst = _operator_pass(seed, c)
        _observe(shapes_random_pass=worst)
        assert worst < TOL_PASS
        for name, kw in BC.RANDOM_ARGS.items():
            sel = BC.part3_selection(seed, name)
            pars, res, _ = c.fit_batch(starts, active, **kw)
            passive = [k for k in range(BC.NP_) if k not in active]
            assert np.array_equal(pars[:, passive], starts[:, passive])
            if name == 'i':
                assert np.all(res['n_omega'] == 1) and np.all(res['iterations'] == 1)
            _check_fit('random_%s' % name, _fit_worst(sel, pars, res, batch.n, len(active)))
    finally:
        c.close()


def test_operator_set_with_the_librarys_pow_and_divisions(monkeypatch):
    """a model with x ** a on a context created under GADFIT_HIP_FAST_DIV=0 (read when the context is created): the same bound"""
    seed = BC.RANDOM_POW_SEED
    tape, active, starts, batch = BC.part3(seed)
    monkeypatch.setenv('GADFIT_HIP_FAST_DIV', '0')
    c = _context(tape, batch)
    try:
        src = c.batch_source(active)
        assert '#define GFH_FAST_DIV 0' in src and 'gfh_pow_ln(' not in src
        worst = _operator_pass(seed, c)
    finally:
        c.close()
    _observe(shapes_random_pass_library_pow=worst)
    assert worst < TOL_PASS
