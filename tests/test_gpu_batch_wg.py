"""The 256-lane form of the batch kernels (gfh_set_batch_lanes(256) / lanes_per_fit=256: a workgroup of four waves per fit, the four
waves' partial sums added in wave order after one barrier per reduction) over spectrum lengths at the edges of each wave's share of
a 256-point row and of one to four rows, every active count 1 ... 8, single fits and cut batches, neighbours filled with NaN, a
batch of more than 65535 workgroups, and the three forms side by side in one context.

The inputs are in tests/batch_wg_cases.py; the rule that selects which fits may be held against the oracle is batch_cases.select
(the oracle's alone: nothing the device returns enters it), and tests/test_cpu_batch_wg.py shows without a GPU what it drops.
Bounds (the project's own): one pass TOL_PASS = 2e-13 scaled as in test_one_pass_against_the_oracle, the counts and the exit reason
equal, lambda TOL_LAMBDA = 1e-14, fitted parameters and chi2 of Part W1 test_gpu_batch.py's TOL_PARS = TOL_CHI2 = 3e-12 and of
Part 2 test_gpu_batch_shapes.py's 1e-10.  The observed maxima go where test_gpu_batch.py's go (GADFIT_BATCH_OBSERVE) under the keys
wg_*; tools/bench_batch.py --workgroup --observed copies them into profiles/batch_workgroup.json."""
import numpy as np
import pytest

from tests import batch_cases as BC
from tests import batch_wg_cases as WC
from tests.test_gpu_batch import COUNTS, SCENARIOS, TOL_CHI2, TOL_LAMBDA, TOL_PARS, TOL_PASS, _observe, _same_bits
from tests.test_gpu_batch_shapes import TOL_FIT, _context, _fit_worst, _pass_worst, _same_pass

pytestmark = pytest.mark.gpu


def _check_fit(key, worst, tol_pars=TOL_PARS, tol_chi2=TOL_CHI2):
    _observe(**{'wg_%s_lambda' % key: worst['lam'], 'wg_%s_pars' % key: worst['pars'], 'wg_%s_chi2' % key: worst['chi2']})
    assert worst['lam'] <= TOL_LAMBDA and worst['pars'] < tol_pars and worst['chi2'] < tol_chi2


class Workgroups:
    """the batch of 138 on one context; every call names its form (lanes_per_fit stays set on a context)"""

    def __init__(self):
        self.tape, self.order, self.truths, self.batch = WC.w1()
        self.n = self.batch.n
        self.ctx = _context(self.tape, self.batch)
        self._fits, self._pass = {}, None

    def fit(self, name, lanes=256):
        """(cached: later tests compare other batches with it bit for bit)"""
        if (name, lanes) not in self._fits:
            off, kw = SCENARIOS[name]
            self._fits[name, lanes] = self.ctx.fit_batch(WC.w1_starts(off), WC.ACTIVE, lanes_per_fit=lanes, **kw)[:2]
            assert self.ctx.batch_lanes_used() == lanes
        return self._fits[name, lanes]

    def one_pass(self):
        if self._pass is None:
            self._pass = self.ctx.batch_pass(WC.w1_starts(0.05), WC.ACTIVE, lanes_per_fit=256)
            assert self.ctx.batch_lanes_used() == 256
        return self._pass


@pytest.fixture(scope='module')
def W():
    s = Workgroups()
    yield s
    s.ctx.close()


# ---- 1: W1 against the oracle --------------------------------------------------------------------------------------------------------
def test_wg_one_pass_against_the_oracle(W):
    """n = 4 ... 4097: one live wave (n <= 64), the last live lane / the first masked lane at each wave's edge of the first row, one
    to four rows with the last one full, one short or followed by a single live lane, and 17 rows; all 138 spectra, none dropped.
    J^T J symmetric bit for bit (_pass_worst)."""
    JTJ, JTr, chi2 = W.one_pass()
    worst = _pass_worst(W.tape, W.batch.items, WC.w1_starts(0.05), WC.ACTIVE, JTJ, JTr, chi2)
    _observe(wg_lengths_pass=worst)
    assert worst < TOL_PASS


@pytest.mark.parametrize('name', WC.FIT_SCENARIOS)
def test_wg_fits_against_the_oracle(W, name):
    """all 138 fits are kept by the rule; (a) runs to convergence with rejections, (c) through STEP 3"""
    sel = WC.w1_selection(name)
    assert all(s[0] for s in sel)
    pars, res = W.fit(name)
    print('wg (%s): iterations %s, exits %s' % (name, sorted(set(res['iterations'].tolist())), sorted(set(res['exit_reason'].tolist()))))
    _check_fit('lengths_%s' % name, _fit_worst(sel, pars, res, W.n, 4))


@pytest.mark.parametrize('name', WC.ONE_SCENARIOS)
def test_wg_with_one_active_parameter(W, name):
    """active = [1]: the 1 x 1 instance of the solve and a sweep image of 3 values (the fits the rule keeps; every one's pass)"""
    sel = WC.w1_selection(name, True)
    off, kw = SCENARIOS[name]
    starts = WC.w1_starts(off, WC.ONE_ACTIVE)
    pars, res, _ = W.ctx.fit_batch(starts, WC.ONE_ACTIVE, lanes_per_fit=256, **kw)
    assert W.ctx.batch_lanes_used() == 256
    assert np.array_equal(pars[:, [0, 2, 3]], starts[:, [0, 2, 3]])          # the passive parameters come back bit for bit
    _check_fit('one_active_%s' % name, _fit_worst(sel, pars, res, W.n, 1))
    JTJ, JTr, chi2 = W.ctx.batch_pass(starts, WC.ONE_ACTIVE, lanes_per_fit=256)
    assert W.ctx.batch_lanes_used() == 256
    worst = _pass_worst(W.tape, W.batch.items, starts, WC.ONE_ACTIVE, JTJ, JTr, chi2)
    _observe(wg_one_active_pass=worst)
    assert worst < TOL_PASS


# ---- 2: every active count, in the caller's order ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def E():
    tape, truths, batch = BC.part2()
    c = _context(tape, batch)
    c.set_batch_lanes(256)
    yield tape, batch, c
    c.close()


@pytest.mark.parametrize('idx', range(8))
@pytest.mark.parametrize('name', sorted(BC.EXP4_ARGS))
def test_wg_every_active_count_against_the_oracle(E, name, idx):
    """1 ... 8 active parameters of model_exp4 at 256 lanes (LDS images of 3 ... 45 values per wave), as Part 2 of
    test_gpu_batch_shapes.py runs them at 64 (128 ... 512 points: one and two rows per pass); 'short' runs STEP 3.  Part 2's
    selection drops none of these fits."""
    tape, batch, c = E
    off, kw = BC.EXP4_ARGS[name]
    active = BC.exp4_sets(name)[idx]
    sel = BC.part2_select(active, off, kw)
    assert all(s[0] for s in sel)
    starts = BC.part2_starts(active, off)
    pars, res, _ = c.fit_batch(starts, active, **kw)
    assert c.batch_lanes_used() == 256
    passive = [k for k in range(8) if k not in active]
    assert np.array_equal(pars[:, passive], starts[:, passive])
    _check_fit('exp4_%s_na%d' % (name, len(active)), _fit_worst(sel, pars, res, batch.n, len(active)), TOL_FIT, TOL_FIT)
    if name == 'conv':
        JTJ, JTr, chi2 = c.batch_pass(starts, active)
        assert c.batch_lanes_used() == 256
        worst = _pass_worst(tape, batch.items, starts, active, JTJ, JTr, chi2)
        _observe(**{'wg_exp4_pass_na%d' % len(active): worst})
        assert worst < TOL_PASS


@pytest.mark.parametrize('which', sorted(BC.EXP4_ORDER))
def test_wg_the_callers_order_reaches_every_column(E, which):
    """[6, 1, 4] and [1, 4, 6] with DTD_min permuted alike, at 256 lanes: each against the oracle given the same list and values, and
    the two device results against each other"""
    tape, batch, c = E
    off, kw = BC.EXP4_ORDER_ARGS
    got = []
    for active, dtd in BC.EXP4_ORDER[which]:
        sel = BC.part2_select(active, off, kw, dtd)
        assert all(s[0] for s in sel)
        starts = BC.part2_starts(active, off)
        pars, res, _ = c.fit_batch(starts, active, DTD_min=dtd, **kw)
        assert c.batch_lanes_used() == 256
        _check_fit('order_%s_%s' % (which, ''.join(str(a) for a in active)), _fit_worst(sel, pars, res, batch.n, 3), TOL_FIT, TOL_FIT)
        got.append((pars, res))
        JTJ, JTr, chi2 = c.batch_pass(starts, active)
        assert _pass_worst(tape, batch.items, starts, active, JTJ, JTr, chi2) < TOL_PASS
    (pa, ra), (pb, rb) = got
    for f in COUNTS:
        assert np.array_equal(ra[f], rb[f]), f
    assert float(np.max(np.abs(pa - pb) / np.abs(pa))) < TOL_FIT


# ---- 3: up to 64 points the workgroup form returns the wave form's bits -----------------------------------------------------------
def test_same_bits_as_the_wave_form_up_to_64_points(W):
    """The 24 spectra of W1 with n = 4, 5, 63, 64 as a batch of their own.  Wave 0's lanes hold the same per-lane values in both forms
    (one row, lane l takes point l); waves 1 ... 3 have w = 0 in every lane, their accumulators start at +0.0 and only +-0 is added
    to them, so their partial sums are exact +0.0 and ((p0 + 0.0) + 0.0) + 0.0 is p0; contraction is decided per source expression
    (-ffp-contract=on) in the one text both forms are compiled from, and the solve is contract(off) in both."""
    idx = [k for k in range(138) if W.n[k] <= WC.SAME_BITS_MAX_N]
    assert len(idx) == 24 and set(W.n[idx]) == {4, 5, 63, 64}
    sub = WC.sub_batch(idx)
    c = _context(W.tape, sub)
    try:
        for active, names in ((WC.ACTIVE, WC.FIT_SCENARIOS), (WC.ONE_ACTIVE, WC.ONE_SCENARIOS)):
            p5 = WC.w1_starts(0.05, active)[idx]
            pass256 = c.batch_pass(p5, active, lanes_per_fit=256)
            assert c.batch_lanes_used() == 256
            pass64 = c.batch_pass(p5, active, lanes_per_fit=64)
            assert c.batch_lanes_used() == 64
            _same_pass(pass256, pass64)
            for name in names:
                off, kw = SCENARIOS[name]
                starts = WC.w1_starts(off, active)[idx]
                p256, r256, _ = c.fit_batch(starts, active, lanes_per_fit=256, **kw)
                assert c.batch_lanes_used() == 256
                p64, r64, _ = c.fit_batch(starts, active, lanes_per_fit=64, **kw)
                assert c.batch_lanes_used() == 64
                _same_bits(p256, r256, p64, r64)
    finally:
        c.close()


# ---- 4: a fit does not depend on its neighbours or on the grid ---------------------------------------------------------------------
def test_a_fit_does_not_depend_on_the_grid_or_its_neighbours(W):
    """each fit alone (a grid of one workgroup), the batch reversed (another workgroup index, other neighbours), and the batch cut to
    5, 2 and 1 fits: every fit returns the bits it returned in the batch of 138, from batch_pass and from fit_batch under (a) and (c)"""
    p5 = WC.w1_starts(0.05)
    full = {name: W.fit(name) for name in ('a', 'c')}
    c = _context(W.tape)
    c.set_batch_lanes(256)
    try:
        def same(idx):
            sub = WC.sub_batch(idx)
            c.set_batch_data(sub.off, sub.x, sub.y, sub.w)
            _same_pass(c.batch_pass(p5[idx], WC.ACTIVE), [v[idx] for v in W.one_pass()])
            for name, (pars, res) in full.items():
                off, kw = SCENARIOS[name]
                p1, r1, _ = c.fit_batch(WC.w1_starts(off)[idx], WC.ACTIVE, **kw)
                _same_bits(p1, r1, pars[idx], res[idx])
            assert c.batch_lanes_used() == 256
        for k in range(138):
            same([k])
        same(list(range(137, -1, -1)))
        for k in WC.CUTS:
            same(list(range(k)))
    finally:
        c.close()


def test_a_fit_reads_no_point_of_its_neighbours(W):
    """Every other spectrum's x, y and w are NaN (both parities): the clean fits return the bits of the undisturbed batch from both
    kernels; the poisoned fits end at their first solve (exit 8, in all four waves alike: the kernel returns) with their start
    parameters.  A NaN that came through a w = 0 mask, or a read past a spectrum's end into its neighbour's, would show."""
    p5 = WC.w1_starts(0.05)
    f = np.arange(138)
    c = _context(W.tape)
    c.set_batch_lanes(256)
    try:
        for clean in (f % 2 == 0, f % 2 == 1):
            pt = np.repeat(clean, W.n)
            x, y, w = (np.where(pt, v, np.nan) for v in (W.batch.x, W.batch.y, W.batch.w))
            c.set_batch_data(W.batch.off, x, y, w)
            _same_pass([v[clean] for v in c.batch_pass(p5, WC.ACTIVE)], [v[clean] for v in W.one_pass()])
            assert c.batch_lanes_used() == 256
            for name in ('a', 'c'):
                off, kw = SCENARIOS[name]
                starts = WC.w1_starts(off)
                pars, res = W.fit(name)
                p1, r1, _ = c.fit_batch(starts, WC.ACTIVE, **kw)
                assert c.batch_lanes_used() == 256
                _same_bits(p1[clean], r1[clean], pars[clean], res[clean])
                bad = ~clean
                assert np.all(r1['exit_reason'][bad] == 8) and np.all(r1['iterations'][bad] == 0)
                assert np.all(r1['n_sweeps'][bad] == 1) and np.all(r1['n_chi2'][bad] == 1)
                assert np.array_equal(p1[bad], starts[bad])
    finally:
        c.close()


# ---- 5: more workgroups than 65535 -------------------------------------------------------------------------------------------------
def test_wg_a_batch_of_70003_fits(W):
    """the 84 spectra of up to 257 points tiled to 70003 fits, one workgroup each, under (b): every copy returns the bits of its first
    occurrence, the first 84 are held against the oracle and are the bits of the same spectra in the batch of 138"""
    short = [k for k in range(138) if W.n[k] <= WC.LARGE_MAX_N]
    assert len(short) == 84
    nf = WC.LARGE_FITS
    assert nf > 65535
    reps = -(-nf // 84)
    sub = WC.sub_batch(short)
    n_all = np.tile(sub.n, reps)[:nf]
    off_all = np.concatenate([[0], np.cumsum(n_all)]).astype(np.int64)
    cut = int(off_all[-1])
    off_b, kw = SCENARIOS['b']
    starts84 = WC.w1_starts(off_b)[short]
    starts = np.tile(starts84, (reps, 1))[:nf]
    c = _context(W.tape)
    try:
        c.set_batch_data(off_all, np.tile(sub.x, reps)[:cut], np.tile(sub.y, reps)[:cut], np.tile(sub.w, reps)[:cut])
        pars, res, _ = c.fit_batch(starts, WC.ACTIVE, lanes_per_fit=256, **kw)
        assert c.batch_lanes_used() == 256
    finally:
        c.close()
    first = np.arange(nf) % 84
    _same_bits(pars, res, pars[first], res[first])
    sel = [WC.w1_selection('b')[k] for k in short]
    _check_fit('large_batch', _fit_worst(sel, pars[:84], res[:84], W.n[short], 4))
    p138, r138 = W.fit('b')
    _same_bits(pars[:84], res[:84], p138[short], r138[short])


# ---- 6: the three forms in one context ---------------------------------------------------------------------------------------------
def test_switching_forms_in_one_context(W):
    """64 -> 256 -> 16 -> 256 -> batch_pass at 256 -> a plain set_data + fit -> 256 once more, on one context and the same data: the
    three forms of the active set are resident side by side (the kernel cache's key carries the form), every result is the bits of
    the first call in that form and of a fresh context, and the plain fit returns what a fresh context returns"""
    off, kw = SCENARIOS['c']
    starts, p5 = WC.w1_starts(off), WC.w1_starts(0.05)
    k = next(i for i in range(138) if W.n[i] == 257)
    x, y, w = W.batch.items[k]
    sigma = 1.0 / w

    def plain(ctx):
        ctx.set_data(x, y, sigma, [0, x.size])
        ctx.init_weights(4)
        return ctx.fit([starts[k]], WC.ACTIVE, [0] * 4, **kw)
    c = _context(W.tape, W.batch)
    try:
        p64, r64, _ = c.fit_batch(starts, WC.ACTIVE, **kw)
        assert c.batch_lanes_used() == 64
        p256, r256, _ = c.fit_batch(starts, WC.ACTIVE, lanes_per_fit=256, **kw)
        assert c.batch_lanes_used() == 256
        _same_bits(p256, r256, *W.fit('c'))                      # (the module's context: another one)
        p16, r16, _ = c.fit_batch(starts, WC.ACTIVE, lanes_per_fit=16, **kw)
        assert c.batch_lanes_used() == 16
        p, r, _ = c.fit_batch(starts, WC.ACTIVE, lanes_per_fit=256, **kw)
        assert c.batch_lanes_used() == 256
        _same_bits(p, r, p256, r256)
        _same_pass(c.batch_pass(p5, WC.ACTIVE, lanes_per_fit=256), W.one_pass())
        assert c.batch_lanes_used() == 256
        out, rp = plain(c)
        p, r, _ = c.fit_batch(starts, WC.ACTIVE, **kw)           # ... and the batch and the setting are still there after the plain fit
        assert c.batch_lanes_used() == 256
        _same_bits(p, r, p256, r256)
    finally:
        c.close()
    f = _context(W.tape, W.batch)
    try:
        p, r, _ = f.fit_batch(starts, WC.ACTIVE, **kw)
        assert f.batch_lanes_used() == 64
        _same_bits(p, r, p64, r64)
        p, r, _ = f.fit_batch(starts, WC.ACTIVE, lanes_per_fit=16, **kw)
        assert f.batch_lanes_used() == 16
        _same_bits(p, r, p16, r16)
        out0, rf = plain(f)
    finally:
        f.close()
    assert np.array_equal(out, out0)
    assert tuple(int(getattr(rp, v)) for v in COUNTS) == tuple(int(getattr(rf, v)) for v in COUNTS)
    assert rp.chi2 == rf.chi2 and rp.lambda_ == rf.lambda_
