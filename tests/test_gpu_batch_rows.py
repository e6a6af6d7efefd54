"""The 16-lane form of the batch kernels (gfh_set_batch_lanes(16) / lanes_per_fit=16: a DPP row per fit, four fits per wave, sixteen
per workgroup) over spectrum lengths at the row's edges, every active count 1 ... 8, batch sizes that leave rows, waves and a last
workgroup without a fit, neighbours filled with NaN inside one wave, a batch of 2^17 + 3 fits, and both forms side by side in one
context.

The inputs are in tests/batch_row_cases.py; the rule that selects which fits may be held against the oracle is batch_cases.select
(the oracle's alone: nothing the device returns enters it), and tests/test_cpu_batch_rows.py shows without a GPU what it drops.
Bounds (the project's own, tests/test_gpu_batch_shapes.py): one pass TOL_PASS = 2e-13 scaled as in test_one_pass_against_the_oracle,
the counts and the exit reason equal, lambda TOL_LAMBDA = 1e-14, fitted parameters and chi2 north_star's 1e-10.  The observed maxima
go where test_gpu_batch.py's go (GADFIT_BATCH_OBSERVE) under the keys rows_*; tools/bench_batch.py copies them into
profiles/batch_rows.json."""
import numpy as np
import pytest

from gadfit_amd import _lib
from tests import batch_cases as BC
from tests import batch_row_cases as RC
from tests.test_gpu_batch import COUNTS, SCENARIOS, TOL_LAMBDA, TOL_PASS, _observe, _same_bits
from tests.test_gpu_batch_shapes import TOL_FIT, _context, _fit_worst, _pass_worst, _same_pass

pytestmark = pytest.mark.gpu


def _check_fit(key, worst):
    _observe(**{'rows_%s_lambda' % key: worst['lam'], 'rows_%s_pars' % key: worst['pars'], 'rows_%s_chi2' % key: worst['chi2']})
    assert worst['lam'] <= TOL_LAMBDA and worst['pars'] < TOL_FIT and worst['chi2'] < TOL_FIT


class Rows:
    """the batch of 114 on one context; every call names its form (lanes_per_fit stays set on a context)"""

    def __init__(self):
        self.tape, self.order, self.truths, self.batch = RC.r1()
        self.n = self.batch.n
        self.ctx = _context(self.tape, self.batch)
        self._fits, self._pass = {}, None

    def fit(self, name, lanes=16):
        """(cached: later tests compare other batches with it bit for bit)"""
        if (name, lanes) not in self._fits:
            off, kw = SCENARIOS[name]
            self._fits[name, lanes] = self.ctx.fit_batch(RC.r1_starts(off), RC.ACTIVE, lanes_per_fit=lanes, **kw)[:2]
            assert self.ctx.batch_lanes_used() == lanes
        return self._fits[name, lanes]

    def one_pass(self):
        if self._pass is None:
            self._pass = self.ctx.batch_pass(RC.r1_starts(0.05), RC.ACTIVE, lanes_per_fit=16)
            assert self.ctx.batch_lanes_used() == 16
        return self._pass


@pytest.fixture(scope='module')
def R():
    s = Rows()
    yield s
    s.ctx.close()


# ---- 1, 2: lengths at the row's edges against the oracle ---------------------------------------------------------------------------
def test_rows_one_pass_against_the_oracle(R):
    """n = 4 ... 257: a quarter of a row, one masked lane (15), a full row (16), one live lane in the second row (17), ... , 17 rows;
    all 114 spectra, those the rule drops from the fit comparisons included.  J^T J symmetric bit for bit (_pass_worst)."""
    JTJ, JTr, chi2 = R.one_pass()
    worst = _pass_worst(R.tape, R.batch.items, RC.r1_starts(0.05), RC.ACTIVE, JTJ, JTr, chi2)
    _observe(rows_lengths_pass=worst)
    assert worst < TOL_PASS


@pytest.mark.parametrize('name', RC.FIT_SCENARIOS)
def test_rows_fits_against_the_oracle(R, name):
    """all 114 fits are kept by the rule; the four fits of a wave have different lengths and leave their loops at different iterations"""
    sel = RC.r1_selection(name)
    assert all(s[0] for s in sel)
    pars, res = R.fit(name)
    print('rows (%s): iterations %s, exits %s' % (name, sorted(set(res['iterations'].tolist())), sorted(set(res['exit_reason'].tolist()))))
    _check_fit('lengths_%s' % name, _fit_worst(sel, pars, res, R.n, 4))


@pytest.mark.parametrize('name', RC.ONE_SCENARIOS)
def test_rows_with_one_active_parameter(R, name):
    """active = [1]: the 1 x 1 instance of the solve and the accumulators in the row form (the fits the rule keeps; every one's pass)"""
    sel = RC.r1_selection(name, True)
    off, kw = SCENARIOS[name]
    starts = RC.r1_starts(off, RC.ONE_ACTIVE)
    pars, res, _ = R.ctx.fit_batch(starts, RC.ONE_ACTIVE, lanes_per_fit=16, **kw)
    assert R.ctx.batch_lanes_used() == 16
    assert np.array_equal(pars[:, [0, 2, 3]], starts[:, [0, 2, 3]])          # the passive parameters come back bit for bit
    _check_fit('one_active_%s' % name, _fit_worst(sel, pars, res, R.n, 1))
    JTJ, JTr, chi2 = R.ctx.batch_pass(starts, RC.ONE_ACTIVE, lanes_per_fit=16)
    worst = _pass_worst(R.tape, R.batch.items, starts, RC.ONE_ACTIVE, JTJ, JTr, chi2)
    _observe(rows_one_active_pass=worst)
    assert worst < TOL_PASS


def test_the_form_is_the_callers_and_64_without_the_argument(R):
    """a context nobody told anything launches the wave form; lanes_per_fit=16 the row form, and the setting stays; set_batch_lanes(64) goes back"""
    off, kw = SCENARIOS['a']
    k = 9
    c = _context(R.tape)
    try:
        c.set_batch_data(*R.batch.first(k))
        assert c.batch_lanes_used() == 0
        c.fit_batch(RC.r1_starts(off)[:k], RC.ACTIVE, **kw)
        assert c.batch_lanes_used() == 64
        c.batch_pass(RC.r1_starts(off)[:k], RC.ACTIVE, lanes_per_fit=16)
        assert c.batch_lanes_used() == 16
        c.fit_batch(RC.r1_starts(off)[:k], RC.ACTIVE, **kw)
        assert c.batch_lanes_used() == 16
        c.set_batch_lanes(64)
        c.batch_pass(RC.r1_starts(off)[:k], RC.ACTIVE)
        assert c.batch_lanes_used() == 64
        c.set_batch_lanes(0)                                     # auto: the rule's form for (4 active, longest of these 9)
        c.fit_batch(RC.r1_starts(off)[:k], RC.ACTIVE, **kw)
        assert c.batch_lanes_used() == _lib.batch_auto_lanes(4, int(R.n[:k].max()))
    finally:
        c.close()


# ---- 3: every active count, in the caller's order ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def E():
    tape, truths, batch = BC.part2()
    c = _context(tape, batch)
    c.set_batch_lanes(16)
    yield tape, batch, c
    c.close()


@pytest.mark.parametrize('idx', range(8))
@pytest.mark.parametrize('name', sorted(BC.EXP4_ARGS))
def test_rows_every_active_count_against_the_oracle(E, name, idx):
    """1 ... 8 active parameters of model_exp4 at 16 lanes, as Part 2 of test_gpu_batch_shapes.py runs them at 64 (128 ... 512 points:
    8 ... 32 rows per pass); 'short' runs STEP 3.  Part 2's selection drops none of these fits."""
    tape, batch, c = E
    off, kw = BC.EXP4_ARGS[name]
    active = BC.exp4_sets(name)[idx]
    sel = BC.part2_select(active, off, kw)
    assert all(s[0] for s in sel)
    starts = BC.part2_starts(active, off)
    pars, res, _ = c.fit_batch(starts, active, **kw)
    assert c.batch_lanes_used() == 16
    passive = [k for k in range(8) if k not in active]
    assert np.array_equal(pars[:, passive], starts[:, passive])
    _check_fit('exp4_%s_na%d' % (name, len(active)), _fit_worst(sel, pars, res, batch.n, len(active)))
    if name == 'conv':
        JTJ, JTr, chi2 = c.batch_pass(starts, active)
        worst = _pass_worst(tape, batch.items, starts, active, JTJ, JTr, chi2)
        _observe(**{'rows_exp4_pass_na%d' % len(active): worst})
        assert worst < TOL_PASS


@pytest.mark.parametrize('which', sorted(BC.EXP4_ORDER))
def test_rows_the_callers_order_reaches_every_column(E, which):
    """[6, 1, 4] and [1, 4, 6] with DTD_min permuted alike, at 16 lanes: each against the oracle given the same list and values, and the
    two device results against each other"""
    tape, batch, c = E
    off, kw = BC.EXP4_ORDER_ARGS
    got = []
    for active, dtd in BC.EXP4_ORDER[which]:
        sel = BC.part2_select(active, off, kw, dtd)
        assert all(s[0] for s in sel)
        starts = BC.part2_starts(active, off)
        pars, res, _ = c.fit_batch(starts, active, DTD_min=dtd, **kw)
        assert c.batch_lanes_used() == 16
        _check_fit('order_%s_%s' % (which, ''.join(str(a) for a in active)), _fit_worst(sel, pars, res, batch.n, 3))
        got.append((pars, res))
        JTJ, JTr, chi2 = c.batch_pass(starts, active)
        assert _pass_worst(tape, batch.items, starts, active, JTJ, JTr, chi2) < TOL_PASS
    (pa, ra), (pb, rb) = got
    for f in COUNTS:
        assert np.array_equal(ra[f], rb[f]), f
    assert float(np.max(np.abs(pa - pb) / np.abs(pa))) < TOL_FIT


# ---- 4: up to 16 points the two forms return the same bits -----------------------------------------------------------------------
def test_same_bits_in_both_forms_up_to_16_points(R):
    """The 42 spectra of R1 with n <= 16 as a batch of their own.  With at most one point per lane both forms add the same values
    through the same row tree -- the wave form adds the exact zeros of its 48 lanes with w = 0 first, and lane 0 of the row form's
    rotation butterfly is the row levels of gfh_wave_sum with operands commuted -- contraction is decided per source expression
    (-ffp-contract=on) in the one text both forms are compiled from, and the solve is contract(off) in both."""
    idx = [k for k in range(114) if R.n[k] <= RC.SAME_BITS_MAX_N]
    assert len(idx) == 42 and set(R.n[idx]) == {4, 5, 7, 8, 9, 15, 16}
    sub = RC.sub_batch(idx)
    c = _context(R.tape, sub)
    try:
        for active, names in ((RC.ACTIVE, RC.FIT_SCENARIOS), (RC.ONE_ACTIVE, RC.ONE_SCENARIOS)):
            p5 = RC.r1_starts(0.05, active)[idx]
            pass16 = c.batch_pass(p5, active, lanes_per_fit=16)
            pass64 = c.batch_pass(p5, active, lanes_per_fit=64)
            assert c.batch_lanes_used() == 64
            _same_pass(pass16, pass64)
            for name in names:
                off, kw = SCENARIOS[name]
                starts = RC.r1_starts(off, active)[idx]
                p16, r16, _ = c.fit_batch(starts, active, lanes_per_fit=16, **kw)
                p64, r64, _ = c.fit_batch(starts, active, lanes_per_fit=64, **kw)
                _same_bits(p16, r16, p64, r64)
    finally:
        c.close()


# ---- 5: a fit does not depend on its row or its neighbours ------------------------------------------------------------------------
def test_a_fit_does_not_depend_on_its_row_or_its_neighbours(R):
    """each fit alone (row 0 of a wave whose other rows are gone), the batch reversed (another row, other neighbours), and the batch cut
    to 17, 16, 15, 5, 4, 3 and 1 fits (a second workgroup with one live row; a full workgroup; a last wave with three rows, one row;
    a full wave; three rows; one): every fit returns the bits it returned in the batch of 114, from batch_pass and from fit_batch
    under (a) and (c)"""
    p5 = RC.r1_starts(0.05)
    full = {name: R.fit(name) for name in ('a', 'c')}
    c = _context(R.tape)
    c.set_batch_lanes(16)
    try:
        def same(idx):
            sub = RC.sub_batch(idx)
            c.set_batch_data(sub.off, sub.x, sub.y, sub.w)
            _same_pass(c.batch_pass(p5[idx], RC.ACTIVE), [v[idx] for v in R.one_pass()])
            for name, (pars, res) in full.items():
                off, kw = SCENARIOS[name]
                p1, r1, _ = c.fit_batch(RC.r1_starts(off)[idx], RC.ACTIVE, **kw)
                _same_bits(p1, r1, pars[idx], res[idx])
            assert c.batch_lanes_used() == 16
        for k in range(114):
            same([k])
        same(list(range(113, -1, -1)))
        for k in RC.CUTS:
            same(list(range(k)))
    finally:
        c.close()


# ---- 6: NaN in the neighbouring rows of a wave -----------------------------------------------------------------------------------
def test_a_fit_reads_no_point_of_the_other_rows_of_its_wave(R):
    """Every other spectrum's x, y and w are NaN (both parities), then all but every fourth (each of the four rows of a wave in turn
    the only clean one: three rows fail at iteration 0 while the fourth runs to convergence under (a), through STEP 3 under (c)): the
    clean fits return the bits of the undisturbed batch from both kernels; the poisoned fits end at their first solve (exit 8) with
    their start parameters.  A NaN that came through a w = 0 mask or a DPP move from another row would show."""
    p5 = RC.r1_starts(0.05)
    f = np.arange(114)
    c = _context(R.tape)
    c.set_batch_lanes(16)
    try:
        for clean in [f % 2 == 0, f % 2 == 1] + [f % 4 == k for k in range(4)]:
            pt = np.repeat(clean, R.n)
            x, y, w = (np.where(pt, v, np.nan) for v in (R.batch.x, R.batch.y, R.batch.w))
            c.set_batch_data(R.batch.off, x, y, w)
            _same_pass([v[clean] for v in c.batch_pass(p5, RC.ACTIVE)], [v[clean] for v in R.one_pass()])
            for name in ('a', 'c'):
                off, kw = SCENARIOS[name]
                starts = RC.r1_starts(off)
                pars, res = R.fit(name)
                p1, r1, _ = c.fit_batch(starts, RC.ACTIVE, **kw)
                _same_bits(p1[clean], r1[clean], pars[clean], res[clean])
                bad = ~clean
                assert np.all(r1['exit_reason'][bad] == 8) and np.all(r1['iterations'][bad] == 0)
                assert np.all(r1['n_sweeps'][bad] == 1) and np.all(r1['n_chi2'][bad] == 1)
                assert np.array_equal(p1[bad], starts[bad])
    finally:
        c.close()


# ---- 7: many fits -------------------------------------------------------------------------------------------------------------------
def test_rows_a_batch_of_131075_fits(R):
    """the 66 spectra of up to 33 points tiled to 2^17 + 3 fits (8193 workgroups, the last with three live rows) under (b): every copy
    returns the bits of its first occurrence -- in whichever row of whichever wave it lands, 66 being no multiple of 4 -- the first 66
    are held against the oracle and are the bits of the same spectra in the batch of 114"""
    short = [k for k in range(114) if R.n[k] <= RC.LARGE_MAX_N]
    assert len(short) == 66
    nf = RC.LARGE_FITS
    reps = -(-nf // 66)
    sub = RC.sub_batch(short)
    n_all = np.tile(sub.n, reps)[:nf]
    off_all = np.concatenate([[0], np.cumsum(n_all)]).astype(np.int64)
    cut = int(off_all[-1])
    off_b, kw = SCENARIOS['b']
    starts66 = RC.r1_starts(off_b)[short]
    starts = np.tile(starts66, (reps, 1))[:nf]
    c = _context(R.tape)
    try:
        c.set_batch_data(off_all, np.tile(sub.x, reps)[:cut], np.tile(sub.y, reps)[:cut], np.tile(sub.w, reps)[:cut])
        pars, res, _ = c.fit_batch(starts, RC.ACTIVE, lanes_per_fit=16, **kw)
        assert c.batch_lanes_used() == 16
    finally:
        c.close()
    first = np.arange(nf) % 66
    _same_bits(pars, res, pars[first], res[first])
    sel = [RC.r1_selection('b')[k] for k in short]
    _check_fit('large_batch', _fit_worst(sel, pars[:66], res[:66], R.n[short], 4))
    p114, r114 = R.fit('b')
    _same_bits(pars[:66], res[:66], p114[short], r114[short])


# ---- 8: both forms in one context ---------------------------------------------------------------------------------------------------
def test_both_forms_in_one_context(R):
    """64 -> 16 -> 64 -> batch_pass at 16 -> a plain set_data + fit -> 16 once more, on one context and the same data: both forms of the
    active set are resident side by side (the kernel cache's key carries the form), every result is the bits of the first call in
    that form and of a fresh context, and the plain fit returns what a fresh context returns"""
    off, kw = SCENARIOS['c']
    starts, p5 = RC.r1_starts(off), RC.r1_starts(0.05)
    k = next(i for i in range(114) if R.n[i] == 257)
    x, y, w = R.batch.items[k]
    sigma = 1.0 / w

    def plain(ctx):
        ctx.set_data(x, y, sigma, [0, x.size])
        ctx.init_weights(4)
        return ctx.fit([starts[k]], RC.ACTIVE, [0] * 4, **kw)
    c = _context(R.tape, R.batch)
    try:
        p64, r64, _ = c.fit_batch(starts, RC.ACTIVE, **kw)
        assert c.batch_lanes_used() == 64
        p16, r16, _ = c.fit_batch(starts, RC.ACTIVE, lanes_per_fit=16, **kw)
        assert c.batch_lanes_used() == 16
        _same_bits(p16, r16, *R.fit('c'))                        # (the module's context: another one)
        p, r, _ = c.fit_batch(starts, RC.ACTIVE, lanes_per_fit=64, **kw)
        assert c.batch_lanes_used() == 64
        _same_bits(p, r, p64, r64)
        _same_pass(c.batch_pass(p5, RC.ACTIVE, lanes_per_fit=16), R.one_pass())
        assert c.batch_lanes_used() == 16
        out, rp = plain(c)
        p, r, _ = c.fit_batch(starts, RC.ACTIVE, **kw)           # ... and the batch and the setting are still there after the plain fit
        assert c.batch_lanes_used() == 16
        _same_bits(p, r, p16, r16)
    finally:
        c.close()
    f = _context(R.tape, R.batch)
    try:
        p, r, _ = f.fit_batch(starts, RC.ACTIVE, **kw)
        assert f.batch_lanes_used() == 64
        _same_bits(p, r, p64, r64)
        out0, rf = plain(f)
    finally:
        f.close()
    assert np.array_equal(out, out0)
    assert tuple(int(getattr(rp, v)) for v in COUNTS) == tuple(int(getattr(rf, v)) for v in COUNTS)
    assert rp.chi2 == rf.chi2 and rp.lambda_ == rf.lambda_
