"""The suite that holds the batch kernels (gfh_k_fit_batch, gfh_k_batch_pass) in each of their forms -- 64, 16 and 256 lanes per fit
(lanes_per_fit / gfh_set_batch_lanes: a wave, a DPP row, a workgroup of four waves per fit) -- written once over the table of forms in
tests/batch_form_cases.py: spectrum lengths at the edges of the form's row of lanes, batch sizes that leave rows, waves and workgroups
without a fit, single fits and the batch reversed, neighbours filled with NaN, every active count 1 ... 8 in the caller's order, a
batch of 2^17 + 3 fits (more than 65535 workgroups at 256 lanes), and the same bits as the wave form where the sums are the same.

The functions here are the tests' bodies, each put on one list (suite_test) with the name it has per form.  tests/test_gpu_batch_shapes.py
(64 lanes), tests/test_gpu_batch_rows.py (16) and tests/test_gpu_batch_wg.py (256) take tests_of(form) -- the fixtures F and E and the
whole list -- into their namespace, so every case keeps the id it has had and no form can miss a test, and hold the tests that only
their form has.  What differs between the forms is data in the table.  Every call names its
form and batch_lanes_used() is asserted after it.  The rule that selects which fits may be held against the oracle is
batch_cases.select (the oracle's alone: nothing the device returns enters it); tests/test_cpu_batch_cases.py shows without a GPU
what it drops.
Bounds (tests/batch_common.py): one pass TOL_PASS = 2e-13 scaled as in test_gpu_batch.test_one_pass_against_the_oracle, the counts
and the exit reason equal, lambda TOL_LAMBDA = 1e-14, fitted parameters and chi2 north_star's 1e-10 (TOL_FIT), at 256 lanes on
Part 1 TOL_PARS = TOL_CHI2 = 3e-12.  The observed maxima go where test_gpu_batch.py's go (GADFIT_BATCH_OBSERVE) under the keys
shapes_* (64 lanes), rows_* (16) and wg_* (256); tools/bench_batch.py copies them into the profiles."""
import functools

import numpy as np
import pytest

from tests import batch_cases as BC
from tests import batch_form_cases as FC
from tests.batch_common import (COUNTS, SCENARIOS, TOL_FIT, TOL_PASS, check_fit, context, fit_worst, observe, pass_worst, same_bits,
                                same_pass)


class FormBatch:
    """a form's batch on one context with its fits and its pass cached: later tests compare other batches with them bit for bit"""

    def __init__(self, form):
        self.form, self.lanes = form, form.lanes
        self.tape, self.order, self.truths, self.batch = FC.batch(form)
        self.n = self.batch.n
        self.ctx = context(self.tape, self.batch)
        self._fits, self._pass = {}, None

    def starts(self, off, active=FC.ACTIVE):
        return FC.starts(self.form, off, active)

    def fit(self, name):
        if name not in self._fits:
            off, kw = SCENARIOS[name]
            self._fits[name] = self.ctx.fit_batch(self.starts(off), FC.ACTIVE, lanes_per_fit=self.lanes, **kw)[:2]
            assert self.ctx.batch_lanes_used() == self.lanes
        return self._fits[name]

    def one_pass(self):
        if self._pass is None:
            self._pass = self.ctx.batch_pass(self.starts(0.05), FC.ACTIVE, lanes_per_fit=self.lanes)
            assert self.ctx.batch_lanes_used() == self.lanes
        return self._pass


SUITE = []          # (test, what makes its parameters of a form or None, which forms it is of or None, its name per form's prefix)


def suite_test(params=None, applies=None, **names):
    """puts a test of the suite on the list, under the name it has in each form's module (shapes=, rows=, wg=); `params(form)` are
    the arguments of a pytest.mark.parametrize of its own per form, `applies(form)` says of which forms it is a test (None: all)"""
    def register(test):
        SUITE.append((test, params, applies, names))
        return test
    return register


def _own(test):
    """`test` as a function of a form's own, to carry that form's mark: the forms share the functions here"""
    @functools.wraps(test)
    def run(*args, **kw):
        return test(*args, **kw)
    return run


def tests_of(form):
    """what a form's test module holds of the suite, by name: the two module-scoped fixtures -- F, the form's batch on one context,
    and E, Part 2 on one context with the form's lanes set -- and every test on the list that is a test of this form, so a form
    cannot miss one: a test without a name for a form it applies to is a KeyError when the module is collected"""
    @pytest.fixture(scope='module')
    def F():
        s = FormBatch(form)
        yield s
        s.ctx.close()

    @pytest.fixture(scope='module')
    def E():
        tape, truths, batch = BC.part2()
        c = context(tape, batch)
        c.set_batch_lanes(form.lanes)
        yield form, tape, batch, c
        c.close()
    out = {'F': F, 'E': E}
    for test, params, applies, names in SUITE:
        if applies is not None and not applies(form):
            assert form.prefix not in names, test
            continue
        if params is not None:
            test = pytest.mark.parametrize(*params(form))(_own(test))
        out[names[form.prefix]] = test
    assert len(out) == 2 + sum(a is None or a(form) for _, _, a, _ in SUITE)          # (no name given twice)
    return out


# ---- Part 1: lengths at the edges of the form's row of lanes ------------------------------------------------------------------
@suite_test(shapes='test_lengths_one_pass_against_the_oracle', rows='test_rows_one_pass_against_the_oracle',
            wg='test_wg_one_pass_against_the_oracle')
def one_pass_against_the_oracle(F):
    """every spectrum of the form, those the rule drops from the fit comparisons included: the first row is also the last, the
    last row is full, has one live lane or one masked lane, and the row loop runs long (tests/batch_form_cases.py lists the
    lengths per form).  J^T J symmetric bit for bit (pass_worst)."""
    JTJ, JTr, chi2 = F.one_pass()
    worst = pass_worst(F.tape, F.batch.items, F.starts(0.05), FC.ACTIVE, JTJ, JTr, chi2)
    observe(**{'%s_lengths_pass' % F.form.prefix: worst})
    assert worst < TOL_PASS


@suite_test(shapes='test_lengths_fits_against_the_oracle', rows='test_rows_fits_against_the_oracle', wg='test_wg_fits_against_the_oracle')
@pytest.mark.parametrize('name', FC.FIT_SCENARIOS)
def fits_against_the_oracle(F, name):
    """all fits are kept by the rule; dof = max(n - 4, 1), the n = 4 fits being the dof = 0 case; neighbouring fits have
    different lengths and leave their loops at different iterations; (a) runs to convergence with rejections, (c) through STEP 3"""
    sel = FC.selection(F.form, name)
    assert all(s[0] for s in sel)
    pars, res = F.fit(name)
    print('%s (%s): iterations %s, exits %s' % (F.form.prefix, name, sorted(set(res['iterations'].tolist())), sorted(set(res['exit_reason'].tolist()))))
    check_fit(F.form.prefix, 'lengths_%s' % name, fit_worst(sel, pars, res, F.n, 4), *F.form.part1_tol)


@suite_test(params=lambda form: ('name', form.one_scenarios), shapes='test_lengths_with_one_active_parameter',
            rows='test_rows_with_one_active_parameter', wg='test_wg_with_one_active_parameter')
def with_one_active_parameter(F, name):
    """the same spectra with active = [1]: the 1 x 1 instance of the solve, the packed triangle and the accumulators (the fits
    the rule keeps: every length stays covered, tests/test_cpu_batch_cases.py; the pass takes every fit)"""
    form = F.form
    sel = FC.selection(form, name, True)
    off, kw = SCENARIOS[name]
    starts = F.starts(off, FC.ONE_ACTIVE)
    pars, res, _ = F.ctx.fit_batch(starts, FC.ONE_ACTIVE, lanes_per_fit=form.lanes, **kw)
    assert F.ctx.batch_lanes_used() == form.lanes
    assert np.array_equal(pars[:, [0, 2, 3]], starts[:, [0, 2, 3]])          # the passive parameters come back bit for bit
    check_fit(form.prefix, 'one_active_%s' % name, fit_worst(sel, pars, res, F.n, 1), *form.part1_tol)
    if name in form.one_pass_scenarios:
        JTJ, JTr, chi2 = F.ctx.batch_pass(starts, FC.ONE_ACTIVE, lanes_per_fit=form.lanes)
        assert F.ctx.batch_lanes_used() == form.lanes
        worst = pass_worst(F.tape, F.batch.items, starts, FC.ONE_ACTIVE, JTJ, JTr, chi2)
        observe(**{'%s_one_active_pass' % form.prefix: worst})
        assert worst < TOL_PASS


# ---- a fit does not depend on its batch ----------------------------------------------------------------------------------------
@suite_test(shapes='test_batch_sizes_that_leave_waves_without_a_fit', rows='test_a_fit_does_not_depend_on_its_row_or_its_neighbours',
            wg='test_a_fit_does_not_depend_on_the_grid_or_its_neighbours')
def a_fit_does_not_depend_on_the_grid_or_its_neighbours(F):
    """the batch cut to its first k fits (form.cuts: rows, waves and workgroups left without a fit) and, where the form's row of
    the table says so, each fit alone and the batch reversed (another row, wave or workgroup, other neighbours): every fit returns
    the bits it returned in the whole batch, from batch_pass and from fit_batch under (a) and (c)"""
    form, total = F.form, len(F.n)
    p5 = F.starts(0.05)
    full = {name: F.fit(name) for name in ('a', 'c')}
    c = context(F.tape)
    try:
        def same(idx):
            sub = FC.sub_batch(form, idx)
            c.set_batch_data(sub.off, sub.x, sub.y, sub.w)
            same_pass(c.batch_pass(p5[idx], FC.ACTIVE, lanes_per_fit=form.lanes), [v[idx] for v in F.one_pass()])
            assert c.batch_lanes_used() == form.lanes
            for name, (pars, res) in full.items():
                off, kw = SCENARIOS[name]
                p1, r1, _ = c.fit_batch(F.starts(off)[idx], FC.ACTIVE, lanes_per_fit=form.lanes, **kw)
                assert c.batch_lanes_used() == form.lanes
                same_bits(p1, r1, pars[idx], res[idx])
        if form.every_single_fit_and_reversed:
            for k in range(total):
                same([k])
            same(list(range(total - 1, -1, -1)))
        for k in form.cuts:
            same(list(range(k)))
    finally:
        c.close()


@suite_test(shapes='test_a_fit_reads_no_point_of_its_neighbours', rows='test_a_fit_reads_no_point_of_the_other_rows_of_its_wave',
            wg='test_a_fit_reads_no_point_of_its_neighbours')
def a_fit_reads_no_point_of_its_neighbours(F):
    """Every spectrum's x, y and w outside a mask of clean fits are NaN (form.nan_clean: one fit, every other fit, every fourth):
    the clean fits return the bits of the undisturbed batch from batch_pass and from fit_batch (STEP 1 + 2, chi2 and, under (c),
    STEP 3 all read the points).  A NaN that came through a w = 0 mask, a DPP move from another row or a read past a spectrum's
    end would show (NaN * 0 = NaN); a finite stray value does not.  The poisoned fits end at their first solve (exit 8: 'ajj > 0'
    is false for a NaN; at 256 lanes in all four waves alike) with their start parameters."""
    form = F.form
    p5 = F.starts(0.05)
    c = context(F.tape)
    try:
        for clean in form.nan_clean(F.n):
            pt = np.repeat(clean, F.n)
            x, y, w = (np.where(pt, v, np.nan) for v in (F.batch.x, F.batch.y, F.batch.w))
            c.set_batch_data(F.batch.off, x, y, w)
            same_pass([v[clean] for v in c.batch_pass(p5, FC.ACTIVE, lanes_per_fit=form.lanes)], [v[clean] for v in F.one_pass()])
            assert c.batch_lanes_used() == form.lanes
            for name in form.nan_scenarios:
                off, kw = SCENARIOS[name]
                starts = F.starts(off)
                pars, res = F.fit(name)
                p1, r1, _ = c.fit_batch(starts, FC.ACTIVE, lanes_per_fit=form.lanes, **kw)
                assert c.batch_lanes_used() == form.lanes
                same_bits(p1[clean], r1[clean], pars[clean], res[clean])
                bad = ~clean
                assert np.all(r1['exit_reason'][bad] == 8) and np.all(r1['iterations'][bad] == 0)
                assert np.all(r1['n_sweeps'][bad] == 1) and np.all(r1['n_chi2'][bad] == 1)
                assert np.array_equal(p1[bad], starts[bad])
    finally:
        c.close()


# ---- many fits -----------------------------------------------------------------------------------------------------------------
@suite_test(shapes='test_a_batch_of_131075_fits', rows='test_rows_a_batch_of_131075_fits', wg='test_wg_a_batch_of_70003_fits')
def a_large_batch(F):
    """the spectra of up to form.large_max_n points tiled to form.large_fits fits under (b) -- 2^17 + 3 (at 16 lanes 8193
    workgroups, the last with three live rows), at 256 lanes 70003, one workgroup each: every copy returns the bits of its first
    occurrence, in whichever row of whichever wave it lands; the first copies are held against the oracle and are the bits of the
    same spectra in the whole batch, where they lie at other offsets beside other neighbours"""
    form = F.form
    short = [k for k in range(len(F.n)) if F.n[k] <= form.large_max_n]
    m, nf = len(short), form.large_fits
    assert m == form.large_spectra and nf > 65535          # (90, 66, 84 spectra)
    reps = -(-nf // m)
    sub = FC.sub_batch(form, short)
    off_all = np.concatenate([[0], np.cumsum(np.tile(sub.n, reps)[:nf])]).astype(np.int64)
    cut = int(off_all[-1])
    off_b, kw = SCENARIOS['b']
    starts = np.tile(F.starts(off_b)[short], (reps, 1))[:nf]
    c = context(F.tape)
    try:
        c.set_batch_data(off_all, np.tile(sub.x, reps)[:cut], np.tile(sub.y, reps)[:cut], np.tile(sub.w, reps)[:cut])
        pars, res, _ = c.fit_batch(starts, FC.ACTIVE, lanes_per_fit=form.lanes, **kw)
        assert c.batch_lanes_used() == form.lanes
    finally:
        c.close()
    first = np.arange(nf) % m
    same_bits(pars, res, pars[first], res[first])
    sel = [FC.selection(form, 'b')[k] for k in short]
    check_fit(form.prefix, 'large_batch', fit_worst(sel, pars[:m], res[:m], F.n[short], 4), *form.part1_tol)
    p_all, r_all = F.fit('b')
    same_bits(pars[:m], res[:m], p_all[short], r_all[short])


# ---- Part 2: every active count, in the caller's order -------------------------------------------------------------------------
@suite_test(shapes='test_every_active_count_against_the_oracle', rows='test_rows_every_active_count_against_the_oracle',
            wg='test_wg_every_active_count_against_the_oracle')
@pytest.mark.parametrize('idx', range(8))
@pytest.mark.parametrize('name', sorted(BC.EXP4_ARGS))
def every_active_count_against_the_oracle(E, name, idx):
    """1 ... 8 active parameters of model_exp4 (128 ... 512 points), the lists as the caller orders them: the oracle is given the
    same list in the same order; 'short' runs STEP 3.  Part 2's selection drops none of these fits."""
    form, tape, batch, c = E
    off, kw = BC.EXP4_ARGS[name]
    active = BC.exp4_sets(name)[idx]
    sel = BC.part2_select(active, off, kw)
    assert all(s[0] for s in sel)
    starts = BC.part2_starts(active, off)
    pars, res, _ = c.fit_batch(starts, active, lanes_per_fit=form.lanes, **kw)
    assert c.batch_lanes_used() == form.lanes
    passive = [k for k in range(8) if k not in active]
    assert np.array_equal(pars[:, passive], starts[:, passive])
    print('exp4 %s %s: iterations %s, exits %s' % (name, active, sorted(set(res['iterations'].tolist())), sorted(set(res['exit_reason'].tolist()))))
    check_fit(form.prefix, 'exp4_%s_na%d' % (name, len(active)), fit_worst(sel, pars, res, batch.n, len(active)), TOL_FIT, TOL_FIT)
    if name == 'conv':
        JTJ, JTr, chi2 = c.batch_pass(starts, active, lanes_per_fit=form.lanes)
        assert c.batch_lanes_used() == form.lanes
        worst = pass_worst(tape, batch.items, starts, active, JTJ, JTr, chi2)
        observe(**{'%s_exp4_pass_na%d' % (form.prefix, len(active)): worst})
        assert worst < TOL_PASS


@suite_test(shapes='test_the_callers_order_reaches_every_column', rows='test_rows_the_callers_order_reaches_every_column',
            wg='test_wg_the_callers_order_reaches_every_column')
@pytest.mark.parametrize('which', sorted(BC.EXP4_ORDER))
def the_callers_order_reaches_every_column(E, which):
    """[6, 1, 4] and [1, 4, 6] with DTD_min permuted alike: each against the oracle given the same list and values, and the two
    device results against each other.  'binding': values that exceed J^T J's diagonal for parameters 6 and 4, so a value on the
    wrong column is another fit."""
    form, tape, batch, c = E
    off, kw = BC.EXP4_ORDER_ARGS
    got = []
    for active, dtd in BC.EXP4_ORDER[which]:
        sel = BC.part2_select(active, off, kw, dtd)
        assert all(s[0] for s in sel)
        starts = BC.part2_starts(active, off)
        pars, res, _ = c.fit_batch(starts, active, DTD_min=dtd, lanes_per_fit=form.lanes, **kw)
        assert c.batch_lanes_used() == form.lanes
        check_fit(form.prefix, 'order_%s_%s' % (which, ''.join(str(a) for a in active)), fit_worst(sel, pars, res, batch.n, 3), TOL_FIT, TOL_FIT)
        got.append((pars, res))
        JTJ, JTr, chi2 = c.batch_pass(starts, active, lanes_per_fit=form.lanes)
        assert c.batch_lanes_used() == form.lanes
        assert pass_worst(tape, batch.items, starts, active, JTJ, JTr, chi2) < TOL_PASS
    (pa, ra), (pb, rb) = got
    for f in COUNTS:
        assert np.array_equal(ra[f], rb[f]), f
    between = float(np.max(np.abs(pa - pb) / np.abs(pa)))
    if form.observes_order_between:
        observe(**{'%s_order_%s_between' % (form.prefix, which): between})
    assert between < TOL_FIT


# ---- the forms that have such a bound (form.same_bits_max_n) ------------------------------------------------------------------------
@suite_test(applies=lambda form: form.same_bits_max_n is not None, rows='test_same_bits_in_both_forms_up_to_16_points',
            wg='test_same_bits_as_the_wave_form_up_to_64_points')
def same_bits_as_the_wave_form(F):
    """The spectra of up to form.same_bits_max_n points as a batch of their own return the wave form's bits.
    16 lanes, n <= 16: with at most one point per lane both forms add the same values through the same row tree -- the wave form
    adds the exact zeros of its 48 lanes with w = 0 first, and lane 0 of the row form's rotation butterfly is the row levels of
    gfh_wave_sum with operands commuted.
    256 lanes, n <= 64: wave 0's lanes hold the same per-lane values in both forms (one row, lane l takes point l); waves 1 ... 3
    have w = 0 in every lane, their accumulators start at +0.0 and only +-0 is added to them, so their partial sums are exact +0.0
    and ((p0 + 0.0) + 0.0) + 0.0 is p0.
    In both, contraction is decided per source expression (-ffp-contract=on) in the one text the forms are compiled from, and the
    solve is contract(off)."""
    form = F.form
    idx = [k for k in range(len(F.n)) if F.n[k] <= form.same_bits_max_n]
    assert len(idx) == FC.SAMPLES * len(form.same_bits_lengths) > 0 and set(F.n[idx]) == set(form.same_bits_lengths)          # (42, 24 fits)
    c = context(F.tape, FC.sub_batch(form, idx))
    try:
        for active, names in ((FC.ACTIVE, FC.FIT_SCENARIOS), (FC.ONE_ACTIVE, form.one_scenarios)):
            p5 = F.starts(0.05, active)[idx]
            mine = c.batch_pass(p5, active, lanes_per_fit=form.lanes)
            assert c.batch_lanes_used() == form.lanes
            wave = c.batch_pass(p5, active, lanes_per_fit=64)
            assert c.batch_lanes_used() == 64
            same_pass(mine, wave)
            for name in names:
                off, kw = SCENARIOS[name]
                starts = F.starts(off, active)[idx]
                p, r, _ = c.fit_batch(starts, active, lanes_per_fit=form.lanes, **kw)
                assert c.batch_lanes_used() == form.lanes
                p64, r64, _ = c.fit_batch(starts, active, lanes_per_fit=64, **kw)
                assert c.batch_lanes_used() == 64
                same_bits(p, r, p64, r64)
    finally:
        c.close()


# ---- a plain fit beside the batch: what the forms' own 'state on one context' tests share --------------------------------------------
def plain_fit(ctx, item, start, kw):
    """a plain set_data + fit of one spectrum (x, y, w) of Part 1 on a context that may hold a batch"""
    x, y, w = item
    ctx.set_data(x, y, 1.0 / w, [0, x.size])
    ctx.init_weights(4)
    return ctx.fit([start], FC.ACTIVE, [0] * 4, **kw)


def same_plain_fit(a, b):
    (out, r), (out0, r0) = a, b
    assert np.array_equal(out, out0)
    assert tuple(int(getattr(r, v)) for v in COUNTS) == tuple(int(getattr(r0, v)) for v in COUNTS)
    assert r.chi2 == r0.chi2 and r.lambda_ == r0.lambda_
