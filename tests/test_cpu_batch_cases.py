"""What the three forms' GPU modules (tests/batch_form_suite.py) rest on, shown without a GPU: the selection rule of
tests/batch_cases.py run by the oracle alone over every case list (Part 1 of every form of tests/batch_form_cases.py, Parts 2 and 3; each part's cap on dropped cases holds),
each part covering what it claims (the exits, rejections and STEP 3 it is there for), and every batch translation unit the GPU tests
ask for at 64 lanes compiling for gfx950 on a compile-only context (tests/test_cpu_batch_rows.py and tests/test_cpu_batch_wg.py
compile the other forms')."""
import numpy as np
import pytest

from gadfit_amd import _lib
from tests import batch_cases as BC
from tests import batch_form_cases as FC


def _counts(sel):
    return [s[1][0] for s in sel]          # (iterations, n_sweeps, n_chi2, n_omega, exit_reason) per fit


@pytest.mark.parametrize('form', FC.FORMS, ids=lambda f: str(f.lanes))
def test_part1_rule_counts(form):
    """6 spectra x the form's lengths.  With four active parameters under (a), (b), (c) the oracle agrees with itself on every fit
    (none dropped); exits 0, 2 and 7, rejections and STEP 3 occur; the lengths start at n = na and hold the form's edges, and the
    order puts short spectra beside long ones.
    With active = [1] a fit is at convergence within a step or two and some then make a chi2 comparison closer than MARGIN (the third
    condition of the rule drops them, and nothing else does): at 64 lanes every seventh under (b) (4e-16 ... 1e-13) -- no scenario
    loses more than a quarter of its 108; at 16 lanes 2 (a: both n = 4) and 6 (b: n = 17, 63, 80, 80, 257, 257), at most 5 % of the
    228; at 256 lanes 2 under (a) (n = 4, s = 1 and 4), at most 3 of the 138 ((b) fails the rule on 23 and is left out).  Every
    length keeps form.one_kept_per_length of its six fits in each scenario, and a dropped fit's first pass is still compared (the
    pass test of the GPU module takes every spectrum)."""
    order = FC.order(form)
    total = form.spectra          # (108, 114, 138)
    assert len(order) == total == FC.SAMPLES * len(form.lengths) == len(FC.batch(form)[3].items) and sorted(set(n for n, _ in order)) == sorted(form.lengths)
    assert min(form.lengths) == len(FC.ACTIVE) and form.edges <= set(form.lengths)
    assert form.short_beside_long([o[0] for o in order])
    exits, rejected, omega, worst = set(), 0, 0, 0.0
    for name in FC.FIT_SCENARIOS:
        sel = FC.selection(form, name)
        assert [b for b, s in enumerate(sel) if not s[0]] == [], name          # none dropped
        worst = max([worst] + [s[2] for s in sel])
        for it, _, n_chi2, n_omega, ex in _counts(sel):
            exits.add(ex); rejected += n_chi2 != it + 1; omega += n_omega > 0
    print('%d lanes: worst self-difference of the parameters %.2e, fits with a rejection %d, with STEP 3 %d' % (form.lanes, worst, rejected, omega))
    assert exits == {0, 2, 7} and rejected > 0 and omega > 0
    dropped, exits = [], set()
    for name in form.one_scenarios:
        sel = FC.selection(form, name, True)
        lost = [order[b] for b, s in enumerate(sel) if not s[0]]
        print('%d lanes, one active (%s): %d of %d dropped: (n, s) = %s' % (form.lanes, name, len(lost), total, lost))
        dropped.append(len(lost))
        for length in form.lengths:
            assert sum(s[0] for b, s in enumerate(sel) if order[b][0] == length) >= form.one_kept_per_length, (name, length)
        assert all(s[2] <= BC.SELF_TOL and s[3] <= BC.MARGIN for s in sel if not s[0]), name          # all of them by the margin alone
        exits |= set(s[1][0][4] for s in sel if s[0])
    assert form.one_cap_each is None or max(dropped) <= form.one_cap_each
    assert form.one_cap_total is None or sum(dropped) <= form.one_cap_total
    assert exits >= ({0, 2, 7} if 'b' in form.one_scenarios else {2})          # (a) converges; the other exits are (b)'s


def test_part2_every_active_count_none_dropped():
    """model_exp4 with 1 ... 8 active parameters, lists in the caller's order: none of the 2 x 8 x 48 fits fails the rule (the
    four-parameter set of 'short' is the one that passes it); 'short' meets exit 7 and STEP 3"""
    for name, (off, kw) in BC.EXP4_ARGS.items():
        sets = BC.exp4_sets(name)
        assert sorted(len(a) for a in sets) == list(range(1, 9))
        assert any(a != sorted(a) for a in sets)
        worst = 0.0
        for a in sets:
            sel = BC.part2_select(a, off, kw)
            assert [b for b, s in enumerate(sel) if not s[0]] == [], (name, a)
            worst = max([worst] + [s[2] for s in sel])
            if name == 'short':
                assert all(c[3] > 0 for c in _counts(sel)), a
        print('part 2 %s: worst self-difference of the parameters %.2e' % (name, worst))
    off, kw = BC.EXP4_ARGS['short']
    assert any(7 in set(c[4] for c in _counts(BC.part2_select(a, off, kw))) for a in BC.exp4_sets('short'))
    # the set that 'short' replaces does fail the rule: the replacement is not a matter of taste
    assert sum(not s[0] for s in BC.part2_select([0, 2, 4, 6], off, kw)) > 0


def test_part2_order_cases_none_dropped_and_dtd_min_binds():
    off, kw = BC.EXP4_ORDER_ARGS
    plain = BC.part2_select([6, 1, 4], off, kw)
    for name, pair in BC.EXP4_ORDER.items():
        (a0, d0), (a1, d1) = pair
        assert sorted(a0) == a1 and [d0[a0.index(k)] for k in a1] == d1          # the same values on the same parameters
        s0, s1 = BC.part2_select(a0, off, kw, d0), BC.part2_select(a1, off, kw, d1)
        assert all(s[0] for s in s0) and all(s[0] for s in s1), name
        # the oracle itself gives the two orders the same fit to reordering noise
        assert max(np.max(np.abs(p[1][1] - q[1][1]) / np.abs(p[1][1])) for p, q in zip(s0, s1)) < BC.SELF_TOL
        changed = sum(not np.array_equal(p[1][1], q[1][1]) for p, q in zip(s0, plain))
        assert changed == (48 if name == 'binding' else 0), (name, changed)


def test_part3_operator_set_cap_and_no_oracle_failure():
    """32 random models and the written erf / abs / unary-minus model x 8 spectra x 3 argument sets: no oracle call raises (a raise
    fails this test), at most 5 % of the 792 fits fail the rule, under (i) every fit runs STEP 3 exactly once, the active lists cover 1 ... 5 parameters
    and are not all ascending, spectra with n = na occur"""
    dropped, total, sizes, unsorted, dof0, worst = 0, 0, set(), 0, 0, 0.0
    for seed in BC.OPERATOR_SEEDS:
        tape, active, starts, batch = BC.part3(seed)
        assert np.all(np.isfinite(batch.y))
        sizes.add(len(active)); unsorted += active != sorted(active); dof0 += int(np.sum(batch.n == len(active)))
        for name in BC.RANDOM_ARGS:
            sel = BC.part3_selection(seed, name)
            dropped += sum(not s[0] for s in sel); total += len(sel)
            assert any(s[0] for s in sel), (seed, name)          # every batch keeps a fit to compare
            worst = max([worst] + [s[2] for s in sel])
            assert all(np.all(np.isfinite(s[1][1])) for s in sel)
            if name == 'i':
                assert all(c[3] == 1 and c[0] == 1 for c in _counts(sel)), seed
    print('part 3: %d of %d fits dropped by the rule (%.1f %%), worst self-difference of the parameters %.2e' % (dropped, total, 100.0 * dropped / total, worst))
    assert total == 792 and dropped <= BC.RANDOM_CAP * total
    assert sizes == {1, 2, 3, 4, 5} and unsorted > 0 and dof0 > 0


def test_part3_tapes_hold_every_elemental():
    """the operator codes of the 33 tapes together: the four arithmetic operations, pow in its forms (POW with an AD or a real
    exponent or base, POWI), every unary function of the tape format -- erf and abs among them -- and NEG; unary minus of an AD
    variable is the reference's 0.0 - a, a SUB whose left operand is a constant"""
    from gadfit_amd import tape as T
    ops, neg_advar, pow_forms = set(), False, set()
    for seed in BC.OPERATOR_SEEDS:
        nodes = BC.part3(seed)[0].subtapes[0][0]
        for op, a, b, flags, c in nodes:
            ops.add(op)
            if op == T.SUB and not (flags & T.F_REAL) and a >= 0 and nodes[a][0] == T.CONST and nodes[a][4] == 0.0:
                neg_advar = True
            if op == T.POW and not (flags & T.F_REAL):
                pow_forms.add((nodes[a][0] == T.CONST, nodes[b][0] == T.CONST))
    assert {T.ADD, T.SUB, T.MUL, T.DIV, T.POW, T.POWI, T.NEG} | set(T.UNARY_NAMES) <= ops
    assert neg_advar
    assert pow_forms >= {(False, False), (False, True), (True, False)}          # a ** a, a ** r, r ** a (a ** n is POWI)
    erf = BC.part3(BC.ERF_NEG_SEED)[0].subtapes[0][0]
    assert {T.ERF, T.ABS, T.NEG} <= set(n[0] for n in erf)


def test_part3_fits_that_accept_a_step_inside_rounding_are_dropped():
    """The two fits on which the device and the oracle first disagreed ((iii), one active parameter: the device rejected the third
    step twice resp. once, the oracle accepted it at once).  The oracle agrees with itself on them over every cut into images (the
    first has 6 points, where a cut reorders next to nothing), but its accepted third step lowers chi2 by 4.0e-16 resp. 1.1e-15
    relative, two ulps: which way 'new_chi2 < old_chi2' falls there is rounding's choice, and the third condition of the rule says so."""
    for seed, b in ((0, 6), (7, 6)):
        kept, one, diff, margin = BC.part3_selection(seed, 'iii')[b]
        assert len(BC.part3(seed)[1]) == 1 and one[0] == (3, 3, 4, 0, 0) and diff <= BC.SELF_TOL
        assert 0.0 < margin < 2e-15 and not kept


def test_every_batch_unit_compiles_for_gfx950(monkeypatch):
    units = FC.units(FC.WAVE) + BC.operator_units()
    assert len(units) + 1 < 60
    c = _lib.Context(-1)
    try:
        for tape, active in units:
            c.set_model(tape)
            c.batch_prepare(active)
        tape, active = BC.part3(BC.RANDOM_POW_SEED)[:2]
        c.set_model(tape)
        src = c.batch_source(active)
        assert src.count('gfh_pow_ln(') >= 2 and '#define GFH_FAST_DIV 1' in src          # defined and called
    finally:
        c.close()
    monkeypatch.setenv('GADFIT_HIP_FAST_DIV', '0')
    c = _lib.Context(-1)
    try:
        c.set_model(tape)
        src = c.batch_source(active)
        assert 'gfh_pow_ln(' not in src and '#define GFH_FAST_DIV 0' in src
        c.batch_prepare(active)
    finally:
        c.close()
