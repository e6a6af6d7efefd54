"""What tests/test_gpu_batch_rows.py rests on, shown without a GPU: the selection rule of tests/batch_cases.py run by the oracle alone
over Part R1 of tests/batch_row_cases.py, the refusals of gfh_set_batch_lanes, both forms of every batch translation unit the GPU tests
ask for compiling for gfx950 on a compile-only context, and the auto rule returning what profiles/batch_rows.json implies."""
import json
import os

import numpy as np
import pytest

from gadfit_amd import _lib
from tests import batch_cases as BC
from tests import batch_row_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_r1_rule_counts():
    """6 spectra x 19 lengths: with four active parameters the oracle agrees with itself on all 3 x 114 fits; with one active
    parameter 2 (a: both n = 4) and 6 (b: n = 17, 63, 80, 80, 257, 257) fail the rule by its margin -- at most 5 % of the 228, every
    length keeps a fit in each scenario (at least four of its six), and a dropped fit's first pass is still compared (the pass test
    of the GPU module takes all 114).  Exits 0, 2 and 7, rejections and STEP 3 occur."""
    order = RC.r1_order()
    assert len(order) == 114 and sorted(set(n for n, _ in order)) == sorted(RC.LENGTHS)
    assert min(RC.LENGTHS) == len(RC.ACTIVE) and {7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65} <= set(RC.LENGTHS)
    n = [o[0] for o in order]          # four neighbours (the rows of a wave) with trip counts that differ: one row of points beside five and more
    assert any(min(n[k:k + 4]) <= 16 and max(n[k:k + 4]) > 64 for k in range(0, 112, 4))
    exits, rejected, omega = set(), 0, 0
    for name in RC.FIT_SCENARIOS:
        sel = RC.r1_selection(name)
        assert [b for b, s in enumerate(sel) if not s[0]] == [], name          # none dropped
        for it, _, n_chi2, n_omega, ex in [s[1][0] for s in sel]:
            exits.add(ex); rejected += n_chi2 != it + 1; omega += n_omega > 0
    assert exits == {0, 2, 7} and rejected > 0 and omega > 0
    dropped = 0
    for name in RC.ONE_SCENARIOS:
        sel = RC.r1_selection(name, True)
        lost = [order[b][0] for b, s in enumerate(sel) if not s[0]]
        print('R1, one active (%s): %d of 114 dropped: n = %s' % (name, len(lost), lost))
        dropped += len(lost)
        for length in RC.LENGTHS:
            assert sum(s[0] for b, s in enumerate(sel) if order[b][0] == length) >= 4, (name, length)
        assert all(s[2] <= BC.SELF_TOL and s[3] <= BC.MARGIN for s in sel if not s[0]), name          # all of them by the margin alone
    assert dropped <= RC.ONE_ACTIVE_CAP * 2 * 114


def test_set_batch_lanes_takes_64_16_and_auto_and_refuses_the_rest():
    c = _lib.Context(-1)
    try:
        assert c.batch_lanes_used() == 0          # no launch yet
        for lanes in (16, 0, 64):
            c.set_batch_lanes(lanes)
        for lanes in (8, 32, -1, 17):
            with pytest.raises(_lib.GadfitHipError, match=r'gfh_set_batch_lanes: %d lanes per fit are not built' % lanes):
                c.set_batch_lanes(lanes)
        tape = RC.r1()[0]
        c.set_model(tape)
        assert '#define GFH_BLANES 64\n' in c.batch_source(RC.ACTIVE)          # a refused value leaves the setting
        c.set_batch_lanes(16)
        src = c.batch_source(RC.ACTIVE)
        assert '#define GFH_BLANES 16\n' in src and 'row_ror' in src
        # every refusal of a batch holds in the row form as in the wave form
        with pytest.raises(_lib.GadfitHipError, match='more than 8 active'):
            c.batch_prepare(list(range(9)))
        x = np.linspace(0.5, 9.5, 20)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_data([0, 3, 20], x, x, x)
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.fit_batch(np.ones((2, 4)), RC.ACTIVE, max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='max_iter is required'):
            c.fit_batch(np.ones((2, 4)), [0, 1], lanes_per_fit=16)
        with pytest.raises(_lib.GadfitHipError, match='8 lanes per fit are not built'):
            c.batch_pass(np.ones((2, 4)), [0, 1], lanes_per_fit=8)
    finally:
        c.close()


def test_auto_is_a_function_of_the_geometry_held():
    """under auto gfh_batch_source acts for the form the rule gives for (active count, longest spectrum of the batch held), and for
    64 where the context holds no batch"""
    tape = RC.r1()[0]
    c = _lib.Context(-1)
    try:
        c.set_model(tape)
        c.set_batch_lanes(0)
        assert '#define GFH_BLANES 64\n' in c.batch_source(RC.ACTIVE)
        for longest in (8, 16, 64, 1000):
            x = np.linspace(0.5, 9.5, 8 + longest)
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                c.set_batch_data([0, 8, 8 + longest], x, x, x)
            for active in (RC.ACTIVE, RC.ONE_ACTIVE):
                assert '#define GFH_BLANES %d\n' % _lib.batch_auto_lanes(len(active), longest) in c.batch_source(active)
    finally:
        c.close()


def test_both_forms_of_every_row_unit_compile_for_gfx950():
    units = RC.row_units()
    assert len(units) == 2 + 10
    c = _lib.Context(-1)
    try:
        for lanes in (16, 64):
            c.set_batch_lanes(lanes)
            for tape, active in units:
                c.set_model(tape)
                c.batch_prepare(active)
                assert '#define GFH_BLANES %d\n' % lanes in c.batch_source(active)
    finally:
        c.close()


def test_the_auto_rule_is_what_the_measurement_implies():
    """profiles/batch_rows.json (tools/bench_batch.py --rows): per active-count class, 16 lanes up to the largest measured length at
    which the row form beat the wave form of the same run by more than the two forms' min-max spread, 64 beyond it and wherever the
    row form won nowhere.  Measured at 4 and at 8 active parameters: 1 ... 4 take the first class, 5 ... 8 the second."""
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'batch_rows.json')))
    implied = RC.implied_rule(rec)
    assert sorted(implied) == [4, 8]
    assert {str(k): v for k, v in implied.items()} == rec['auto_rule']['sixteen_lanes_up_to']
    lengths = sorted(set(int(m['points']) for m in rec['measurements']))
    assert lengths == [8, 16, 32, 64, 128, 256, 1000]
    for na in range(1, 9):
        up_to = implied[4 if na <= 4 else 8]
        for n in lengths:
            assert _lib.batch_auto_lanes(na, n) == (16 if n <= up_to else 64), (na, n)
    assert _lib.batch_auto_lanes(0, 8) == 64 and _lib.batch_auto_lanes(9, 8) == 64
