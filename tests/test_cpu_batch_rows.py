"""What tests/test_gpu_batch_rows.py rests on, shown without a GPU (the selection rule over its spectra is run by
tests/test_cpu_batch_cases.py): the refusals of gfh_set_batch_lanes, both forms of every batch translation unit the GPU tests ask for
compiling for gfx950 on a compile-only context, and the auto rule returning what profiles/batch_rows.json implies."""
import json
import os

import numpy as np
import pytest

from gadfit_amd import _lib
from tests import batch_form_cases as FC
from tests import batch_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_batch_lanes_takes_64_16_and_auto_and_refuses_the_rest():
    c = _lib.Context(-1)
    try:
        assert c.batch_lanes_used() == 0          # no launch yet
        for lanes in (16, 0, 64):
            c.set_batch_lanes(lanes)
        for lanes in (8, 32, -1, 17):
            with pytest.raises(_lib.GadfitHipError, match=r'gfh_set_batch_lanes: %d lanes per fit are not built' % lanes):
                c.set_batch_lanes(lanes)
        tape = FC.batch(FC.ROWS)[0]
        c.set_model(tape)
        assert '#define GFH_BLANES 64\n' in c.batch_source(FC.ACTIVE)          # a refused value leaves the setting
        c.set_batch_lanes(16)
        src = c.batch_source(FC.ACTIVE)
        assert '#define GFH_BLANES 16\n' in src and 'row_ror' in src
        # every refusal of a batch holds in the row form as in the wave form
        with pytest.raises(_lib.GadfitHipError, match='more than 8 active'):
            c.batch_prepare(list(range(9)))
        x = np.linspace(0.5, 9.5, 20)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_data([0, 3, 20], x, x, x)
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.fit_batch(np.ones((2, 4)), FC.ACTIVE, max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='max_iter is required'):
            c.fit_batch(np.ones((2, 4)), [0, 1], lanes_per_fit=16)
        with pytest.raises(_lib.GadfitHipError, match='8 lanes per fit are not built'):
            c.batch_pass(np.ones((2, 4)), [0, 1], lanes_per_fit=8)
    finally:
        c.close()


def test_auto_is_a_function_of_the_geometry_held():
    """under auto gfh_batch_source acts for the form the rule gives for (active count, longest spectrum of the batch held), and for
    64 where the context holds no batch"""
    tape = FC.batch(FC.ROWS)[0]
    c = _lib.Context(-1)
    try:
        c.set_model(tape)
        c.set_batch_lanes(0)
        assert '#define GFH_BLANES 64\n' in c.batch_source(FC.ACTIVE)
        for longest in (8, 16, 64, 1000):
            x = np.linspace(0.5, 9.5, 8 + longest)
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                c.set_batch_data([0, 8, 8 + longest], x, x, x)
            for active in (FC.ACTIVE, FC.ONE_ACTIVE):
                assert '#define GFH_BLANES %d\n' % _lib.batch_auto_lanes(len(active), longest) in c.batch_source(active)
    finally:
        c.close()


def test_both_forms_of_every_row_unit_compile_for_gfx950():
    units = FC.units(FC.ROWS)
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
    implied = batch_records.implied_rule(rec)
    assert sorted(implied) == [4, 8]
    assert {str(k): v for k, v in implied.items()} == rec['auto_rule']['sixteen_lanes_up_to']
    lengths = sorted(set(int(m['points']) for m in rec['measurements']))
    assert lengths == [8, 16, 32, 64, 128, 256, 1000]
    for na in range(1, 9):
        up_to = implied[4 if na <= 4 else 8]
        for n in lengths:
            assert _lib.batch_auto_lanes(na, n) == (16 if n <= up_to else 64), (na, n)
    assert _lib.batch_auto_lanes(0, 8) == 64 and _lib.batch_auto_lanes(9, 8) == 64
