"""What tests/test_gpu_batch_wg.py rests on, shown without a GPU (the selection rule over its spectra is run
by tests/test_cpu_batch_cases.py): gfh_set_batch_lanes taking 256 and the refusals holding under it, the auto rule never returning
256, the 256-lane form of every batch translation unit the GPU tests ask for compiling for gfx950 on a compile-only context, and
profiles/batch_workgroup.json holding the cells it was asked for with the two must-win cells won."""
import json
import os

import numpy as np
import pytest

from gadfit_amd import _lib
from tests import batch_form_cases as FC
from tests import batch_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_batch_lanes_takes_256_and_the_refusals_hold_under_it():
    c = _lib.Context(-1)
    try:
        tape = FC.batch(FC.WORKGROUP)[0]
        c.set_model(tape)
        c.set_batch_lanes(256)
        assert c.batch_lanes_used() == 0          # a setting, not a launch
        src = c.batch_source(FC.ACTIVE)
        assert '#define GFH_BLANES 256\n' in src and '__syncthreads' in src
        with pytest.raises(_lib.GadfitHipError, match=r'gfh_set_batch_lanes: 8 lanes per fit are not built'):
            c.set_batch_lanes(8)
        assert '#define GFH_BLANES 256\n' in c.batch_source(FC.ACTIVE)          # a refused value leaves the setting
        with pytest.raises(_lib.GadfitHipError, match=r'256'):                 # ... and the refusal names the value that is built
            c.set_batch_lanes(32)
        # every refusal of a batch holds in the workgroup form as in the others
        with pytest.raises(_lib.GadfitHipError, match='more than 8 active'):
            c.batch_prepare(list(range(9)))
        x = np.linspace(0.5, 9.5, 20)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_data([0, 3, 20], x, x, x)
        with pytest.raises(_lib.GadfitHipError, match='More independent fitting parameters than data points'):
            c.fit_batch(np.ones((2, 4)), FC.ACTIVE, max_iter=1)
        with pytest.raises(_lib.GadfitHipError, match='max_iter is required'):
            c.fit_batch(np.ones((2, 4)), [0, 1], lanes_per_fit=256)
        with pytest.raises(_lib.GadfitHipError, match='8 lanes per fit are not built'):
            c.batch_pass(np.ones((2, 4)), [0, 1], lanes_per_fit=8)
        assert '#define GFH_BLANES 256\n' in c.batch_source([0, 1])
        for lanes in (64, 16, 0, 256):          # the other values are taken as before, and 256 after them
            c.set_batch_lanes(lanes)
    finally:
        c.close()


def test_auto_never_returns_256():
    lengths = sorted(set([8, 9, 10 ** 6] + [int(round(10 ** (k / 8.0))) for k in range(8, 49)] + [2 ** k + e for k in range(3, 20) for e in (-1, 0, 1)]))
    lengths = [n for n in lengths if 8 <= n <= 10 ** 6]
    assert lengths[0] == 8 and lengths[-1] == 10 ** 6
    for na in range(1, 9):
        for n in lengths:
            assert _lib.batch_auto_lanes(na, n) in (16, 64), (na, n)
    # ... and under auto a context that holds a long batch acts for 64
    c = _lib.Context(-1)
    try:
        c.set_model(FC.batch(FC.WORKGROUP)[0])
        c.set_batch_lanes(0)
        x = np.linspace(0.5, 9.5, 8 + 65536)
        with pytest.raises(_lib.GadfitHipError, match='no GPU'):
            c.set_batch_data([0, 8, 8 + 65536], x, x, x)
        assert '#define GFH_BLANES 64\n' in c.batch_source(FC.ACTIVE)
    finally:
        c.close()


def test_the_workgroup_form_of_every_unit_compiles_for_gfx950():
    units = FC.units(FC.WORKGROUP)
    assert len(units) == 2 + 10
    c = _lib.Context(-1)
    try:
        c.set_batch_lanes(256)
        for tape, active in units:
            c.set_model(tape)
            c.batch_prepare(active)
            assert '#define GFH_BLANES 256\n' in c.batch_source(active)
    finally:
        c.close()


def test_the_record_holds_the_cells_and_the_two_must_win_cells_are_won():
    """profiles/batch_workgroup.json (tools/bench_batch.py --workgroup): both forms of one run per (model, fits per launch, points per
    spectrum), every cell of the grid up to 2^30 points in total, and the 256-lane form faster than the 64-lane form of the same run
    by more than the two forms' min-max spread (batch_records.row_wins) at 256 fits of 16384 and of 65536 points, both models.
    The compiler's figures of the 256-lane kernels: no scratch."""
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'batch_workgroup.json')))
    for model, na in (('gauss4', 4), ('exp4', 8)):
        for fits in (64, 256, 1024, 16384):
            for points in (1000, 4096, 16384, 65536):
                m = batch_records.cell(rec, model, fits, points)
                if fits * points > 2 ** 30:
                    assert m is None, (model, fits, points)
                    continue
                assert m is not None, (model, fits, points)
                assert int(m['n_active']) == na
                for lanes in ('64', '256'):
                    e = m['lanes'][lanes]
                    assert 0.0 < e['device_ms_min'] <= e['device_ms'] <= e['device_ms_max'] and e['finite']
                assert m['workgroup_wins'] == bool(batch_records.row_wins(m['lanes']['256'], m['lanes']['64']))
    for model, fits, points in batch_records.MUST_WIN:
        m = batch_records.cell(rec, model, fits, points)
        assert batch_records.row_wins(m['lanes']['256'], m['lanes']['64']), (model, fits, points, m['lanes'])
    regs = rec['registers']
    for unit in ('gauss4', 'exp4', 'exp2'):
        for kernel in ('gfh_k_fit_batch', 'gfh_k_batch_pass'):
            r = regs['%s_lanes256' % unit][kernel]
            assert r['scratch_bytes_per_lane'] == 0 and 0 < r['lds_bytes_per_block'] <= 2 * 4 * 45 * 8, (unit, kernel, r)
