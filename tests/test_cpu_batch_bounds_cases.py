"""The inputs of tests/test_gpu_batch_bounds.py are sound by the reference alone (tests/batch_bounds_cases.py states the rules): every
rule is run here with the oracle, without a GPU, and each case and scenario must keep at least CAP of its 16 spectra."""
import numpy as np
import pytest

from tests import batch_bounds_cases as BB


def test_the_lengths_and_the_cases():
    assert BB.LENGTHS == (4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 255, 256, 257, 300)
    truths, batch = BB.exp2_batch()
    assert tuple(batch.n) == BB.LENGTHS and np.all(truths[:, 3] > 27.0) and np.all(truths[:, 3] < 33.0)
    # a case pins a parameter that is not last in the active order, and one runs on all 8 active parameters of model_exp4
    assert any(c.j < len(c.active) - 1 and c.model == 'exp2' for c in BB.PINNED)
    assert any(c.model == 'exp4' and len(c.active) == 8 for c in BB.PINNED)
    for c in BB.PINNED:
        lo, hi = c.box()
        s = c.starts(0.05)
        assert np.all(s[:, c.active[c.j]] == c.value) and (hi if c.side > 0 else lo)[c.j] == c.value
        assert np.sum(np.isfinite(lo)) + np.sum(np.isfinite(hi)) == 1


@pytest.mark.parametrize('name', BB.NAMES)
@pytest.mark.parametrize('key', [c.key for c in BB.PINNED])
def test_pinned_cases_keep_the_reduced_fit_and_point_outward(key, name):
    """select keeps the reduced fit, and J^T r of the full active set points outward at the pinned parameter at the start and at
    every accepted iterate: at least CAP of 16"""
    sel = BB.pinned_selection(key, name)
    kept = sum(1 for s in sel if s[0])
    print('%s (%s): kept %d of %d, smallest outward cosine of the kept %.3g, of all %.3g'
          % (key, name, kept, len(sel), min(s[4] for s in sel if s[0]), min(s[4] for s in sel)))
    assert len(sel) == 16 and kept >= BB.CAP
    for ok, one, diff, margin, cos in sel:
        if ok:
            assert cos > 0.0 and diff <= 1e-12 and margin > 2e-13


@pytest.mark.parametrize('name', BB.NAMES)
def test_released_case_stays_below_the_wall(name):
    sel = BB.released_selection(name)
    kept = sum(1 for s in sel if s[0])
    print('released (%s): kept %d of %d, the largest trial p[3] of the kept %.6g' % (name, kept, len(sel), max(s[1] for s in sel if s[0])))
    assert len(sel) == 16 and kept >= BB.CAP
    truths = BB.exp2_batch()[0]
    assert np.all(truths[:, 3] < BB.RELEASED_WALL) and np.all(BB.released_starts(0.05)[:, 3] == BB.RELEASED_WALL)


def test_mixed_case_starts_inside_and_ends_outside_without_a_box():
    """the starts lie inside the box, and the oracle's unbounded fits end well beyond the wall: the box binds in every fit"""
    starts = BB.mixed_starts()
    assert len(BB.MIXED_LENGTHS) == 24 and np.all(starts[:, 3] == BB.MIXED_START) and BB.MIXED_START < BB.MIXED_WALL
    ends = BB.unbounded_end(BB.mixed_batch().items, starts)
    print('unbounded p[3] at the end: %.3f ... %.3f' % (ends.min(), ends.max()))
    assert np.all(ends > 26.0) and np.all(ends < 34.0)
    ref = BB.mixed_reference()
    conv = [r for n, r in zip(BB.MIXED_LENGTHS, ref) if n >= BB.MIXED_CONVERGED_FROM]
    print('the reduced fits of n >= %d: stationarity %.2e ... %.2e, spread between two starts %.2e ... %.2e'
          % (BB.MIXED_CONVERGED_FROM, min(r[1] for r in conv), max(r[1] for r in conv), min(r[2] for r in conv), max(r[2] for r in conv)))
    # what the thresholds of test 6 are taken from is itself small where the reference converges
    assert len(conv) == 18 and all(r[1] < 1e-6 and r[2] < 1e-5 for r in conv)
    # the rule that selects them (converged with room, batch_bounds_cases.MIXED_ROOM) keeps exactly the lengths the reference converges on
    assert [r[3] for r in ref] == [n >= BB.MIXED_CONVERGED_FROM for n in BB.MIXED_LENGTHS]


def test_cube_case_by_the_oracle():
    x, Y = BB.cube()
    assert Y.dtype == np.uint16 and Y.shape == (BB.CUBE_FITS, BB.CUBE_N)
    ends = BB.unbounded_end(BB.cube_items(), BB.cube_starts(0.05, BB.CUBE_START))
    print('unbounded p[3] at the end: %.3f ... %.3f' % (ends.min(), ends.max()))
    assert np.all(ends > 1.2 * BB.CUBE_WALL) and BB.CUBE_START < BB.CUBE_WALL
    ref = BB.cube_reference()
    print('converged with room: %s' % [r[3] for r in ref])
    assert sum(1 for r in ref if r[3]) >= BB.CUBE_FITS // 2 and all(r[1] < 1e-6 and r[2] < 1e-5 for r in ref if r[3])
