"""Batched fits inside a box on the device (gfh_fit_batch_bounded: the kernel gfh_k_fit_batch_bounded) on the three lane forms.  The
inputs and the rules that select them are tests/batch_bounds_cases.py (run by the oracle alone in tests/test_cpu_batch_bounds_cases.py);
the bounds are the project's own (tests/batch_common.py).

 3. No bound, no change: with infinite bounds, and with +-1e300, parameters and records are fit_batch's bits and at_bound is 0.
 4. Pinned throughout equals the reduced fit: the oracle's fit with the pinned parameter passive, count for count.
 5. Released at once: a start ON a wall with the truth inside gives fit_batch's bits.
 6. The mixed regime: inside the box, at_bound exact, chi2 not above the start's, independent of the batch, and a constrained
    stationary point by the oracle's sweep() -- thresholds from the oracle's reduced fit, computed here at run time, on the
    spectra on which that fit converges with room (batch_bounds_cases.MIXED_ROOM).
 7. gadf_fit_batch, gadf_fit_cube and gadf_fit_frames with bounds= return Context.fit_batch_bounded's bits."""
import numpy as np
import pytest

from gadfit_amd import _lib
from oracle import binding as orc
from tests import batch_bounds_cases as BB
from tests.batch_common import SCENARIOS, TOL_CHI2, TOL_PARS, check_fit, context, fit_worst, observe, same_bits

pytestmark = pytest.mark.gpu

FORMS = (64, 16, 256)
INF = float('inf')


@pytest.fixture(scope='module')
def C2():
    c = context(BB.tape2(), BB.exp2_batch()[1])
    yield c
    c.close()


@pytest.fixture(scope='module')
def C4():
    c = context(BB.tape4(), BB.exp4_batch()[1])
    yield c
    c.close()


@pytest.fixture(scope='module')
def CM():
    c = context(BB.tape2(), BB.mixed_batch())
    yield c
    c.close()


@pytest.fixture(scope='module')
def CC():
    c = context(BB.tape2())
    x, Y = BB.cube()
    c.set_batch_cube(x, Y, BB.CUBE_ERROR)
    yield c
    c.close()


def _unchanged(c, starts, active, lanes, kw):
    p0, r0, _ = c.fit_batch(starts, active, lanes_per_fit=lanes, **kw)
    na = len(active)
    for lo, hi in (([-INF] * na, [INF] * na), ([-1e300] * na, [1e300] * na)):
        p, r, at, _ = c.fit_batch_bounded(starts, active, lo, hi, lanes_per_fit=lanes, **kw)
        same_bits(p, r, p0, r0)
        assert at.dtype == np.int32 and np.all(at == 0)
    assert c.batch_lanes_used() == lanes
    return r0


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', BB.NAMES)
@pytest.mark.parametrize('lanes', FORMS)
def test_no_bound_no_change(C2, C4, lanes, name):
    off, kw = SCENARIOS[name]
    for active in ([0], [0, 1, 2, 3], [3, 1]):
        r = _unchanged(C2, BB.exp2_starts(off), active, lanes, kw)
    print('exp2 (%s, %d lanes): exits %s' % (name, lanes, sorted(set(r['exit_reason'].tolist()))))
    _unchanged(C4, BB.exp4_starts(off), list(range(8)), lanes, kw)


@pytest.mark.parametrize('name', BB.NAMES)
def test_no_bound_no_change_on_a_uint16_cube(CC, name):
    off, kw = SCENARIOS[name]
    _unchanged(CC, BB.cube_starts(off), BB.ACTIVE, 64, kw)
    assert CC.batch_form_used() == ('cube', 2, BB.CUBE_ERROR)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', BB.NAMES)
@pytest.mark.parametrize('key', [c.key for c in BB.PINNED])
@pytest.mark.parametrize('lanes', FORMS)
def test_pinned_throughout_equals_the_reduced_fit(C2, C4, lanes, key, name):
    case = next(c for c in BB.PINNED if c.key == key)
    off, kw = SCENARIOS[name]
    c = C2 if case.model == 'exp2' else C4
    lo, hi = case.box()
    pars, res, at, _ = c.fit_batch_bounded(case.starts(off), case.active, lo, hi, lanes_per_fit=lanes, **kw)
    sel = BB.pinned_selection(key, name)
    kept = [b for b, s in enumerate(sel) if s[0]]
    assert len(kept) >= BB.CAP
    worst = fit_worst(BB.expanded(case, sel), pars, res, case.batch().n, len(case.active))
    # the pinned parameter comes back as the bits of its bound, and says so
    wall = np.float64(case.value)
    for b in kept:
        assert pars[b, case.active[case.j]].view(np.uint64) == wall.view(np.uint64), b
        assert int(at[b]) == case.bit(), (b, int(at[b]))
    check_fit('bounds_pinned_lanes%d' % lanes, '%s_%s' % (key, name), worst, TOL_PARS, TOL_CHI2)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', BB.NAMES)
@pytest.mark.parametrize('lanes', FORMS)
def test_released_at_once(C2, lanes, name):
    off, kw = SCENARIOS[name]
    starts = BB.released_starts(off)
    kept = np.array([b for b, s in enumerate(BB.released_selection(name)) if s[0]])
    assert kept.size >= BB.CAP
    lo, hi = BB.box(4, hi3=BB.RELEASED_WALL)
    p0, r0, _ = C2.fit_batch(starts, BB.ACTIVE, lanes_per_fit=lanes, **kw)
    p, r, at, _ = C2.fit_batch_bounded(starts, BB.ACTIVE, lo, hi, lanes_per_fit=lanes, **kw)
    same_bits(p[kept], r[kept], p0[kept], r0[kept])
    moved = kept[r0['iterations'][kept] > 0]
    assert np.all(at[moved] == 0) and np.all(p[moved, 3] < BB.RELEASED_WALL)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def _at_bound(p, active, lo, hi):
    at = np.zeros(p.shape[0], dtype=np.int64)
    for j, a in enumerate(active):
        at |= np.where(p[:, a] == lo[j], 1 << j, 0) | np.where(p[:, a] == hi[j], 1 << (8 + j), 0)
    return at


def _mixed(c, set_data, items, starts, wall, reference, lanes, key):
    """test 6 on the batch `c` holds; set_data(ctx, order) gives a fresh context the spectra `order` of it"""
    lo, hi = BB.box(4, hi3=wall)
    kw = BB.MIXED_KW
    n = len(items)
    pars, res, at, _ = c.fit_batch_bounded(starts, BB.ACTIVE, lo, hi, lanes_per_fit=lanes, **kw)
    print('%s: iterations %s, exits %s, at_bound %s' % (key, sorted(set(res['iterations'].tolist())), sorted(set(res['exit_reason'].tolist())),
                                                       sorted(set(at.tolist()))))
    # inside the box, exactly; at_bound is exact equality on what came back
    assert np.all(pars[:, BB.ACTIVE] >= lo) and np.all(pars[:, BB.ACTIVE] <= hi)
    assert np.array_equal(at, _at_bound(pars, BB.ACTIVE, lo, hi))
    # chi2 did not rise: the start's is the oracle's
    for b, (x, y, w) in enumerate(items):
        chi0 = orc.OracleProblem(BB.tape2(), [x], [y], [w], [starts[b]], BB.ACTIVE, [0] * 4).chi2()[0]
        assert res['chi2'][b] <= chi0, (b, res['chi2'][b], chi0)
    # the same bits alone, in the batch and in the batch reversed
    other = context(BB.tape2())
    try:
        set_data(other, list(range(n))[::-1])
        pr, rr, ar, _ = other.fit_batch_bounded(starts[::-1], BB.ACTIVE, lo, hi, lanes_per_fit=lanes, **kw)
        same_bits(pr[::-1], rr[::-1], pars, res)
        assert np.array_equal(ar[::-1], at)
        for b in range(n):
            set_data(other, [b])
            p1, r1, a1, _ = other.fit_batch_bounded(starts[b:b + 1], BB.ACTIVE, lo, hi, lanes_per_fit=lanes, **kw)
            same_bits(p1, r1, pars[b:b + 1], res[b:b + 1])
            assert a1[0] == at[b]
    finally:
        other.close()
    # a constrained stationary point by the oracle's sweep(), where the reference itself converges
    worst = dict(grad=0.0, pars=0.0)
    for b, (x, y, w) in enumerate(items):
        end0, g0, spread, converged = reference[b]
        if not converged:
            continue
        assert int(at[b]) == 1 << 11 and pars[b, 3] == wall, (b, int(at[b]), pars[b, 3])
        g, JTr, _ = BB.stationarity(BB.tape2(), x, y, w, pars[b], BB.ACTIVE, [0, 1, 2])
        assert JTr[3] > 0.0, (b, JTr[3])                      # the pinned coordinate: descent pushes through the wall
        diff = float(np.max(np.abs(pars[b, :3] - end0[:3]) / np.abs(end0[:3])))
        print('%s fit %d (n = %d): free gradient %.2e (reference %.2e), free parameters off the reduced fit by %.2e (its spread %.2e)'
              % (key, b, x.size, np.max(g), g0, diff, spread))
        worst['grad'] = max(worst['grad'], float(np.max(g)) / g0); worst['pars'] = max(worst['pars'], diff / spread)
    observe(**{'bounds_mixed_%s_gradient_over_reference' % key: worst['grad'], 'bounds_mixed_%s_pars_over_spread' % key: worst['pars']})
    assert worst['grad'] <= 10.0 and worst['pars'] <= 10.0


@pytest.mark.parametrize('lanes', FORMS)
def test_mixed_regime(CM, lanes):
    batch = BB.mixed_batch()

    def set_data(ctx, order):
        sub = BB.BC.Batch([batch.items[b] for b in order])
        ctx.set_batch_data(sub.off, sub.x, sub.y, sub.w)
    _mixed(CM, set_data, batch.items, BB.mixed_starts(), BB.MIXED_WALL, BB.mixed_reference(), lanes, 'lanes%d' % lanes)


def test_mixed_regime_on_a_uint16_cube(CC):
    x, Y = BB.cube()

    def set_data(ctx, order):
        ctx.set_batch_cube(x, np.ascontiguousarray(Y[order]), BB.CUBE_ERROR)
    _mixed(CC, set_data, BB.cube_items(), BB.cube_starts(0.05, BB.CUBE_START), BB.CUBE_WALL, BB.cube_reference(), 64, 'cube')


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_the_session_calls_return_the_context_calls_bits():
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    kw = dict(lambda_=1.0, max_iter=30, chi2_rel=2.0 ** -20)          # (exact in real32, as the session passes them)
    gf.gadf_close()
    gf.gadf_init(exp2())
    try:
        batch = BB.exp2_batch()[1]
        starts = BB.exp2_starts(0.05).copy()
        starts[:, 3] = 15.0
        for k in range(4):
            gf.gadf_set(k + 1, float(starts[0][k]), True)
        lo, hi = BB.box(4, hi3=BB.MIXED_WALL, lo0=0.0)
        p, r, e = gf.gadf_fit_batch([it[0] for it in batch.items], [it[1] for it in batch.items], [it[2] for it in batch.items], starts,
                                    bounds=([0.0, None, None, None], [None, INF, None, BB.MIXED_WALL]), **kw)
        assert sorted(e) == ['at_bound'] and np.any(e['at_bound'] == 1 << 11)
        p0, r0, at0, _ = gf._S.ctx.fit_batch_bounded(starts, BB.ACTIVE, lo, hi, **kw)
        same_bits(p, r, p0, r0)
        assert np.array_equal(e['at_bound'], at0)
        assert len(gf.gadf_fit_batch([it[0] for it in batch.items], [it[1] for it in batch.items], [it[2] for it in batch.items], starts, **kw)) == 2
        # the cube and the frames
        x, Y = BB.cube()
        cs = BB.cube_starts(0.05, BB.CUBE_START)
        gf.gadf_set_errors(gf.SQRT_Y)
        box = ([None] * 4, [None, None, None, BB.CUBE_WALL])
        pc, rc, ec = gf.gadf_fit_cube(x, Y, cs, bounds=box, **kw)
        p0, r0, at0, _ = gf._S.ctx.fit_batch_bounded(cs, BB.ACTIVE, *BB.box(4, hi3=BB.CUBE_WALL), **kw)
        same_bits(pc, rc, p0, r0)
        assert np.array_equal(ec['at_bound'], at0) and np.any(at0 == 1 << 11)
        pf, rf, ef = gf.gadf_fit_frames(x, np.ascontiguousarray(Y.T), cs, bounds=box, **kw)
        same_bits(pf, rf, p0, r0)
        assert np.array_equal(ef['at_bound'], at0)
    finally:
        gf.gadf_close()
