"""CPU tests of the loss of a batch (gfh_set_batch_loss, Context.set_batch_loss, the loss= / loss_scale= arguments of the batch calls;
GenConfig::batch_loss): the setter's refusals by message, the plain fit's gfh_set_loss still refused in every batch call, the loss units
compiled for gfx950 on a compile-only context, the text of every linear-loss unit byte for byte what it was before a batch had a loss
(tests/golden/batch_linear_sha1.json: recorded at the commit before), the argument checks of the session calls, and the selection
rule of tests/batch_loss_cases.py over exactly the cases tests/test_gpu_batch_loss.py uses.  That module holds the values."""
import hashlib
import json
import os

import numpy as np
import pytest

from gadfit_amd import _lib
from gadfit_amd.ad import trace_model
from tests import batch_cases as BC
from tests import batch_form_cases as FC
from tests import batch_loss_cases as LC
from tests import models as M
from tests.batch_common import TOL_FIT

INF = float('inf')
NAN = float('nan')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'batch_linear_sha1.json')


def _ctx(model=M.model_exp2, n=4):
    c = _lib.Context(-1)
    c.set_model(trace_model(model, n))
    return c


def _data(c, sizes=(10, 12, 9)):
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    with pytest.raises(_lib.GadfitHipError, match='no GPU'):
        c.set_batch_data(off, np.linspace(0.5, 9.5, n), np.ones(n), np.ones(n))
    return len(sizes)


def test_the_setter_refuses_by_message_and_needs_neither_gpu_nor_model():
    c = _lib.Context(-1)
    try:
        assert c.batch_loss_used() is None and c.batch_loss() == (0, 1.0)
        for loss in (0, 1, 2):
            for scale in (1.0, 1.345, 2.0 ** 10, 1e-3):
                c.set_batch_loss(loss, scale)
        c.set_batch_loss(2)          # scale defaults to 1
        assert c.batch_loss() == (2, 1.0)
        for loss in (-1, 3, 17):
            with pytest.raises(_lib.GadfitHipError, match=r'gfh_set_batch_loss: unknown loss %d \(0: linear, 1: cauchy, 2: huber\)' % loss):
                c.set_batch_loss(loss, 1.0)
        with pytest.raises(_lib.GadfitHipError, match='gfh_set_batch_loss: the residual scale is NaN'):
            c.set_batch_loss(1, NAN)
        for scale in (INF, -INF):
            with pytest.raises(_lib.GadfitHipError, match='gfh_set_batch_loss: the residual scale is infinite'):
                c.set_batch_loss(1, scale)
        for scale in (0.0, -0.0, -1.0, 1e-310):          # (1 / 1e-310 is infinite)
            with pytest.raises(_lib.GadfitHipError, match='gfh_set_batch_loss: the residual scale must be positive'):
                c.set_batch_loss(2, scale)
        # an unknown loss is named before a bad scale; a refused call leaves the setting
        with pytest.raises(_lib.GadfitHipError, match='unknown loss'):
            c.set_batch_loss(5, NAN)
        assert c.batch_loss() == (2, 1.0)
        c.set_model(trace_model(M.model_exp2, 4))
        assert '#define GFH_BLOSS 2\n' in c.batch_source([0, 1, 2, 3])
        assert c.batch_loss_used() is None          # a setting is no launch
    finally:
        c.close()


def test_the_plain_fits_loss_stays_refused_in_every_batch_call():
    c = _ctx()
    try:
        nf = _data(c)
        start = np.tile(M.EXP2_TRUTH, (nf, 1))
        a = [0, 1, 2, 3]
        for batch_loss in (0, 1, 2):
            c.set_batch_loss(batch_loss, 2.0)
            c.set_loss(1)
            calls = (('gfh_fit_batch', lambda: c.fit_batch(start, a, max_iter=2)),
                     ('gfh_fit_batch_errors', lambda: c.fit_batch_errors(start, a, max_iter=2)),
                     ('gfh_fit_batch_bounded', lambda: c.fit_batch_bounded(start, a, [-INF] * 4, [INF] * 4, max_iter=2)),
                     ('gfh_batch_pass', lambda: c.batch_pass(start, a)),
                     ('gfh_batch_covariance', lambda: c.batch_covariance(start, a)),
                     ('gfh_batch_eval', lambda: c.batch_eval(start, a)),
                     ('gfh_batch_source', lambda: c.batch_source(a)),
                     ('gfh_batch_source_bounded', lambda: c.batch_source(a, bounded=True)),
                     ('gfh_batch_prepare', lambda: c.batch_prepare(a)),
                     ('gfh_batch_prepare_bounded', lambda: c.batch_prepare(a, bounded=True)))
            for who, call in calls:
                with pytest.raises(_lib.GadfitHipError, match=who + r': a robust loss \(gfh_set_loss\) is not carried by the batch kernels.*gfh_set_batch_loss'):
                    call()
            c.set_loss(0)
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):          # ... and with it gone the call gets as far as the device
                c.fit_batch(start, a, max_iter=2)
    finally:
        c.close()


def test_keywords_of_the_calls_set_the_loss_and_none_leaves_it():
    c = _ctx()
    try:
        nf = _data(c)
        start = np.tile(M.EXP2_TRUTH, (nf, 1))
        a = [0, 1, 2, 3]
        for call in (lambda **kw: c.fit_batch(start, a, max_iter=2, **kw), lambda **kw: c.fit_batch_errors(start, a, max_iter=2, **kw),
                     lambda **kw: c.fit_batch_bounded(start, a, [-INF] * 4, [INF] * 4, max_iter=2, **kw),
                     lambda **kw: c.batch_pass(start, a, **kw), lambda **kw: c.batch_covariance(start, a, **kw)):
            c.set_batch_loss(0, 1.0)
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                call(loss=2, loss_scale=1.345)
            assert '#define GFH_BLOSS 2\n' in c.batch_source(a)          # it stays set
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                call()                                                    # None leaves the setting
            assert '#define GFH_BLOSS 2\n' in c.batch_source(a)
            with pytest.raises(_lib.GadfitHipError, match='no GPU'):
                call(loss=1)                                              # the scale alone is left
            assert '#define GFH_BLOSS 1\n' in c.batch_source(a) and c.batch_loss() == (1, 1.345)
            with pytest.raises(_lib.GadfitHipError, match='the residual scale must be positive'):
                call(loss_scale=-2.0)
            with pytest.raises(_lib.GadfitHipError, match='unknown loss 7'):
                call(loss=7)
    finally:
        c.close()


@pytest.mark.parametrize('lanes', [16, 64, 256])
def test_the_loss_units_compile_for_gfx950(lanes):
    """model_exp2 with 4 and model_exp4 with 8 active parameters, the four kernels' unit and the bounded one, both losses"""
    for model, n in ((M.model_exp2, 4), (M.model_exp4, 8)):
        c = _ctx(model, n)
        try:
            c.set_batch_lanes(lanes)
            for loss in LC.LOSSES:
                c.set_batch_loss(loss, 1.345)
                c.batch_prepare(list(range(n)))
                c.batch_prepare(list(range(n)), bounded=True)
        finally:
            c.close()


def test_the_loss_units_of_a_uint16_cube_compile():
    c = _ctx()
    try:
        LC.hold_text_cube(c)
        for loss in LC.LOSSES:
            c.set_batch_loss(loss, 2.0)
            src = c.batch_source([0, 1, 2, 3])
            assert '#define GFH_BCUBE 1' in src and '#define GFH_BYTYPE 2' in src and '#define GFH_BLOSS %d\n' % loss in src
            c.batch_prepare([0, 1, 2, 3])
            c.batch_prepare([0, 1, 2, 3], bounded=True)
    finally:
        c.close()


def test_the_text_of_every_linear_unit_is_what_it_was():
    """set_batch_loss(0, 7.0): the scale is no part of the text, and the linear units' text equals the record made at the commit
    before this feature, byte for byte (sha1)"""
    with open(GOLDEN) as fh:
        gold = json.load(fh)
    seen = 0
    for name, (model, n, active) in LC.TEXT_MODELS.items():
        for data in LC.TEXT_DATA:
            c = _ctx(model, n)
            try:
                if data != 'ragged':
                    LC.hold_text_cube(c)
                for lanes in LC.TEXT_LANES:
                    c.set_batch_lanes(lanes)
                    for bounded in (False, True):
                        c.set_batch_loss(1, 3.0)
                        robust = c.batch_source(active, bounded=bounded)
                        c.set_batch_loss(0, 7.0)
                        src = c.batch_source(active, bounded=bounded)
                        assert hashlib.sha1(src.encode()).hexdigest() == gold[LC.text_key(name, data, lanes, bounded)], (name, data, lanes, bounded)
                        assert 'GFH_BLOSS' not in src and 'inv_c' not in src
                        # the loss unit: its define, the argument, and no unresolved region
                        assert robust != src and '#define GFH_BLOSS 1\n' in robust and 'const double inv_c' in robust
                        assert not any(line in ('#if GFH_BLOSS', '#else  // GFH_BLOSS', '#endif  // GFH_BLOSS') for line in robust.split('\n'))
                        assert '#define GFH_LOSS 0\n' in robust          # the plain units' switch stays 0 in a batch unit
                        c.set_batch_loss(1, 5.0)
                        assert c.batch_source(active, bounded=bounded) == robust          # the scale is an argument, not text
                        seen += 1
            finally:
                c.close()
    assert seen == len(gold) == 24


def test_every_unit_the_gpu_tests_ask_for_compiles():
    """... into the in-tree cache, where the GPU tests find them (build() compiles the same list)"""
    assert LC.prepare_units(lambda: _lib.Context(-1)) > 0


def test_the_loss_arguments_of_the_session_calls():
    from gadfit_amd import gadfit as gf
    from gadfit_amd.ad import exp

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    x = np.linspace(0.5, 9.5, 10)
    gf.gadf_close()
    gf.gadf_init(exp2())
    try:
        for k in range(4):
            gf.gadf_set(k + 1, float(M.EXP2_TRUTH[k]), True)
        calls = (('gadf_fit_batch', lambda **kw: gf.gadf_fit_batch([x], [x], None, [M.EXP2_TRUTH], max_iter=1, **kw)),
                 ('gadf_fit_cube', lambda **kw: gf.gadf_fit_cube(x, np.ones((1, 10)), [M.EXP2_TRUTH], max_iter=1, **kw)),
                 ('gadf_fit_frames', lambda **kw: gf.gadf_fit_frames(x, np.ones((10, 1)), [M.EXP2_TRUTH], max_iter=1, **kw)))
        for who, call in calls:
            for bad in (3, -1, 'cauchy', 1.0, True):
                with pytest.raises(gf.GadfitError, match=who + ': loss must be None, LOSS_LINEAR, LOSS_CAUCHY or LOSS_HUBER'):
                    call(loss=bad)
            for bad in (0.0, -1.0, NAN, INF, 'wide', True):
                with pytest.raises(gf.GadfitError, match=who + r': loss_scale must be a finite number > 0'):
                    call(loss=gf.LOSS_HUBER, loss_scale=bad)
    finally:
        gf.gadf_close()


# ---- the selection rule over exactly the cases of the GPU module ---------------------------------------------------------------------------
# The rule is evaluated by the oracle alone: these tests check the INPUTS of the GPU module, not the kernels.  Each of them first asks the
# library for the unit of every case it is about to judge (_accepted: set_batch_loss with the case's loss and scale on a compile-only
# context, and the unit's text carrying that loss), so that a case the library would refuse cannot pass the rule unseen.
def _accepted(tape, cases, lanes=64, cube=False):
    """cases: [(active, loss, c)]"""
    c = _lib.Context(-1)
    try:
        c.set_model(tape)
        c.set_batch_lanes(lanes)
        if cube:
            LC.hold_text_cube(c)
        for active, loss, scale in cases:
            c.set_batch_loss(loss, scale)
            assert c.batch_loss() == (loss, scale) and '#define GFH_BLOSS %d\n' % loss in c.batch_source(active)
    finally:
        c.close()


@pytest.mark.parametrize('name', ['conv', 'conv_acc', 'far_acc'])
def test_the_rule_over_part_a(name):
    """A case is (scenario, loss, c) over the eight active sets: 384 fits.  The caps hold per set of 48.  Not vacuous: in each case at
    least half of the kept fits make 3 iterations or more, and EVERY kept fit's robust parameters differ from the oracle's linear ones
    by more than 100 TOL_FIT (the smallest difference is 5.9e-4).  Per set the first does not hold everywhere: under Huber at c = 2
    the sets [6, 1, 4] and [0, 2, 4, 6] converge in two iterations in 40 and 36 of their 48 fits (every fit of every set makes two
    or more but for [0, 1], where up to three spectra stop at their start in either implementation)."""
    cases = [k for k in LC.fit_cases(64) if k[0] == name]
    _accepted(LC.part_a()[0], [k[1:] for k in cases])
    assert cases and all(k in cases for lanes in (16, 256) for k in LC.fit_cases(lanes) if k[0] == name)
    for loss, c in dict.fromkeys((k[2], k[3]) for k in cases):
        kept_all, total, three = 0, 0, 0
        for active in [k[1] for k in cases if (k[2], k[3]) == (loss, c)]:
            sel = LC.selection_a(active, name, loss, c)
            kept = [s for s in sel if s[0]]
            kept_all += len(kept); total += len(sel)
            assert len(sel) - len(kept) <= LC.CAP_A[name], (name, active, loss, c, len(kept))
            three += sum(1 for s in kept if s[1][0][0] >= 3)
            lin = LC.linear_pars_a(active, name)
            moved = [float(np.max(np.abs(s[1][1][active] - lin[b][active]) / np.abs(lin[b][active]))) for b, s in enumerate(sel) if s[0]]
            assert min(moved) > 100.0 * TOL_FIT, (name, active, loss, c, min(moved))
        print('%s, %s, c = %g: the rule keeps %d of %d fits, %d of them make 3 iterations or more' % (name, LC.LOSS_NAMES[loss], c, kept_all, total, three))
        assert total == 48 * len(LC.SETS) and 2 * three >= kept_all
        if LC.CAP_A[name] == 0:
            assert kept_all == total


@pytest.mark.parametrize('form', FC.FORMS, ids=lambda f: str(f.lanes))
def test_the_rule_over_part_b(form):
    _accepted(LC.part_b(form)[0], [(LC.ACTIVE2, loss, 1.0) for loss in LC.LOSSES], form.lanes)
    for loss in LC.LOSSES:
        sel = LC.selection_b(form, loss)
        kept = sum(1 for s in sel if s[0])
        print('%d lanes, %s: the rule keeps %d of %d fits' % (form.lanes, LC.LOSS_NAMES[loss], kept, len(sel)))
        assert len(sel) == 2 * len(form.edges) and len(sel) - kept <= BC.RANDOM_CAP * len(sel)


def test_the_rule_over_the_pinned_case():
    from tests import batch_bounds_cases as BB
    _accepted(LC.PINNED.tape(), [(LC.PINNED.active, LC.CAUCHY, 1.0)])
    sel = LC.pinned_selection()
    kept = sum(1 for s in sel if s[0])
    print('pinned under cauchy: the rule keeps %d of %d fits' % (kept, len(sel)))
    assert kept >= BB.CAP


def test_the_cube_holds_its_steps():
    _accepted(LC.part_b(FC.WAVE)[0], [(LC.ACTIVE2, LC.CUBE_LOSS, LC.CUBE_SCALE)], cube=True)
    x, Y, starts = LC.cube()
    assert Y.dtype == np.uint16 and Y.shape == (LC.CUBE_FITS, LC.CUBE_N) and x.shape == (LC.CUBE_N,) and starts.shape == (LC.CUBE_FITS, 4)
