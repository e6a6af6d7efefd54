"""The 16-lane form of the batch kernels (gfh_set_batch_lanes(16) / lanes_per_fit=16: a DPP row per fit, four fits per wave, sixteen
per workgroup) under the suite of tests/batch_form_suite.py -- the form's row of the table in tests/batch_form_cases.py: n = 4 ... 257
at the row's edges, every single fit, the batch reversed and cuts that leave rows, waves and a last workgroup without a fit, NaN in
the other rows of a wave, 8193 workgroups -- and what only this form's module holds: whose form a launch takes, and both forms side
by side in one context.  The observed maxima go under the keys rows_*; tools/bench_batch.py copies them into profiles/batch_rows.json."""
import pytest

pytest.register_assert_rewrite('tests.batch_form_suite')
from gadfit_amd import _lib  # noqa: E402
from tests import batch_form_cases as FC  # noqa: E402
from tests import batch_form_suite as S  # noqa: E402
from tests.batch_common import SCENARIOS, context, same_bits, same_pass  # noqa: E402

pytestmark = pytest.mark.gpu

globals().update(S.tests_of(FC.ROWS))          # F, E and the suite's tests under the names they have had here


def test_the_form_is_the_callers_and_64_without_the_argument(F):
    """a context nobody told anything launches the wave form; lanes_per_fit=16 the row form, and the setting stays; set_batch_lanes(64) goes back"""
    off, kw = SCENARIOS['a']
    k = 9
    starts = F.starts(off)[:k]
    c = context(F.tape)
    try:
        c.set_batch_data(*F.batch.first(k))
        assert c.batch_lanes_used() == 0
        c.fit_batch(starts, FC.ACTIVE, **kw)
        assert c.batch_lanes_used() == 64
        c.batch_pass(starts, FC.ACTIVE, lanes_per_fit=16)
        assert c.batch_lanes_used() == 16
        c.fit_batch(starts, FC.ACTIVE, **kw)
        assert c.batch_lanes_used() == 16
        c.set_batch_lanes(64)
        c.batch_pass(starts, FC.ACTIVE)
        assert c.batch_lanes_used() == 64
        c.set_batch_lanes(0)                                     # auto: the rule's form for (4 active, longest of these 9)
        c.fit_batch(starts, FC.ACTIVE, **kw)
        assert c.batch_lanes_used() == _lib.batch_auto_lanes(4, int(F.n[:k].max()))
    finally:
        c.close()


def test_both_forms_in_one_context(F):
    """64 -> 16 -> 64 -> batch_pass at 16 -> a plain set_data + fit -> 16 once more, on one context and the same data: both forms of
    the active set are resident side by side (the kernel cache's key carries the form), every result is the bits of the first call
    in that form and of a fresh context, and the plain fit returns what a fresh context returns"""
    off, kw = SCENARIOS['c']
    starts, p5 = F.starts(off), F.starts(0.05)
    k = next(i for i in range(len(F.n)) if F.n[i] == 257)
    c = context(F.tape, F.batch)
    try:
        p64, r64, _ = c.fit_batch(starts, FC.ACTIVE, **kw)
        assert c.batch_lanes_used() == 64
        p16, r16, _ = c.fit_batch(starts, FC.ACTIVE, lanes_per_fit=16, **kw)
        assert c.batch_lanes_used() == 16
        same_bits(p16, r16, *F.fit('c'))                         # (the module's context: another one)
        p, r, _ = c.fit_batch(starts, FC.ACTIVE, lanes_per_fit=64, **kw)
        assert c.batch_lanes_used() == 64
        same_bits(p, r, p64, r64)
        same_pass(c.batch_pass(p5, FC.ACTIVE, lanes_per_fit=16), F.one_pass())
        assert c.batch_lanes_used() == 16
        plain = S.plain_fit(c, F.batch.items[k], starts[k], kw)
        p, r, _ = c.fit_batch(starts, FC.ACTIVE, **kw)           # ... and the batch and the setting are still there after the plain fit
        assert c.batch_lanes_used() == 16
        same_bits(p, r, p16, r16)
    finally:
        c.close()
    f = context(F.tape, F.batch)
    try:
        p, r, _ = f.fit_batch(starts, FC.ACTIVE, **kw)
        assert f.batch_lanes_used() == 64
        same_bits(p, r, p64, r64)
        fresh = S.plain_fit(f, F.batch.items[k], starts[k], kw)
    finally:
        f.close()
    S.same_plain_fit(plain, fresh)
