"""The 256-lane form of the batch kernels (gfh_set_batch_lanes(256) / lanes_per_fit=256: a workgroup of four waves per fit, the four
waves' partial sums added in wave order after one barrier per reduction) under the suite of tests/batch_form_suite.py -- the form's
row of the table in tests/batch_form_cases.py: n = 4 ... 4097 at the edges of each wave's share of a 256-point row and of one to four
rows, every single fit, the batch reversed and cut, NaN neighbours, 70003 workgroups -- and what only this form's module holds: the
three forms side by side in one context.  The observed maxima go under the keys wg_*; tools/bench_batch.py --workgroup --observed
copies them into profiles/batch_workgroup.json."""
import pytest

pytest.register_assert_rewrite('tests.batch_form_suite')
from tests import batch_form_cases as FC  # noqa: E402
from tests import batch_form_suite as S  # noqa: E402
from tests.batch_common import SCENARIOS, context, same_bits, same_pass  # noqa: E402

pytestmark = pytest.mark.gpu

globals().update(S.tests_of(FC.WORKGROUP))          # F, E and the suite's tests under the names they have had here


def test_switching_forms_in_one_context(F):
    """64 -> 256 -> 16 -> 256 -> batch_pass at 256 -> a plain set_data + fit -> 256 once more, on one context and the same data: the
    three forms of the active set are resident side by side (the kernel cache's key carries the form), every result is the bits of
    the first call in that form and of a fresh context, and the plain fit returns what a fresh context returns"""
    off, kw = SCENARIOS['c']
    starts, p5 = F.starts(off), F.starts(0.05)
    k = next(i for i in range(len(F.n)) if F.n[i] == 257)
    c = context(F.tape, F.batch)
    try:
        p64, r64, _ = c.fit_batch(starts, FC.ACTIVE, **kw)
        assert c.batch_lanes_used() == 64
        p256, r256, _ = c.fit_batch(starts, FC.ACTIVE, lanes_per_fit=256, **kw)
        assert c.batch_lanes_used() == 256
        same_bits(p256, r256, *F.fit('c'))                       # (the module's context: another one)
        p16, r16, _ = c.fit_batch(starts, FC.ACTIVE, lanes_per_fit=16, **kw)
        assert c.batch_lanes_used() == 16
        p, r, _ = c.fit_batch(starts, FC.ACTIVE, lanes_per_fit=256, **kw)
        assert c.batch_lanes_used() == 256
        same_bits(p, r, p256, r256)
        same_pass(c.batch_pass(p5, FC.ACTIVE, lanes_per_fit=256), F.one_pass())
        assert c.batch_lanes_used() == 256
        plain = S.plain_fit(c, F.batch.items[k], starts[k], kw)
        p, r, _ = c.fit_batch(starts, FC.ACTIVE, **kw)           # ... and the batch and the setting are still there after the plain fit
        assert c.batch_lanes_used() == 256
        same_bits(p, r, p256, r256)
    finally:
        c.close()
    f = context(F.tape, F.batch)
    try:
        p, r, _ = f.fit_batch(starts, FC.ACTIVE, **kw)
        assert f.batch_lanes_used() == 64
        same_bits(p, r, p64, r64)
        p, r, _ = f.fit_batch(starts, FC.ACTIVE, lanes_per_fit=16, **kw)
        assert f.batch_lanes_used() == 16
        same_bits(p, r, p16, r16)
        fresh = S.plain_fit(f, F.batch.items[k], starts[k], kw)
    finally:
        f.close()
    S.same_plain_fit(plain, fresh)
