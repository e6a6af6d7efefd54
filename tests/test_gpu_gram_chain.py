"""The kernels of the unfused Gram chain, each at a size where it is the one that runs (tests/gram_chain_cases.py: the cases, what each
is there to reach, and the launches it expects): every instantiation of launch_gram behind the plain sweep, the three assembling
kernels and the two finishes of a J^T v product.  Every case is one full pass against the CPU oracle at the unchanged tolerances of
tests/parity_common.py: _device_vs_oracle (Jacobian, residuals, J^T J exactly symmetric, J^T r, chi2 from the sweep and from chi2(),
STEP 3 and the convergence sums; Part H without STEP 3), and then, on the same data,
 - Context.debug_layout() equals the case's expectation and Context.debug_chain() -- what the host launched: the Gram instantiations
   with their block origins, the assembling step, the J^T v finish -- equals expect_chain(): the case ran the kernels it is here for,
 - chi2() at the sweep's parameters is bitwise the sweep's sum of squares wherever launch.cpp claims it (the fused kernel,
   k_gram_small, k_gram_block),
 - parts G and H: further contexts with one switch off each (GADFIT_HIP_MERGE_SMALL, GADFIT_HIP_SPARSE, GADFIT_HIP_TAIL) return bit
   for bit the same J^T J (both triangles), J^T r, chi2, J^T omega and aux(0) through the other kernels.
tests/test_cpu_gram_chain_cases.py shows without a GPU that the oracle is a sound reference on these inputs."""
import numpy as np
import pytest

from gadfit_amd import _lib
from tests import gram_chain_cases as CH
from tests.parity_common import _device_vs_oracle

pytestmark = pytest.mark.gpu


class _KeepsModel:
    """a context whose set_model is skipped while the tape is the one it holds: the kernels loaded for it stay (set_data alone between
    the sizes of a count)"""

    def __init__(self, ctx):
        self._ctx, self._held = ctx, None

    def set_model(self, tape):
        if tape is not self._held:
            self._ctx.set_model(tape)
            self._held = tape

    def __getattr__(self, name):
        return getattr(self._ctx, name)


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield _KeepsModel(c)
    c.close()


@pytest.fixture(scope='module')
def unfused():
    """one context created under GADFIT_HIP_FUSED=0 (the switch is read at creation): plain sweep + the stand-alone Gram kernels"""
    mp = pytest.MonkeyPatch()
    mp.setenv('GADFIT_HIP_FUSED', '0')
    try:
        c = _lib.Context(0)
    finally:
        mp.undo()
    yield _KeepsModel(c)
    c.close()


def _check(ctx, c, with_omega=True, **switches):
    """the pass against the oracle, the layout and the launches against the case module, chi2() against the sweep's sum; returns
    (the oracle problem, (J^T J, J^T r, chi2) of a sweep at its parameters)"""
    xs, ys, ws, start = c.data()
    p = _device_vs_oracle(ctx, c.tape(), xs, ys, ws, start, c.active, c.is_global, with_omega=with_omega)
    assert p.dim == c.dim
    if not with_omega:
        ctx.aux(0, dim=p.dim)          # (a J^T v product, so that the report has a finish)
    want = CH.expect_chain(c, **switches)
    got = ctx.debug_chain()
    print('%s: %s' % (c.id, got))
    assert ctx.debug_layout() == c.expect(**{k: v for k, v in switches.items() if k != 'merge_small'}), c.id
    assert got == want, (c.id, got, want)
    stored = ctx.sweep(p.pars, c.active, p.jac, p.dim)
    chi_k = ctx.chi2(p.pars)
    print('%s: chi2 of the sweep %.17g, of chi2() %.17g' % (c.id, stored[2], chi_k))
    if CH.chi2_is_bitwise(c, switches.get('fused_on', True)):
        assert chi_k == stored[2], (c.id, stored[2], chi_k)
    return p, stored


def _products(k, c, p, d1):
    """(J^T J, J^T r, chi2, J^T omega or None, aux(0)) of context k, in this order of calls"""
    JTJ, JTr, chi2 = k.sweep(p.pars, c.active, p.jac, p.dim)
    jto = k.omega(p.pars, d1) if d1 is not None else None
    return JTJ, JTr, chi2, jto, k.aux(0, dim=p.dim)


def _other_context(c, p, d1, monkeypatch, switch):
    """(_products, debug_layout(), debug_chain()) of a fresh context created with the environment switch off"""
    xs, ys, ws, _ = c.data()
    monkeypatch.setenv(switch, '0')
    k = _lib.Context(0)
    try:
        k.set_model(c.tape())
        k.set_data(np.concatenate(xs), np.concatenate(ys), np.concatenate(ws), np.concatenate([[0], np.cumsum(c.sizes)]))
        return _products(k, c, p, d1), k.debug_layout(), k.debug_chain()
    finally:
        k.close()
        monkeypatch.delenv(switch)


def _bitwise(a, b, what):
    for name, u, v in zip(('JTJ', 'JTres', 'chi2', 'JTomega', 'aux0'), a, b):
        if u is None and v is None:
            continue
        assert np.array_equal(np.asarray(u), np.asarray(v)), (what, name, float(np.max(np.abs(np.asarray(u) - np.asarray(v)))))
    assert np.array_equal(a[0], a[0].T) and np.array_equal(b[0], b[0].T), what


@pytest.mark.parametrize('c', CH.part_e(), ids=repr)
def test_every_block_shape_beyond_the_fused_kernel(ctx, c):
    """Part E: 145 and 160 active (T = 10: <4,4,true> twice, <2,2,true>, <4,4,false>, <4,2,false> twice), 161 and 176 (T = 11: <3,3,true>,
    <4,3,false>), 193 (T = 13: three block rows, a second off-diagonal column offset, <1,1,true>, <4,1,false>) at 65, 1025 and 2049 points"""
    assert c.active[:3] == [0, 1, 2] and c.active[3] > 3 and not c.fused
    _check(ctx, c)
    assert all(g.startswith('block<') for g in ctx.debug_chain()['gram'])


@pytest.mark.parametrize('c', CH.part_f(), ids=repr)
def test_standalone_gram_kernels_under_the_fused_switch(unfused, c):
    """Part F: GADFIT_HIP_FUSED=0 -- Part A's counts (k_gram<T> with one live row and with one padding row in the last tile; <5,5,true>,
    <6,6,true>, T = 8 and 9 through the block loop), layout B1 of every fused form at 65, 1025 and 2049 points, T = 7 at 97 and 111,
    k_gram_small<1 ... 8> at 1, 1025 and 2049 points, and layout B2 at 32 and 96 (the scatter through inv[] behind these kernels)"""
    _check(unfused, c, fused_on=False)
    assert unfused.debug_layout()['fused'] == 0 and unfused.debug_chain()['gram']


@pytest.mark.parametrize('nd', CH.G_DATASETS, ids=lambda nd: 'G-%d' % nd)
def test_many_datasets_finish_at_its_limit_and_dense_fallback(ctx, nd, monkeypatch):
    """Part G: 512 datasets (n_datasets * na = 4096: k_jtv_finish with V[] full) and 513 (the three-launch chain); the pattern-only
    image through k_gather_sum, and bit for bit the same through the chain finish (GADFIT_HIP_MERGE_SMALL=0), through k_assemble on
    the dense image of more than 2^18 entries (GADFIT_HIP_SPARSE=0) and under GADFIT_HIP_TAIL=0"""
    c = CH.part_g_case(nd)
    p, stored = _check(ctx, c)
    d1 = _lib.potr(stored[0] + np.diag(np.diag(stored[0])), stored[1])
    mine = _products(ctx, c, p, d1)
    assert ctx.debug_chain() == CH.expect_chain(c)
    _bitwise(mine[:3], stored, c.id)
    for switch, kw in (('GADFIT_HIP_MERGE_SMALL', dict(merge_small=False)), ('GADFIT_HIP_SPARSE', dict(sparse_ok=False)), ('GADFIT_HIP_TAIL', dict(tail_on=False))):
        other, lay, chain = _other_context(c, p, d1, monkeypatch, switch)
        print('%s under %s=0: %s' % (c.id, switch, chain))
        assert lay == c.expect(**{k: v for k, v in kw.items() if k != 'merge_small'}), (c.id, switch)
        assert chain == CH.expect_chain(c, **kw), (c.id, switch, chain)
        _bitwise(other, mine, (c.id, switch))
    assert CH.expect_chain(c, merge_small=False)['jtv_finish'] == 'chain' and CH.expect_chain(c, sparse_ok=False)['assemble'] == 'k_assemble'


@pytest.mark.parametrize('nd', CH.H_DATASETS, ids=lambda nd: 'H-%d' % nd)
def test_pattern_only_image_on_either_side_of_the_gather_limit(ctx, nd, monkeypatch):
    """Part H: 128 active parameters per dataset, 76 of them global: 48 datasets (k_gather_sum with its longest lists: 48 terms) and 49
    (k_assemble_sparse); under GADFIT_HIP_SPARSE=0 k_assemble forms the dense image bit for bit (same terms, same order)"""
    c = CH.part_h_case(nd)
    p, stored = _check(ctx, c, with_omega=False)
    mine = _products(ctx, c, p, None)
    _bitwise(mine[:3], stored, c.id)
    other, lay, chain = _other_context(c, p, None, monkeypatch, 'GADFIT_HIP_SPARSE')
    assert lay == c.expect(sparse_ok=False) and lay['sparse'] == 0
    assert chain == CH.expect_chain(c, sparse_ok=False) and chain['assemble'] == 'k_assemble', chain
    _bitwise(other, mine, c.id)
    # exact zeros off the pattern: local parameters of two different datasets do not couple
    jac = np.asarray(p.jac)
    loc = [j for j in range(c.na) if not c.is_global[c.active[j]]]
    assert mine[0][jac[3][loc[0]], jac[5][loc[1]]] == 0.0 and mine[0][jac[3][loc[0]], jac[3][loc[1]]] != 0.0
