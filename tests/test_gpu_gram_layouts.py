"""The fused sweep + Gram kernel's matrix-core forms over the layouts of the points (tests/gram_layout_cases.py: the cases, what each
is there to reach, and the dispatch it expects).  Every case is one full pass against the CPU oracle at the tolerances of
tests/parity_common.py: _device_vs_oracle (Jacobian, residuals, J^T J exactly symmetric, J^T r, chi2 from the sweep and from chi2(),
STEP 3 and the convergence sums), and then, on the same data,
 - Context.debug_layout() equals the case's expectation: the case ran on the path it is here for,
 - chi2() at the sweep's parameters is bitwise the sweep's sum of squares (129 and 130 active parameters: in a test of their own),
 - fused forms: the kernel without the Jacobian store returns bitwise the storing kernel's J^T J, J^T r and chi2, and jacobian() then
   fails with 'Jacobian was not kept',
 - where the in-kernel tail served the case: a second context under GADFIT_HIP_TAIL=0 (the reduce / assemble launches) returns
   bitwise the same three.
tests/test_cpu_gram_layout_cases.py shows without a GPU that the oracle is a sound reference on these inputs."""
import numpy as np
import pytest

from gadfit_amd import _lib
from oracle import binding as orc
from tests import gram_layout_cases as GL
from tests.parity_common import TOL_FIT, TOL_PASS, _close, _device_vs_oracle

pytestmark = pytest.mark.gpu


class _KeepsModel:
    """a context whose set_model is skipped while the tape is the one it holds: the kernels loaded for it stay (set_data alone between
    the sizes of layout B1)"""

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
    yield c
    c.close()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _second_context(c, pars, jac, dim, monkeypatch, switch, moved=False):
    """(the sweep, the sweep at moved parameters if asked for, debug_layout()) of a fresh context created with the environment switch off"""
    xs, ys, ws, _ = c.data()
    monkeypatch.setenv(switch, '0')
    k = _lib.Context(0)
    try:
        k.set_model(c.tape())
        k.set_data(np.concatenate(xs), np.concatenate(ys), np.concatenate(ws), np.concatenate([[0], np.cumsum(c.sizes)]))
        return k.sweep(pars, c.active, jac, dim), k.sweep(pars * 1.02, c.active, jac, dim) if moved else None, k.debug_layout()
    finally:
        k.close()
        monkeypatch.delenv(switch)


def _check(ctx, c, monkeypatch):
    xs, ys, ws, start = c.data()
    if c.images != 1:          # (B4: the oracle as the reference on several images, tests/gram_layout_cases.py: ORACLE_SUM_TOL)
        one_image = orc.OracleProblem.sweep
        monkeypatch.setattr(orc.OracleProblem, 'sweep', lambda self, n_images=c.images, want_J=False: one_image(self, n_images, want_J))
    p = _device_vs_oracle(ctx, c.tape(), xs, ys, ws, start, c.active, c.is_global)
    monkeypatch.undo()
    want = c.expect()
    assert ctx.debug_layout() == want, c.id
    assert p.dim == c.dim
    stored = ctx.sweep(p.pars, c.active, p.jac, p.dim)
    chi_k = ctx.chi2(p.pars)
    print('%s: chi2 of the sweep %.17g, of chi2() %.17g' % (c.id, stored[2], chi_k))
    if c.fused:          # (beyond the fused kernel: test_chi2_is_bitwise_the_sweeps_beyond_the_fused_kernel)
        assert chi_k == stored[2], c.id
    if c.fused:
        ctx.set_keep_jacobian(0)
        try:
            assert _same(ctx.sweep(p.pars, c.active, p.jac, p.dim), stored), c.id
            assert ctx.debug_layout() == want, c.id
            with pytest.raises(_lib.GadfitHipError, match='Jacobian was not kept'):
                ctx.jacobian(c.na)
        finally:
            ctx.set_keep_jacobian(1)
    if want['tail_mode']:
        a, _, lay = _second_context(c, p.pars, p.jac, p.dim, monkeypatch, 'GADFIT_HIP_TAIL')
        assert lay == c.expect(tail_on=False) and lay['tail_mode'] == 0, c.id
        assert _same(a, stored), c.id
    return p, stored


@pytest.mark.parametrize('c', GL.part_a(), ids=repr)
def test_tile_edge_active_counts(ctx, c, monkeypatch):
    """Part A: the first active count of every form (9, 17, 49, 65, 81, 113, 129: one live row in the last tile, fifteen of padding) and
    one below every full tile (15, 31, 47, 63, 79, 127: one padding row), active lists with a gap in the middle"""
    assert c.active[:3] == [0, 1, 2] and c.active[3] > 3
    _check(ctx, c, monkeypatch)


UNFUSED = [c for c in GL.all_cases() if not c.fused]


@pytest.mark.parametrize('c', UNFUSED, ids=repr)
def test_chi2_is_bitwise_the_sweeps_beyond_the_fused_kernel(ctx, c):
    """The cases of parts A and B with more than 128 active parameters (129, 130): chi2() at the sweep's parameters against the sweep's
    sum of squares, bit for bit, as for every other case.  k_gram_block used to add r^2 four consecutive points per lane and its four
    waves in order, gfh_k_chi2 one point per lane and pass over eight waves: three of these four cases differed in the last bit
    (1.6e-16, 1.9e-16, 1.4e-16 relative).  It now adds them in gfh_k_chi2's map and order."""
    assert len(UNFUSED) == 4
    xs, ys, ws, start = c.data()
    ctx.set_model(c.tape())
    ctx.set_data(np.concatenate(xs), np.concatenate(ys), np.concatenate(ws), np.concatenate([[0], np.cumsum(c.sizes)]))
    jac, dim = ctx.jacobian_indices(c.active, c.is_global)
    _, _, chi2 = ctx.sweep(start, c.active, jac, dim)
    chi_k = ctx.chi2(start)
    print('%s: chi2 of the sweep %.17g, of chi2() %.17g, relative difference %.2e' % (c.id, chi2, chi_k, abs(chi_k - chi2) / chi2))
    assert ctx.debug_layout()['fused'] == 0
    assert chi_k == chi2, (c.id, chi2, chi_k)


@pytest.mark.parametrize('na', list(GL.FORMS), ids=lambda na: 'B1-%d' % na)
def test_one_dataset_sizes(na, monkeypatch):
    """B1: a lone partial wave, 63 / 64 / 65, one pass and one slot more, the last size with one workgroup and the first with several,
    34 gram blocks; one context and its kernels over all sizes"""
    k = _lib.Context(0)
    try:
        keeps = _KeepsModel(k)
        for n in (GL.B1_SIZES if na <= GL.FUSED_MAX else GL.B1_SIZES_UNFUSED):
            _check(keeps, GL.b1(na, n), monkeypatch)
    finally:
        k.close()


@pytest.mark.parametrize('na', list(GL.FORMS), ids=lambda na: 'B2-%d' % na)
def test_small_global_fit_in_the_tail(ctx, na, monkeypatch):
    """B2: datasets of 1, 700 and 65 points (1 and 700 from 96 active on), the decay times global: one workgroup per dataset, the
    in-kernel tail scatters through inv[] over several datasets"""
    c = GL.b2(na)
    assert c.small and c.expect()['tail_mode'] == (2 if c.fused else 0)
    _check(ctx, c, monkeypatch)


@pytest.mark.parametrize('na', [na for na in GL.FORMS if na <= GL.FUSED_MAX], ids=lambda na: 'B3-%d' % na)
def test_global_fit_beyond_the_tail(ctx, na, monkeypatch):
    """B3: eight ragged datasets, launch chain, pattern-only image, parameter block by pointer; under GADFIT_HIP_SPARSE=0 the dense
    image gives bitwise the same J^T J (both triangles, exact zeros off the pattern), J^T r and chi2"""
    c = GL.b3(na)
    want = c.expect()
    assert not c.small and want['tail_mode'] == 0 and want['sparse'] == 1 and want['kernarg'] == 0
    p, stored = _check(ctx, c, monkeypatch)
    moved = ctx.sweep(p.pars * 1.02, c.active, p.jac, p.dim)
    a, b, lay = _second_context(c, p.pars, p.jac, p.dim, monkeypatch, 'GADFIT_HIP_SPARSE', moved=True)
    assert lay == c.expect(sparse_ok=False) and lay['sparse'] == 0
    assert _same(a, stored) and _same(b, moved)
    assert np.array_equal(stored[0], stored[0].T)
    jac = np.asarray(p.jac)
    loc = [j for j in range(c.na) if not c.is_global[c.active[j]]]
    assert stored[0][jac[3][loc[0]], jac[5][loc[1]]] == 0.0 and stored[0][jac[3][loc[0]], jac[3][loc[1]]] != 0.0


@pytest.mark.parametrize('n', GL.B4_SIZES, ids=lambda n: 'B4-n%d' % n)
def test_padded_tail_at_256_and_257_workgroups(ctx, n, monkeypatch):
    """B4: 16 active parameters, where two workgroups fit a CU: 256 gram blocks take the tail under its LDS pad, 257 the chain"""
    c = GL.b4(n)
    want = c.expect()
    assert (want['n_gb'], want['tail_mode']) == ((256, 2) if n == 131072 else (257, 0))
    _check(ctx, c, monkeypatch)


@pytest.mark.parametrize('K', [24, 8], ids=lambda K: 'B5-gauss-%d' % (4 * K))
def test_gaussians_three_datasets_pass_and_fit(ctx, K, monkeypatch):
    """B5: gaussK(24) with 96 active per dataset (cooperative form, chain, pattern-only) and gaussK(8) with 32 (tail), centres global:
    the pass and a 4-iteration fit against the oracle's"""
    c = GL.b5(K)
    p, _ = _check(ctx, c, monkeypatch)
    out, r = ctx.fit(p.pars.copy(), c.active, c.is_global, **c.fit)
    r0 = p.fit(**c.fit)
    assert r.iterations == r0.iterations
    _close('pars_fit', out, p.pars, TOL_FIT)


@pytest.mark.parametrize('c,nranks', GL.part_c(), ids=lambda v: repr(v) if isinstance(v, GL.Case) else 'ranks%d' % v)
def test_pseudo_ranks_on_the_matrix_core_forms(ctx, c, nranks):
    """Part C: layout B3 sharded by the reference's rule; ranks alternate set_data and set_data_local; the per-rank J^T J, J^T r, chi2,
    chi2() and J^T omega sum to the single-context result (the tolerances of test_rank_sharding_on_one_gpu), residuals() has the rank's
    length, and every rank's debug_layout() is what the case module derives for it"""
    xs, ys, ws, pars = c.data()
    X, Y, W = np.concatenate(xs), np.concatenate(ys), np.concatenate(ws)
    pos = np.concatenate([[0], np.cumsum(c.sizes)])
    ctx.set_model(c.tape()); ctx.set_data(X, Y, W, pos)
    jac, dim = ctx.jacobian_indices(c.active, c.is_global)
    JTJ, JTr, chi2 = ctx.sweep(pars, c.active, jac, dim)
    d1 = _lib.potr(JTJ + np.diag(np.diag(JTJ)), JTr)
    jto = ctx.omega(pars, d1)
    accJ = np.zeros_like(JTJ); accr = np.zeros_like(JTr); accc = 0.0; acco = np.zeros_like(jto); accchi = 0.0; total = 0
    for r in range(nranks):
        k = _lib.Context(0)
        try:
            k.debug_set_rank(nranks, r)
            k.set_model(c.tape())
            b, n = _lib.partition(X.size, nranks, r)
            assert (b, n) == GL.partition(X.size, nranks, r)
            if r % 2 == 0:
                k.set_data(X, Y, W, pos)
            else:
                k.set_data_local(X.size, pos, b, X[b:b + n], Y[b:b + n], W[b:b + n])
            assert (k.local_begin(), k.local_count()) == (b, n)
            total += n
            a, br, cc = k.sweep(pars, c.active, jac, dim)
            assert k.debug_layout() == c.expect(nranks, r), (c.id, nranks, r)
            accJ += a; accr += br; accc += cc
            accchi += k.chi2(pars)
            acco += k.omega(pars, d1)
            assert k.residuals().shape == (n,)
        finally:
            k.close()
    assert total == X.size
    sc = np.sqrt(np.outer(np.diag(JTJ), np.diag(JTJ)))
    _close('JTJ_ranks', accJ, JTJ, 1e-12, sc)
    _close('JTres_ranks', accr, JTr, TOL_PASS, np.max(np.abs(JTr)))
    _close('chi2_ranks', [accc, accchi], [chi2, chi2], 1e-12)
    _close('JTomega_ranks', acco, jto, TOL_PASS, np.max(np.abs(jto)))
