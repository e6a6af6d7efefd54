"""What tests/test_gpu_gram_layouts.py rests on, shown without a GPU: on every case of tests/gram_layout_cases.py the oracle alone is a
sound reference (finite rows, no column whose scale underflows, no abscissa on a start centre, Jacobian rows equal to a
numpy.longdouble closed form to a tenth of the Jacobian tolerance); the dispatch each case expects, spelled out by hand, covers every
form x path the GPU file claims; and every translation unit that file asks for compiles for gfx950 on a compile-only context."""
import time

import numpy as np

from gadfit_amd import _lib
from oracle import binding as orc
from tests import gram_layout_cases as GL
from tests import models as M

JTOL = 7e-13          # tests/parity_common.py: _device_vs_oracle's jtol


def test_the_oracle_is_a_sound_reference_on_every_case():
    """per case: rows finite; every J^T J diagonal entry >= 1e-60 of the largest (the scale sqrt(JTJ_ii JTJ_jj) + 1e-300 of the J^T J metric
    stays in the normal range); gaussK: no abscissa within 1e-6 of a start centre (the forward-mode a**n NaN of the reference); the
    oracle's Jacobian rows and residuals against the closed form in longdouble, under _device_vs_oracle's own per-entry metric"""
    worst = dict(J=0.0, res=0.0, ratio=1.0)
    for c in GL.all_cases():
        xs, ys, ws, start = c.data()
        p = orc.OracleProblem(c.tape(), xs, ys, ws, start, c.active, c.is_global)
        JTJ, JTr, res, JT = p.sweep(want_J=True)
        assert np.all(np.isfinite(JT)) and np.all(np.isfinite(res)) and np.all(np.isfinite(JTJ)) and np.all(np.isfinite(JTr)), c.id
        dg = np.diag(JTJ)
        ratio = float(dg.min() / dg.max())
        assert ratio >= 1e-60, (c.id, ratio)
        errJ = errR = 0.0
        for d in range(c.nd):
            if c.model == 'gauss':
                gap = float(np.min(np.abs(xs[d][:, None] - start[d][1::4][None, :])))
                assert gap > 1e-6, (c.id, d, gap)
            sl = slice(p.dp[d], p.dp[d + 1])
            f, g = c.rows(start[d], xs[d])
            w = ws[d].astype(np.longdouble)
            want = g[:, c.active] * w[:, None]
            got = JT[sl][:, p.jac[d]]
            scale = np.maximum(np.abs(want), 1e-6 * np.max(np.abs(want), axis=0, keepdims=True) + 1e-300)
            errJ = max(errJ, float(np.max(np.abs(got - want) / scale)))
            r = (ys[d].astype(np.longdouble) - f) * w
            errR = max(errR, float(np.max(np.abs(res[sl] - r)) / max(1.0, float(np.max(np.abs(r))))))
            # columns of other datasets' local parameters are exact zeros in this dataset's rows
            other = np.setdiff1d(np.arange(p.dim), p.jac[d])
            assert not np.any(JT[sl][:, other]), c.id
        print('%-15s na %3d dim %3d: smallest / largest J^T J diagonal %.1e, oracle against longdouble: Jacobian %.2e, residuals %.2e'
              % (c.id, c.na, c.dim, ratio, errJ, errR))
        assert errJ <= 0.1 * JTOL and errR <= 0.1 * JTOL, (c.id, errJ, errR)
        worst = dict(J=max(worst['J'], errJ), res=max(worst['res'], errR), ratio=min(worst['ratio'], ratio))
    print('worst over %d cases: Jacobian %.2e, residuals %.2e, diagonal ratio %.1e' % (len(GL.all_cases()), worst['J'], worst['res'], worst['ratio']))


def _longdouble_sums(c, p, xs, ys, ws, start):
    JTJ = np.zeros((p.dim, p.dim), dtype=np.longdouble); JTr = np.zeros(p.dim, dtype=np.longdouble); chi = np.longdouble(0)
    for d in range(c.nd):
        f, g = c.rows(start[d], xs[d])
        w = ws[d].astype(np.longdouble)
        J = g[:, c.active] * w[:, None]
        r = (ys[d].astype(np.longdouble) - f) * w
        ix = p.jac[d]
        JTJ[np.ix_(ix, ix)] += J.T @ J; JTr[ix] += J.T @ r; chi += r @ r
    return JTJ, JTr, chi


def _sum_errors(p, images, want):
    JTJ, JTr, _, _ = p.sweep(n_images=images)
    chi = p.chi2(n_images=images)[0]
    dg = np.diag(JTJ)
    return (float(np.max(np.abs(JTJ - want[0]) / (np.sqrt(np.outer(dg, dg)) + 1e-300))), float(np.max(np.abs(JTr - want[1]) / (np.sqrt(dg * chi) + 1e-300))),
            float(abs(chi - want[2]) / chi))


def test_the_oracles_own_sums_leave_the_device_half_the_tolerance():
    """J^T J, J^T r and chi2 of the oracle, added the way each case has it added (one image; B4: 64), against the same sums of the
    closed-form rows in longdouble, under _device_vs_oracle's metrics: at most ORACLE_SUM_TOL = half of the 1e-13 the device is held to.
    B4 on one image misses that (2.4e-13, 2.2e-13), which is why it is not compared that way."""
    assert GL.ORACLE_SUM_TOL == 0.5 * 1e-13
    worst = 0.0
    for c in GL.all_cases():
        xs, ys, ws, start = c.data()
        p = orc.OracleProblem(c.tape(), xs, ys, ws, start, c.active, c.is_global)
        want = _longdouble_sums(c, p, xs, ys, ws, start)
        e = _sum_errors(p, c.images, want)
        print('%-15s oracle on %2d image(s) against longdouble sums: J^T J %.2e, J^T r %.2e, chi2 %.2e' % ((c.id, c.images) + e))
        assert max(e) <= GL.ORACLE_SUM_TOL, (c.id, e)
        worst = max(worst, max(e))
        if c.images != 1:
            one = _sum_errors(p, 1, want)
            print('%-15s ... on one image: J^T J %.2e, J^T r %.2e, chi2 %.2e' % ((c.id,) + one))
            assert one[0] > 1e-13 and c.part == 'B4'
    print('worst %.2e' % worst)
    assert [c.id for c in GL.all_cases() if c.images != 1] == ['B4-16-n131072', 'B4-16-n131073']


def test_models_are_what_the_case_module_says():
    K = 4
    t = GL.expK_truth(K)
    assert t.size == 9 and t[8] == 0.5 and list(t[0::2][:4]) == [1.0, 1.0 + 2.0 * 3 / 4, 1.0 + 2.0 * 2 / 4, 1.0 + 2.0 * 1 / 4]
    assert np.allclose(t[1::2], 40.0 ** ((np.arange(4) + 0.5) / 4), rtol=1e-15)
    x = np.array([0.5, 7.0, 59.0])
    f, g = GL.expK_rows(K, t, x)
    assert np.allclose(np.asarray(f, dtype=float), GL.expK_numpy(K)(t, x), rtol=1e-14)
    v = orc.eval_reverse(GL.tape_of('exp', K), 7.0, t, [1] * 9)
    assert abs(v[0] - float(f[1])) <= 1e-14 * abs(v[0]) and np.allclose(v[1], np.asarray(g[1], dtype=float), rtol=1e-13)
    tg = M.gaussK_truth(3)
    fg, gg = GL.gaussK_rows(3, tg, np.array([49.0]))
    v = orc.eval_reverse(GL.tape_of('gauss', 3), 49.0, tg, [1] * 12)
    assert abs(v[0] - float(fg[0])) <= 1e-14 * abs(v[0]) and np.allclose(v[1], np.asarray(gg[0], dtype=float), rtol=1e-12, atol=1e-300)


def test_forms_by_hand():
    """codegen.h: the waves per workgroup and the form at every active count of Part A and Part B, and where the forms switch"""
    waves = {9: 8, 15: 8, 16: 8, 17: 8, 31: 8, 32: 8, 47: 4, 48: 4, 49: 4, 63: 4, 65: 4, 79: 4, 80: 4, 81: 4, 96: 4, 113: 4, 127: 4, 128: 4}
    for na, fw in waves.items():
        assert GL.fused_waves_for(na) == fw, na
    assert [GL.form_of(na) for na in (8, 9, 64, 65, 80, 81, 128, 129)] == ['valu', 'full', 'full', 'half', 'half', 'coop', 'coop', 'unfused']
    assert GL.fused_waves_for(32) == 8 and GL.fused_waves_for(33) == 4          # 8 full stages of 3 tiles do not fit 160 KB
    assert [GL.tiles(na) for na in GL.A_FIRST] == [1, 2, 4, 5, 6, 8, 9] and [GL.tiles(na) for na in GL.A_BELOW] == [1, 2, 3, 4, 5, 8]
    assert [16 * GL.tiles(na) - na for na in GL.A_FIRST] == [7, 15, 15, 15, 15, 15, 15] and all(16 * GL.tiles(na) - na == 1 for na in GL.A_BELOW)
    # LDS of a workgroup: 16 active parameters leave room for two workgroups on a CU, 17 and more do not
    assert GL.fused_lds_bytes(16) == 8 * 17 * 66 * 8 + 273 * 8 + 64 == 74056 and not GL.tail_one_workgroup_per_cu(16)
    assert GL.fused_lds_bytes(17) == 8 * 33 * 66 * 8 + 801 * 8 + 64 == 145864 and GL.tail_one_workgroup_per_cu(17)
    assert all(GL.tail_one_workgroup_per_cu(na) for na in (32, 48, 80, 96, 128)) and not GL.tail_one_workgroup_per_cu(9)
    assert [GL.form_of(na) for na in GL.FORMS] == ['full', 'full', 'full', 'half', 'coop', 'coop', 'unfused']
    assert all(GL.fused_lds_bytes(na) <= GL.LDS_BYTES for na in range(1, 129))


def test_part_a_by_hand():
    cases = GL.part_a()
    assert [c.na for c in cases] == [9, 17, 49, 65, 81, 113, 129, 15, 31, 47, 63, 79, 127]
    assert [(c.model, c.K) for c in cases[:7]] == [('gauss', k) for k in (4, 6, 14, 18, 22, 30, 34)]
    assert all(c.model == 'exp' and c.n_pars == c.na + 4 for c in cases[7:])
    for c in cases:
        assert c.sizes == [1501] and c.active != list(range(c.na)) and c.active[:4] == [0, 1, 2, 3 + c.n_pars - c.na]
        e = c.expect()
        assert (e['n_slots'], e['n_gb'], e['datasets_with_blocks'], e['sparse'], e['kernarg']) == (1536, 1, 1, 0, c.n_pars)
        assert (e['fused'], e['tail_mode']) == ((1, 2) if c.na <= 128 else (0, 0))          # one workgroup: the tail's shortcut
    assert [c.expect()['waves'] for c in cases] == [8, 8, 4, 4, 4, 4, 0, 8, 8, 4, 4, 4, 4]


def test_part_b_by_hand():
    # B1: one dataset, the parameter block by value
    lay = {1: (512, 1), 63: (512, 1), 64: (512, 1), 65: (512, 1), 512: (512, 1), 513: (1024, 1), 2048: (2048, 1), 2049: (2560, 5), 16897: (17408, 34)}
    for na, (K, n_glob, n_loc) in GL.FORMS.items():
        for n in (GL.B1_SIZES if na <= 128 else GL.B1_SIZES_UNFUSED):
            e = GL.b1(na, n).expect()
            assert (e['n_slots'], e['n_gb']) == lay[n] and e['kernarg'] == 2 * K + 1 <= 480 and e['sparse'] == 0
            assert (e['fused'], e['tail_mode']) == ((1, 2) if na <= 128 else (0, 0)), (na, n)
        assert len(GL.b1(na, 1).active) == na and GL.b1(na, 1).active != list(range(na))
    assert [GL.b1(na, 65).expect()['waves'] for na in GL.FORMS] == [8, 8, 4, 4, 4, 4, 0]
    # 34 gram blocks: slices 0 and 1 of the tail's first level have two members (blocks 0, 32 and 1, 33), the other thirty one
    assert [(34 - sl + 31) >> 5 for sl in (0, 1, 2, 31)] == [2, 2, 1, 1]
    # B2: small, the tail over several datasets with one workgroup each; by pointer
    dims = {16: 38, 32: 64, 48: 96, 80: 146, 96: 144, 128: 180, 130: 180}
    for na in GL.FORMS:
        c = GL.b2(na); e = c.expect()
        assert c.dim == dims[na] and c.nd == (3 if na < 96 else 2) and c.dim ** 2 * c.nd <= 65536 and c.small
        assert (e['n_slots'], e['n_gb'], e['datasets_with_blocks']) == ((2048, 3, 3) if na < 96 else (1536, 2, 2))
        assert (e['fused'], e['tail_mode'], e['sparse'], e['kernarg']) == ((1, 2, 0, 0) if na <= 128 else (0, 0, 0, 0))
        assert c.nd * c.n_pars > 480
        # (from 96 on the three datasets of the other forms would not be small: 192, 232 and 230 columns)
        three = GL.Case('three', 'B2', 'exp', c.K, c.active, GL.B2_SIZES, c.is_global)
        assert three.small == (na < 96) and three.dim == {16: 38, 32: 64, 48: 96, 80: 146, 96: 192, 128: 232, 130: 230}[na]
    # B3: beyond the tail: launch chain, pattern-only image, by pointer; 14 gram blocks over 8 datasets
    dims = {16: 93, 32: 144, 48: 216, 80: 311, 96: 432, 128: 492}
    for na, dim in dims.items():
        c = GL.b3(na); e = c.expect()
        assert c.dim == dim and dim * dim * 8 > 65536 and not c.small and 8 * c.n_pars > 480
        assert e == dict(n_slots=7168, n_gb=14, datasets_with_blocks=8, fused=1, waves=GL.fused_waves_for(na), tail_mode=0, sparse=1, kernarg=0)
        assert c.expect(sparse_ok=False)['sparse'] == 0
    assert GL.block_layout(GL.B3_SIZES)[1] == [1, 2, 1, 5, 1, 2, 1, 1]
    # B4: 16 active parameters: the padded tail up to 256 workgroups, the chain from 257 on
    e0, e1 = GL.b4(131072).expect(), GL.b4(131073).expect()
    assert (e0['n_slots'], e0['n_gb'], e0['tail_mode']) == (131072, 256, 2) and (e1['n_slots'], e1['n_gb'], e1['tail_mode']) == (131584, 257, 0)
    assert e0['waves'] == e1['waves'] == 8 and e0['fused'] == e1['fused'] == 1
    # ... while 32 active parameters (one workgroup per CU) would keep the tail at 257
    assert GL.b1(32, 131073).expect()['tail_mode'] == 2
    # B5
    c96, c32 = GL.b5(24), GL.b5(8)
    assert (c96.na, c96.dim, c96.small) == (96, 240, False) and (c32.na, c32.dim, c32.small) == (32, 80, True)
    assert c96.expect() == dict(n_slots=4096, n_gb=8, datasets_with_blocks=3, fused=1, waves=4, tail_mode=0, sparse=1, kernarg=288)
    assert c32.expect() == dict(n_slots=4096, n_gb=8, datasets_with_blocks=3, fused=1, waves=8, tail_mode=2, sparse=0, kernarg=96)
    assert all(n >= 900 for c in GL.all_cases() if c.model == 'gauss' for n in c.sizes)
    # what the cases reach, taken together
    every = GL.all_cases()
    reach = set((GL.form_of(c.na), 'tail1' if e['tail_mode'] and e['n_gb'] == 1 else 'tail' if e['tail_mode'] else 'chain', 'pattern' if e['sparse'] else 'dense',
                 'value' if e['kernarg'] else 'pointer') for c in every for e in [c.expect()])
    for form in ('full', 'half', 'coop'):
        assert {(form, 'tail1', 'dense', 'value'), (form, 'tail', 'dense', 'value'), (form, 'tail', 'dense', 'pointer'), (form, 'chain', 'pattern', 'pointer')} <= reach, form
    assert ('unfused', 'chain', 'dense', 'value') in reach and ('unfused', 'chain', 'dense', 'pointer') in reach
    assert ('full', 'chain', 'dense', 'value') in reach          # B4 at 257 blocks
    assert len(every) == 13 + 6 * 9 + 2 + 7 + 6 + 2 + 2


def test_part_c_by_hand():
    """3 and 8 pseudo-ranks over the 4043 points of layout B3: who holds what"""
    assert sum(GL.B3_SIZES) == 4043
    assert [GL.partition(4043, 3, r) for r in range(3)] == [(0, 1348), (1348, 1348), (2696, 1347)]
    assert [GL.partition(4043, 8, r)[1] for r in range(8)] == [506, 506, 506, 505, 505, 505, 505, 505]
    assert [GL.partition(4043, 8, r) for r in range(8)] == [_lib.partition(4043, 8, r) for r in range(8)]
    held3 = [GL.local_sizes(GL.B3_SIZES, 3, r) for r in range(3)]
    assert held3 == [[1, 1024, 323, 0, 0, 0, 0, 0], [0, 0, 10, 1338, 0, 0, 0, 0], [0, 0, 0, 711, 57, 513, 2, 64]]
    held8 = [GL.local_sizes(GL.B3_SIZES, 8, r) for r in range(8)]
    assert held8[0] == [1, 505, 0, 0, 0, 0, 0, 0] and held8[7] == [0, 0, 0, 0, 0, 439, 2, 64]
    assert all(sum(n == 0 for n in h) >= 5 for h in held8)          # every one of the 8 ranks holds nothing of at least five datasets
    assert [sum(h) for h in held8] == [506, 506, 506, 505, 505, 505, 505, 505]
    cases = GL.part_c()
    assert [(c.na, n) for c, n in cases] == [(32, 3), (32, 8), (96, 3), (96, 8)]
    for c, nranks in cases:
        for r in range(nranks):
            e = c.expect(nranks, r)
            held = GL.local_sizes(c.sizes, nranks, r)
            assert e['datasets_with_blocks'] == sum(n > 0 for n in held) < 8 and e['n_slots'] == sum((n + 511) // 512 * 512 for n in held)
            # the layout of the image is every rank's own business nowhere: pattern-only and by pointer on all of them, never the tail
            assert (e['fused'], e['tail_mode'], e['sparse'], e['kernarg'], e['waves']) == (1, 0, 1, 0, 8 if c.na == 32 else 4)
    assert [GL.b3(32).expect(3, r)['n_gb'] for r in range(3)] == [3, 2, 7]
    assert [GL.b3(32).expect(8, r)['n_gb'] for r in range(8)] == [2, 1, 3, 1, 1, 1, 3, 3]


N_UNITS = 55


def test_every_unit_compiles_for_gfx950():
    """13 + 12 units of Part A (129 active: no fused kernel, so no form without the store), 4 per fused form of Part B and 2 for 130
    active, 2 x 2 for B5: each compiled alone on a compile-only context, the seconds printed"""
    units = GL.units()
    print('%d translation units' % len(units))
    assert len(units) == N_UNITS
    c = _lib.Context(-1)
    try:
        t0 = time.perf_counter()
        for tape, active, nd, store in units:
            t1 = time.perf_counter()
            c.set_model(tape)
            c.model_prepare_form(active, nd, store)
            by_value = nd * tape.n_pars if nd * tape.n_pars <= 480 else 0
            print('  %3d active of %3d parameters, %s, %s: %.1f s' % (len(active), tape.n_pars, 'by value (%d)' % by_value if by_value else 'by pointer',
                                                                      'stores J' if store else 'no store', time.perf_counter() - t1))
        print('compiled (or found in the cache) in %.1f s' % (time.perf_counter() - t0))
        src = c.model_source(units[-1][1])
        assert '#define GFH_NA 32\n' in src
    finally:
        c.close()


def test_the_librarys_own_layout_agrees_with_the_case_module():
    """gfh_debug_packed_layout derives, without a GPU, the gram workgroups, the datasets held and whether the image is pattern-only from
    data.cpp and packed_layout.cpp themselves: the case module's restatement of those rules agrees on every case and every pseudo-rank"""
    todo = [(c, 1, 0) for c in GL.all_cases()] + [(c, n, r) for c, n in GL.part_c() for r in range(n)]
    for c, nranks, r in todo:
        jac, dim = GL.jacobian_indices(c.nd, c.active, c.is_global)
        pos = np.concatenate([[0], np.cumsum(c.sizes)])
        for sparse_ok in (True, False):
            got = _lib.debug_packed_layout(nranks, r, int(pos[-1]), pos, jac, dim, sparse_ok=sparse_ok)
            e = c.expect(nranks, r, sparse_ok=sparse_ok)
            assert (got['pattern_only'], got['datasets_held'], got['gram_blocks']) == (e['sparse'], sum(n > 0 for n in GL.local_sizes(c.sizes, nranks, r)), e['n_gb']), (c.id, nranks, r)
