"""What tests/test_gpu_gram_chain.py rests on, shown without a GPU: on every new input of tests/gram_chain_cases.py the oracle alone is a
sound reference (Jacobian rows and residuals against a numpy.longdouble closed form to a tenth of the Jacobian tolerance, its sums
within ORACLE_SUM_TOL of the same sums in longdouble); the launches each case expects, spelled out by hand, name every instantiation
the GPU file claims; the arithmetic of parts G and H is what the case module says; the library's own layout agrees with the
restated rules; every new translation unit compiles for gfx950 on a compile-only context; and the report the GPU tests read is
declared, exported, bound and empty before any launch."""
import re
import time

import numpy as np

from gadfit_amd import _lib
from oracle import binding as orc
from tests import gram_chain_cases as CH
from tests import gram_layout_cases as GL
from tests.test_cpu_gram_layout_cases import JTOL, _longdouble_sums, _sum_errors


def test_the_oracle_is_a_sound_reference_on_every_new_input():
    """per new input (the others are cases of tests/gram_layout_cases.py, shown there): finite, no J^T J diagonal entry below 1e-60 of the
    largest, rows and residuals against the closed form under _device_vs_oracle's per-entry metric, and the oracle's own sums on one
    image within ORACLE_SUM_TOL of the longdouble sums -- so no case needs the oracle on several images"""
    def inputs(c):
        return (c.model, c.K, tuple(c.active), tuple(c.sizes), tuple(c.is_global))
    known = set(inputs(c) for c in GL.all_cases()) | set(inputs(c) for c in CH.new_inputs())
    assert all(inputs(c) in known for c in CH.all_cases())
    worst = dict(J=0.0, res=0.0, sums=0.0)
    for c in CH.new_inputs():
        assert c.images == 1
        xs, ys, ws, start = c.data()
        p = orc.OracleProblem(c.tape(), xs, ys, ws, start, c.active, c.is_global)
        JTJ, JTr, res, JT = p.sweep(want_J=True)
        assert np.all(np.isfinite(JT)) and np.all(np.isfinite(res)) and np.all(np.isfinite(JTJ)) and np.all(np.isfinite(JTr)), c.id
        dg = np.diag(JTJ)
        ratio = float(dg.min() / dg.max())
        assert ratio >= 1e-60, (c.id, ratio)
        errJ = errR = 0.0
        for d in range(c.nd):
            sl = slice(p.dp[d], p.dp[d + 1])
            f, g = c.rows(start[d], xs[d])
            w = ws[d].astype(np.longdouble)
            want = g[:, c.active] * w[:, None]
            got = JT[sl][:, p.jac[d]]
            scale = np.maximum(np.abs(want), 1e-6 * np.max(np.abs(want), axis=0, keepdims=True) + 1e-300)
            errJ = max(errJ, float(np.max(np.abs(got - want) / scale)))
            r = (ys[d].astype(np.longdouble) - f) * w
            errR = max(errR, float(np.max(np.abs(res[sl] - r)) / max(1.0, float(np.max(np.abs(r))))))
        e = _sum_errors(p, 1, _longdouble_sums(c, p, xs, ys, ws, start))
        print('%-18s na %3d dim %4d: diagonal ratio %.1e, oracle against longdouble: Jacobian %.2e, residuals %.2e, J^T J %.2e, J^T r %.2e, chi2 %.2e'
              % ((c.id, c.na, c.dim, ratio, errJ, errR) + e))
        assert errJ <= 0.1 * JTOL and errR <= 0.1 * JTOL, (c.id, errJ, errR)
        assert max(e) <= GL.ORACLE_SUM_TOL, (c.id, e)
        worst = dict(J=max(worst['J'], errJ), res=max(worst['res'], errR), sums=max(worst['sums'], max(e)))
    print('worst over %d new inputs: Jacobian %.2e, residuals %.2e, sums %.2e' % (len(CH.new_inputs()), worst['J'], worst['res'], worst['sums']))


def test_gram_launches_by_hand():
    """gram.hip: launch_gram, spelled out at the counts of parts E and F"""
    assert [CH.gram_launches(na) for na in range(1, 9)] == [['small<%d>' % na] for na in range(1, 9)]
    assert [CH.gram_launches(na) for na in (9, 16, 17, 32, 33, 48, 49, 64)] == [['gram<%d>' % t] for t in (1, 1, 2, 2, 3, 3, 4, 4)]
    assert CH.gram_launches(65) == CH.gram_launches(80) == ['block<5,5,true>@(0,0)']
    assert CH.gram_launches(81) == CH.gram_launches(96) == ['block<6,6,true>@(0,0)']
    t7 = ['block<4,4,true>@(0,0)', 'block<4,3,false>@(0,4)', 'block<3,3,true>@(4,4)']
    assert CH.gram_launches(97) == CH.gram_launches(111) == t7
    assert CH.gram_launches(113) == CH.gram_launches(128) == ['block<4,4,true>@(0,0)', 'block<4,4,false>@(0,4)', 'block<4,4,true>@(4,4)']
    t9 = ['block<4,4,true>@(0,0)', 'block<4,4,false>@(0,4)', 'block<4,1,false>@(0,8)', 'block<4,4,true>@(4,4)', 'block<4,1,false>@(4,8)', 'block<1,1,true>@(8,8)']
    assert CH.gram_launches(129) == CH.gram_launches(130) == t9
    t10 = ['block<4,4,true>@(0,0)', 'block<4,4,false>@(0,4)', 'block<4,2,false>@(0,8)', 'block<4,4,true>@(4,4)', 'block<4,2,false>@(4,8)', 'block<2,2,true>@(8,8)']
    assert CH.gram_launches(145) == CH.gram_launches(160) == t10
    assert CH.gram_launches(161) == CH.gram_launches(176) == [g.replace(',2,', ',3,').replace('<2,', '<3,') for g in t10]
    assert CH.gram_launches(193) == ['block<4,4,true>@(0,0)', 'block<4,4,false>@(0,4)', 'block<4,4,false>@(0,8)', 'block<4,1,false>@(0,12)',
                                     'block<4,4,true>@(4,4)', 'block<4,4,false>@(4,8)', 'block<4,1,false>@(4,12)',
                                     'block<4,4,true>@(8,8)', 'block<4,1,false>@(8,12)', 'block<1,1,true>@(12,12)']
    # every tile pair of the upper triangle exactly once
    for na in (97, 129, 145, 161, 193, 300):
        T = GL.tiles(na); seen = []
        for g in CH.gram_launches(na):
            tr, tc, sym, r0, c0 = re.fullmatch(r'block<(\d),(\d),(true|false)>@\((\d+),(\d+)\)', g).groups()
            tr, tc, r0, c0 = int(tr), int(tc), int(r0), int(c0)
            assert (sym == 'true') == (r0 == c0) and r0 + tr <= T and c0 + tc <= T
            seen += [(r0 + i, c0 + j) for i in range(tr) for j in range(tc) if sym == 'false' or j >= i]
        assert sorted(seen) == [(i, j) for i in range(T) for j in range(i, T)], na


def test_part_e_by_hand():
    cases = CH.part_e()
    assert [(c.na, c.sizes[0]) for c in cases] == [(na, n) for na in (145, 160, 161, 176, 193) for n in (65, 1025, 2049)]
    assert [GL.tiles(na) for na in CH.E_COUNTS] == [10, 10, 11, 11, 13] and [16 * GL.tiles(na) - na for na in CH.E_COUNTS] == [15, 0, 15, 0, 15]
    lay = {65: (512, 1), 1025: (1536, 1), 2049: (2560, 5)}
    for c in cases:
        assert (c.model, c.K, c.n_pars) == ('exp', 120, 241) and c.active != list(range(c.na)) and c.active[:4] == [0, 1, 2, 3 + 241 - c.na]
        e = c.expect()
        assert (e['n_slots'], e['n_gb']) == lay[c.sizes[0]] and (e['fused'], e['waves'], e['tail_mode'], e['sparse'], e['kernarg']) == (0, 0, 0, 0, 241)
        ch = CH.expect_chain(c)
        assert ch == dict(gram=CH.gram_launches(c.na), assemble='k_gather_sum', jtv_finish='k_jtv_finish') and len(ch['gram']) == (10 if c.na == 193 else 6)
        assert CH.chi2_is_bitwise(c)
    assert (1536 // 512) % 2 == 1          # 1025 points: k_gram_block's loop over sum r^2 and k_gram_small's two-point trip end on a lone pass


def test_part_f_by_hand():
    cases = CH.part_f()
    assert len(cases) == 13 + 18 + 3 + 24 + 2 and len(set(c.id for c in cases)) == len(cases)
    for c in cases:
        e = c.expect(fused_on=False)
        assert (e['fused'], e['waves'], e['tail_mode']) == (0, 0, 0), c.id
        ch = CH.expect_chain(c, fused_on=False)
        assert ch['gram'] == CH.gram_launches(c.na) and ch['assemble'] == 'k_gather_sum' and ch['jtv_finish'] == 'k_jtv_finish', c.id
        assert c.expect()['fused'] == 1 or c.na == 129
    reach = {}
    for c in cases:
        for g in CH.gram_launches(c.na):
            reach.setdefault(g.split('@')[0], set()).add(16 * GL.tiles(c.na) - c.na)
    # every k_gram<T> with one live row (15 rows of padding; 7 at T = 1), with one padding row, and with full tiles
    assert all(reach['gram<%d>' % t] >= {15 if t > 1 else 7, 1, 0} for t in (1, 2, 3))          # (T = 3 with one live row: 33, added here)
    assert reach['gram<4>'] >= {15, 1}          # (64 active, the full fourth tile: test_unfused_gram_kernels_every_tile_count_vs_oracle)
    assert reach['block<5,5,true>'] >= {15, 1, 0} and reach['block<6,6,true>'] >= {15, 0}
    assert reach['block<3,3,true>'] >= {15, 1} and reach['block<4,3,false>'] >= {15, 1}          # T = 7
    assert set('small<%d>' % n for n in range(1, 9)) <= set(reach)
    assert [(c.na, c.K, c.n_pars) for c in CH.f_small()[::3]] == [(1, 1, 3), (2, 1, 3), (3, 2, 5), (4, 2, 5), (5, 3, 7), (6, 3, 7), (7, 4, 9), (8, 4, 9)]
    assert [c.expect(fused_on=False)['n_slots'] for c in CH.f_small()[:3]] == [512, 1536, 2560]
    assert [(c.na, c.K, c.active[:4]) for c in CH.f_t7()] == [(33, 18, [0, 1, 2, 7]), (97, 50, [0, 1, 2, 7]), (111, 57, [0, 1, 2, 7])]
    # where launch.cpp claims chi2() bitwise on the two-kernel path: up to 8 active, and the block kernels
    assert [na for na in (1, 8, 9, 16, 64, 65, 97, 129) if CH.chi2_is_bitwise(GL.Case('x', 'F', 'exp', 120, list(range(na)), [65]), fused_on=False)] == [1, 8, 65, 97, 129]
    # B2 under the switch: several datasets by pointer, the dense image of a small global fit through k_gather_sum
    for c in CH.f_b2():
        assert c.nd == (3 if c.na < 96 else 2) and c.expect(fused_on=False)['kernarg'] == 0 and c.small
        assert c.sizes == ([1, 700, 65] if c.na < 96 else [1, 700])


def test_part_g_by_hand():
    """512 datasets x 8 active = 4096 exactly, dim 519; 513: the chain, dim 520; the dense image is past 2^18 entries"""
    g512, g513 = CH.part_g()
    assert (g512.nd * g512.na, g512.dim, g513.nd * g513.na, g513.dim) == (4096, 519, 4104, 520) and CH.JTV_FINISH_MAX == 4096
    assert sum(g512.is_global[a] for a in g512.active) == 7 and g512.active == list(range(8)) and g512.n_pars == 9
    assert g512.sizes[:5] == [1, 2, 3, 65, 1] and g512.kernarg == 0 and not g512.small
    assert CH.image_entries(g512, sparse_ok=False) == 519 * 519 + 519 + 1 == 269881 > CH.GATHER_MAX == 262144
    assert CH.image_entries(g513, sparse_ok=False) == 270921 > CH.GATHER_MAX
    assert GL.pattern_nnz(g512.nd, g512.active, g512.is_global) == 7 * 8 // 2 + 512 * 8 == 4124 and CH.image_entries(g512) == 4124 + 520
    assert 512 // 8 == 64 and 513 // 8 == 64 and 513 % 8 == 1          # k_assemble: 64 steps of eight datasets per global entry; 513: and a lone one
    assert 512 // 16 == 32 and 513 % 16 == 1                            # k_gather_sum: 32 lists of sixteen; 513: and a lone term
    assert CH.expect_chain(g512) == dict(gram=[], assemble='k_gather_sum', jtv_finish='k_jtv_finish')
    assert CH.expect_chain(g513) == dict(gram=[], assemble='k_gather_sum', jtv_finish='chain')
    for c in (g512, g513):
        assert CH.expect_chain(c, merge_small=False)['jtv_finish'] == 'chain'
        assert CH.expect_chain(c, sparse_ok=False)['assemble'] == 'k_assemble' and c.expect(sparse_ok=False)['sparse'] == 0
        assert CH.expect_chain(c, tail_on=False) == CH.expect_chain(c) and c.expect()['tail_mode'] == 0 and c.expect()['sparse'] == 1
        assert c.expect()['n_gb'] == c.nd and c.expect()['waves'] == 8


def test_part_h_by_hand():
    """the pattern-only image of 48 and 49 datasets straddles 2^18 entries; the dense one is far beyond it"""
    h48, h49 = CH.part_h()
    assert (h48.na, h48.dim, h49.dim) == (128, 76 + 52 * 48, 76 + 52 * 49) and sum(h48.is_global) == 76
    per_dataset = 76 * 52 + 52 * 53 // 2
    assert GL.pattern_nnz(48, h48.active, h48.is_global) == 76 * 77 // 2 + 48 * per_dataset
    assert CH.image_entries(h48) == 261339 <= CH.GATHER_MAX < CH.image_entries(h49) == 266721
    assert min(h49.sizes) == 3 and max(h49.sizes) == 60 and h48.sizes == h49.sizes[:48]
    assert CH.expect_chain(h48) == dict(gram=[], assemble='k_gather_sum', jtv_finish='chain')
    assert CH.expect_chain(h49) == dict(gram=[], assemble='k_assemble_sparse', jtv_finish='chain')
    for c in (h48, h49):
        assert c.expect() == dict(n_slots=512 * c.nd, n_gb=c.nd, datasets_with_blocks=c.nd, fused=1, waves=4, tail_mode=0, sparse=1, kernarg=0)
        assert CH.expect_chain(c, sparse_ok=False)['assemble'] == 'k_assemble' and c.dim ** 2 > CH.GATHER_MAX
        assert c.nd * CH.partial_stride(8) < 1 << 31 and (c.nd + 1) * c.dim < 1 << 31          # the kernels' int indices


def test_every_instantiation_named_appears_in_some_expected_report():
    every = [(c, CH.expect_chain(c)) for c in CH.part_e() + CH.part_g() + CH.part_h()] + [(c, CH.expect_chain(c, fused_on=False)) for c in CH.part_f()]
    every += [(c, CH.expect_chain(c, sparse_ok=False)) for c in CH.part_g() + CH.part_h()] + [(c, CH.expect_chain(c, merge_small=False)) for c in CH.part_g()]
    gram = set(g.split('@')[0] for _, ch in every for g in ch['gram'])
    assert gram == set(['small<%d>' % n for n in range(1, 9)] + ['gram<%d>' % t for t in range(1, 5)] + ['block<5,5,true>', 'block<6,6,true>'] +
                       ['block<%d,%d,true>' % (t, t) for t in range(1, 5)] + ['block<4,%d,false>' % t for t in range(1, 5)])
    assert set(ch['assemble'] for _, ch in every) == {'k_gather_sum', 'k_assemble_sparse', 'k_assemble'}
    assert {c.id: (c.nd * c.na, CH.expect_chain(c)['jtv_finish']) for c in CH.part_g()} == {'G-512': (4096, 'k_jtv_finish'), 'G-513': (4104, 'chain')}
    assert _block_origins(every) >= {(0, 12), (4, 12), (8, 12), (12, 12), (0, 8), (4, 8), (8, 8)}


def _block_origins(every):
    return set(tuple(int(v) for v in re.search(r'@\((\d+),(\d+)\)', g).groups()) for _, ch in every for g in ch['gram'] if '@' in g)


def test_the_librarys_own_layout_agrees_with_the_case_module():
    """gfh_debug_packed_layout derives the gram workgroups, the pattern and the length of the packed image from data.cpp and packed_layout.cpp
    themselves: the restated rules agree on every case, with and without the pattern"""
    for c in CH.part_e() + CH.f_t7() + CH.f_small() + CH.part_g() + CH.part_h():
        jac, dim = GL.jacobian_indices(c.nd, c.active, c.is_global)
        pos = np.concatenate([[0], np.cumsum(c.sizes)])
        for sparse_ok in (True, False):
            got = _lib.debug_packed_layout(1, 0, int(pos[-1]), pos, jac, dim, sparse_ok=sparse_ok)
            e = c.expect(sparse_ok=sparse_ok)
            assert (got['pattern_only'], got['datasets_held'], got['gram_blocks']) == (e['sparse'], c.nd, e['n_gb']), c.id
            assert got['packed_n'] == CH.image_entries(c, sparse_ok), (c.id, got)


N_UNITS = 17


def test_every_new_unit_compiles_for_gfx950():
    """5 units of Part E, 3 for 33 active and T = 7 and 8 for 1 ... 8 active of Part F, 1 for Part G (by pointer); the rest of parts F and H are units
    of tests/gram_layout_cases.py.  Each compiled alone on a compile-only context created under GADFIT_HIP_FUSED=0 -- the unit is the
    same with the switch on: it is no part of the generated source -- the seconds printed"""
    units = CH.units()
    print('%d translation units' % len(units))
    assert len(units) == N_UNITS
    assert sorted(len(a) for _, a, _, _ in units) == sorted([145, 160, 161, 176, 193, 33, 97, 111] + list(range(1, 9)) + [8])
    import os
    before = os.environ.get('GADFIT_HIP_FUSED')
    os.environ['GADFIT_HIP_FUSED'] = '0'
    try:
        c = _lib.Context(-1)
    finally:
        if before is None:
            del os.environ['GADFIT_HIP_FUSED']
        else:
            os.environ['GADFIT_HIP_FUSED'] = before
    d = _lib.Context(-1)
    try:
        t0 = time.perf_counter()
        for tape, active, nd, store in units:
            t1 = time.perf_counter()
            c.set_model(tape)
            c.model_prepare_form(active, nd, store)
            src = c.model_source(active)
            d.set_model(tape)
            assert src == d.model_source(active)
            print('  %3d active of %3d parameters, %d dataset(s): %.1f s' % (len(active), tape.n_pars, nd, time.perf_counter() - t1))
        print('compiled (or found in the cache) in %.1f s' % (time.perf_counter() - t0))
    finally:
        c.close(); d.close()


def test_the_report_is_declared_exported_and_empty_before_any_launch():
    assert 'gfh_debug_chain' in _lib.SYMBOLS
    c = _lib.Context(-1)
    try:
        assert c.debug_chain() == dict(gram=[], assemble=None, jtv_finish=None)
    finally:
        c.close()
