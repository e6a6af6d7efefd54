"""Batched independent fits on the device (gfh_fit_batch, gfh_batch_pass) against the CPU oracle, one OracleProblem per spectrum.

512 spectra of model_exp2 with 64 ... 512 points each; for spectrum b
    u = (splitmix64(4, SEED + 1000 (b + 1)) >> 11) / 2**53,  truth = EXP2_TRUTH (0.8 + 0.4 u),  n_b = 64 + (37 b) % 449,
    x, y, s = make_single(exp2_numpy, truth, n_b, 0.5, 100.0, seed=SEED + b),  weights 1 / s,  start = truth (1 +- off), + on even indices.
On these inputs the oracle agrees with itself count for count when its point sums are cut into three images (another order of
additions): they cover early exits at different iterations, rejections, retrials, the give-up exit and STEP 3, and none of the 512
fits sits on a decision that rounding alone takes.  (max_iter = 8 or a rel_error exit would let the fits run past convergence, where
accept / reject is decided by rounding: SURVEY section 4.)

The scenarios, the bounds and the record of observed maxima (GADFIT_BATCH_OBSERVE) are in tests/batch_common.py."""
import numpy as np
import pytest

from gadfit_amd import _lib
from gadfit_amd.ad import exp, trace_model
from oracle import binding as orc
from tests import models as M
from tests.batch_common import COUNTS, SCENARIOS, TOL_CHI2, TOL_LAMBDA, TOL_PARS, TOL_PASS, observe, same_bits, spectrum4, start_of

pytestmark = pytest.mark.gpu

B = 512
ACTIVE = [0, 1, 2, 3]


def spectrum(b):
    u = (M.splitmix64(4, M.SEED + 1000 * (b + 1)) >> np.uint64(11)).astype(np.float64) / 9007199254740992.0
    truth = M.EXP2_TRUTH * (0.8 + 0.4 * u)
    x, y, s = M.make_single(M.exp2_numpy, truth, 64 + (37 * b) % 449, 0.5, 100.0, seed=M.SEED + b)
    return truth, x, y, 1.0 / s, s


class Spectra:
    def __init__(self):
        self.tape = trace_model(M.model_exp2, 4)
        self.items = [spectrum(b) for b in range(B)]
        self.off = np.concatenate([[0], np.cumsum([it[1].size for it in self.items])]).astype(np.int64)
        self.x = np.concatenate([it[1] for it in self.items]); self.y = np.concatenate([it[2] for it in self.items])
        self.w = np.concatenate([it[3] for it in self.items])
        self.ctx = _lib.Context(0)
        self.ctx.set_model(self.tape)
        self.ctx.set_batch_data(self.off, self.x, self.y, self.w)
        self._fits = {}

    def starts(self, off):
        return np.array([start_of(it[0], off) for it in self.items])

    def oracle(self, b, start):
        _, x, y, w, _ = self.items[b]
        return orc.OracleProblem(self.tape, [x], [y], [w], [start], ACTIVE, [0] * 4)

    def fit(self, name):
        """the batch of 512 under a scenario (cached: the later tests compare other settings with it bit for bit)"""
        if name not in self._fits:
            off, kw = SCENARIOS[name]
            self._fits[name] = self.ctx.fit_batch(self.starts(off), ACTIVE, **kw)[:2]
        return self._fits[name]


@pytest.fixture(scope='module')
def S():
    s = Spectra()
    yield s
    s.ctx.close()


def test_one_pass_against_the_oracle(S):
    """gfh_batch_pass at the 5 %-off start values: every fit's J^T J, J^T r and chi2 against OracleProblem.sweep."""
    starts = S.starts(0.05)
    JTJ, JTr, chi2 = S.ctx.batch_pass(starts, ACTIVE)
    worst = dict(JTJ=0.0, JTres=0.0, chi2=0.0)
    for b in range(B):
        p = S.oracle(b, starts[b])
        JTJ0, JTr0, _, _ = p.sweep()
        chi0, _ = p.chi2()
        sc = np.sqrt(np.outer(np.diag(JTJ0), np.diag(JTJ0))) + 1e-300
        worst['JTJ'] = max(worst['JTJ'], np.max(np.abs(JTJ[b] - JTJ0) / sc))
        worst['JTres'] = max(worst['JTres'], np.max(np.abs(JTr[b] - JTr0) / (np.sqrt(np.diag(JTJ0) * chi0) + 1e-300)))
        worst['chi2'] = max(worst['chi2'], abs(chi2[b] - chi0) / chi0)
        assert np.array_equal(JTJ[b], JTJ[b].T)
    observe(pass_JTJ=worst['JTJ'], pass_JTres=worst['JTres'], pass_chi2=worst['chi2'])
    assert worst['JTJ'] < TOL_PASS and worst['JTres'] < TOL_PASS and worst['chi2'] <= TOL_PASS


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_fits_against_the_oracle(S, name):
    """fit_batch against OracleProblem.fit with the same arguments, for all 512 fits: the counts equal, lambda to 1e-14, parameters
    and chi2 to 3e-12 (north_star asks for 1e-10)."""
    off, kw = SCENARIOS[name]
    starts = S.starts(off)
    pars, res = S.fit(name)
    worst = dict(lam=0.0, pars=0.0, chi2=0.0)
    mismatches = []
    for b in range(B):
        p = S.oracle(b, starts[b])
        r0 = p.fit(**kw)
        got = tuple(int(res[f][b]) for f in COUNTS); want = tuple(int(getattr(r0, f)) for f in COUNTS)
        if got != want:
            mismatches.append((b, got, want))
            continue
        assert int(res['dof'][b]) == r0.dof
        worst['lam'] = max(worst['lam'], abs(res['lambda_'][b] - r0.lambda_) / r0.lambda_)
        worst['pars'] = max(worst['pars'], np.max(np.abs(pars[b] - p.pars.ravel()) / np.abs(p.pars.ravel())))
        worst['chi2'] = max(worst['chi2'], abs(res['chi2'][b] - r0.chi2) / r0.chi2)
    print('scenario (%s): iterations %s, exits %s, fits with a rejection %d' % (
        name, sorted(set(res['iterations'].tolist())), sorted(set(res['exit_reason'].tolist())),
        int(np.sum(res['n_chi2'] != res['iterations'] + 1))))
    observe(**{'fit_%s_lambda' % name: worst['lam'], 'fit_%s_pars' % name: worst['pars'], 'fit_%s_chi2' % name: worst['chi2']})
    assert not mismatches, '%d of %d fits differ in (iterations, n_sweeps, n_chi2, n_omega, exit_reason): %s' % (len(mismatches), B, mismatches[:8])
    assert worst['lam'] <= TOL_LAMBDA and worst['pars'] < TOL_PARS and worst['chi2'] < TOL_CHI2


def test_against_gfh_fit_one_spectrum_at_a_time(S):
    """64 of the spectra through set_data + fit on one context, scenario (b)'s arguments: the same counts, parameters within
    the bound of the oracle comparison (the two differ by the order of the point sums only)."""
    off, kw = SCENARIOS['b']
    starts = S.starts(off)
    pars, res = S.fit('b')
    c = _lib.Context(0)
    worst = 0.0
    try:
        c.set_model(S.tape)
        for b in range(0, B, 8):
            _, x, y, _, sigma = S.items[b]
            c.set_data(x, y, sigma, [0, x.size])
            c.init_weights(4)
            out, r = c.fit([starts[b]], ACTIVE, [0] * 4, **kw)
            assert tuple(int(res[f][b]) for f in COUNTS) == tuple(int(getattr(r, f)) for f in COUNTS), b
            worst = max(worst, np.max(np.abs(pars[b] - out.ravel()) / np.abs(out.ravel())))
    finally:
        c.close()
    observe(vs_gfh_fit_pars=worst)
    assert worst < TOL_PARS


def test_a_fit_does_not_depend_on_its_batch(S):
    """Fit k's parameters, chi2, lambda and counts are the same bits in the batch of 512, in a batch of that spectrum alone and in
    the batch reversed: a wave owns a fit, nothing about the batch reaches its sums."""
    for name in ('b', 'c'):
        off, kw = SCENARIOS[name]
        starts = S.starts(off)
        pars, res = S.fit(name)
        c = _lib.Context(0)
        try:
            c.set_model(S.tape)
            for k in (0, 1, 3, 130, 257, 511):
                _, x, y, w, _ = S.items[k]
                c.set_batch_data([0, x.size], x, y, w)
                p1, r1, _ = c.fit_batch(starts[k:k + 1], ACTIVE, **kw)
                same_bits(p1, r1, pars[k:k + 1], res[k:k + 1])
            rev = S.items[::-1]
            off_r = np.concatenate([[0], np.cumsum([it[1].size for it in rev])])
            c.set_batch_data(off_r, np.concatenate([it[1] for it in rev]), np.concatenate([it[2] for it in rev]),
                             np.concatenate([it[3] for it in rev]))
            pr, rr, _ = c.fit_batch(starts[::-1], ACTIVE, **kw)
            same_bits(pr[::-1], rr[::-1], pars, res)
        finally:
            c.close()


def test_a_failing_fit_stays_alone(S):
    """One spectrum's weights replaced by zeros: its J^T J is the zero matrix and the first pivot is 0.  It ends with exit reason 8 and
    its start parameters; every other fit's outputs are the bits of the undisturbed batch."""
    off, kw = SCENARIOS['d']
    starts = S.starts(off)
    pars, res = S.fit('d')
    k = 77
    w = S.w.copy()
    w[S.off[k]:S.off[k + 1]] = 0.0
    c = _lib.Context(0)
    try:
        c.set_model(S.tape)
        c.set_batch_data(S.off, S.x, S.y, w)
        p1, r1, _ = c.fit_batch(starts, ACTIVE, **kw)
        mem = c.device_memory()['workspace_pool']
        assert mem >= 3 * 8 * S.x.size + 8 * (B + 1) + B * (4 * 8 + 40)          # the batch's blocks are reported
    finally:
        c.close()
    assert r1['exit_reason'][k] == 8 and r1['iterations'][k] == 0 and np.array_equal(p1[k], starts[k])
    assert r1['n_sweeps'][k] == 1 and r1['n_chi2'][k] == 1 and r1['chi2'][k] == 0.0
    keep = np.arange(B) != k
    same_bits(p1[keep], r1[keep], pars[keep], res[keep])


def test_python_api_returns_what_fit_batch_returns(S):
    """gadf_fit_batch on 16 spectra (the fit arguments pass through real32, as gadf_fit's)."""
    from gadfit_amd import gadfit as gf

    class exp2(gf.fitfunc):
        def init(self):
            self.allocate(4)

        def eval(self, x):
            return self.pars[0] * exp(-(x / self.pars[1])) + self.pars[2] * exp(-(x / self.pars[3]))

    items = S.items[:16]
    starts = S.starts(0.05)[:16]
    kw = dict(lambda_=1.0, max_iter=50, chi2_rel=float(np.float32(1e-6)))
    c = _lib.Context(0)
    try:
        c.set_model(S.tape)
        c.set_batch_data(S.off[:17], S.x[:S.off[16]], S.y[:S.off[16]], S.w[:S.off[16]])
        p0, r0, _ = c.fit_batch(starts, ACTIVE, **kw)
    finally:
        c.close()
    gf.gadf_init(exp2())
    try:
        for j in range(4):
            gf.gadf_set(j + 1, float(M.EXP2_TRUTH[j]), True)
        p1, r1 = gf.gadf_fit_batch([it[1] for it in items], [it[2] for it in items], [it[3] for it in items], starts,
                                   lambda_=1.0, max_iter=50, chi2_rel=1e-6)
    finally:
        gf.gadf_close()
    same_bits(p1, r1, p0, r0)
    assert set(r0['exit_reason'].tolist()) == {2}


def test_group_handles_are_refused():
    c = _lib.Context(devices=[0])
    try:
        c.set_model(trace_model(M.model_exp2, 4))
        x = np.linspace(0.5, 9.5, 10)
        with pytest.raises(_lib.GadfitHipError, match='device-group handle'):
            c.set_batch_data([0, 10], x, x, x)
        c.n_fits = 1
        with pytest.raises(_lib.GadfitHipError, match='device-group handle'):
            c.fit_batch([M.EXP2_TRUTH], ACTIVE, max_iter=1)
    finally:
        c.close()


# ---- the other kernel shapes: 8 active parameters, a subset of the parameters active, the options beside the defaults -----------
# 48 spectra of model_exp4 (128 ... 512 points): truth = EXP4_TRUTH (0.9 + 0.2 u), u from splitmix64(8, SEED + 2000 (b + 1)),
# make_single(exp4_numpy, truth, 128 + (53 b) % 385, 0.05, 100.0, seed=SEED + 7 b + 3), weights 1 / s; the active parameters start at
# truth (1 +- off), the passive ones at each fit's own truth.  Chosen like the inputs above: under every argument set below the
# oracle agrees with itself count for count when its point sums are cut into three images (worst parameter difference 4.7e-14),
# which it does NOT once a three-parameter fit is allowed to run past convergence (max_iter = 6 there: 19 of 48 differ).
# Bounds: the counts equal, lambda to 1e-14, parameters and chi2 to north_star's 1e-10.
B4 = 48
EXP4_CASES = {
    'all8_converging': (list(range(8)), 0.05, dict(lambda_=1.0, max_iter=50, chi2_rel=1e-6)),                     # iterations 6 ... 9, exit 2
    'all8_rejecting': (list(range(8)), 0.3, dict(lambda_=1e-6, lam_incs=1, max_iter=3)),                          # 44 of 48 give up (exit 7) after 2 trials
    'subset_lam': ([1, 4, 6], 0.3, dict(lambda_=1e-2, lam_up=5.0, lam_down=7.0, lam_incs=3, damp_max=0, max_iter=3)),
    'subset_chi2_abs': ([1, 4, 6], 0.3, dict(lambda_=1.0, DTD_min=[1e-3] * 3, chi2_abs=1.5, rel_error=1e-2, max_iter=20)),      # exit 1
    'subset_rel_error': ([1, 4, 6], 0.3, dict(lambda_=10.0, DTD_min=[1e3] * 3, rel_error=5e-2, max_iter=20)),                   # exit 5
}


@pytest.fixture(scope='module')
def S4():
    tape = trace_model(M.model_exp4, 8)
    items = [spectrum4(b) for b in range(B4)]
    c = _lib.Context(0)
    c.set_model(tape)
    c.set_batch_data(np.concatenate([[0], np.cumsum([it[1].size for it in items])]), np.concatenate([it[1] for it in items]),
                     np.concatenate([it[2] for it in items]), np.concatenate([it[3] for it in items]))
    yield tape, items, c
    c.close()


@pytest.mark.parametrize('name', sorted(EXP4_CASES))
def test_eight_parameters_subsets_and_the_other_options_against_the_oracle(S4, name):
    tape, items, c = S4
    active, off, kw = EXP4_CASES[name]
    sign = np.where(np.arange(8) % 2 == 0, 1.0 + off, 1.0 - off)
    starts = np.array([it[0] for it in items])
    starts[:, active] *= sign[active]
    pars, res, _ = c.fit_batch(starts, active, **kw)
    worst = dict(lam=0.0, pars=0.0, chi2=0.0)
    for b in range(B4):
        truth, x, y, w = items[b]
        p = orc.OracleProblem(tape, [x], [y], [w], [starts[b]], active, [0] * 8)
        r0 = p.fit(**kw)
        assert tuple(int(res[f][b]) for f in COUNTS) == tuple(int(getattr(r0, f)) for f in COUNTS), b
        assert int(res['dof'][b]) == r0.dof
        passive = [k for k in range(8) if k not in active]
        assert np.array_equal(pars[b][passive], starts[b][passive])
        worst['lam'] = max(worst['lam'], abs(res['lambda_'][b] - r0.lambda_) / r0.lambda_)
        worst['pars'] = max(worst['pars'], np.max(np.abs(pars[b] - p.pars.ravel()) / np.abs(p.pars.ravel())))
        worst['chi2'] = max(worst['chi2'], abs(res['chi2'][b] - r0.chi2) / r0.chi2)
    print('exp4 %s: iterations %s, exits %s' % (name, sorted(set(res['iterations'].tolist())), sorted(set(res['exit_reason'].tolist()))))
    observe(**{'exp4_%s_lambda' % name: worst['lam'], 'exp4_%s_pars' % name: worst['pars'], 'exp4_%s_chi2' % name: worst['chi2']})
    assert worst['lam'] <= TOL_LAMBDA and worst['pars'] < 1e-10 and worst['chi2'] < 1e-10


def test_one_pass_with_eight_parameters_against_the_oracle(S4):
    tape, items, c = S4
    starts = np.array([it[0] for it in items]) * np.where(np.arange(8) % 2 == 0, 1.05, 0.95)
    JTJ, JTr, chi2 = c.batch_pass(starts, list(range(8)))
    worst = 0.0
    for b in range(B4):
        _, x, y, w = items[b]
        p = orc.OracleProblem(tape, [x], [y], [w], [starts[b]], list(range(8)), [0] * 8)
        JTJ0, JTr0, _, _ = p.sweep()
        chi0, _ = p.chi2()
        sc = np.sqrt(np.outer(np.diag(JTJ0), np.diag(JTJ0))) + 1e-300
        worst = max(worst, np.max(np.abs(JTJ[b] - JTJ0) / sc), np.max(np.abs(JTr[b] - JTr0) / (np.sqrt(np.diag(JTJ0) * chi0) + 1e-300)),
                    abs(chi2[b] - chi0) / chi0)
    observe(exp4_pass=worst)
    assert worst < TOL_PASS

