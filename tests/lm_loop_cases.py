"""The inputs of tests/test_gpu_lm_loop.py: whole plain fits (gfh_fit: lm.cpp, lm_options.h, normal_eq.cpp) held to the oracle on every
exit test and lambda policy, and the rule that selects which fits a device may be held against count for count
(tests/test_cpu_lm_loop_cases.py runs the rule and the coverage conditions without a GPU).  Everything here is deterministic and needs
no GPU; the device's results never enter the rule.

THE PROBLEMS, the smallest that reach each form of the sweep:
  exp2      model_exp2, 257 points, one dataset, 4 active                        the VALU fused form
  gauss8    model_gauss8, 321 points, one dataset, 32 active                     the matrix-core form
  global7   model_global7, datasets of 65, 40, 129 points, all 7 active,         dim = 15: the arrow-structured solve, the packed image
            is_global = [0, 0, 0, 0, 1, 1, 1]
  global7s  as global7 with active = [6, 0, 4, 3] in that order                  passive parameters, an active list that does not ascend
Starts are truth x (1 +- pert), alternating in sign with the parameter's index (the passive parameters of global7s too: they stay
there); the global parameters start at one value in every dataset.  Thresholds pass through np.float32, as
tests/test_gpu_parity.py::test_fit_vs_oracle_lm_options passes them.

THE RULE.  Past convergence, LM's decisions are made by rounding: model_exp2 under lam_incs = 1 converges and then leaves with exit 7
after a comparison of two chi2 that differ by 4e-16.  Such a fit is not compared count for count.  A case is KEPT only if
 1. the oracle at n_images = 1 and at n_images = 3 (another order of the point sums) gives equal
    (iterations, n_sweeps, n_chi2, n_omega, exit_reason),
 2. and fitted parameters within SELF_TOL = 1e-13 relative = parity_common.TOL_FIT / 10: TOL_FIT then keeps the project's usual
    10 x margin over what reordering the sums does to the reference itself;
 3. min_margin > TOL_PASS (2e-13): every 'new_chi2 < old_chi2' of STEP 4, as in tests/batch_cases.py;
 4. min_exit_margin > EXIT_MARGIN = 1e-3: the closest relative distance |value - threshold| / |threshold| over every OTHER
    data-dependent comparison the loop evaluated (orc_fit_result.min_exit_margin: the STEP 5 tests, fired or not, coordinate by
    coordinate; acc_ratio against accth; under uphill (1 - beta)^uphill new_chi2 against old_chi2; under umnigh |beta| itself).
    1e-3 is a condition, not a measurement: the compared quantities come out of a solve and agree between two summation orders to
    about 1e-9 on these problems.
At most one row in five may fail the rule (CAP), and no coverage condition may rest on a dropped row: rows that fail are replaced,
the rule is not loosened."""
import functools

import numpy as np

from gadfit_amd.ad import trace_model
from oracle import binding as orc
from tests import models as M
from tests.batch_common import COUNTS
from tests.parity_common import TOL_FIT, TOL_PASS

SELF_TOL = TOL_FIT / 10
MARGIN = TOL_PASS
EXIT_MARGIN = 1e-3
CAP = 0.2
F32_KEYS = ('lambda_', 'lam_up', 'lam_down', 'accth', 'grad_chi2', 'cos_phi', 'rel_error', 'rel_error_global', 'chi2_rel', 'chi2_abs')
GLOBAL7_LENGTHS = (65, 40, 129)
GLOBAL7_IS_GLOBAL = [0, 0, 0, 0, 1, 1, 1]
IMAGES = (1, 2, 3, 5, 8, 64)          # the oracle's own spread of a case: its point sums cut into this many images


class Problem:
    """a model, its datasets, the truth [n_datasets][n_pars], the active list and the global flags"""

    def __init__(self, name, model, n_pars, xs, ys, ws, truth, active, is_global):
        self.name, self.tape, self.xs, self.ys, self.ws = name, trace_model(model, n_pars), xs, ys, ws
        self.truth = np.atleast_2d(np.asarray(truth, dtype=np.float64))
        self.active, self.is_global, self.n_pars = list(active), list(is_global), n_pars
        self.pos = np.concatenate([[0], np.cumsum([x.size for x in xs])]).astype(np.int64)
        self.x, self.y, self.w = np.concatenate(xs), np.concatenate(ys), np.concatenate(ws)

    def start(self, pert):
        return self.truth * np.where(np.arange(self.n_pars) % 2 == 0, 1.0 + pert, 1.0 - pert)

    def oracle(self, start):
        return orc.OracleProblem(self.tape, self.xs, self.ys, self.ws, start, self.active, self.is_global)

    @property
    def is_global_fit(self):
        return len(self.xs) > 1


@functools.lru_cache(maxsize=None)
def problem(name):
    if name == 'exp2':
        x, y, s = M.make_single(M.exp2_numpy, M.EXP2_TRUTH, 257, 0.0, 100.0)
        return Problem(name, M.model_exp2, 4, [x], [y], [1.0 / s], M.EXP2_TRUTH, [0, 1, 2, 3], [0] * 4)
    if name == 'gauss8':
        truth = M.gauss8_truth()
        x, y, s = M.make_single(M.gauss8_numpy, truth, 321, 0.0, 100.0)
        return Problem(name, M.model_gauss8, 32, [x], [y], [1.0 / s], truth, list(range(32)), [0] * 32)
    if name in ('global7', 'global7s'):
        xs, ys, ss, truths = M.make_global7(3, list(GLOBAL7_LENGTHS))
        return Problem(name, M.model_global7, 7, xs, ys, [1.0 / s for s in ss], truths, list(range(7)) if name == 'global7' else [6, 0, 4, 3],
                       GLOBAL7_IS_GLOBAL)
    raise KeyError(name)


PROBLEMS = ('exp2', 'gauss8', 'global7', 'global7s')
SINGLE = ('exp2', 'gauss8')
GLOBAL = ('global7', 'global7s')

# DTD_min with unequal entries: J^T J's diagonal at the start of these fits spans orders of magnitude, so one vector binds for some
# coordinates and not for others (tests/test_cpu_lm_loop_cases.py asserts both from the oracle's first pass)
DTD_EXP2 = (1e8, 1e-3, 1e-3, 1e5)
DTD_GLOBAL7 = (1e-3, 1e9, 1e-3, 1e-3, 1e7, 1e-3, 1e-3, 1e-3, 1e9, 1e-3, 1e-3, 1e9, 1e-3, 1e-3, 1e-3)

# (problem, pert, label, options).  The labels are the test ids; the options as gadf_fit takes them (DTD_min a tuple of dim values)
TABLE = (
    # ---- exp2: every exit reason a single-dataset problem can reach, each test alone with max_iter
    ('exp2', 0.3, 'max_iter', dict(lambda_=1.0, max_iter=3)),
    ('exp2', 0.3, 'chi2_abs', dict(lambda_=1.0, chi2_abs=2.0, max_iter=30)),
    ('exp2', 0.3, 'chi2_rel', dict(lambda_=1.0, chi2_rel=1e-2, max_iter=30)),
    ('exp2', 0.3, 'grad_chi2', dict(lambda_=1.0, grad_chi2=30.0, max_iter=30)),
    ('exp2', 0.3, 'cos_phi', dict(lambda_=1.0, cos_phi=1e-2, max_iter=30)),
    ('exp2', 0.3, 'rel_error', dict(lambda_=1.0, rel_error=1e-3, max_iter=30)),
    ('exp2', 0.3, 'no_max_iter', dict(lambda_=1.0, chi2_rel=1e-2)),
    # (a threshold between (old_old - old) / old and (old_old - old) / old_old of the iteration that ends the fit: the denominator shows)
    ('exp2', 0.6, 'chi2_rel_denominator', dict(lambda_=1.0, chi2_rel=0.5, max_iter=30)),
    ('exp2', 0.6, 'lam_incs_1_first', dict(lambda_=1e-8, lam_incs=1, lam_up=2.0)),
    # (accepted at lambda = 1, then lambda / 1e4 and lambda / 5e3 are both rejected: far from convergence, where exit 7 is rounding's)
    ('exp2', 0.8, 'lam_incs_1_later', dict(lambda_=1.0, lam_incs=1, lam_up=2.0, lam_down=1e4)),
    # ---- exp2: the lambda policies, each with an accepted and a rejected trial
    ('exp2', 0.6, 'plain_3_7', dict(lam_up=3.0, lam_down=7.0, lambda_=1e-4, lam_incs=8, max_iter=5)),
    ('exp2', 0.6, 'nielsen', dict(lambda_=1e-4, lam_incs=6, nielsen=1, max_iter=6)),
    # (under umnigh a rejected trial LOWERS lambda, gadfit.F90:785-808, so on exp2 a rejection repeats until exit 7 in iteration 0 or
    # never comes; the cases of these two policies that hold both kinds of trial are global7's below)
    ('exp2', 0.3, 'umnigh_accepting', dict(lambda_=1e-2, lam_incs=12, umnigh=1, max_iter=4)),
    ('exp2', 0.45, 'nielsen_umnigh_accepting', dict(lambda_=1e-2, lam_incs=12, nielsen=1, umnigh=1, max_iter=4)),
    ('exp2', 0.3, 'umnigh_uphill_1', dict(lambda_=1e-2, lam_incs=12, umnigh=1, uphill=1, max_iter=4)),
    ('exp2', 0.45, 'uphill_2', dict(lambda_=1e-4, lam_incs=8, uphill=2, max_iter=4)),
    # ---- exp2: the damping matrix and the acceleration
    ('exp2', 0.3, 'damp_max_0', dict(lambda_=1.0, damp_max=0, max_iter=4)),
    ('exp2', 0.3, 'dtd_min', dict(lambda_=1.0, DTD_min=DTD_EXP2, max_iter=4)),
    ('exp2', 0.3, 'accth_taken', dict(lambda_=1.0, accth=0.75, max_iter=4)),
    ('exp2', 0.6, 'accth_zeroed', dict(lambda_=1.0, accth=0.05, max_iter=4)),
    # ---- gauss8: the matrix-core form
    ('gauss8', 0.03, 'max_iter', dict(lambda_=1.0, max_iter=3)),
    ('gauss8', 0.03, 'cos_phi', dict(lambda_=1.0, cos_phi=0.2, max_iter=30)),
    ('gauss8', 0.03, 'chi2_rel', dict(lambda_=1.0, chi2_rel=0.5, max_iter=30)),
    ('gauss8', 0.03, 'accth', dict(lambda_=1.0, accth=0.75, max_iter=4)),
    ('gauss8', 0.05, 'nielsen', dict(lambda_=1e-2, lam_incs=12, nielsen=1, max_iter=3)),
    ('gauss8', 0.03, 'umnigh_uphill_1', dict(lambda_=1e-2, lam_incs=12, umnigh=1, uphill=1, max_iter=4)),
    ('gauss8', 0.05, 'plain_3_7', dict(lam_up=3.0, lam_down=7.0, lambda_=1e-2, lam_incs=12, max_iter=3)),
    ('gauss8', 0.05, 'uphill_2', dict(lambda_=1e-2, lam_incs=12, uphill=2, max_iter=3)),
    ('gauss8', 0.05, 'nielsen_umnigh', dict(lambda_=0.1, lam_incs=2, nielsen=1, umnigh=1, max_iter=6)),
    # ---- global7: every exit reason, each test alone with max_iter
    ('global7', 0.3, 'max_iter', dict(lambda_=1.0, max_iter=3)),
    ('global7', 0.3, 'chi2_abs', dict(lambda_=1.0, chi2_abs=3.0, max_iter=40)),
    ('global7', 0.2, 'chi2_rel', dict(lambda_=1.0, chi2_rel=0.5, max_iter=40)),
    ('global7', 0.3, 'grad_chi2', dict(lambda_=1.0, grad_chi2=100.0, max_iter=40)),
    ('global7', 0.3, 'cos_phi', dict(lambda_=1.0, cos_phi=1e-2, max_iter=40)),
    ('global7', 0.3, 'rel_error', dict(lambda_=1.0, rel_error=1e-3, max_iter=40)),
    ('global7', 0.3, 'rel_error_global', dict(lambda_=1.0, rel_error_global=1e-3, max_iter=40)),
    ('global7', 0.2, 'lam_incs_1', dict(lambda_=1e-3, lam_incs=1, umnigh=1)),
    ('global7', 0.3, 'nielsen', dict(lambda_=1e-4, lam_incs=8, nielsen=1, max_iter=4)),
    ('global7', 0.2, 'plain_3_7', dict(lam_up=3.0, lam_down=7.0, lambda_=1.0, lam_incs=8, max_iter=4)),
    ('global7', 0.2, 'umnigh', dict(lambda_=1e-3, lam_incs=12, umnigh=1, max_iter=4)),
    # (the rule keeps this row at 6.5e-14 between 1 and 3 images, but over IMAGES the oracle's own parameters spread by 1.0e-12, TOL_FIT
    # itself -- spread() -- so a device that exceeds TOL_FIT here is to be judged against that spread; the policy's other case is gauss8's)
    ('global7', 0.25, 'nielsen_umnigh', dict(lambda_=1e-3, lam_incs=4, nielsen=1, umnigh=1, max_iter=6)),
    # (an ACCEPTED step that goes uphill, new_chi2 > old_chi2: old_chi2 stays the smaller of the two, gadfit.F90:829; the CPU module
    # shows the step)
    ('global7', 0.2, 'uphill_step_taken', dict(lambda_=1e-2, lam_incs=2, umnigh=1, uphill=1, max_iter=8)),
    ('global7', 0.3, 'uphill_1_lam_down_100', dict(lambda_=1e-2, lam_incs=8, uphill=1, lam_down=100.0, max_iter=5)),
    ('global7', 0.3, 'dtd_min', dict(lambda_=1.0, DTD_min=DTD_GLOBAL7, max_iter=3)),
    ('global7', 0.3, 'accth', dict(lambda_=1.0, accth=0.75, max_iter=3)),
    # ---- global7s: passive parameters, an active list that does not ascend
    ('global7s', 0.3, 'rel_error_global', dict(lambda_=1.0, rel_error_global=1e-3, max_iter=40)),
    # (lam_down /= lam_up: Nielsen's factor is bounded below by 1 / lam_down, and a good step reaches the bound)
    ('global7s', 0.3, 'nielsen_lam_down_4', dict(lambda_=1e-4, lam_incs=8, nielsen=1, lam_down=4.0, max_iter=4)),
    ('global7s', 0.3, 'chi2_rel', dict(lambda_=1.0, chi2_rel=0.9, max_iter=30)),
    ('global7s', 0.3, 'damp_max_0', dict(lambda_=1.0, damp_max=0, max_iter=3)),
)


def case_id(row):
    return '%s-%g-%s' % row[:3]


def options(row):
    """the options of a row as both OracleProblem.fit and Context.fit take them: thresholds rounded to real32, then plain floats"""
    return {k: (float(np.float32(v)) if k in F32_KEYS else (list(v) if k == 'DTD_min' else v)) for k, v in row[3].items()}


def oracle_fit(row, n_images=1, umnigh_a=0.5, start=None):
    """one fit of a row by the oracle: (the FitResult, the OracleProblem: its pars are the fitted parameters [n_datasets][n_pars], its
    umnigh_a what the fit hands on, its JTJ0 ... delta2_0 the first iteration's)"""
    prob = problem(row[0])
    p = prob.oracle(prob.start(row[1]) if start is None else start)
    return p.fit(n_images=n_images, umnigh_a=umnigh_a, **options(row)), p


def counts(r):
    return tuple(int(getattr(r, f)) for f in COUNTS)


class Selected:
    """a row under the rule: kept, the n_images = 1 fit (r, p as oracle_fit returns them; pars, umnigh_a), the relative difference of
    the parameters between 1 and 3 images, and why a dropped row was dropped.  Nothing here is written to after it is made."""

    def __init__(self, row):
        self.row, self.id, self.problem, self.options = row, case_id(row), problem(row[0]), options(row)
        self.r, self.p = oracle_fit(row, 1)
        self.pars, self.umnigh_a = self.p.pars.copy(), float(self.p.umnigh_a)
        r3, p3 = oracle_fit(row, 3)
        pars3 = p3.pars
        act = self.problem.active
        self.diff = float(np.max(np.abs(self.pars[:, act] - pars3[:, act]) / np.abs(self.pars[:, act])))
        self.margin, self.exit_margin = float(self.r.min_margin), float(self.r.min_exit_margin)
        self.why = [w for w, bad in (('counts', counts(self.r) != counts(r3)), ('parameters', not self.diff <= SELF_TOL),
                                     ('margin', not self.margin > MARGIN), ('exit margin', not self.exit_margin > EXIT_MARGIN)) if bad]
        self.kept = not self.why


@functools.lru_cache(maxsize=None)
def selected(row_index):
    return Selected(TABLE[row_index])


def kept():
    """the kept rows: [Selected]"""
    return [s for s in (selected(k) for k in range(len(TABLE))) if s.kept]


def kept_ids():
    return [s.id for s in kept()]


def by_id(cid):
    return next(s for s in kept() if s.id == cid)


def spread(row, images=IMAGES):
    """the oracle's own spread of a row: the largest relative difference of its fitted parameters over the image counts"""
    act = problem(row[0]).active
    fits = [oracle_fit(row, n)[1].pars[:, act] for n in images]
    return max(float(np.max(np.abs(f - fits[0]) / np.abs(fits[0]))) for f in fits[1:])


# ---- umnigh_a from fit to fit (the SAVEd local of gadfit.F90:515) -------------------------------------------------------------------------
# the ids of the rows fitted twice in a row, the second fit given the umnigh_a the first hands on, and once more with 0.5 again
CARRY = ('exp2-0.3-umnigh_accepting', 'global7-0.2-umnigh')


def carry_start(s):
    """the start of the later fits of a carry-over: the row's own again, so that umnigh_a is all that differs between them"""
    return s.problem.start(s.row[1])


# ---- gfh_lm_iterate: its scheme restated over the oracle's passes -----------------------------------------------------------------
def lm_iterate_restated(prob, start, n_iter, lambda_, n_images=1):
    """gfh_lm_iterate's scheme (include/gadfit_hip.h): one trial per iteration; accept gives lambda / 10, reject restores the
    parameters and gives lambda * 10; DTD is the running maximum of J^T J's diagonal.  Returns (parameters, lambda, chi2, accepted
    count, DTD, the closest |new_chi2 - old_chi2| / old_chi2)"""
    p = prob.oracle(start)
    chi2, lam, accepted, margin = p.chi2(n_images)[0], lambda_, 0, np.inf
    DTD = np.zeros(p.dim)
    for _ in range(n_iter):
        old = p.pars.copy()
        JTJ, JTr, _, _ = p.sweep(n_images)
        DTD = np.maximum(DTD, np.diag(JTJ))
        delta = orc.potr(JTJ + lam * np.diag(DTD), JTr)
        for d in range(p.nd):
            p.pars[d, p.active] += delta[p.jac[d]]
        new = p.chi2(n_images)[0]
        margin = min(margin, abs(new - chi2) / chi2)
        if new < chi2:
            chi2, lam, accepted = new, lam / 10.0, accepted + 1
        else:
            p.pars[:] = old
            lam = lam * 10.0
    return p.pars.copy(), lam, chi2, accepted, DTD, margin


# (problem, pert, lambda at the start): 6 iterations from a start that contains a rejection
LM_ITERATE = (('exp2', 0.6, 1e-4), ('global7', 0.2, 1e-2))
LM_ITERATE_N = 6


# ---- every translation unit the GPU tests ask for ---------------------------------------------------------------------------------
def units():
    """[(tape, active list, n_datasets, with the Jacobian store)]: each problem in the form that stores J and, for the contexts under
    keep_jacobian 2 and a deferred store, in the form that does not"""
    return [(problem(n).tape, problem(n).active, len(problem(n).xs), store) for n in PROBLEMS for store in (True, False)]
