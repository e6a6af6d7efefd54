"""The inputs of tests/test_cpu_plain_errors.py and tests/test_gpu_plain_errors.py: the errors and the curves of a plain fit
(gfh_covariance, gfh_invert_normal, gfh_eval; the kernels of device/eval.hip), their reference and the rule that selects what is
held against it.  Everything here is deterministic and needs no GPU.  The algebra, the rule, the reference inverse and the error
measure are those of tests/batch_cov_cases.py, imported, not restated: A~ is J^T J scaled to unit diagonal, the reference inverse is
formed in numpy.longdouble, a case is compared entry-wise only where kappa_2(A~) <= KAPPA_MAX = 1e8 on the ORACLE's matrix.

THE CASES (all at the data's truths, the weights 1 / sigma):
  exp2       model_exp2, four active, one dataset of 4, 255, 256, 257, 513 and 1000 points: a part tile, an exact tile, a tile + 1, two
             tiles + 1 (a tile is 256 slots).  The abscissas are spaced geometrically over 0.25 ... 100, so that even four points span
             both decay times: batch_cases.spectrum_n's even spacing puts kappa_2 at 1e12 at four points, which the rule would drop.
  global7    model_global7 over three datasets of 255, 256 and 300 points: four local and three global parameters, dim 15 (the dense
             form: the arrow form starts above dim 16).
  gauss8     model_gauss8, 32 active, 513 points.
  exp4       model_exp4 with [6, 1, 4] and [1, 4, 6] active (five passive), 257 points.
  piecewise2 tests/branching.py: a branching eval(), decided per point on the device, 300 points.
  aux        a model that reads an auxiliary per-point column, 300 points.
The rule keeps every one of them (tests/test_cpu_plain_errors.py asserts it and prints the kappas).

THE YARDSTICK FOR THE ALGEBRA.  r_host() is measured on the library's own host code, gfh_invert_normal, not assumed from the batch
kernel's: the largest err(gfh_invert_normal, longdouble) / (eps kappa_2(A~)) over the oracle's matrices of the cases above, dense and
-- where the column map has the arrow structure -- arrow, and over the synthetic matrices of synthetic() (dim 1, 4, 8, 32 and
model_global7's pattern over 3 and 40 datasets)."""
import functools

import numpy as np

from gadfit_amd import _lib
from gadfit_amd import tape as T
from gadfit_amd.ad import aux, exp, trace_model
from oracle import binding as orc
from tests import batch_cov_cases as CV
from tests import branching as B
from tests import models as M

EPS = CV.EPS
KAPPA_MAX = CV.KAPPA_MAX
LENGTHS = (4, 255, 256, 257, 513, 1000)
GLOBAL7_LENGTHS = (255, 256, 300)
GLOBAL7_ACTIVE = list(range(7))
GLOBAL7_IS_GLOBAL = [0, 0, 0, 0, 1, 1, 1]
PERMUTED = CV.PERMUTED                 # ([6, 1, 4], [1, 4, 6])
GRIDS = (1, 255, 257)


class Case:
    """one fit: the model, its datasets, its parameters and its active and global sets"""

    def __init__(self, name, tape, xs, ys, ws, pars, active, is_global, aux_columns=None):
        self.name, self.tape, self.xs, self.ys, self.ws = name, tape, xs, ys, ws
        self.pars = np.atleast_2d(np.asarray(pars, dtype=np.float64))
        self.active, self.is_global, self.aux = list(active), list(is_global), aux_columns
        self.n_pars = self.pars.shape[1]
        self.pos = np.concatenate([[0], np.cumsum([x.size for x in xs])]).astype(np.int64)

    def oracle(self, loss=0, use_ad=True):
        return orc.OracleProblem(self.tape, self.xs, self.ys, self.ws, self.pars, self.active, self.is_global, loss=loss, aux=self.aux,
                                 use_ad=use_ad)

    def x(self):
        return np.concatenate(self.xs)

    def y(self):
        return np.concatenate(self.ys)

    def w(self):
        return np.concatenate(self.ws)

    def context(self, device=0):
        c = _lib.Context(device)
        c.set_model(self.tape)
        c.set_data(self.x(), self.y(), self.w(), self.pos)
        if self.aux is not None:
            c.set_aux(self.aux)
        return c


def _noisy(f, seed):
    sigma = 0.01 * (1.0 + np.abs(f))
    return f + sigma * M.normal(f.size, seed), 1.0 / sigma


def geometric(n):
    return 0.25 * (400.0 ** ((np.arange(n) + 0.5) / n))


@functools.lru_cache(maxsize=None)
def exp2(n):
    x = geometric(n)
    y, w = _noisy(M.exp2_numpy(M.EXP2_TRUTH, x), M.SEED + 31 * n)
    return Case('exp2_%d' % n, trace_model(M.model_exp2, 4), [x], [y], [w], M.EXP2_TRUTH, [0, 1, 2, 3], [0] * 4)


@functools.lru_cache(maxsize=None)
def global7():
    xs, ys, ss, truths = M.make_global7(3, list(GLOBAL7_LENGTHS))
    return Case('global7', trace_model(M.model_global7, 7), xs, ys, [1.0 / s for s in ss], truths, GLOBAL7_ACTIVE, GLOBAL7_IS_GLOBAL)


@functools.lru_cache(maxsize=None)
def gauss8():
    truth = M.gauss8_truth()
    x, y, s = M.make_single(M.gauss8_numpy, truth, 513, 0.0, 100.0)
    return Case('gauss8', trace_model(M.model_gauss8, 32), [x], [y], [1.0 / s], truth, list(range(32)), [0] * 32)


@functools.lru_cache(maxsize=None)
def exp4(order):
    x, y, s = M.make_single(M.exp4_numpy, M.EXP4_TRUTH, 257, 0.05, 100.0)
    return Case('exp4_%s' % '_'.join(map(str, PERMUTED[order])), trace_model(M.model_exp4, 8), [x], [y], [1.0 / s], M.EXP4_TRUTH, PERMUTED[order], [0] * 8)


@functools.lru_cache(maxsize=None)
def piecewise2():
    x, y, s = B.make_data(B.piecewise2_numpy, B.PIECEWISE2_TRUTH, 300)
    V = T.Variants(B.model_piecewise2, 4)
    V.explore([x[0], x[-1]], B.PIECEWISE2_TRUTH)
    return Case('piecewise2', V, [x], [y], [1.0 / s], B.PIECEWISE2_TRUTH, [0, 1, 2, 3], [0] * 4)


AUX_TRUTH = np.array([2.0, 3.0, 0.05])


def model_aux(p, x):
    return p[0] * aux(0) + p[1] * exp(-(x * p[2]))


@functools.lru_cache(maxsize=None)
def auxiliary():
    n = 300
    x = 100.0 * (np.arange(n) + 0.5) / n
    col = 1.0 / (1.0 + 1.0e-3 * x ** 2)                  # a real function of x alone, tabulated per point
    y, w = _noisy(AUX_TRUTH[0] * col + AUX_TRUTH[1] * np.exp(-x * AUX_TRUTH[2]), M.SEED + 77)
    return Case('aux', trace_model(model_aux, 3), [x], [y], [w], AUX_TRUTH, [0, 1, 2], [0] * 3, aux_columns=col[None, :])


def all_cases():
    return [exp2(n) for n in LENGTHS] + [global7(), gauss8(), exp4(0), exp4(1), piecewise2(), auxiliary()]


# ---- the oracle's matrices, the rule and the yardstick -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_pass(name, loss=0):
    """(J^T J, chi2(), kappa_2 of J^T J scaled to unit diagonal, jac_idx, dim) of a case by name, on the oracle alone"""
    case = {c.name: c for c in all_cases()}[name]
    p = case.oracle(loss=loss)
    A = p.sweep()[0]
    return A, p.chi2()[0], CV.kappa(A), p.jac.copy(), p.dim


def global7_pattern(nd, seed=5):
    """(jac_idx, dim, a well-conditioned J^T J) with model_global7's column map over nd datasets of 30 rows each"""
    na = 7
    act = np.arange(na, dtype=np.int32); glob = np.array(GLOBAL7_IS_GLOBAL, dtype=np.int32)
    jac = np.zeros((nd, na), dtype=np.int32)
    dim = _lib.lib().gfh_jacobian_indices(nd, na, _lib.ip(act), _lib.ip(glob), _lib.ip(jac))
    rng = np.random.default_rng(seed + nd)
    J = np.zeros((30 * nd, dim))
    for d in range(nd):
        J[30 * d:30 * (d + 1), jac[d]] = rng.standard_normal((30, na))
    return jac, dim, J.T @ J


def dense_matrix(dim, seed=3):
    rng = np.random.default_rng(seed + dim)
    J = rng.standard_normal((3 * dim + 5, dim)) * (10.0 ** rng.uniform(-2, 2, size=dim))          # columns of very different sizes
    return np.arange(dim, dtype=np.int32)[None, :], dim, J.T @ J


def synthetic():
    """[(label, jac_idx, dim, A)]: dim 1, 4, 8, 32 dense, and model_global7's pattern over 3 (dim 15) and 40 (dim 163) datasets"""
    return [('dense%d' % n,) + dense_matrix(n) for n in (1, 4, 8, 32)] + [('global7x%d' % nd,) + global7_pattern(nd) for nd in (3, 40)]


def algebra_ratio(jac, dim, A, use_structure):
    """(err(gfh_invert_normal, longdouble) / (eps kappa), kappa, form taken)"""
    cov, _, info, form = _lib.invert_normal(jac, dim, A, use_structure)
    assert info == 0
    k = CV.kappa(A)
    return CV.scaled_error(cov, CV.longdouble_inverse(A), CV.scale_of(A)) / (EPS * k), k, form


@functools.lru_cache(maxsize=None)
def host_ratios():
    """{label: ratio} over the synthetic matrices and the oracle's matrices of the cases, dense and with the structure on"""
    out = {}
    for label, jac, dim, A in synthetic():
        for s in (False, True):
            out[(label, s)] = algebra_ratio(jac, dim, A, s)[0]
    for c in all_cases():
        A, _, k, jac, dim = oracle_pass(c.name)
        if k <= KAPPA_MAX:
            for s in (False, True):
                out[(c.name, s)] = algebra_ratio(jac, dim, A, s)[0]
    return out


def r_host():
    return max(host_ratios().values())


# ---- the references of the curves ----------------------------------------------------------------------------------------------------
def oracle_points(case, use_ad=True):
    """(f0 [N], g0 [N][na] unweighted in the caller's order, res0 [N] the plain residual) of a case from OracleProblem.sweep's stored
    Jacobian and residuals: g0 = J / w per dataset through Jacobian_indices, f0 = y - res0 / w (one subtraction and one division on
    numbers of the size of y: 2 eps (|y| + |f0|), far inside TOL_PASS |f0| where f0 is not small against y -- true of every case)"""
    p = case.oracle(use_ad=use_ad)
    _, _, res0, JT = p.sweep(want_J=True)
    w, y = case.w(), case.y()
    na = len(case.active)
    g0 = np.empty((w.size, na))
    for d in range(len(case.xs)):
        s = slice(case.pos[d], case.pos[d + 1])
        g0[s] = JT[s][:, p.jac[d]] / w[s, None]
    return y - res0 / w, g0, res0
