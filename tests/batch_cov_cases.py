"""The inputs of tests/test_cpu_batch_cov.py and tests/test_gpu_batch_cov.py: the errors of a batch (gfh_batch_covariance,
gfh_fit_batch_errors; the kernel gfh_k_batch_cov), their reference and the rule that selects which fits may be held against it.
Everything here is deterministic and needs no GPU; the spectra, the active sets and the starts are those of tests/batch_cases.py and
tests/batch_form_cases.py, imported, not restated.

THE REFERENCE.  For a spectrum at given parameters A is J^T J, A~ = A / sqrt(diag(A) diag(A)^T) is A scaled to unit diagonal, and the
reference inverse is formed in numpy.longdouble (Gauss-Jordan with partial pivoting: numpy's linalg takes no longdouble).  Errors are
measured in the scaling of A~: with D = diag(sqrt(diag(A))) the covariance C has the scaled form C~ = D C D, the inverse of A~, and
    err(C, C_ref) = ||C~ - C~_ref||_2 / ||C~_ref||_2.
THE RULE.  A fit is compared with the reference only where kappa_2(A~) <= KAPPA_MAX = 1e8, evaluated on the ORACLE's A
(OracleProblem.sweep) alone: nothing the device returns enters it.  Kept: all eight EXP4_SETS over the 48 spectra of Part 2
(kappa_2 <= 3.6e3), every length of LENGTHS from 8 up with the four parameters of model_exp2 active (<= 1.8e7 at n = 8, <= 1.8e3 at 16
and 17, <= 30 from 63 on), and every length with ONE_ACTIVE (kappa_2 = 1).  Dropped, four parameters from four to six points: all six
spectra of n = 4 (1.0e12 ... 1.8e14), all six of n = 5 (3.8e8 ... 4.7e11) and two of n = 6 (6.8e8, 2.8e9; its other four lie at
8.1e6 ... 5.6e7 and are kept): DROPPED = 14 of 78.  The GPU module holds the dropped ones through the residual || C~ A~ - I || alone.
tests/test_cpu_batch_cov.py asserts these counts.
THE YARDSTICK FOR THE ALGEBRA.  host_cholesky_inverse is the kernel's algebra in plain doubles on the host (upper factor, its inverse,
the product with its transpose; one rounding per operation).  r_host() is the largest err(host, longdouble) / (eps kappa_2(A~)) over
the kept matrices; the GPU bounds are multiples of it, not of anything the device returns.

Part 1: model_exp2, spectrum_n(n, s), s = 0 ... 5, n over LENGTHS from both ends inwards (short beside long), at the spectrum's truth.
Part 2: model_exp4, batch_cases.part2 at its truths, every active set of EXP4_SETS and the two orders of EXP4_ORDER.
THE SINGULAR SPECTRUM: every abscissa 0.  Every row of its Jacobian is then w (1, 0, 1, 0) EXACTLY -- exp(-0 / p) = 1 and the
derivatives by the decay times carry the factor x = 0 -- so J^T J has rank 1 with an exact zero on its diagonal, pivot 1 is an exact
0 on any implementation (info = 2) and A~ is not defined.  A common abscissa x != 0 also gives rank 1, but then the later pivots are
rounding residues of either sign and whether a factorisation notices is not a property one can hold it to."""
import functools

import numpy as np

from gadfit_amd.ad import trace_model
from oracle import binding as orc
from tests import batch_cases as BC
from tests import models as M
from tests.batch_common import start_of

EPS = float(np.finfo(np.float64).eps)
KAPPA_MAX = 1e8
ACTIVE = [0, 1, 2, 3]
ONE_ACTIVE = [1]
LENGTHS = (4, 5, 6, 8, 16, 17, 63, 64, 65, 255, 256, 257, 1000)
SAMPLES = 6
OFF = 0.0                          # the parameters of every comparison: the spectra's truths
PERMUTED = ([6, 1, 4], [1, 4, 6])
EXP4_LISTS = [list(a) for a in BC.EXP4_SETS] + [PERMUTED[1]]          # every unit of these is one of batch_cases.part2_units
CUTS = (7, 5, 3, 2, 1)
DROPPED = {4: 6, 5: 6, 6: 2}          # of Part 1 with ACTIVE, per length; nothing else is dropped


# ---- the algebra ---------------------------------------------------------------------------------------------------------------------
def scale_of(A):
    return np.sqrt(np.diag(A))


def scaled(A, d):
    return A / np.outer(d, d)


def kappa(A):
    """kappa_2 of A scaled to unit diagonal; inf where that is not defined"""
    d = scale_of(A)
    if not (np.all(np.isfinite(d)) and np.all(d > 0.0)):
        return float('inf')
    s = np.linalg.svd(scaled(A, d), compute_uv=False)
    return float('inf') if not s[-1] > 0.0 else float(s[0] / s[-1])


def longdouble_inverse(A):
    """the inverse of A in numpy.longdouble by Gauss-Jordan elimination with partial pivoting"""
    n = A.shape[0]
    W = np.concatenate([np.asarray(A, dtype=np.longdouble), np.eye(n, dtype=np.longdouble)], axis=1)
    for j in range(n):
        p = j + int(np.argmax(np.abs(W[j:, j])))
        if p != j:
            W[[j, p]] = W[[p, j]]
        W[j] = W[j] / W[j, j]
        for i in range(n):
            if i != j:
                W[i] = W[i] - W[i, j] * W[j]
    return W[:, n:]


def host_cholesky_inverse(A):
    """(C, info): gfh_k_batch_cov's algebra in plain doubles -- A = U^T U, V = U^-1, C = V V^T, every entry formed once; info j + 1
    where pivot j is not positive and finite (C is then None)"""
    n = A.shape[0]
    U = np.zeros((n, n))
    for j in range(n):
        ajj = A[j, j]
        for k in range(j):
            ajj = ajj - U[k, j] * U[k, j]
        if not (ajj > 0.0 and ajj < np.inf):
            return None, j + 1
        ajj = np.sqrt(ajj); U[j, j] = ajj
        rinv = 1.0 / ajj
        for c in range(j + 1, n):
            t = A[j, c]
            for k in range(j):
                t = t - U[k, j] * U[k, c]
            U[j, c] = t * rinv
    V = U
    for j in range(n):
        vjj = 1.0 / V[j, j]
        for i in range(j):
            t = V[i, i] * V[i, j]
            for k in range(i + 1, j):
                t = t + V[i, k] * V[k, j]
            V[i, j] = -(t * vjj)
        V[j, j] = vjj
    C = np.zeros((n, n))
    for a in range(n):
        for b in range(a, n):
            t = V[a, b] * V[b, b]
            for k in range(b + 1, n):
                t = t + V[a, k] * V[b, k]
            C[a, b] = C[b, a] = t
    return C, 0


def norm2(M_):
    return float(np.linalg.norm(np.asarray(M_, dtype=np.float64), 2))


def scaled_error(C, C_ref, d):
    """err(C, C_ref) in the scaling of A~ (d = scale_of(A)); C_ref may be longdouble: the difference is formed there"""
    D = np.outer(d, d).astype(np.longdouble)
    ref = np.asarray(C_ref, dtype=np.longdouble) * D
    return norm2((np.asarray(C, dtype=np.longdouble) * D) - ref) / norm2(ref)


def residual(C, A, d):
    """(|| C~ A~ - I ||_2, || A~ ||_2, || C~ ||_2)"""
    Ct, At = C * np.outer(d, d), scaled(A, d)
    return norm2(Ct @ At - np.eye(A.shape[0])), norm2(At), norm2(Ct)


# ---- Part 1 --------------------------------------------------------------------------------------------------------------------------
def order():
    """(n, s) in batch order: per s the lengths from both ends inwards (4, 1000, 5, 257, ...), the middle one last"""
    ln = LENGTHS
    per_s = [n for i in range(len(ln) // 2) for n in (ln[i], ln[-1 - i])] + list(ln[len(ln) // 2:(len(ln) + 1) // 2])
    return [(n, s) for s in range(SAMPLES) for n in per_s]


@functools.lru_cache(maxsize=None)
def part1():
    """(tape, order [(n, s)], starts [78][4], Batch)"""
    sp = [BC.spectrum_n(n, s) for n, s in order()]
    starts = np.array([start_of(it[0], OFF) for it in sp])
    return trace_model(M.model_exp2, 4), order(), starts, BC.Batch([it[1:4] for it in sp])


def part2_starts(active):
    return BC.part2_starts(list(active), OFF)


# ---- the oracle's matrices, the rule and the yardstick -------------------------------------------------------------------------------
def oracle_pass(tape, item, start, active):
    """(A, chi2) of one spectrum at `start`: OracleProblem.sweep's J^T J and chi2()"""
    x, y, w = item
    p = orc.OracleProblem(tape, [x], [y], [w], [start], list(active), [0] * tape.n_pars)
    return p.sweep()[0], p.chi2()[0]


@functools.lru_cache(maxsize=None)
def oracle_matrices(part, active):
    """[(A, chi2, kappa_2(A~))] of a part's spectra under an active tuple"""
    tape, starts, batch = (part1()[0], part1()[2], part1()[3]) if part == 1 else (BC.part2()[0], part2_starts(active), BC.part2()[2])
    out = []
    for k, item in enumerate(batch.items):
        A, chi2 = oracle_pass(tape, item, starts[k], active)
        out.append((A, chi2, kappa(A)))
    return out


def kept(part, active):
    return np.array([m[2] <= KAPPA_MAX for m in oracle_matrices(part, tuple(active))])


def all_sets():
    """[(part, active tuple)] of every comparison"""
    return [(1, tuple(ACTIVE)), (1, tuple(ONE_ACTIVE))] + [(2, tuple(a)) for a in EXP4_LISTS] + [(2, tuple(PERMUTED[0]))]


@functools.lru_cache(maxsize=None)
def host_ratios():
    """{(part, active): [err(host double, longdouble) / (eps kappa) of the kept fits]}"""
    out = {}
    for part, active in dict.fromkeys(all_sets()):
        r = []
        for A, _, k in oracle_matrices(part, active):
            if k <= KAPPA_MAX:
                C, info = host_cholesky_inverse(A)
                assert info == 0
                r.append(scaled_error(C, longdouble_inverse(A), scale_of(A)) / (EPS * k))
        out[(part, active)] = r
    return out


def r_host():
    return max(max(r) for r in host_ratios().values())


# ---- a singular fit ------------------------------------------------------------------------------------------------------------------
def singular_item(n=16):
    """every abscissa 0 (see the module's text): (x, y, w)"""
    return np.zeros(n), np.linspace(1.0, 2.0, n), np.full(n, 3.0)


def nan_item(n=16):
    return np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)


SINGULAR_NEIGHBOURS = (0, 1, 13)          # spectra of Part 1 that lie between and around the two (n = 4, 1000, 4)
