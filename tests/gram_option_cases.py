"""The inputs of tests/test_gpu_gram_options.py: the options that change what the kernels compute per point -- the robust losses
(gfh_set_loss: 1 Cauchy, 2 Huber) and use_ad = .false. (forward differences, central second difference) -- crossed with the forms of the
fused sweep + Gram kernel.  GFH_ROBUST(R, Wl) stands once in every form of csrc/device/fused_sweep_gram.hip and once in sweep.hip, and
under either option STEP 3 leaves gfh_k_omega_jt for gfh_k_omega + k_jtv over the stored (loss-scaled) Jacobian; the other GPU files
reach all of that at 8 active parameters and fewer, the VALU form.  The cases are tests/gram_layout_cases.py's own (GL.Case, GL.b1 ...
GL.b5 and their expect()): neither option may change the dispatch.  Everything here is deterministic and needs no GPU;
tests/test_cpu_gram_option_cases.py shows that the oracle is a sound reference under every option and compiles every unit.

D1: loss x form, one dataset.  D2: loss x layouts of several datasets.  D3: finite differences x form.  D4: fits under a loss."""
import numpy as np

from tests import gram_layout_cases as GL
from tests.parity_common import TOL_FIT, TOL_FIT_LOSS_96

CAUCHY, HUBER = 1, 2


class Opt:
    """a case of tests/gram_layout_cases.py under a loss or under finite differences"""

    def __init__(self, part, case, loss=0, use_ad=True, fits=(), fit_tol=None):
        self.part, self.case, self.loss, self.use_ad, self.fits, self.fit_tol = part, case, loss, use_ad, tuple(fits), fit_tol
        self.id = '%s-%s-%s' % (part, 'fd' if not use_ad else {1: 'cauchy', 2: 'huber'}[loss], case.id)

    def __repr__(self):
        return self.id


def loss_scale(loss, r):
    """sqrt(rho'(r^2)) in the precision of r: Cauchy rho = ln(1 + z), Huber rho = z up to z = 1 and 2 sqrt(z) - 1 beyond (lm_solver.cpp:255-284)"""
    if loss == CAUCHY:
        return np.sqrt(1 / (1 + r * r))
    if loss == HUBER:
        return np.where(r * r > 1, np.sqrt(1 / np.maximum(np.abs(r), 1)), np.ones_like(r))
    return np.ones_like(r)


def longdouble_rows(o, d, pars=None):
    """(plain residuals, residuals, Jacobian rows [n][na]) of dataset d of an AD case in numpy.longdouble from the closed form, under the case's loss"""
    xs, ys, ws, start = o.case.data()
    f, g = o.case.rows(start[d] if pars is None else pars, xs[d])
    w = ws[d].astype(np.longdouble)
    plain = (ys[d].astype(np.longdouble) - f) * w
    ls = loss_scale(o.loss, plain)
    return plain, plain * ls, g[:, o.case.active] * (w * ls)[:, None]


def longdouble_sums(J, res, dp, jac, dim):
    """(J^T J, J^T r, sum r^2) in numpy.longdouble of rows J [N][na] and residuals [N], dataset d's columns scattered through jac[d]"""
    JTJ = np.zeros((dim, dim), dtype=np.longdouble); JTr = np.zeros(dim, dtype=np.longdouble); chi = np.longdouble(0)
    for d in range(len(dp) - 1):
        Jd = np.asarray(J[dp[d]:dp[d + 1]], dtype=np.longdouble); r = np.asarray(res[dp[d]:dp[d + 1]], dtype=np.longdouble)
        ix = np.asarray(jac[d])
        JTJ[np.ix_(ix, ix)] += Jd.T @ Jd; JTr[ix] += Jd.T @ r; chi += r @ r
    return JTJ, JTr, chi


def sum_errors(JTJ, JTr, chi, want):
    """tests/parity_common.py: _device_vs_oracle's metrics for J^T J, J^T r and chi2, against longdouble_sums()"""
    dg = np.diag(want[0]).astype(float)
    return (float(np.max(np.abs(JTJ - want[0]) / (np.sqrt(np.outer(dg, dg)) + 1e-300))),
            float(np.max(np.abs(JTr - want[1]) / (np.sqrt(dg * float(want[2])) + 1e-300))), float(abs(chi - want[2]) / want[2]))


# ---- D1: loss x form, one dataset ---------------------------------------------------------------------------------------------------
D1_SIZES = (1, 65, 2049)          # a lone lane; a full wave plus one point; 5 gram blocks: several workgroups and the reduction
D1_SIZES_UNFUSED = (65, 2049)     # as B1 has it for 130 active


def d1_sizes(na):
    return D1_SIZES if na <= GL.FUSED_MAX else D1_SIZES_UNFUSED


def d1():
    return [Opt('D1', GL.b1(na, n), loss) for loss in (CAUCHY, HUBER) for na in GL.FORMS for n in d1_sizes(na)]


# ---- D2: loss x layouts with several datasets ---------------------------------------------------------------------------------------
D2_FORMS = (32, 96)


def d2():
    """B2: in-kernel tail, inv[] scatter; B3: launch chain, pattern-only image, parameter block by pointer"""
    return [Opt('D2', GL.b2(na), CAUCHY) for na in D2_FORMS] + [Opt('D2', GL.b3(na), CAUCHY) for na in D2_FORMS]


# ---- D3: finite differences x form --------------------------------------------------------------------------------------------------
# expK((na + 1) // 2) with its first na parameters active: the value body is inlined na + 1 times, so K stays as small as it can.
D3_ACTIVE = (17, 65, 81)          # full stage, half stage, cooperative
D3_SIZES = (65, 2049)
D3_NO_STORE = (17,)               # the sweep without the Jacobian store, once


def d3_case(na, n):
    K = (na + 1) // 2
    return GL.Case('D3-%d-n%d' % (na, n), 'D3', 'exp', K, list(range(na)), [n])


def d3():
    return [Opt('D3', d3_case(na, n), use_ad=False) for na in D3_ACTIVE for n in D3_SIZES]


FD_STEP = 2.0 ** -26              # sqrt(epsilon(1d0)): fitfunction.F90:164


def fd_steps(pars):
    """the step the forward difference divides by, (p + sqrt(eps) p) - p in double (fitfunction.F90:164-169)"""
    p = np.asarray(pars, dtype=np.float64)
    return (p + FD_STEP * p) - p


def expK_fd_rows(K, pars, x, active):
    """(f, [n][len(active)] forward differences of f) in numpy.longdouble: the closed form at p and at p + step, divided by the double step"""
    p = np.asarray(pars, dtype=np.float64)
    f0, _ = GL.expK_rows(K, p, x)
    g = np.zeros((np.size(x), len(active)), dtype=np.longdouble)
    step = fd_steps(p)
    for j, a in enumerate(active):
        q = p.copy(); q[a] = p[a] + FD_STEP * p[a]
        g[:, j] = (GL.expK_rows(K, q, x)[0] - f0) / np.longdouble(step[a])
    return f0, g


def expK_fd_bound(K, pars, x, w, active):
    """eps S_i w_i / |step_j| with S_i = |p_2K| + sum_k |a_k| exp(-x_i / tau_k): the size of one rounding error of f, which is a sum of
    that many positive terms, after the division by the step.  [n][len(active)] in double"""
    p = np.asarray(pars, dtype=np.float64)
    S = np.full(np.size(x), abs(p[2 * K]))
    for k in range(K):
        S += abs(p[2 * k]) * np.exp(-np.asarray(x) / p[2 * k + 1])
    return np.finfo(np.float64).eps * (S * np.asarray(w))[:, None] / np.abs(fd_steps(p)[list(active)])[None, :]


# The device's forward-difference Jacobian against the longdouble forward difference, entry by entry in units of expK_fd_bound.
# tests/test_cpu_gram_option_cases.py measures the oracle's own distance C_ref in these units over the D3 cases; the device is held to
# 4 C_ref: gfh_exp is good to 3 ulp where libm's exp is to less than 1, and the device contracts a * e + y into one rounding.
FD_C_REF = 1.96                   # [C_ref = 1.9577 over the D3 cases, 1.37 ... 1.96 per case: test_fd_oracle_against_longdouble_forward_differences]
FD_DEVICE_FACTOR = 4.0


# ---- D4: fits under a loss on the matrix-core forms ---------------------------------------------------------------------------------
D4_FIT_ACC = dict(lambda_=1.0, accth=0.9, max_iter=4)
D4_FIT_PLAIN = dict(lambda_=1.0, max_iter=4)


def d4():
    """gaussK(8): 32 active per dataset, tail; gaussK(24): 96 active per dataset, cooperative, chain"""
    return [Opt('D4', GL.b5(K), CAUCHY, fits=(D4_FIT_ACC, D4_FIT_PLAIN), fit_tol=tol) for K, tol in ((8, TOL_FIT), (24, TOL_FIT_LOSS_96))]


D4_IMAGES = (2, 3, 8, 64)         # the oracle's sums cut into that many images: a perturbation of J^T J at the level of its rounding


def all_cases():
    return d1() + d2() + d3() + d4()


def units():
    """[(tape, active list, n_datasets, store the Jacobian?, loss, use_ad)]: every distinct translation unit the cases ask for.  The
    loss and use_ad are part of the generated source, so each has units of its own: D1 2 losses x (6 fused forms x 2 + 1), D2 2 x 2 (B2
    and B3 of a form share the by-pointer unit), D3 3 + 1, D4 2 x 2 (a mode-0 or plain mode-2 fit runs the sweep without the store)"""
    seen, out = set(), []
    for o in all_cases():
        c = o.case
        key = (c.model, c.K, tuple(c.active), c.kernarg, o.loss, o.use_ad)
        if key in seen:
            continue
        seen.add(key)
        if not o.use_ad:
            stores = (True, False) if c.na in D3_NO_STORE else (True,)
        else:
            stores = (True, False) if c.fused else (True,)
        out += [(c.tape(), c.active, c.nd, store, o.loss, o.use_ad) for store in stores]
    return out
