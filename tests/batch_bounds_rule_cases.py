"""The statement of the tests of THE RULE of gfh_k_fit_batch_bounded (device/batch_fit_bounded.hip; DESIGN section 3a, Bounds of a
batch): the kernel's loop restated over the reference's passes, the cases that exercise each of its five rules, and the rule that
selects which fits a device fit may be held against count for count.  tests/test_cpu_batch_bounds_rule.py runs everything here by
the reference alone; tests/test_gpu_batch_bounds_rule.py holds the device to it.  Everything is deterministic and needs no GPU, and
nothing a device returns enters a rule of this module.

THE RESTATED LOOP (restated_bounded_fit) is the kernel line for line:
  passes   least squares: OracleProblem.sweep(n_images, want_J=True), .chi2(n_images), .omega; under a loss the same with loss= and the
           weights w / c (tests/batch_loss_cases.py), the plain chi2 wherever chi2 is compared and the loss-scaled J^T r in the pin;
           under the Poisson estimator batch_mle_cases.reference_pass and deviance, the first deviance NaN ending with reason 8.
  rule 1   pin from the exact comparisons P_j == lower_j and J^T r_j < 0, P_j == upper_j and J^T r_j > 0, once per iteration behind the
           DTD update, used by every solve of the iteration.
  rule 2   orc.potr on the free rows and columns of A + lambda diag(DTD), delta_j = 0 for a pinned j; the pinned diagonals A_jj +
           lambda DTD_j must be > 0 and finite as the kernel's `ok` wants them; a failed factorisation is exit 8.
  rule 3   P + delta1 + delta2 / 2 and every retrial old + delta1 are clamped per coordinate.
  rule 4   a coordinate whose accepted value equals a bound does not hold the rel_error exit open; delta1 is the last solve's.
  rule 5   at_bound from the returned parameters.
It returns a Fit: the counts in batch_common.COUNTS order, the parameters, lambda, chi2 (D under the estimator), at_bound, FOUR
MARGINS and an EVENT RECORD.  The margins are each the minimum over the fit of a relative distance of a data-dependent decision from
its threshold:
  accept   |new - old| / old over every comparison of STEP 4;
  pin      |J^T r_j| / sqrt(A_jj chi2) for every coordinate that sits on a wall at the top of an iteration;
  clamp    |v_j - wall_j| / max(|wall_j|, |v_j|) over every unclamped trial point v and every finite wall with v_j != wall_j (a
           coordinate with delta_j = 0 exactly that sits on its wall has no clamp decision; one that lands on the wall by rounding
           has margin 0);
  exit     |value - threshold| / |threshold| of every chi2_abs, chi2_rel, rel_error (over the coordinates that are not exempt) and
           acc_ratio test, fired or not.
The events: iterations with a non-empty pin; iterations in which a bit pinned in the iteration before is clear (a release); first
trials clamped; retrials clamped; the largest popcount of pin; whether rule 4's exemption decided the exit (reason 5 that the
unexempted test would not have given); and the union of all pins.

THE SELECTION RULE (select) is run by the reference alone.  A fit is KEPT when over three evaluations -- n_images = 1, n_images = 3,
and n_images = 1 with the points reversed -- the counts, at_bound and the event records are equal, the parameters agree within SELF_TOL
= TOL_FIT / 10, and accept > TOL_PASS, pin > 1e-9, clamp > 1e-9, exit > 1e-3; under the estimator every deviance is RESOLVED as in
tests/batch_mle_cases.py.  The thresholds are conditions in the sense of batch_cases.MARGIN: they say which decisions two
implementations held to TOL_PASS per pass can be expected to share.  At most one fit in five of a case may be dropped (CAP), per case
and per lane form's sub-list.

THE ALTERED RULES.  _alter= applies one change to the REFERENCE (never to device code; nothing altered runs on a card):
  M1 pin regardless of the sign of J^T r       M2 retrial solves unpinned            M3 retrials not clamped
  M4 no exemption in rule 4                    M5 delta2 solved unpinned             M6 a pin, once set, kept for the rest of the fit
  M7 first trial not clamped                   M8 the retrial's pin recomputed from the rejected trial point
  M9 at_bound from the last pinned set instead of the position
The unaltered fit records in `touched` which changes could have acted at all (M2: a retrial with a non-empty pin, ...): an altered
fit whose change was never touched performs the unaltered fit's operations and is not evaluated again.

THE CASES: the table CASES below; what each is there for is its `covers` line, asserted on a quarter of its kept fits."""
import functools

import numpy as np

from oracle import binding as orc
from tests import batch_bounds_cases as BB
from tests import batch_loss_cases as LC
from tests import batch_mle_cases as MC
from tests.batch_common import SCENARIOS, TOL_FIT, TOL_PASS, start_of

SELF_TOL = TOL_FIT / 10
ACCEPT_MARGIN = TOL_PASS
PIN_MARGIN = 1e-9
CLAMP_MARGIN = 1e-9
EXIT_MARGIN = 1e-3
CAP = 0.2
ALTERED = ('M1', 'M2', 'M3', 'M4', 'M5', 'M6', 'M7', 'M8', 'M9')
NOTICED_MIN = 8
INF = float('inf')
ACTIVE = [0, 1, 2, 3]


# ---- the passes ------------------------------------------------------------------------------------------------------------------------
class _Squares:
    """the reference's least-squares passes, under a loss with the weights w / c; sums and chi2 in the oracle's units (1 / c^2 times the
    device's: every ratio the loop forms commutes with the factor)"""

    def __init__(self, tape, x, y, w, start, active, n_images, loss, scale):
        self.p = orc.OracleProblem(tape, [x], [y], [w / scale], [start], list(active), [0] * tape.n_pars, loss=loss)
        self.n_images, self.units = n_images, scale * scale
        self.JT = None

    def chi2(self, P):
        self.p.pars[0, :] = P
        return self.p.chi2(self.n_images)[0], 0.0

    def sweep(self, P):
        self.p.pars[0, :] = P
        A, b, _, self.JT = self.p.sweep(self.n_images, want_J=True)
        return A, b

    def omega(self, P, delta1):
        self.p.pars[0, :] = P
        return self.p.omega(delta1, self.JT)[1]


class _Poisson:
    """batch_mle_cases' reference pass and deviance; chi2() returns (D, bound / D)"""

    def __init__(self, tape, x, y, m, active, n_images):
        self.a = (tape, x, y, m)
        self.active, self.n_images, self.units = list(active), n_images, 1.0

    def chi2(self, P):
        D, bound = MC.deviance(*self.a, P)
        return D, (bound / D if D == D else 0.0)

    def sweep(self, P):
        A, b, _, _ = MC.reference_pass(*self.a, P, self.active, self.n_images)
        return A, b

    def omega(self, P, delta1):
        raise ValueError('the estimator refuses accth')


def _solve_pinned(A, DTD, lam, rhs, pin):
    """rule 2: the reduced system by orc.potr, delta_j = 0 for the pinned j; None where the kernel's `ok` is false"""
    na = rhs.size
    Ad = A + lam * np.diag(DTD)
    d = np.diag(Ad)
    if not (np.all(d > 0.0) and np.all(d < INF)):
        return None
    free = [j for j in range(na) if not (pin >> j) & 1]
    out = np.zeros(na)
    if not free:
        return out
    sub, b = Ad[np.ix_(free, free)], rhs[free]
    if not (np.all(np.isfinite(sub)) and np.all(np.isfinite(b))):
        return None
    try:
        out[free] = orc.potr(sub, b)
    except Exception:
        return None
    return out if np.all(np.isfinite(out)) else None


def _dtd(a, DTD, b):
    s = 0.0
    for i in range(a.size):
        s += a[i] * (DTD[i] * b[i])
    return s


def _pin_of(Pa, b, lo, hi, always=False):
    pin = 0
    for j in range(Pa.size):
        if always:
            hit = Pa[j] == lo[j] or Pa[j] == hi[j]
        else:
            hit = (Pa[j] == lo[j] and b[j] < 0.0) or (Pa[j] == hi[j] and b[j] > 0.0)
        pin |= (1 << j) if hit else 0
    return pin


def _at_bound(Pa, lo, hi):
    at = 0
    for j in range(Pa.size):
        at |= (1 << j if Pa[j] == lo[j] else 0) | (1 << (8 + j) if Pa[j] == hi[j] else 0)
    return at


class Fit:
    """what restated_bounded_fit returns"""
    __slots__ = ('counts', 'pars', 'lam', 'chi2', 'at_bound', 'accept', 'pin', 'clamp', 'exit', 'unresolved', 'events', 'touched')

    def margins(self):
        return (self.accept, self.pin, self.clamp, self.exit)

    def record(self):
        """(counts, parameters, lambda, chi2) as batch_common.fit_worst reads a selection's fit"""
        return self.counts, self.pars, self.lam, self.chi2


EVENTS = ('pinned_iterations', 'releases', 'first_clamped', 'retrials_clamped', 'popcount', 'exempted', 'pinned_bits')


def restated_bounded_fit(tape, x, y, w, start, active, lower, upper, kw, n_images=1, loss=0, scale=1.0, estimator=0, _alter=None):
    """gfh_k_fit_batch_bounded over the reference's passes: see the module's text"""
    assert _alter is None or _alter in ALTERED
    active = list(active)
    na = len(active)
    lo, hi = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    lam, lam_up, lam_down, lam_incs = float(kw.get('lambda_', 1.0)), float(kw.get('lam_up', 10.0)), float(kw.get('lam_down', 10.0)), int(kw.get('lam_incs', 2))
    accth = kw.get('accth')
    P = np.array(start, dtype=np.float64)
    if estimator:
        assert loss == 0 and accth is None
        ps = _Poisson(tape, x, y, w, active, n_images)
    else:
        ps = _Squares(tape, x, y, w, P, active, n_images, loss, scale)
    old = P[active].copy()
    DTD = np.zeros(na)
    dof_ = int(x.size) - na
    dof = 1.0 if dof_ == 0 else float(dof_)
    m = dict(accept=INF, pin=INF, clamp=INF, exit=INF)
    ev = dict.fromkeys(EVENTS, 0)
    touched = set()

    def near(key, value, thr):
        d = abs(value - thr) / abs(thr)
        if not d >= m[key]:
            m[key] = float(d)

    def clamp(v, delta, on):
        """rule 3 on the unclamped trial v = base + delta, with its margin; `on`: whether the clamp is applied"""
        for j in range(na):
            for wall in (lo[j], hi[j]):
                if np.isfinite(wall) and not (delta[j] == 0.0 and v[j] == wall):
                    d = abs(v[j] - wall) / max(abs(wall), abs(v[j])) if v[j] != wall else 0.0
                    if not d >= m['clamp']:
                        m['clamp'] = float(d)
        c = np.where(v < lo, lo, np.where(v > hi, hi, v))
        changed = bool(np.any((c != v) & (v == v)))
        return (c if on else v), changed

    old_chi2, unresolved = ps.chi2(P)
    it, n_sweeps, n_chi2, n_omega, reason = 0, 0, 1, 0, -1
    if estimator and old_chi2 != old_chi2:
        reason = 8
    pin, sticky, prev_pin = 0, 0, 0
    delta1 = np.zeros(na)
    while reason < 0:
        A, b = ps.sweep(P)
        n_sweeps += 1
        DTD = np.maximum(DTD, np.diag(A))
        for j in range(na):                                                                   # rule 1
            if P[active[j]] == lo[j] or P[active[j]] == hi[j]:
                d = abs(b[j]) / np.sqrt(A[j, j] * old_chi2)
                if not d >= m['pin']:
                    m['pin'] = float(d)
        pin = _pin_of(P[active], b, lo, hi)
        if _pin_of(P[active], b, lo, hi, always=True) != pin:
            touched.add('M1')
        if _alter == 'M1':
            pin = _pin_of(P[active], b, lo, hi, always=True)
        if sticky & ~pin:
            touched.add('M6')
        if _alter == 'M6':
            pin |= sticky
        sticky |= pin
        ev['pinned_iterations'] += 1 if pin else 0
        ev['releases'] += 1 if prev_pin & ~pin else 0
        ev['popcount'] = max(ev['popcount'], bin(pin).count('1'))
        ev['pinned_bits'] |= pin
        prev_pin = pin
        delta1 = _solve_pinned(A, DTD, lam, b, pin)                                            # rule 2
        if delta1 is None:
            reason = 8
            break
        delta2 = np.zeros(na)
        if accth is not None:                                                                 # STEP 3
            JTo = ps.omega(P, delta1)
            n_omega += 1
            if pin:
                touched.add('M5')
            delta2 = _solve_pinned(A, DTD, lam, JTo, 0 if _alter == 'M5' else pin)
            if delta2 is None:
                reason = 8
                break
            acc_ratio = np.sqrt(_dtd(delta2, DTD, delta2) / _dtd(delta1, DTD, delta1))
            near('exit', acc_ratio, float(accth))
            if acc_ratio > accth:
                delta2 = np.zeros(na)
        step = delta1 + 0.5 * delta2
        v, changed = clamp(P[active] + delta1 + 0.5 * delta2, step, _alter != 'M7')          # rule 3
        if changed:
            ev['first_clamped'] += 1
            touched.add('M7')
        P[active] = v
        new_chi2 = 0.0
        for i in range(1, lam_incs + 2):                                                      # STEP 4
            new_chi2, u = ps.chi2(P)
            n_chi2 += 1
            if new_chi2 == new_chi2:
                near('accept', new_chi2, old_chi2)
                unresolved = max(unresolved, u)
            if new_chi2 < old_chi2:
                lam = lam / lam_down
                break
            elif i <= lam_incs:
                lam = lam_up * lam
                at_trial = _pin_of(P[active], b, lo, hi)
                P[active] = old
                if pin:
                    touched.add('M2')
                if at_trial != pin:
                    touched.add('M8')
                delta1 = _solve_pinned(A, DTD, lam, b, 0 if _alter == 'M2' else at_trial if _alter == 'M8' else pin)
                if delta1 is None:
                    reason = 8
                    break
                v, changed = clamp(P[active] + delta1, delta1, _alter != 'M3')
                if changed:
                    ev['retrials_clamped'] += 1
                    touched.add('M3')
                P[active] = v
            else:
                P[active] = old
                reason = 7
                break
        if reason >= 0:
            break
        old = P[active].copy()
        old_old, old_chi2 = old_chi2, min(old_chi2, new_chi2)
        it += 1
        if 'chi2_abs' in kw:                                                                  # STEP 5
            near('exit', old_chi2 * ps.units / dof, float(kw['chi2_abs']))
            if old_chi2 * ps.units / dof < kw['chi2_abs']:
                reason = 1
                break
        if 'chi2_rel' in kw:
            near('exit', (old_old - old_chi2) / old_chi2, float(kw['chi2_rel']))
            if (old_old - old_chi2) / old_chi2 < kw['chi2_rel']:
                reason = 2
                break
        if 'rel_error' in kw:                                                                 # rule 4
            thr = float(kw['rel_error'])
            ruled, plain = True, True          # the kernel's `all`, and the test without the exemption
            for j in range(na):
                pj = P[active[j]]
                exempt = (pj == lo[j] or pj == hi[j]) and _alter != 'M4'
                if pj == lo[j] or pj == hi[j]:
                    touched.add('M4')
                with np.errstate(divide='ignore', invalid='ignore'):
                    r = abs(np.float64(delta1[j]) / pj)
                if not exempt:
                    near('exit', r, thr)
                plain = plain and not r > thr
                ruled = ruled and (exempt or not r > thr)
            if ruled:
                ev['exempted'] = 0 if plain else 1
                reason = 5
                break
        if 'max_iter' in kw and it >= kw['max_iter']:
            reason = 0
            break
    f = Fit()
    f.counts, f.pars, f.lam, f.chi2 = (it, n_sweeps, n_chi2, n_omega, reason), P, lam, old_chi2 * ps.units
    f.at_bound = _at_bound(P[active], lo, hi)                                                 # rule 5
    last = 0
    for j in range(na):
        if (pin >> j) & 1:
            last |= (1 << j if P[active[j]] == lo[j] else 0) | (1 << (8 + j) if P[active[j]] == hi[j] else 0)
    if last != f.at_bound:
        touched.add('M9')
    if _alter == 'M9':
        f.at_bound = last
    f.accept, f.pin, f.clamp, f.exit = m['accept'], m['pin'], m['clamp'], m['exit']
    f.unresolved, f.events, f.touched = float(unresolved), tuple(ev[k] for k in EVENTS), frozenset(touched)
    return f


def _reversed(a):
    return np.ascontiguousarray(np.asarray(a)[::-1])


def three(tape, x, y, w, start, active, lower, upper, kw, **how):
    """the three evaluations of the rule: n_images = 1, n_images = 3, n_images = 1 with the points reversed"""
    return (restated_bounded_fit(tape, x, y, w, start, active, lower, upper, kw, 1, **how),
            restated_bounded_fit(tape, x, y, w, start, active, lower, upper, kw, 3, **how),
            restated_bounded_fit(tape, _reversed(x), _reversed(y), _reversed(w), start, active, lower, upper, kw, 1, **how))


def select(tape, x, y, w, start, active, lower, upper, kw, **how):
    """the rule: (kept, (counts, parameters, lambda, chi2) of the n_images = 1 fit, the parameters' largest relative difference among
    the three evaluations, the four margins, the n_images = 1 Fit whole)"""
    one, *others = three(tape, x, y, w, start, active, lower, upper, kw, **how)
    act = list(active)
    with np.errstate(divide='ignore', invalid='ignore'):
        d = [np.abs(one.pars[act] - o.pars[act]) / np.abs(one.pars[act]) for o in others]
    diff = float(max(np.max(np.where(one.pars[act] == o.pars[act], 0.0, di)) for o, di in zip(others, d)))
    every = (one,) + tuple(others)
    margins = tuple(min(f.margins()[k] for f in every) for k in range(4))
    ok = (all(o.counts == one.counts and o.at_bound == one.at_bound and o.events == one.events for o in others) and diff <= SELF_TOL
          and margins[0] > ACCEPT_MARGIN and margins[1] > PIN_MARGIN and margins[2] > CLAMP_MARGIN and margins[3] > EXIT_MARGIN
          and (not how.get('estimator') or max(f.unresolved for f in every) <= MC.RESOLVED))
    return bool(ok), one.record(), diff, margins, one


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
LENGTHS = BB.MIXED_LENGTHS + (513,)
# the fits of a case that a lane form runs: each form's row edges (16 lanes up to 33, 64 lanes 63 / 64 / 65 / 129, 256 lanes 255 / 256 /
# 257 / 513) and what lies beside them
FORM_RANGE = {16: (16, 48), 64: (31, 257), 256: (127, 513)}
C_KW = dict(lambda_=1e-2, accth=0.9, max_iter=12)
RELEASE_KW = dict(lambda_=1e-3, max_iter=40, chi2_rel=1e-6)


def _ev(f, name):
    return f.events[EVENTS.index(name)]


COVERS = {
    'clamps then pins': lambda f: _ev(f, 'first_clamped') >= 1 and _ev(f, 'pinned_iterations') >= 1,
    'delta2 with a pinned row': lambda f: f.counts[3] >= 1 and 'M5' in f.touched,
    'release >= 1 and popcount 2': lambda f: _ev(f, 'releases') >= 1 and _ev(f, 'popcount') >= 2,
    'two pinned at once': lambda f: _ev(f, 'popcount') >= 2,
    'lower wall, at_bound bit 3': lambda f: f.at_bound == 1 << 3 and _ev(f, 'pinned_bits') & 8,
    'row 0 pinned': lambda f: _ev(f, 'pinned_bits') & 1,
    'the control: the box is mostly untouched': lambda f: True,
    'exit 5 decided by the exemption': lambda f: f.counts[4] == 5 and _ev(f, 'exempted') == 1,
    'exit 5 under rule 4': lambda f: f.counts[4] == 5 and 'M4' in f.touched,
    'pin >= 1 and clamp >= 1': lambda f: _ev(f, 'pinned_iterations') >= 1 and _ev(f, 'first_clamped') + _ev(f, 'retrials_clamped') >= 1,
}


class Case:
    """a row of the table: key, the start (exp2_starts' off, then {parameter: value} for all spectra alike), the box, the options, what it
    is there for"""

    def __init__(self, key, start, box, kw, covers, kind='lsq'):
        self.key, self.start, self.at, self.kw, self.covers, self.kind = key, start, box, dict(kw), covers, kind

    # -- what a kind fits
    def tape(self):
        return BB.tape2()

    def active(self):
        return ACTIVE

    def how(self):
        return {}

    def box(self):
        return BB.box(len(self.active()), **self.at)

    def batch(self):
        return BB.exp2_batch(LENGTHS)[1]

    def starts(self):
        s = BB.exp2_starts(self.start[0], LENGTHS).copy()
        for k, v in self.start[1].items():
            s[:, k] = v
        return s

    def form(self, lanes):
        """the indices of the case's fits that the lane form runs"""
        a, b = FORM_RANGE[lanes]
        return [k for k, n in enumerate(self.batch().n) if a <= n <= b]

    def shown(self, f):
        return bool(COVERS[self.covers](f))


class LossCase(Case):
    """batch_loss_cases Part A (model_exp4, its 48 spectra): every form runs every fit"""

    def __init__(self, key, loss, start, box, kw, covers):
        Case.__init__(self, key, start, box, kw, covers, kind=LC.LOSS_NAMES[loss])
        self.loss = loss

    def tape(self):
        return LC.part_a()[0]

    def active(self):
        return LC.SETS[7]

    def how(self):
        return dict(loss=self.loss, scale=LOSS_SCALE)

    def batch(self):
        return LC.part_a()[1]

    def starts(self):
        s = LC.starts_a(self.active(), 'conv').copy()
        s[:, self.start[0]] = self.start[1]
        return s

    def form(self, lanes):
        return list(range(len(self.batch().items)))


class PoissonCase(Case):
    """batch_mle_cases.batch() in the 'high' regime"""

    def __init__(self, key, start, box, kw, covers):
        Case.__init__(self, key, start, box, kw, covers, kind='poisson')

    def how(self):
        return dict(estimator=MC.POISSON)

    def batch(self):
        return _poisson_batch()[1]

    def starts(self):
        od, _, truths = MC.batch()
        s = np.array([start_of(t, self.start[0]) for (n, r), t in zip(od, truths) if r == 'high'])
        for k, v in self.start[1].items():          # a value, or (column, factor): that multiple of another column's start
            s[:, k] = s[:, v[0]] * v[1] if isinstance(v, tuple) else v
        return s

    def form(self, lanes):
        return [k for k, n in enumerate(_poisson_batch()[0]) if n in MC.FORM_LENGTHS[lanes]]


LOSS_SCALE = 1.345


@functools.lru_cache(maxsize=None)
def _poisson_batch():
    """(lengths, Batch) of the 'high' spectra of batch_mle_cases.batch(), in its order"""
    od, b, _ = MC.batch()
    keep = [k for k, (n, r) in enumerate(od) if r == 'high']
    return [od[k][0] for k in keep], BB.BC.Batch([b.items[k] for k in keep])


A_KW = SCENARIOS['a'][1]
# Every start lies inside its box: gfh_fit_batch_bounded refuses one that does not.  c_two: p[1] overshoots hi1 on the way and comes back
# (a release with two pinned at once); d_two and lo0_hi3 start p[0] just above a lower wall that lies above its truth (4.6 ... 5.1).
CASES = (
    Case('a_hi3', (0.05, {3: 15.0}), dict(hi3=20.0), A_KW, 'clamps then pins'),
    Case('c_hi3', (0.4, {3: 15.0}), dict(hi3=20.0), C_KW, 'delta2 with a pinned row'),
    Case('c_two', (0.4, {3: 15.0}), dict(hi3=20.0, hi1=1.4), C_KW, 'release >= 1 and popcount 2'),
    Case('d_two', (0.4, {0: 5.3, 3: 15.0}), dict(hi3=20.0, lo0=5.2, lo1=0.5, lo2=2.5), SCENARIOS['d'][1], 'two pinned at once'),
    Case('lo3', (0.05, {3: 45.0}), dict(lo3=35.0), A_KW, 'lower wall, at_bound bit 3'),
    Case('lo0_hi3', (0.05, {0: 5.3, 3: 15.0}), dict(lo0=5.2, hi3=20.0), A_KW, 'row 0 pinned'),
    Case('release', (0.3, {3: 40.0}), dict(hi3=40.0, hi1=2.5, lo2=0.5), RELEASE_KW, 'the control: the box is mostly untouched'),
    Case('relerr_1', (0.05, {3: 18.0}), dict(hi3=20.0), dict(lambda_=1e-2, max_iter=30, rel_error=0.1), 'exit 5 decided by the exemption'),
    Case('relerr_n', (0.0, {3: 19.9}), dict(hi3=20.0), dict(lambda_=1e-2, max_iter=30, rel_error=5e-2), 'exit 5 under rule 4'),
)
LSQ_KEYS = tuple(c.key for c in CASES)


def case(key):
    return next(c for c in ALL_CASES if c.key == key)


# the loss cases: p[2], the second amplitude of model_exp4 (truth 2.7 ... 3.3), under the wall 2.5 from a start at 2 -- a wall below
# the truth reached from inside, as a_hi3's (p[7] <= 20 from 15, the slow decay time, fails the cap on Part A under Cauchy: 36 of 48
# kept); the estimator's: a wall below the slow decay time's truth, and lower = 0 on both amplitudes from a start whose
# second component decays faster than its first (p[3] = 0.8 p[1]), so that the components change places on the way and an amplitude
# runs into its wall
POISSON_KW = dict(lambda_=1.0, max_iter=50, chi2_rel=1e-6)
LOSS_CASES = (
    LossCase('cauchy_hi2', LC.CAUCHY, (2, 2.0), dict(hi2=2.5), A_KW, 'pin >= 1 and clamp >= 1'),
    LossCase('huber_hi2', LC.HUBER, (2, 2.0), dict(hi2=2.5), A_KW, 'pin >= 1 and clamp >= 1'),
)
POISSON_CASES = (
    PoissonCase('poisson_hi3', (0.05, {3: 15.0}), dict(hi3=20.0), POISSON_KW, 'pin >= 1 and clamp >= 1'),
    PoissonCase('poisson_lo02', (0.05, {3: (1, 0.8)}), dict(lo0=0.0, lo2=0.0), POISSON_KW, 'pin >= 1 and clamp >= 1'),
)
ALL_CASES = CASES + LOSS_CASES + POISSON_CASES
KEYS = tuple(c.key for c in ALL_CASES)


@functools.lru_cache(maxsize=None)
def selection(key):
    """the rule over a case's fits, in batch order (cached: one evaluation serves the three forms)"""
    c = case(key)
    lo, hi = c.box()
    st = c.starts()
    return [select(c.tape(), x, y, w, st[k], c.active(), lo, hi, c.kw, **c.how()) for k, (x, y, w) in enumerate(c.batch().items)]


@functools.lru_cache(maxsize=None)
def altered(key, k, change):
    """fit k of a case under one altered rule (n_images = 1), or the unaltered Fit where the change was never touched"""
    c = case(key)
    one = selection(key)[k][4]
    if change not in one.touched:
        return one
    lo, hi = c.box()
    x, y, w = c.batch().items[k]
    return restated_bounded_fit(c.tape(), x, y, w, c.starts()[k], c.active(), lo, hi, c.kw, 1, _alter=change, **c.how())


def noticed(one, other, active):
    """whether an altered fit differs from the unaltered one in counts, at_bound, or parameters beyond TOL_FIT"""
    if other is one:
        return False
    if other.counts != one.counts or other.at_bound != one.at_bound:
        return True
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.where(one.pars[active] == other.pars[active], 0.0, np.abs(one.pars[active] - other.pars[active]) / np.abs(one.pars[active]))
    return bool(np.max(d) > TOL_FIT)


# ---- the cube: a_hi3's box and options on batch_bounds_cases.cube() with CUBE_WALL -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cube_selection():
    lo, hi = BB.box(4, hi3=BB.CUBE_WALL)
    st = BB.cube_starts(0.05, BB.CUBE_START)
    return [select(BB.tape2(), x, y, w, st[k], ACTIVE, lo, hi, A_KW) for k, (x, y, w) in enumerate(BB.cube_items())]
