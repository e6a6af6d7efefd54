"""Procedural driver API -- mirror of the reference's ``module gadfit``
(fortran/gadfit/gadfit.F90:41-58): gadf_init, gadf_add_dataset, gadf_set, gadf_set_errors,
gadf_set_verbosity, gadf_fit, gadf_print, gadf_close and the readable ``fitfuncs``.

Same names, argument meaning (1-based dataset / parameter indices, parameter names) and
error behaviour (errors raise ``GadfitError`` with the reference's message instead of
``error stop``).  All state is module-global like the reference: one fit at a time per
process.  The hot path (STEP 1-3 and chi2 of gadf_fit) runs on the GPU through
libgadfit_hip.so; there is no CPU fallback.
"""
import copy
import os

import numpy as np

from . import _lib
from .fitfunction import fitfunc

NONE, SQRT_Y, PROPTO_Y, INVERSE_Y, USER = 0, 1, 2, 3, 4          # gadfit.F90:45-48
GLOBAL, LOCAL, GLOBAL_AND_LOCAL = 0, 1, 2
GAUSS_KRONROD_15P, GAUSS_KRONROD_21P, GAUSS_KRONROD_31P = 15, 21, 31
GAUSS_KRONROD_41P, GAUSS_KRONROD_51P, GAUSS_KRONROD_61P = 41, 51, 61


class GadfitError(RuntimeError):
    pass


class _State:
    def __init__(self):
        self.reset()

    def reset(self):
        self.fitfuncs = None
        self.active = None        # per parameter: bool
        self.is_global = None
        self.datasets = []        # (x, y, weights-or-None)
        self.n_datasets = 0
        self.error_type = NONE
        self.ctx = None
        self.tape = None
        self.uploaded = False
        self.set_count = 0
        self.verbosity = 0
        self.iterations = 0
        self.last_result = None
        self.umnigh_a = 0.5
        self.integration = {}
        self.device = 0
        self.comm = None
        self.loss = 0
        self.lb_on = False


_S = _State()
fitfuncs = None   # rebound by gadf_init (gadfit.F90:64)


def _need_init():
    if _S.fitfuncs is None:
        raise GadfitError('Number of datasets is undetermined. Call gadf_init first.')


def gadf_init(f, num_datasets=1, sweep_size=None, trace_size=None, const_size=None, ws_size=None,
              ws_size_inner=None, integration_rule=None, ad_memory=None, rel_error_inner=None, rel_error=None,
              device=None, comm=None):
    """gadfit.F90:133-184.  The AD tape-size arguments are accepted and ignored: the tape is
    recorded once per model, not per point; the quadrature workspace sizes are honoured on the device.  ``device``: HIP device index (default
    LOCAL_RANK or 0); ``comm``: (nranks, rank, unique_id) to shard over several GPUs."""
    global fitfuncs
    if not isinstance(f, fitfunc):
        raise GadfitError('f must extend fitfunc')
    _S.reset()
    _S.fitfuncs = []
    for _ in range(num_datasets):
        g = copy.copy(f)
        g.init()
        _S.fitfuncs.append(g)
    fitfuncs = _S.fitfuncs
    n = len(_S.fitfuncs[0].pars)
    _S.active = [False] * n
    _S.is_global = [False] * n
    _S.n_datasets = num_datasets
    _S.integration = dict(rel_error=rel_error, rel_error_inner=rel_error_inner, rule=integration_rule,
                          dbl=(rel_error_inner is not None or ws_size_inner is not None),
                          ws_size=ws_size, ws_size_inner=ws_size_inner)        # workspace sizes travel with the tape (NI:114-135)
    _S.device = int(os.environ.get('LOCAL_RANK', '0')) if device is None else device
    _S.comm = comm


def gadf_add_dataset(*args):
    """gadf_add_dataset(path) | gadf_add_dataset(x_data, y_data [, weights]) (gadfit.F90:189-246)."""
    _need_init()
    if len(_S.datasets) >= _S.n_datasets:
        raise GadfitError('Too many calls to gadf_add_dataset (%d/%d).' % (len(_S.datasets) + 1, _S.n_datasets))
    if len(args) == 1 and isinstance(args[0], str):
        # read_data (gadfit.F90:212-215, 422-437) through the library's reader (reader.cpp): records that do not begin with a number
        # are skipped; three columns if every record has them (the third is used under USER errors), else two
        if not os.path.exists(args[0]):
            raise GadfitError('Cannot open ' + args[0])
        try:
            x, y, w = _lib.read_columns(args[0], 3)
        except _lib.GadfitHipError:
            try:
                x, y = _lib.read_columns(args[0], 2); w = None
            except _lib.GadfitHipError as e:
                raise GadfitError(str(e))
        if x.size == 0:
            raise GadfitError(args[0] + ' contains no valid data points.')
        _S.datasets.append((x, y, w))
    else:
        x = np.asarray(args[0], dtype=np.float64); y = np.asarray(args[1], dtype=np.float64)
        w = np.asarray(args[2], dtype=np.float64) if len(args) > 2 and args[2] is not None else None
        _S.datasets.append((x, y, w))
    _S.uploaded = False


def gadf_set(*args):
    """gadf_set(dataset_i, par, val [, active]) (local) | gadf_set(par, val [, active]) (global);
    par is a 1-based index or a name (8 specifics of gadfit.F90:54-58, 255-342)."""
    _need_init()
    a = list(args)
    active = False
    if isinstance(a[-1], (bool, np.bool_)):
        active = bool(a.pop())
    if len(a) == 3:
        ds, par, val = a
        if ds > len(_S.fitfuncs):
            raise GadfitError('Invalid dataset index. Call gadf_init with the correct number of datasets.')
        i = _S.fitfuncs[0].get_index(par) if isinstance(par, str) else int(par)
        _S.is_global[i - 1] = False
        _S.fitfuncs[ds - 1].set(i, float(val))
        _S.active[i - 1] = active
        _S.set_count += 1
    elif len(a) == 2:
        par, val = a
        i = _S.fitfuncs[0].get_index(par) if isinstance(par, str) else int(par)
        for g in _S.fitfuncs:
            g.set(i, float(val))
            _S.set_count += 1
        _S.active[i - 1] = active
        _S.is_global[i - 1] = True
    else:
        raise GadfitError('gadf_set: wrong number of arguments')


def gadf_set_errors(e):
    _need_init()
    _S.error_type = e     # gadfit.F90:392-395


LOSS_LINEAR, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2


def gadf_set_loss(loss):
    """Robust cost function -- the C++ solver's `settings.loss` (c++/gadfit/lm_solver.h:76-83, 208); the
    Fortran reference has no such switch.  Applies to the fits that follow."""
    _need_init()
    if loss not in (LOSS_LINEAR, LOSS_CAUCHY, LOSS_HUBER):
        raise GadfitError('gadf_set_loss: unknown loss function')
    _S.loss = loss


def gadf_set_verbosity(scope=None, digits=None, timings=None, memory=None, workloads=None, delta1=None, delta2=None,
                       cos_phi=None, grad_chi2=None, uphill=None, acc=None, output=None):
    """gadfit.F90:356-385; only on/off of the per-iteration log is honoured."""
    _S.verbosity = 0 if output in ('/dev/null', os.devnull) else 1


RECORD_SAMPLE = 2048       # abscissas per dataset at which a branching eval() is recorded before the fit


def _ensure_device():
    if len(_S.datasets) != _S.n_datasets:        # read_data, gadfit.F90:403-405 (checked before touching the device)
        raise GadfitError('Some datasets are missing. gadf_add_dataset must be called %d times.' % _S.n_datasets)
    if _S.ctx is None:
        _S.ctx = _lib.Context(_S.device)
        if 'GADFIT_HIP_KEEP_J' not in os.environ:
            # the Jacobian has no reader behind this API (private in the reference): written only for the fits whose
            # options read it back; same J^T J / J^T r / chi2 bit for bit (gfh_set_keep_jacobian mode 2)
            _S.ctx.set_keep_jacobian(2)
        if _S.comm is not None:
            _S.ctx.comm_init(*_S.comm)
    if _S.tape is not None and not _tape_is_current():
        _S.tape = None                    # eval() has changed since it was recorded (a global it reads): record it again
    if _S.tape is None:
        ig = _S.integration
        configure = None
        if ig.get('dbl') or ig.get('rel_error') is not None or ig.get('rule') is not None or ig.get('ws_size') is not None:
            def configure(t):
                t.set_integration(rel_error=ig['rel_error'], rel_error_inner=ig['rel_error_inner'], rule=ig['rule'],
                                  dbl=ig['dbl'], ws_size=ig.get('ws_size'), ws_size_inner=ig.get('ws_size_inner'))
        try:
            _S.tape = _S.fitfuncs[0].trace()
            if configure is not None:
                configure(_S.tape)
        except TypeError as e:
            if 'eval() branches' not in str(e) and 'comparison inside an integrand' not in str(e):
                raise
            # eval() compares AD variables: one tape per path (gfh_set_model_variants).  Recorded over the data at the current
            # parameter values -- first, last and up to RECORD_SAMPLE evenly spaced abscissas of every dataset; a path the sample
            # misses, or one that only appears once the parameters have moved, is reported by the device during the fit and
            # recorded then (the handler _lib.Context.set_model installs)
            _S.tape = _S.fitfuncs[0].trace_variants(configure)
            for d, f in enumerate(_S.fitfuncs):
                x = np.asarray(_S.datasets[d][0], dtype=np.float64)
                if x.size == 0:
                    continue
                idx = np.unique(np.concatenate([[0, x.size - 1], np.linspace(0, x.size - 1, min(x.size, RECORD_SAMPLE)).astype(np.int64)]))
                _S.tape.explore(x[idx], [p.val for p in f.pars])
            if len(_S.tape) == 0:
                raise GadfitError('There are no data points.')
        _S.ctx.set_model(_S.tape)
    if not _S.uploaded:
        if len(_S.datasets) != _S.n_datasets:
            raise GadfitError('Some datasets are missing. gadf_add_dataset must be called %d times.' % _S.n_datasets)
        xs = np.concatenate([d[0] for d in _S.datasets]); ys = np.concatenate([d[1] for d in _S.datasets])
        if _S.error_type == USER:
            if any(d[2] is None for d in _S.datasets):
                raise GadfitError('USER errors requested but a dataset has no weights column')
            ws = np.concatenate([d[2] for d in _S.datasets])
        else:
            ws = np.ones_like(xs)
        pos = np.zeros(_S.n_datasets + 1, dtype=np.int64)
        for i, d in enumerate(_S.datasets):
            pos[i + 1] = pos[i] + len(d[0])
        _S.ctx.set_data(xs, ys, ws, pos)
        _S.ctx.init_weights(_S.error_type)     # init_weights on the device (gadfit.F90:445-470)
        _S.uploaded = True


def _f32(v):
    return None if v is None else float(np.float32(v))   # the first ten arguments are real(real32)


def _tape_is_current():
    """a later gadf_fit: is the recorded model still what eval() does?  (the reference calls eval() afresh at every point of every
    fit, gadfit.F90:679-690: a global the model reads and the program changed between two fits takes effect in the second)"""
    try:
        if hasattr(_S.tape, 'is_current'):
            return _S.tape.is_current([p.val for p in _S.fitfuncs[0].pars])
        return _S.fitfuncs[0].trace().signature()[0] == _S.tape.signature()[0]
    except TypeError:
        return False


def gadf_fit(lambda_=None, lam_up=None, lam_down=None, accth=None, grad_chi2=None, cos_phi=None, rel_error=None,
             rel_error_global=None, chi2_rel=None, chi2_abs=None, DTD_min=None, lam_incs=None, uphill=None,
             max_iter=None, damp_max=None, nielsen=None, umnigh=None, load_balancing=None, use_ad=None, **kw):
    """gadfit.F90:502-1035.  ``lambda`` is spelled ``lambda_`` (also accepted through **kw)."""
    _need_init()
    if 'lambda' in kw:
        lambda_ = kw.pop('lambda')
    if kw:
        raise GadfitError('gadf_fit: unknown arguments %s' % sorted(kw))
    active = [i for i, a in enumerate(_S.active) if a]
    if not active:
        raise GadfitError('There are no active parameters.')
    _ensure_device()
    _S.ctx.set_loss(_S.loss)
    if bool(load_balancing) != _S.lb_on:                # adaptive parallelism: the library copies the data when they are set
        _S.ctx.set_load_balancing(bool(load_balancing)); _S.lb_on = bool(load_balancing)
        if _S.lb_on:
            _S.uploaded = False
            _ensure_device()
    _S.ctx.set_use_ad(use_ad is None or bool(use_ad))      # gadfit.F90:583-584; False: fitfunction.F90:155-203 on the device
    pars = np.array([[p.val for p in g.pars] for g in _S.fitfuncs])
    out, r = _S.ctx.fit(pars, active, [int(g) for g in _S.is_global], DTD_min=DTD_min, verbosity=_S.verbosity,
                        umnigh_a=_S.umnigh_a,
                        lambda_=_f32(lambda_), lam_up=_f32(lam_up), lam_down=_f32(lam_down), accth=_f32(accth),
                        grad_chi2=_f32(grad_chi2), cos_phi=_f32(cos_phi), rel_error=_f32(rel_error),
                        rel_error_global=_f32(rel_error_global), chi2_rel=_f32(chi2_rel), chi2_abs=_f32(chi2_abs),
                        lam_incs=lam_incs, uphill=uphill, max_iter=max_iter,
                        damp_max=None if damp_max is None else int(damp_max),
                        nielsen=None if nielsen is None else int(nielsen),
                        umnigh=None if umnigh is None else int(umnigh))
    _S.umnigh_a = _S.ctx.umnigh_a
    for g, row in zip(_S.fitfuncs, out):
        for p, v in zip(g.pars, row):
            p.val = float(v)
    _S.iterations = r.iterations
    _S.last_result = r
    return r


def _batch_context(who):
    """the session's context with its model current, for a batch call (gadf_fit_batch, gadf_fit_cube, gadf_fit_frames)"""
    if _S.ctx is None:
        _S.ctx = _lib.Context(_S.device)
        if 'GADFIT_HIP_KEEP_J' not in os.environ:
            _S.ctx.set_keep_jacobian(2)       # (as _ensure_device: a gadf_fit of this session may follow)
    if _S.tape is None or not _tape_is_current():
        try:
            _S.tape = _S.fitfuncs[0].trace()
        except TypeError as e:
            raise GadfitError('%s: %s' % (who, e))
        _S.ctx.set_model(_S.tape)
        _S.uploaded = False
    _S.ctx.set_loss(_S.loss)
    _S.ctx.set_use_ad(True)


_BATCH_ERRORS = {None: None, 'unscaled': False, 'scaled': True}


def _batch_errors(who, errors):
    """the ``errors`` argument of the batch calls: None (no error outputs), else batch_covariance's scale"""
    if not (errors is None or isinstance(errors, str)) or errors not in _BATCH_ERRORS:
        raise GadfitError("%s: errors must be None, 'unscaled' (the inverse of J^T J) or 'scaled' (that times chi2 / dof), got %r" % (who, errors))
    return _BATCH_ERRORS[errors]


def _batch_bounds(who, bounds, errors):
    """the ``bounds`` argument of the batch calls: None, or (lower, upper), each one number per active parameter in the order of the
    active set gadf_set left, None or -inf / +inf for no bound on that side; returned as two float64 arrays"""
    if bounds is None:
        return None
    if errors is not None:
        raise GadfitError('%s: bounds together with errors= is not carried in this version (the covariance of a fit with pinned parameters is '
                          'that of its free ones only, and the pinned set differs from fit to fit); call batch_covariance afterwards' % who)
    na = sum(1 for a in _S.active if a)
    try:
        lower, upper = bounds
        lower = np.array([-np.inf if v is None else v for v in lower], dtype=np.float64)
        upper = np.array([np.inf if v is None else v for v in upper], dtype=np.float64)
    except (TypeError, ValueError):
        raise GadfitError('%s: bounds must be (lower, upper), each a sequence of one number (or None) per active parameter' % who)
    if lower.shape != (na,) or upper.shape != (na,):
        raise GadfitError('%s: bounds must hold one lower and one upper value per active parameter (%d), got %d and %d'
                          % (who, na, lower.size, upper.size))
    return lower, upper


def _batch_loss(who, loss, loss_scale):
    """the ``loss`` and ``loss_scale`` arguments of the batch calls as set_batch_loss takes them: None is the linear loss and scale 1, so
    that every call sets the batch loss itself and nothing stays behind from an earlier one"""
    loss = LOSS_LINEAR if loss is None else loss
    if isinstance(loss, bool) or not isinstance(loss, (int, np.integer)) or loss not in (LOSS_LINEAR, LOSS_CAUCHY, LOSS_HUBER):
        raise GadfitError('%s: loss must be None, LOSS_LINEAR, LOSS_CAUCHY or LOSS_HUBER, got %r' % (who, loss))
    scale = 1.0 if loss_scale is None else loss_scale
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not (np.isfinite(scale) and scale > 0):
        raise GadfitError('%s: loss_scale must be a finite number > 0 (the weighted residual at which the loss switches), got %r' % (who, loss_scale))
    return int(loss), float(scale)


def _batch_estimator(who, estimator):
    """the ``estimator`` argument of the batch calls as set_batch_estimator takes it: None is least squares, so that every call sets
    the estimator itself and nothing stays behind from an earlier one"""
    if estimator is None:
        return 0
    if isinstance(estimator, bool) or estimator not in (0, 1, 'lsq', 'poisson'):
        raise GadfitError("%s: estimator must be None, 0 or 'lsq' (least squares), 1 or 'poisson', got %r" % (who, estimator))
    return {'lsq': 0, 'poisson': 1}.get(estimator, estimator) if isinstance(estimator, str) else int(estimator)


def _batch_fit(pars, active, scale, bounds, **kw):
    """fit_batch, fit_batch_errors under errors= or fit_batch_bounded under bounds=: what the batch calls return"""
    if bounds is not None:
        out, res, at, _ = _S.ctx.fit_batch_bounded(pars, active, bounds[0], bounds[1], **kw)
        return out, res, dict(at_bound=at)
    if scale is None:
        out, res, _ = _S.ctx.fit_batch(pars, active, **kw)
        return out, res
    out, res, (cov, sigma, info), _ = _S.ctx.fit_batch_errors(pars, active, scale=scale, **kw)
    return out, res, dict(cov=cov, sigma=sigma, info=info)


def gadf_fit_batch(xs, ys, ws, pars, lambda_=None, lam_up=None, lam_down=None, accth=None, rel_error=None, chi2_rel=None,
                   chi2_abs=None, DTD_min=None, lam_incs=None, max_iter=None, damp_max=None, lanes_per_fit=None, errors=None, bounds=None,
                   loss=None, loss_scale=None, estimator=None, **kw):
    """Many independent fits of the session's model in one kernel launch (gfh_fit_batch): gadf_fit's loop (gadfit.F90:670-915) per
    spectrum, each with its own data, start parameters, lambda history and exit.  On a session initialised with one dataset slot
    (``gadf_init(f)``); the active set is the one ``gadf_set`` left.  ``xs, ys, ws``: one array per spectrum (``ws``: the weights as
    used in (y - f) * w; None = ones); ``pars`` [n_fits][n_pars] start values, passive entries included.  The fit arguments are
    gadf_fit's; those a device-resident loop does not carry (uphill, nielsen, umnigh, grad_chi2, cos_phi, rel_error_global) are refused
    by the library, and max_iter is required.  ``lanes_per_fit``: 64 a wave per fit, 16 a row of 16 lanes per fit and four fits per wave
    (short spectra), 256 a workgroup of four waves per fit (few, long spectra), 0 auto (16 or 64); None leaves the session's setting (64 unless set before).  Returns (parameters [n_fits][n_pars], record array of per-fit results with the fields
    iterations, exit_reason, n_sweeps, n_chi2, n_omega, dof, lambda_, chi2).  ``errors``: None, or 'unscaled' / 'scaled' for a third
    element, a dict of each fit's parameter covariance ``cov`` [n_fits][na][na] at the fitted parameters -- the inverse of J^T J, under
    'scaled' times chi2 / dof --, the standard errors ``sigma`` [n_fits][na] and ``info`` [n_fits] (0, or j + 1: pivot j of that fit's
    factor failed and its cov and sigma are NaN), computed on the device behind the fit (gfh_fit_batch_errors).  ``bounds``: None, or
    (lower, upper) -- one box for all fits, each a sequence of one number per active parameter in the order of the active set, None
    or -inf / +inf for no bound on that side: the projected loop of gfh_fit_batch_bounded, and a third element ``dict(at_bound=...)``
    [n_fits] (bit j: the returned active parameter j equals lower[j], bit 8 + j: upper[j]).  ``bounds`` with ``errors`` is refused.
    ``loss``: None or LOSS_LINEAR, LOSS_CAUCHY, LOSS_HUBER -- the batch's own robust cost (gfh_set_batch_loss), set by this call for this
    call -- and ``loss_scale`` the weighted residual |(y - f) w| at which it switches (None: 1, the reference's costs); the steps are
    accepted on the plain chi2, which is also the records'.  The session's ``gadf_set_loss`` is the plain fit's and stays refused here.
    ``estimator``: None, 0 or 'lsq' for least squares, 1 or 'poisson' for the Poisson maximum-likelihood fit of counted data
    (gfh_set_batch_estimator), set by this call for this call: the loop minimises the deviance 2 sum [f - y + y ln(y / f)] over the points
    of non-zero weight by Fisher scoring, ``ws`` is a mask and nothing more, the records' chi2 is the deviance, ``errors`` gives the
    inverse Fisher matrix ('scaled': times deviance / dof).  Refused with ``loss`` and with ``accth``."""
    _need_init()
    batch_estimator = _batch_estimator('gadf_fit_batch', estimator)
    batch_loss = _batch_loss('gadf_fit_batch', loss, loss_scale)
    scale = _batch_errors('gadf_fit_batch', errors)
    bounds = _batch_bounds('gadf_fit_batch', bounds, errors)
    if 'lambda' in kw:
        lambda_ = kw.pop('lambda')
    if _S.n_datasets != 1:
        raise GadfitError('gadf_fit_batch needs a session with one dataset slot: gadf_init(f)')
    active = [i for i, a in enumerate(_S.active) if a]
    if not active:
        raise GadfitError('There are no active parameters.')
    xs = [np.asarray(v, dtype=np.float64).ravel() for v in xs]; ys = [np.asarray(v, dtype=np.float64).ravel() for v in ys]
    ws = [np.ones_like(v) for v in xs] if ws is None else [np.asarray(v, dtype=np.float64).ravel() for v in ws]
    if not (len(xs) == len(ys) == len(ws)) or not xs or any(not (a.size == b.size == c.size) for a, b, c in zip(xs, ys, ws)):
        raise GadfitError('gadf_fit_batch: xs, ys and ws must hold one array per spectrum, of equal lengths')
    pars = np.asarray(pars, dtype=np.float64)
    if pars.shape != (len(xs), len(_S.fitfuncs[0].pars)):
        raise GadfitError('gadf_fit_batch: pars must be [n_fits][n_pars] = [%d][%d]' % (len(xs), len(_S.fitfuncs[0].pars)))
    if _S.comm is not None:
        raise GadfitError('gadf_fit_batch: the fits are independent; split the batch over the ranks instead of sharing a communicator')
    _batch_context('gadf_fit_batch')
    off = np.zeros(len(xs) + 1, dtype=np.int64)
    np.cumsum([v.size for v in xs], out=off[1:])
    try:
        _S.ctx.set_batch_data(off, np.concatenate(xs), np.concatenate(ys), np.concatenate(ws))
        return _batch_fit(pars, active, scale, bounds, DTD_min=DTD_min, lanes_per_fit=lanes_per_fit, loss=batch_loss[0], loss_scale=batch_loss[1], estimator=batch_estimator, lambda_=_f32(lambda_), lam_up=_f32(lam_up), lam_down=_f32(lam_down),
                          accth=_f32(accth), rel_error=_f32(rel_error), chi2_rel=_f32(chi2_rel), chi2_abs=_f32(chi2_abs),
                          lam_incs=lam_incs, max_iter=max_iter, damp_max=None if damp_max is None else int(damp_max),
                          **{k: v for k, v in kw.items() if v is not None})
    except _lib.GadfitHipError as e:
        raise GadfitError(str(e))


def _fit_cube(who, frames, x, Y, pars, sigma, DTD_min, lanes_per_fit, frames_per_put, errors, bounds, loss, loss_scale, estimator, kw):
    """gadf_fit_cube and gadf_fit_frames: one body, the data spectrum-major (Y [n_fits][n_points]) or frame-major (F [n_points][n_fits])"""
    _need_init()
    batch_estimator = _batch_estimator(who, estimator)
    batch_loss = _batch_loss(who, loss, loss_scale)
    scale = _batch_errors(who, errors)
    bounds = _batch_bounds(who, bounds, errors)
    if _S.n_datasets != 1:
        raise GadfitError('%s needs a session with one dataset slot: gadf_init(f)' % who)
    active = [i for i, a in enumerate(_S.active) if a]
    if not active:
        raise GadfitError('There are no active parameters.')
    x = np.asarray(x, dtype=np.float64).ravel()
    name, fits_axis = ('F', 1) if frames else ('Y', 0)
    if not isinstance(Y, np.ndarray) or Y.ndim != 2 or Y.shape[1 - fits_axis] != x.size or Y.shape[fits_axis] < 1:
        raise GadfitError('%s: F must be a numpy array [n_points][n_fits] with one row (a frame) per abscissa of x (%d)' % (who, x.size) if frames else
                          '%s: Y must be a numpy array [n_fits][n_points] with one column per abscissa of x (%d)' % (who, x.size))
    n_fits = Y.shape[fits_axis]
    if _S.error_type == USER:
        if sigma is None:
            raise GadfitError('%s: USER errors requested but no sigma was given' % who)
        sigma = np.asarray(sigma, dtype=np.float64)
        if sigma.shape != Y.shape:
            raise GadfitError('%s: sigma must have the shape of %s' % (who, name))
    elif sigma is not None:
        raise GadfitError('%s: sigma is taken under USER errors alone (gadf_set_errors)' % who)
    pars = np.asarray(pars, dtype=np.float64)
    if pars.shape != (n_fits, len(_S.fitfuncs[0].pars)):
        raise GadfitError('%s: pars must be [n_fits][n_pars] = [%d][%d]' % (who, n_fits, len(_S.fitfuncs[0].pars)))
    if _S.comm is not None:
        raise GadfitError('%s: the fits are independent; split the cube over the ranks instead of sharing a communicator' % who)
    _batch_context(who)
    try:
        if frames:
            _S.ctx.set_batch_frames(x, Y, _S.error_type, None if sigma is None else 1.0 / sigma, frames_per_put)
        else:
            _S.ctx.set_batch_cube(x, Y, _S.error_type, None if sigma is None else 1.0 / sigma)
        return _batch_fit(pars, active, scale, bounds, DTD_min=DTD_min, lanes_per_fit=lanes_per_fit, loss=batch_loss[0], loss_scale=batch_loss[1], estimator=batch_estimator, **kw)
    except _lib.GadfitHipError as e:
        raise GadfitError(str(e))


def _cube_fit_args(lambda_, lam_up, lam_down, accth, rel_error, chi2_rel, chi2_abs, lam_incs, max_iter, damp_max, kw):
    if 'lambda' in kw:
        lambda_ = kw.pop('lambda')
    return dict(lambda_=_f32(lambda_), lam_up=_f32(lam_up), lam_down=_f32(lam_down), accth=_f32(accth), rel_error=_f32(rel_error),
                chi2_rel=_f32(chi2_rel), chi2_abs=_f32(chi2_abs), lam_incs=lam_incs, max_iter=max_iter,
                damp_max=None if damp_max is None else int(damp_max), **{k: v for k, v in kw.items() if v is not None})


def gadf_fit_cube(x, Y, pars, sigma=None, lambda_=None, lam_up=None, lam_down=None, accth=None, rel_error=None, chi2_rel=None,
                  chi2_abs=None, DTD_min=None, lam_incs=None, max_iter=None, damp_max=None, lanes_per_fit=None, errors=None, bounds=None,
                  loss=None, loss_scale=None, estimator=None, **kw):
    """gadf_fit_batch over a data cube (gfh_set_batch_cube): every spectrum on the one grid ``x`` [n_points], ``Y`` [n_fits][n_points] a
    C-contiguous numpy array of float64, float32 or uint16 that is uploaded as it is.  The weights follow from ``Y`` on the device by
    the session's ``gadf_set_errors`` type (NONE, SQRT_Y, PROPTO_Y, INVERSE_Y: no weight array exists anywhere; gadf_fit_batch ignores
    that type, this call takes it); under USER ``sigma`` [n_fits][n_points] is required and 1 / sigma is passed.  ``pars``, the fit
    arguments, ``lanes_per_fit``, ``errors``, ``bounds``, ``loss``, ``loss_scale`` and what is returned are gadf_fit_batch's; the weights
    are formed on the device, so ``loss_scale`` is the one way to move a loss's threshold here.  ``estimator`` is gadf_fit_batch's: a
    cube of counts under 'poisson' wants ``gadf_set_errors(NONE)`` -- any rule works as a mask, but SQRT_Y pays a sqrt and a division
    per point for nothing."""
    return _fit_cube('gadf_fit_cube', False, x, Y, pars, sigma, DTD_min, lanes_per_fit, 0, errors, bounds, loss, loss_scale, estimator,
                     _cube_fit_args(lambda_, lam_up, lam_down, accth, rel_error, chi2_rel, chi2_abs, lam_incs, max_iter, damp_max, kw))


def gadf_fit_frames(x, F, pars, sigma=None, lambda_=None, lam_up=None, lam_down=None, accth=None, rel_error=None, chi2_rel=None,
                    chi2_abs=None, DTD_min=None, lam_incs=None, max_iter=None, damp_max=None, lanes_per_fit=None, frames_per_put=0, errors=None,
                    bounds=None, loss=None, loss_scale=None, estimator=None, **kw):
    """gadf_fit_cube for a stack of frames (gfh_set_batch_frames): ``F`` [n_points][n_fits], one image per abscissa of ``x`` with the
    fit (pixel) index fastest, as instruments deliver it -- C-contiguous in float64, float32 or uint16, uploaded as it is and
    transposed into the cube on the device, so no ``np.ascontiguousarray(F.T)`` runs on the host.  ``sigma`` (under USER) is
    frame-major as ``F``; ``frames_per_put``: frames per upload, 0 the library's rule.  Everything else, and what is returned (the
    bits included), is gadf_fit_cube's on the transposed arrays -- ``estimator`` too: a stack of counts under 'poisson' wants
    ``gadf_set_errors(NONE)``."""
    return _fit_cube('gadf_fit_frames', True, x, F, pars, sigma, DTD_min, lanes_per_fit, frames_per_put, errors, bounds, loss, loss_scale, estimator,
                     _cube_fit_args(lambda_, lam_up, lam_down, accth, rel_error, chi2_rel, chi2_abs, lam_incs, max_iter, damp_max, kw))


def gadf_batch_curves(pars, cov=None, x=None, residuals=False, first_fit=0, n_fits=None):
    """The fitted curves of the batch that the session's last gadf_fit_batch / gadf_fit_cube / gadf_fit_frames left on its context,
    computed on the device from the data held there and the session's model (gfh_batch_eval): for fits [first_fit, first_fit +
    n_fits) (``n_fits`` None: to the end of the batch) at ``pars`` [n_fits][n_pars] -- the rows of those fits, as the fit returned
    them -- with the active set ``gadf_set`` left.  Returns a dict: ``model`` f(x_i); ``residual`` (y_i - f) w_i under
    ``residuals=True``, else None; ``band``, the 1-sigma band sqrt(g^T C g) of the curve with C = ``cov`` [n_fits][na][na], what
    ``errors=`` returned (``out[2]['cov']``; its rows of those fits), else None; ``offsets`` [n_fits + 1].  ``x`` None: on the fits'
    own points -- [n_fits][n_points] after gadf_fit_cube / gadf_fit_frames, flat arrays after gadf_fit_batch, which ``offsets``
    splits.  ``x`` [n_eval]: ``model`` and ``band`` on that grid, [n_fits][n_eval]; residuals are refused there.  A fit whose
    covariance failed (``info`` != 0) has a NaN band and nothing else."""
    _need_init()
    if _S.ctx is None or getattr(_S.ctx, 'n_fits', 0) < 1:
        raise GadfitError('gadf_batch_curves: the session holds no batch (gadf_fit_batch, gadf_fit_cube or gadf_fit_frames comes first)')
    active = [i for i, a in enumerate(_S.active) if a]
    if not active:
        raise GadfitError('There are no active parameters.')
    _batch_context('gadf_batch_curves')
    try:
        model, residual, band, offsets, _ = _S.ctx.batch_eval(pars, active, cov=cov, x_eval=x, residuals=residuals, first_fit=first_fit, n_fits=n_fits)
    except _lib.GadfitHipError as e:
        raise GadfitError(str(e))
    return dict(model=model, residual=residual, band=band, offsets=offsets)


def _plain_call():
    """(context, pars [n_datasets][n_pars], active, is_global) of a call on the session's fit at its current parameters"""
    _need_init()
    active = [i for i, a in enumerate(_S.active) if a]
    if not active:
        raise GadfitError('There are no active parameters.')
    _ensure_device()
    _S.ctx.set_loss(_S.loss)
    return _S.ctx, np.array([[p.val for p in g.pars] for g in _S.fitfuncs]), active, [int(g) for g in _S.is_global]


def gadf_errors(scaled=False):
    """The parameter covariance and the standard errors of the session's fit at its current parameters -- what gadf_fit left, or
    what gadf_set set -- with the active and global sets gadf_set left, under the loss of gadf_set_loss and the use_ad of the last
    gadf_fit: (J^T J)^-1 from one sweep on the device (the reference's LMsolver::getInvJTJ; gfh_covariance), under ``scaled=True``
    times chi2 / dof.  Returns a dict: ``cov`` [dim][dim]; ``sigma`` [dim], the square roots of its diagonal; ``info``, 0, or j + 1
    where the pivot of column j failed (cov and sigma are then NaN); ``columns`` [dim], the (dataset, parameter) of every column,
    both 1-based as gadf_set takes them, the dataset 0 for a global parameter."""
    ctx, pars, active, is_global = _plain_call()
    try:
        cov, sigma, info = ctx.covariance(pars, active, is_global, scale=bool(scaled))
    except _lib.GadfitHipError as e:
        raise GadfitError(str(e))
    jac, dim = ctx.jacobian_indices(active, is_global)
    columns = [None] * dim
    for d in range(jac.shape[0]):
        for j, p in enumerate(active):
            columns[jac[d, j]] = (0 if is_global[p] else d + 1, p + 1)
    return dict(cov=cov, sigma=sigma, info=info, columns=columns)


def gadf_curves(cov=None, x=None, residuals=False):
    """The fitted curves of the session's fit at its current parameters, computed on the device from the data held there and the
    session's model (gfh_eval).  Returns a dict of lists with one array per dataset, split at the data positions: ``model`` f(x_i);
    ``residual`` (y_i - f) w_i under ``residuals=True``, else None; ``band``, the 1-sigma band sqrt(g^T C g) of each curve with C
    the dataset's block of ``cov`` [dim][dim] as gadf_errors returned it, else None.  ``x`` None: on the data's own points.  ``x``
    [n_eval]: ``model`` and ``band`` of every dataset on that grid; residuals are refused there."""
    ctx, pars, active, is_global = _plain_call()
    try:
        model, residual, band, _ = ctx.eval(pars, active, is_global, cov=cov, x_eval=x, residuals=residuals)
    except _lib.GadfitHipError as e:
        raise GadfitError(str(e))
    if x is None:
        pos = np.concatenate([[0], np.cumsum([len(d[0]) for d in _S.datasets])])
        split = lambda v: None if v is None else [v[pos[i]:pos[i + 1]] for i in range(_S.n_datasets)]
    else:
        split = lambda v: None if v is None else [v[i] for i in range(_S.n_datasets)]
    return dict(model=split(model), residual=split(residual), band=split(band))


def gadf_print(begin=None, end=None, points=None, output=None, grouped=None, logplot=None):
    """gadfit.F90:1255-1395 writes curve / parameter files; here only the parameter table."""
    _need_init()
    lines = []
    for i, g in enumerate(_S.fitfuncs):
        for j, p in enumerate(g.pars):
            lines.append('%d %s %.17g' % (i + 1, p.name or ('par%d' % (j + 1)), p.val))
    text = '\n'.join(lines) + '\n'
    if output:
        with open(output + '_parameters', 'w') as fh:
            fh.write(text)
    return text


def gadf_close():
    """gadfit.F90:1399-1412: frees everything."""
    global fitfuncs
    if _S.ctx is not None:
        _S.ctx.close()
    _S.reset()
    fitfuncs = None


def context():
    """The device context of the current fit (timers, read-back); creates it if needed."""
    _need_init()
    _ensure_device()
    return _S.ctx
