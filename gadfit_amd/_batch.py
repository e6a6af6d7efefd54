"""The batch methods of _lib.Context: batched independent fits behind gfh_set_batch_data / _cube / _frames (the batch a context holds)
and gfh_fit_batch, gfh_fit_batch_errors, gfh_fit_batch_bounded, gfh_batch_covariance, gfh_batch_pass, gfh_batch_eval (what is done with it).  The C ABI
takes plain pointers, so the lengths it will read and write are checked here; everything else is the library's to refuse."""
import ctypes as C

import numpy as np

from ._lib import (BATCH_RESULT_DTYPE, BatchResult, FitOptions, GadfitHipError, _CUBE_TYPES, _FIT_OPTION_FIELDS, _dp, _i64, _vp, dp, ip,
                   lib)


def _samples(who, what, A, types, names, axes):
    """A is uploaded as it is: a numpy array of one of `types` (worded `names`), 2-D with the axes `axes` and C-contiguous"""
    if not isinstance(A, np.ndarray) or A.dtype not in types:
        raise GadfitHipError('%s: %s must be a numpy array of %s (it is uploaded as it is), got %s'
                             % (who, what, names, A.dtype if isinstance(A, np.ndarray) else type(A).__name__))
    if A.ndim != 2 or not A.flags['C_CONTIGUOUS']:
        raise GadfitHipError('%s: %s must be 2-D %s and C-contiguous' % (who, what, axes))


def _weights(who, name, w, what, A):
    """the USER weights of the samples A as float64, or None"""
    if w is None:
        return None
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.shape != A.shape:
        raise GadfitHipError('%s: %s must have the shape of %s %s, got %s' % (who, name, what, A.shape, w.shape))
    return w


def _sized(who, name, a, note, names, dims):
    if a.size != int(np.prod(dims)):
        raise GadfitHipError('%s: %s must hold %s%s = %s values, got %d'
                             % (who, name, note, ' x '.join(names), ' x '.join('%d' % d for d in dims), a.size))


def _error_outputs(n, na):
    """(cov [n][na][na], sigma [n][na], info [n]) for gfh_batch_covariance and gfh_fit_batch_errors to fill"""
    return np.zeros((n, na, na)), np.zeros((n, na)), np.zeros(n, dtype=np.int32)


class BatchCalls:
    # --- the batch held (gfh_set_batch_data, gfh_set_batch_cube, gfh_batch_frames_begin, gfh_batch_frames_put, gfh_set_batch_frames)
    def _held(self, rc, n_fits, cube_dtype, off, points):
        """what this object knows of the batch held after a setter of the library returned rc.  A compile-only context ends in `no
        GPU`: the library has checked the geometry and the form by then and keeps them, so does this object"""
        self._batch_off, self._batch_points = off, points
        try:
            self._chk(rc)
        except GadfitHipError as e:
            self.n_fits, self._cube_dtype = (n_fits, cube_dtype) if 'no GPU bound' in str(e) else (0, None)
            raise
        self.n_fits, self._cube_dtype = n_fits, cube_dtype

    def set_batch_data(self, offsets, x, y, w):
        """the spectra of a batch back to back: fit f owns points [offsets[f], offsets[f + 1]); w are the weights of (y - f) * w"""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        x = np.ascontiguousarray(x, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if off.ndim != 1 or off.size < 2:
            raise GadfitHipError('set_batch_data: offsets must hold n_fits + 1 >= 2 values')
        if not (x.size == y.size == w.size == off[-1]):
            raise GadfitHipError('set_batch_data: x, y and w must hold offsets[-1] = %d values each, got %d, %d, %d'
                                 % (off[-1], x.size, y.size, w.size))
        self._held(lib().gfh_set_batch_data(self._h, off.size - 1, off.ctypes.data_as(C.POINTER(_i64)), dp(x), dp(y), dp(w)),
                   off.size - 1, None, off.copy(), None)

    def set_batch_cube(self, x, Y, error_type=0, w=None):
        """a batch as a cube: every spectrum on the one grid x [n_points], Y [n_fits][n_points] C-contiguous in float64, float32 or
        uint16 (uploaded as it is; any other dtype is refused, nothing is converted), the weights formed on the device by
        error_type's rule (init_weights' numbers: 0 NONE, 1 SQRT_Y, 2 PROPTO_Y, 3 INVERSE_Y) or, under 4 (USER), w [n_fits][n_points],
        the weights as used in (y - f) * w -- gfh_set_batch_cube"""
        self._set_cube('set_batch_cube', x, Y, 'Y', '[n_fits][n_points]', 1, 'column', error_type, w)

    def _set_cube(self, who, x, A, what, axes, points_axis, per, error_type, w, *more):
        """set_batch_cube or set_batch_frames (who): the samples A (`what`, with the axes `axes`, the points along points_axis), the
        grid, the weights; `more`: the call's arguments behind w"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        _samples(who, what, A, _CUBE_TYPES, 'float64, float32 or uint16', axes)
        n_points, n_fits = A.shape[points_axis], A.shape[1 - points_axis]
        if x.ndim != 1 or x.size != n_points:
            raise GadfitHipError('%s: x must hold one abscissa per %s of %s (%d), got %d' % (who, per, what, n_points, x.size))
        w = _weights(who, 'w', w, what, A)
        self._held(getattr(lib(), 'gfh_' + who)(self._h, n_fits, n_points, dp(x), A.ctypes.data_as(_vp), _CUBE_TYPES[A.dtype],
                                                int(error_type), None if w is None else dp(w), *more), n_fits, A.dtype, None, n_points)

    def batch_frames_begin(self, x, n_fits, dtype, error_type=0):
        """begins a cube that is filled frame by frame: the grid x [n_points], n_fits spectra, the sample type dtype (float64, float32
        or uint16) and the weight rule as set_batch_cube; every frame is missing until batch_frames_put has put it --
        gfh_batch_frames_begin"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        try:
            dtype = np.dtype(dtype)
        except TypeError:
            dtype = None
        if dtype not in _CUBE_TYPES:
            raise GadfitHipError('batch_frames_begin: dtype must be float64, float32 or uint16, got %s' % (dtype,))
        if x.ndim != 1:
            raise GadfitHipError('batch_frames_begin: x must be 1-D [n_points]')
        self._held(lib().gfh_batch_frames_begin(self._h, int(n_fits), x.size, dp(x), _CUBE_TYPES[dtype], int(error_type)),
                   int(n_fits), dtype, None, x.size)

    def batch_frames_put(self, first_frame, F_piece, w_piece=None):
        """frames [first_frame, first_frame + len(F_piece)) of the begun batch: F_piece [n_frames][n_fits] C-contiguous in the begun
        dtype, uploaded as it is; under USER w_piece alike, the weights as used in (y - f) * w.  In any order and any piece sizes; a
        frame put again holds the later data -- gfh_batch_frames_put"""
        if self.batch_frames_missing() < 0:
            raise GadfitHipError('batch_frames_put: no batch has been begun (batch_frames_begin; set_batch_data and set_batch_cube replace a begun batch)')
        _samples('batch_frames_put', 'F_piece', F_piece, (self._cube_dtype,), np.dtype(self._cube_dtype).name, '[n_frames][n_fits]')
        if F_piece.shape[1] != self.n_fits:
            raise GadfitHipError('batch_frames_put: F_piece must hold one sample per fit of the batch in every frame (%d), got %d'
                                 % (self.n_fits, F_piece.shape[1]))
        w_piece = _weights('batch_frames_put', 'w_piece', w_piece, 'F_piece', F_piece)
        self._chk(lib().gfh_batch_frames_put(self._h, int(first_frame), F_piece.shape[0], F_piece.ctypes.data_as(_vp),
                                             None if w_piece is None else dp(w_piece)))

    def set_batch_frames(self, x, F, error_type=0, w=None, frames_per_put=0):
        """a batch as a stack of frames: every spectrum on the one grid x [n_points], F [n_points][n_fits] C-contiguous in float64,
        float32 or uint16 -- one image per abscissa, the fit index fastest, uploaded as it is and transposed into the cube on the
        device; error_type and w (frame-major as F) as set_batch_cube.  frames_per_put: frames per upload, 0 the library's rule (at
        most 256 MiB of staging).  From here on the batch is the cube set_batch_cube(x, F.T) holds -- gfh_set_batch_frames"""
        self._set_cube('set_batch_frames', x, F, 'F', '[n_points][n_fits]', 0, 'frame', error_type, w, int(frames_per_put))

    def batch_frames_missing(self):
        """frames of the begun batch not yet put; -1: the batch held was not begun by batch_frames_begin / set_batch_frames --
        gfh_debug_batch_frames_missing"""
        return int(lib().gfh_debug_batch_frames_missing(self._h))

    def batch_frames_seconds(self):
        """device time of the transposing kernels of every put since the batch was begun -- gfh_debug_batch_frames_seconds"""
        return float(lib().gfh_debug_batch_frames_seconds(self._h))

    def debug_batch_read(self, which, first, count):
        """elements [first, first + count) of the cube held, row-major [n_fits][n_points], as stored: which 0 the samples in the
        dtype this object set or began the cube with, 1 the USER weights as float64 -- gfh_debug_batch_read"""
        dtype = getattr(self, '_cube_dtype', None)
        if dtype is None or getattr(self, 'n_fits', 0) < 1:
            raise GadfitHipError('debug_batch_read: this object holds no cube (set_batch_cube, set_batch_frames, batch_frames_begin)')
        out = np.empty(int(count), dtype=np.float64 if which == 1 else dtype)
        self._chk(lib().gfh_debug_batch_read(self._h, int(which), int(first), int(count), out.ctypes.data_as(_vp)))
        return out

    # --- the lane form (gfh_set_batch_lanes) and what the last launch used
    def set_batch_lanes(self, lanes):
        """lanes per fit of the batch kernels from here on: 64 a wave per fit (the default), 16 a DPP row per fit and four fits per
        wave (short spectra), 256 a workgroup of four waves per fit (few, long spectra), 0 auto (batch_auto_lanes of the active count
        and the longest spectrum: 16 or 64, never 256) -- gfh_set_batch_lanes"""
        self._chk(lib().gfh_set_batch_lanes(self._h, int(lanes)))

    def batch_lanes_used(self):
        """64, 16 or 256: the form of the last batch launch (0: none yet) -- gfh_debug_batch_lanes"""
        return int(lib().gfh_debug_batch_lanes(self._h))

    # --- the loss of a batch (gfh_set_batch_loss) and what the last launch ran under
    def set_batch_loss(self, loss, scale=1.0):
        """the loss of the batch calls from here on (it stays set): 0 linear (the default), 1 Cauchy, 2 Huber, switching at |r| = scale in
        units of the weighted residual r = (y - f) w (scale 1: the reference's costs).  The acceptance test, the records and
        batch_pass keep the plain chi2; a context's set_loss stays refused in a batch -- gfh_set_batch_loss"""
        self._chk(lib().gfh_set_batch_loss(self._h, int(loss), float(scale)))

    def batch_loss(self):
        """(loss, scale) as set_batch_loss left them; (0, 1.0) until it is called -- gfh_get_batch_loss"""
        scale = C.c_double()
        return int(lib().gfh_get_batch_loss(self._h, C.cast(C.byref(scale), _dp))), scale.value

    def batch_loss_used(self):
        """(loss, scale) of the last batch launch that sweeps, None: none yet -- gfh_debug_batch_loss"""
        scale = C.c_double()
        loss = int(lib().gfh_debug_batch_loss(self._h, C.cast(C.byref(scale), _dp)))
        return None if loss < 0 else (loss, scale.value)

    def _loss(self, loss, loss_scale):
        """loss and loss_scale of a call: as set_batch_loss (they stay set); None leaves that part of the context's setting"""
        if loss is not None or loss_scale is not None:
            held = self.batch_loss()          # (the library's own record: the one source of the setting)
            self.set_batch_loss(held[0] if loss is None else loss, held[1] if loss_scale is None else loss_scale)

    # --- the estimator of a batch (gfh_set_batch_estimator) and what the last launch ran under
    _ESTIMATORS = {'lsq': 0, 'poisson': 1}

    def set_batch_estimator(self, estimator):
        """what the batch calls minimise from here on (it stays set): 0 or 'lsq' the weighted sum of squares (the default), 1 or
        'poisson' the Poisson deviance 2 sum [f - y + y ln(y / f)] over the points of non-zero weight, by Fisher scoring -- the
        maximum-likelihood fit of counted data.  The deviance then stands wherever chi2 stood (the records, batch_pass's third output,
        chi2_abs and chi2_rel, the factor of scale=True) and the covariance is the inverse Fisher matrix.  The data form's weight is a
        mask there: a cube under this estimator wants error_type NONE -- any rule works as a mask, but SQRT_Y pays a sqrt and a
        division per point for nothing.  Refused with a batch loss, with accth and for batch_eval's residuals -- gfh_set_batch_estimator"""
        if isinstance(estimator, str):
            if estimator not in self._ESTIMATORS:
                raise GadfitHipError("set_batch_estimator: unknown estimator %r (0 or 'lsq': least squares, 1 or 'poisson')" % (estimator,))
            estimator = self._ESTIMATORS[estimator]
        self._chk(lib().gfh_set_batch_estimator(self._h, int(estimator)))

    def batch_estimator(self):
        """the estimator as set_batch_estimator left it; 0 until it is called -- gfh_get_batch_estimator"""
        return int(lib().gfh_get_batch_estimator(self._h))

    def batch_estimator_used(self):
        """the estimator of the last batch launch that sweeps, None: none yet -- gfh_debug_batch_estimator"""
        e = int(lib().gfh_debug_batch_estimator(self._h))
        return None if e < 0 else e

    def batch_form_used(self):
        """the data form of the last batch launch: None (none yet), 'ragged', or ('cube', y_type, error_type) -- gfh_debug_batch_form"""
        f = int(lib().gfh_debug_batch_form(self._h))
        return None if f < 0 else 'ragged' if f == 0 else ('cube', (f - 1) % 3, (f - 1) // 3)

    def batch_pass_seconds(self):
        """device time of the kernel of this context's last batch_pass (0.0: none yet) -- gfh_debug_batch_pass_seconds"""
        return float(lib().gfh_debug_batch_pass_seconds(self._h))

    # --- the calls on the batch held
    def _n_held(self, who):
        n = getattr(self, 'n_fits', 0)
        if n < 1:
            raise GadfitHipError(who + ': no batch data (set_batch_data, set_batch_cube)')
        return n

    def _active(self, who, active):
        a = np.ascontiguousarray(active, dtype=np.int32)
        if a.size < 1 or a.min() < 0 or a.max() >= self.n_pars:
            raise GadfitHipError('%s: active parameter indices must lie in [0, %d)' % (who, self.n_pars))
        return a

    def _lanes(self, lanes_per_fit):
        """lanes_per_fit of a call: as set_batch_lanes (it stays set), None leaves the context's setting"""
        if lanes_per_fit is not None:
            self.set_batch_lanes(lanes_per_fit)

    def _batch_args(self, who, pars, active, lanes_per_fit, loss=None, loss_scale=None, estimator=None):
        """a copy of pars as [n_fits][n_pars], the active set and n_fits of a call on every fit of the batch held"""
        n = self._n_held(who)
        p = np.ascontiguousarray(pars, dtype=np.float64).copy()
        _sized(who, 'pars', p, '', ('n_fits', 'n_pars'), (n, self.n_pars))
        a = self._active(who, active)
        self._lanes(lanes_per_fit)
        self._loss(loss, loss_scale)
        if estimator is not None:
            self.set_batch_estimator(estimator)
        return p.reshape(n, self.n_pars), a, n

    def _batch_options(self, who, a, DTD_min, kw):
        """the FitOptions of a batch fit from fit()'s keyword arguments, and what must outlive the call with them"""
        o = FitOptions()
        for k, v in kw.items():
            if v is None:
                continue
            name = 'lambda' if k in ('lambda_', 'lam', 'lambda') else k
            if 'has_' + name not in _FIT_OPTION_FIELDS:
                raise GadfitHipError('%s: unknown fit argument %r' % (who, k))
            setattr(o, 'lambda_' if name == 'lambda' else name, v)
            setattr(o, 'has_' + name, 1)
        o.umnigh_a = 0.5
        dm = None
        if DTD_min is not None:
            dm = np.ascontiguousarray(DTD_min, dtype=np.float64)
            if dm.size != a.size:
                raise GadfitHipError('%s: DTD_min must hold one value per active parameter (%d), got %d' % (who, a.size, dm.size))
            o.DTD_min = dp(dm)
        return o, dm

    def fit_batch(self, pars, active, DTD_min=None, lanes_per_fit=None, loss=None, loss_scale=None, estimator=None, **kw):
        """every spectrum of the batch fitted in one launch.  pars [n_fits][n_pars]; keyword arguments as fit(); lanes_per_fit: as
        set_batch_lanes (it stays set), None leaves the context's setting; loss, loss_scale: as set_batch_loss (they stay set), None
        leaves the setting; estimator: as set_batch_estimator (0 / 'lsq', 1 / 'poisson'; it stays set), None leaves the setting -- under
        'poisson' a cube wants error_type NONE and the records' chi2 is the deviance.  Returns the fitted parameters, a numpy record array of
        BatchResult [n_fits] and the device time of the launch in seconds."""
        return self._fit('fit_batch', pars, active, None, DTD_min, lanes_per_fit, kw, loss, loss_scale, estimator)

    def _fit(self, who, pars, active, scale, DTD_min, lanes_per_fit, kw, loss=None, loss_scale=None, estimator=None):
        """fit_batch or fit_batch_errors (who): the same arguments, the second with scale and the error outputs behind them"""
        p, a, n = self._batch_args(who, pars, active, lanes_per_fit, loss, loss_scale, estimator)
        o, _keep = self._batch_options(who, a, DTD_min, kw)
        res = np.zeros(n, dtype=BATCH_RESULT_DTYPE)
        sec = C.c_double()
        args = (self._h, dp(p), a.size, ip(a), C.byref(o), res.ctypes.data_as(C.POINTER(BatchResult)))
        if who == 'fit_batch':
            self._chk(lib().gfh_fit_batch(*args, C.cast(C.byref(sec), _dp)))
            return p, res.view(np.recarray), sec.value
        cov, sigma, info = _error_outputs(n, a.size)
        self._chk(lib().gfh_fit_batch_errors(*args, int(scale), dp(cov), dp(sigma), ip(info), C.cast(C.byref(sec), _dp)))
        return p, res.view(np.recarray), (cov, sigma, info), sec.value

    def fit_batch_bounded(self, pars, active, lower, upper, DTD_min=None, lanes_per_fit=None, loss=None, loss_scale=None, estimator=None, **kw):
        """fit_batch inside one box per batch: lower and upper hold one value per active parameter, in the order of `active`, -inf /
        +inf for no bound on that side.  Returns the fitted parameters, the records, at_bound [n_fits] (int32: bit j where the
        returned active parameter j equals lower[j], bit 8 + j where it equals upper[j]) and the device time of the launch in seconds.
        With no finite bound the parameters and records are fit_batch's bits; loss, loss_scale as fit_batch (under a loss a parameter
        is pinned on the sign of the loss-scaled J^T r); estimator as fit_batch (under 'poisson' the sign is that of sum g (y - f) / f; a
        cube wants error_type NONE) -- gfh_fit_batch_bounded"""
        who = 'fit_batch_bounded'
        p, a, n = self._batch_args(who, pars, active, lanes_per_fit, loss, loss_scale, estimator)
        lo = np.ascontiguousarray(lower, dtype=np.float64); hi = np.ascontiguousarray(upper, dtype=np.float64)
        for name, v in (('lower', lo), ('upper', hi)):
            if v.ndim != 1 or v.size != a.size:
                raise GadfitHipError('%s: %s must hold one value per active parameter (%d), got %d' % (who, name, a.size, v.size))
        o, _keep = self._batch_options(who, a, DTD_min, kw)
        res = np.zeros(n, dtype=BATCH_RESULT_DTYPE)
        at = np.zeros(n, dtype=np.int32)
        sec = C.c_double()
        self._chk(lib().gfh_fit_batch_bounded(self._h, dp(p), a.size, ip(a), dp(lo), dp(hi), C.byref(o), res.ctypes.data_as(C.POINTER(BatchResult)),
                                              ip(at), C.cast(C.byref(sec), _dp)))
        return p, res.view(np.recarray), at, sec.value

    def fit_batch_errors(self, pars, active, scale=False, DTD_min=None, lanes_per_fit=None, loss=None, loss_scale=None, estimator=None, **kw):
        """fit_batch and, behind it on the device, each fit's parameter covariance at the fitted parameters: returns the fitted
        parameters, the records, (cov [n_fits][na][na], sigma [n_fits][na], info [n_fits]) as batch_covariance returns them and the
        device time of the two launches in seconds.  The parameters and records are fit_batch's bits; loss, loss_scale and estimator as
        fit_batch (under 'poisson' cov is the inverse Fisher matrix, under scale=True times deviance / dof; a cube wants error_type NONE)
        -- gfh_fit_batch_errors"""
        return self._fit('fit_batch_errors', pars, active, scale, DTD_min, lanes_per_fit, kw, loss, loss_scale, estimator)

    def batch_covariance(self, pars, active, scale=False, lanes_per_fit=None, loss=None, loss_scale=None, estimator=None):
        """(cov [n_fits][na][na], sigma [n_fits][na], info [n_fits]) of every spectrum at pars [n_fits][n_pars]: cov = (J^T J)^-1
        (the reference's LMsolver::getInvJTJ), under scale=True times the fit's chi2 / dof; sigma = sqrt of its diagonal; info 0, or
        j + 1 where pivot j of the Cholesky factor failed (that fit's cov and sigma are NaN).  Rows and columns in the order of
        `active`; lanes_per_fit, loss and loss_scale as fit_batch: under a loss J is the loss-scaled Jacobian and the chi2 of
        scale=True stays the plain one; estimator as fit_batch: under 'poisson' J^T J is the Fisher matrix sum g g^T / f and scale=True
        multiplies by deviance / dof (a cube wants error_type NONE) -- gfh_batch_covariance"""
        p, a, n = self._batch_args('batch_covariance', pars, active, lanes_per_fit, loss, loss_scale, estimator)
        cov, sigma, info = _error_outputs(n, a.size)
        self._chk(lib().gfh_batch_covariance(self._h, dp(p), a.size, ip(a), int(scale), dp(cov), dp(sigma), ip(info)))
        return cov, sigma, info

    def batch_pass(self, pars, active, lanes_per_fit=None, loss=None, loss_scale=None, estimator=None):
        """(JTJ [n_fits][na][na], JTres [n_fits][na], chi2 [n_fits]) of every spectrum at pars [n_fits][n_pars] -- gfh_batch_pass;
        lanes_per_fit, loss and loss_scale as fit_batch (under a loss JTJ and JTres are the loss-scaled sums, chi2 the plain one);
        estimator as fit_batch: under 'poisson' JTJ = sum g g^T / f, JTres = sum g (y - f) / f and the third output is the deviance (a
        cube wants error_type NONE)"""
        p, a, n = self._batch_args('batch_pass', pars, active, lanes_per_fit, loss, loss_scale, estimator)
        JTJ = np.zeros((n, a.size, a.size)); JTr = np.zeros((n, a.size)); chi2 = np.zeros(n)
        self._chk(lib().gfh_batch_pass(self._h, dp(p), a.size, ip(a), dp(JTJ), dp(JTr), dp(chi2)))
        return JTJ, JTr, chi2

    def batch_eval(self, pars, active, cov=None, x_eval=None, residuals=False, first_fit=0, n_fits=None, lanes_per_fit=None, model=True):
        """the fitted curves of fits [first_fit, first_fit + n_fits) of the batch held (n_fits None: to its end), computed on the
        device: returns (model, residual or None, band or None, offsets, seconds).  pars [n_fits][n_pars] and cov [n_fits][na][na]
        (batch_covariance's, or None: no band) hold the rows of the evaluated fits only.  x_eval None: on the fits' own points, in
        the data's layout -- a cube gives [n_fits][n_points], the ragged form flat arrays that `offsets` [n_fits + 1] (relative to
        the range) splits; model = f(x_i), residual = (y_i - f) w_i under residuals=True, band = sqrt(g^T C g) with g the gradient by
        the active parameters in the order of `active`.  x_eval [n_eval]: model and band on that grid, [n_fits][n_eval]; residuals
        are refused.  model=False leaves the model out (None).  A fit whose cov is NaN gets NaN bands alone.  seconds: the device
        time of the kernel; lanes_per_fit as fit_batch -- gfh_batch_eval"""
        nb = self._n_held('batch_eval')
        first = int(first_fit)
        n = nb - first if n_fits is None else int(n_fits)
        a = self._active('batch_eval', active)
        p = np.ascontiguousarray(pars, dtype=np.float64)
        xe = None if x_eval is None else np.ascontiguousarray(x_eval, dtype=np.float64).ravel()
        ok = first >= 0 and n >= 1 and first + n <= nb          # (otherwise the library words the refusal)
        rows = 'the rows of the evaluated fits, '
        if ok:
            _sized('batch_eval', 'pars', p, rows, ('n_fits', 'n_pars'), (n, self.n_pars))
        if cov is not None:
            cov = np.ascontiguousarray(cov, dtype=np.float64)
            if ok:
                _sized('batch_eval', 'cov', cov, rows, ('n_fits', 'na', 'na'), (n, a.size, a.size))
        self._lanes(lanes_per_fit)
        offsets = None
        if not ok:
            shape = (0,)
        elif xe is not None:
            shape = (n, xe.size)
        elif self._batch_off is None:
            shape = (n, self._batch_points)
        else:
            offsets = self._batch_off[first:first + n + 1] - self._batch_off[first]
            shape = (int(offsets[-1]),)
        if offsets is None and ok:
            offsets = np.arange(n + 1, dtype=np.int64) * shape[1]
        out_m = np.empty(shape) if model else None
        out_r = np.empty(shape) if residuals else None
        out_b = np.empty(shape) if cov is not None else None
        sec = C.c_double()
        self._chk(lib().gfh_batch_eval(self._h, dp(p), a.size, ip(a), None if cov is None else dp(cov), None if xe is None else dp(xe),
                                       0 if xe is None else xe.size, first, n, *[None if v is None else dp(v) for v in (out_m, out_r, out_b)],
                                       C.cast(C.byref(sec), _dp)))
        return out_m, out_r, out_b, offsets, sec.value

    def batch_source(self, active, bounded=False):
        """the text of the batch unit of an active set; bounded=True: of the unit that holds gfh_k_fit_batch_bounded"""
        source = lib().gfh_batch_source_bounded if bounded else lib().gfh_batch_source
        a = np.ascontiguousarray(active, dtype=np.int32)
        n = source(self._h, a.size, ip(a), None, 0)
        if n < 0:
            self._chk(1)
        buf = C.create_string_buffer(n)
        source(self._h, a.size, ip(a), buf, n)
        return buf.value.decode()

    def batch_prepare(self, active, bounded=False):
        a = np.ascontiguousarray(active, dtype=np.int32)
        self._chk((lib().gfh_batch_prepare_bounded if bounded else lib().gfh_batch_prepare)(self._h, a.size, ip(a)))
