"""Batched independent fits (gfh_fit_batch) measured against what the project offered for them before, on the problem of
profiles/r05_small_fits.txt: 1000 points, a Gaussian on a background, 4 parameters, lambda0 = 1, max_iter = 30.

    python tools/bench_batch.py [--sizes 1024,16384,131072] [--launches 7] [--warmup 2] [--one-at-a-time 200]
                                [--points 1000] [--lanes 64] [--observed FILE [--observed-only]] [--out profiles/batch_fits.json]
    python tools/bench_batch.py --rows [--points 8,16,32,64,128,256,1000] [--lanes 64,16] [--sizes 131072] [--registers]
                                [--observed FILE [--observed-only]] [--out profiles/batch_rows.json]
    python tools/bench_batch.py --workgroup [--points 1000,4096,16384,65536] [--sizes 64,256,1024,16384] [--models gauss4,exp4]
                                [--registers] [--observed FILE [--observed-only]] [--out profiles/batch_workgroup.json]
    python tools/bench_batch.py --cube [--cells gauss4:64:16384:1000,...] [--registers] [--out profiles/batch_cube.json]
    python tools/bench_batch.py --frames [--cells uint16:1:64:131072:1000,...] [--out profiles/batch_frames.json]
    python tools/bench_batch.py --cov [--sizes 16384,131072] [--points 1000] [--lanes 64] [--out profiles/batch_cov.json]
    python tools/bench_batch.py --bounds [--sizes 16384] [--points 1000] [--lanes 64] [--out profiles/batch_bounds.json]
    python tools/bench_batch.py --loss [--registers] [--sizes 16384] [--points 1000] [--lanes 64] [--out profiles/batch_loss.json]
    python tools/bench_batch.py --estimator [--registers] [--cells gauss4:64:16384:1000,...] [--out profiles/batch_mle.json]
    python tools/bench_batch.py --eval [--cells gauss4:64:16384:1000,...] [--registers] [--observed FILE] [--out profiles/batch_eval.json]

Per batch size: warm-up launches, then the median of the timed launches -- device time from the HIP events around the kernel
(gfh_fit_batch's `seconds`) and wall time around the whole call (parameters down, launch, results back).  Two yardsticks, neither of
them the code under test:
 1. the same spectra one at a time through Context.set_data + Context.fit on ONE context in this process (no context cycle, kernels
    loaded: the cheapest form the one-at-a-time path has);
 2. the per-point rate of the model's N-sized kernels (gfh_time_kernel: fused sweep and chi2) on the points of 16384 spectra as one
    dataset -- what the card does per point evaluation when it is full and streams every point from HBM once per pass -- against
    the batch kernel's time for the same passes (whose spectra stay in cache from one pass of a fit to the next).
Needs a GPU; there is no fallback.  --observed: a JSON file of observed parity maxima copied into the record, written under
GADFIT_BATCH_OBSERVE by tests/test_gpu_batch_shapes.py and tests/test_gpu_batch.py run in ONE pytest process (the maxima are kept per
process, so a module run alone writes its own keys only).  --observed-only: the record's timings stay, its maxima are replaced.

--points, --lanes: the spectrum length and the lanes per fit (gfh_set_batch_lanes) of the measurement above.
--rows: the two forms of the batch kernels against each other, the table the auto rule of gfh_set_batch_lanes(0) is written from.
Per model (this file's 4-parameter Gaussian; exp4, four exponentials with all 8 parameters active), spectrum length and form:
--sizes[0] fits per launch, the median and the min-max of the timed launches, device and wall time per fit.  The yardstick of the row
form is the wave form on the same card in the same run, never the row form's own time: `row_wins` is tests/batch_records.row_wins
(the medians differ by more than the sum of the two forms' min-max spreads), and `auto_rule` is the largest measured length with
row_wins per active-count class.  --registers: the compiler's register, scratch and occupancy figures of the four kernels
(hipcc -Rpass-analysis=kernel-resource-usage on the generated source; needs hipcc, no GPU).
--workgroup: the 256-lane form (a workgroup of four waves per fit) against the 64-lane form by the recipe of --rows, over points per
spectrum AND fits per launch, since what the workgroup form buys is occupancy when the fits are fewer than the card's SIMDs: per
(model, fits, points) both forms alternating launch by launch on one context; cells above 2^30 points in total are dropped.  The
yardstick of the 256-lane form is the 64-lane form of the same run; `workgroup_wins` is tests/batch_records.row_wins.  With
--registers: the compiler's figures (LDS included) of the 256-lane kernels of the three units of the --rows table.
--cube: a batch as a data cube (gfh_set_batch_cube: one shared grid, narrow samples, the weight formed in the load) against the
ragged form of the same spectra with precomputed SQRT_Y weights -- the yardstick, measured in the same run, never the cube's own time.
The spectra are counts (the models above scaled by 1000 and rounded, so that uint16 holds them); per cell (model, lanes, fits,
points) the five forms -- ragged, float64 / USER (the shared grid alone), float64 / SQRT_Y (against it: the price of the in-load
weight), float32 / SQRT_Y, uint16 / SQRT_Y -- alternate launch by launch on one context of one card, each launch behind the upload
of its own data, by the recipe of --rows; all five hold the same values, so they run the same passes (checked: the totals must be
equal).  `upload_ms` is the wall time of the set call, median of 3.  `wins` is tests/batch_records.row_wins against the ragged
form.  With --registers: the compiler's figures of the uint16 / SQRT_Y and float64 / USER units of model_exp2 and model_exp4 at the
three lane forms (no GPU); model_exp2's must have no scratch.
--frames: a stack of frames F [points][fits] (gfh_set_batch_frames: uploaded as stored, transposed into the cube on the device) against
the two routes a caller had before, over the shapes of the --cube table; cells are sample type:error type:lanes:fits:points.  Per cell
the wall time of the set call through five routes that alternate call by call on one context: set_batch_cube of the already transposed
array (the floor: the upload alone), np.ascontiguousarray(F.T) + set_batch_cube (the yardstick: the route before), set_batch_frames with
the default pieces, with one put and with eight puts; the transposing kernel's device time (HIP events) and the bytes it moves per second.  fit_batch must
return the same parameters and counts from all three routes, and at 131072 x 1000 uint16 the frames route must beat the host
transpose by tests/batch_records.row_wins, or the tool fails.
--cov: the errors of a batch (gfh_fit_batch_errors: the fit, then gfh_k_batch_cov on the same stream) on this tool's problem with 4
(gauss4) and 8 (exp4) active parameters, per batch size three routes that alternate call by call on one context: fit_batch alone (the
first yardstick), fit_batch_errors, and the route a caller had before (the second yardstick): fit_batch, batch_pass at the fitted
parameters, numpy.linalg.inv over the batch on the host.  Wall time around each route, and the device time the library reports for
fit_batch and for fit_batch_errors (HIP events around the one launch and around the two): their difference is what gfh_k_batch_cov
adds on the device.  The library takes no events around gfh_k_batch_pass, so that kernel's own device time is not in the record.  No
ratio is asserted; the medians and the min-max are written down.
--bounds: the bounded loop (gfh_fit_batch_bounded: the kernel gfh_k_fit_batch_bounded, in a unit of its own) against gfh_fit_batch on
this tool's problem with 4 active parameters and on the four exponentials with 8, 16384 fits of 1000 points at 64 lanes: fit_batch,
fit_batch_bounded with every bound infinite (the same bits, checked) and fit_batch_bounded with a binding box, alternating call by call
in one run on one card; device and wall time, median and min-max.  The ratio of the first two is written down with whether it lies
beyond the two routes' own spread; nothing is asserted on it.
--loss: the loss units of the batch kernels (gfh_set_batch_loss: Cauchy and Huber at c = 1) against the linear unit -- the parent
commit's kernels, whose text did not change -- on this tool's problem with 4 active parameters and on the four exponentials with 8,
16384 fits of 1000 points at 64 lanes.  The weights are 1 / sigma with sigma = 1e-3, the amplitude of the spectra's ripple, and 1 % of
the samples (a fixed pattern) are displaced by +12 sigma.  Linear, Cauchy and Huber alternate call by call on one context; per loss
batch_pass (the per-pass cost, free of the iteration counts; HIP events around its kernel) and fit_batch (events around its kernel,
with the fits' total sweeps, chi2 passes and omega passes beside it, under accth so that the omega pass is in it); median and min-max.
No ratio is asserted.  --registers: only the compiler's figures of the linear and the loss units of model_exp2 (4 active) and
model_exp4 (8 active) at the three lane forms, the bounded unit included; no GPU is needed.
--estimator: the Poisson unit of the batch kernels (gfh_set_batch_estimator(1): the deviance by Fisher scoring) against the least-squares
unit -- the parent commit's kernels, whose text did not change -- at shapes of the tables above (model:lanes:fits:points).  The spectra
are counts (the models scaled by 1000 and rounded, as --cube's) in the ragged form with the weights 1 / sqrt(y), which the least-squares
unit uses and the Poisson unit reads as a mask: both load the same arrays.  The two alternate call by call on one context; per
estimator batch_pass (HIP events around its kernel) and fit_batch (events around its kernel; the fits' total sweeps and chi2 passes
beside it, and the device time per pass = fit time / (sweeps + chi2 passes)); median and min-max.  No ratio is asserted.  --registers:
only the compiler's figures of the two units of model_exp2 (4 active) and model_exp4 (8 active) at the three lane forms, the bounded
unit included; no GPU is needed.

--eval: the curves of a batch (gfh_batch_eval: the kernel gfh_k_batch_eval) at the cells of the cube table, on the ragged form and on
the uint16 cube under SQRT_Y of the same counts, at the start parameters with the device's own covariance.  Per cell and form three
calls alternate on one context: batch_pass (the first yardstick: code of the parent commit with the same loads and the same
gfh_point_grad, timed by HIP events around its kernel), batch_eval for the model alone, and batch_eval for model, residual and band.
Device time (events around the kernel; min, median and max over the launches) and wall time around the call.  The second yardstick:
the bytes the kernel must move -- what the form's load reads per point (ragged 24, the uint16 cube 2: its grid is shared) plus 8 per
requested output -- divided by the device time, as a fraction of 8 TB/s.  No ratio is asserted.  --registers: only the compiler's
figures of gfh_k_batch_eval for model_exp2 and model_exp4 at the three lane forms; no GPU is needed.  --observed FILE: the eval_*
maxima a GADFIT_BATCH_OBSERVE run of tests/test_gpu_batch_eval.py left, into the record; nothing is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gadfit_amd import _lib                       # noqa: E402
from gadfit_amd.ad import exp, trace_model        # noqa: E402

N_POINTS, MAX_ITER, LAMBDA0 = 1000, 30, 1.0          # (N_POINTS: --points)
START = np.array([2.5, 4.3, 1.0, 0.3])
ACTIVE = [0, 1, 2, 3]


def model(p, x):
    return p[0] * exp(-((x - p[1]) / p[2]) ** 2) + p[3]


def spectra(n_fits, n_points=None):
    """bench_many_small_fits.F90's spectrum k, with the peak position spread over [4, 5) so that a large batch holds no two alike"""
    n_points = n_points or N_POINTS
    x = 10.0 * (np.arange(n_points) + 0.5) / n_points
    k = np.arange(1, n_fits + 1, dtype=np.float64)
    pos = _gauss_pos(k)
    y = np.empty((n_fits, n_points))
    for lo in range(0, n_fits, 8192):
        hi = min(n_fits, lo + 8192)
        y[lo:hi] = _gauss_rows(x, k[lo:hi])
    return x, y, pos


def _gauss_pos(k):
    return 4.0 + np.mod(k * 0.6180339887498949, 1.0)


def _gauss_rows(x, k):
    """spectra k (numbered from 1, as float64) of spectra() on the abscissae x"""
    return 3.0 * np.exp(-((x[None, :] - _gauss_pos(k)[:, None]) / 0.8) ** 2) + 0.5 + 1.0e-3 * np.sin(977.0 * x[None, :] + k[:, None])


def model_exp4(p, x):
    y = p[0] * exp(-(x / p[1]))
    for k in range(1, 4):
        y = y + p[2 * k] * exp(-(x / p[2 * k + 1]))
    return y


EXP4_TRUTH = np.array([5.0, 0.5, 3.0, 2.0, 2.0, 8.0, 1.0, 30.0])


def spectra_exp4(n_fits, n_points):
    """four exponentials on x in (0.05, 100): the amplitudes spread by +-10 % from fit to fit, a ripple of 1e-3 as in spectra()"""
    x = 0.05 + 99.95 * (np.arange(n_points) + 0.5) / n_points
    k = np.arange(1, n_fits + 1, dtype=np.float64)
    y = np.empty((n_fits, n_points))
    for lo in range(0, n_fits, 8192):
        hi = min(n_fits, lo + 8192)
        y[lo:hi] = _exp4_rows(x, k[lo:hi])
    return x, y


def _exp4_rows(x, k):
    """spectra k (numbered from 1, as float64) of spectra_exp4() on the abscissae x"""
    amp = 0.9 + 0.2 * np.mod(k[:, None] * 0.6180339887498949 + 0.25 * np.arange(4)[None, :], 1.0)
    y = 1.0e-3 * np.sin(977.0 * x[None, :] + k[:, None])
    for j in range(4):
        y += (EXP4_TRUTH[2 * j] * amp[:, j:j + 1]) * np.exp(-x[None, :] / EXP4_TRUTH[2 * j + 1])
    return y


def spectra_flat(name, n_fits, n_points):
    """(x, y, w) back to back as set_batch_data takes them: the spectra of spectra() ('gauss4') or spectra_exp4() ('exp4'), computed
    in blocks of at most 2^22 points on up to 16 threads, so that a batch of 2^30 points costs no temporaries of its own size"""
    from concurrent.futures import ThreadPoolExecutor
    if name == 'gauss4':
        x, rows = 10.0 * (np.arange(n_points) + 0.5) / n_points, _gauss_rows
    else:
        x, rows = 0.05 + 99.95 * (np.arange(n_points) + 0.5) / n_points, _exp4_rows
    y = np.empty((n_fits, n_points)); xs = np.empty((n_fits, n_points))
    step = max(1, (1 << 22) // n_points)

    def block(lo):
        hi = min(n_fits, lo + step)
        y[lo:hi] = rows(x, np.arange(lo + 1, hi + 1, dtype=np.float64))
        xs[lo:hi] = x[None, :]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(block, range(0, n_fits, step)))
    return xs.reshape(-1), y.reshape(-1), np.ones(n_fits * n_points)


ROW_MODELS = {
    'gauss4': dict(model=model, n_pars=4, active=ACTIVE, start=START, what='gaussian on a background, 4 of 4 parameters active'),
    'exp4': dict(model=model_exp4, n_pars=8, active=list(range(8)), start=EXP4_TRUTH * np.where(np.arange(8) % 2 == 0, 1.05, 0.95),
                 what='four exponentials, 8 of 8 parameters active'),
}


def kernel_registers(src):
    """{kernel: {vgprs, agprs, sgprs, scratch_bytes_per_lane, waves_per_simd, lds_bytes_per_block}} of the four batch kernels of a generated source"""
    import re
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, 'unit.hip')
        with open(f, 'w') as fh:
            fh.write('#include <hip/hip_runtime.h>\n' + src)
        r = subprocess.run([os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', 'hipcc'), '-O3', '-std=c++17', '--offload-arch=gfx950',
                            '-ffp-contract=on', '--cuda-device-only', '-c', f, '-o', os.path.join(d, 'unit.o'),
                            '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True, check=True)
    out, name = {}, None
    keys = {'VGPRs': 'vgprs', 'AGPRs': 'agprs', 'TotalSGPRs': 'sgprs', 'SGPRs Spill': 'sgprs_spilled', 'VGPRs Spill': 'vgprs_spilled', 'ScratchSize [bytes/lane]': 'scratch_bytes_per_lane',
            'Occupancy [waves/SIMD]': 'waves_per_simd', 'LDS Size [bytes/block]': 'lds_bytes_per_block'}
    for line in r.stderr.splitlines():
        m = re.search(r'remark:\s+(.*?): (\S+) \[-Rpass', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            name = m.group(2) if m.group(2) in ('gfh_k_fit_batch', 'gfh_k_batch_pass', 'gfh_k_batch_cov', 'gfh_k_batch_eval', 'gfh_k_fit_batch_bounded') else None
            if name:
                out[name] = {}
        elif name and m.group(1) in keys:
            out[name][keys[m.group(1)]] = int(m.group(2))
    return out


def registers_record(forms=(64, 16)):
    rec = {}
    c = _lib.Context(-1)
    exp2 = dict(model=lambda p, x: p[0] * exp(-(x / p[1])) + p[2] * exp(-(x / p[3])), n_pars=4, active=ACTIVE)      # (tests/models.py: model_exp2)
    for name, m in list(ROW_MODELS.items()) + [('exp2', exp2)]:
        c.set_model(trace_model(m['model'], m['n_pars']))
        for lanes in forms:
            c.set_batch_lanes(lanes)
            rec['%s_lanes%d' % (name, lanes)] = kernel_registers(c.batch_source(m['active']))
    c.close()
    return rec


CUBE_SCALE = 1000.0                  # counts = round(CUBE_SCALE * the model's spectrum): 500 ... 3500 (gauss4), 40 ... 11000 (exp4)
CUBE_FORMS = (('ragged', None, None), ('float64_user', np.float64, 4), ('float64_sqrt_y', np.float64, 1), ('float32_sqrt_y', np.float32, 1),
              ('uint16_sqrt_y', np.uint16, 1))
CUBE_CELLS = 'gauss4:64:16384:1000,gauss4:64:131072:1000,gauss4:16:131072:64,gauss4:256:256:65536,exp4:64:16384:1000'


def cube_registers_record():
    from tests import models as M
    rec = {}
    c = _lib.Context(-1)
    for name, fn, n_pars in (('exp2', M.model_exp2, 4), ('exp4', M.model_exp4, 8)):
        c.set_model(trace_model(fn, n_pars))
        for lanes in (64, 16, 256):
            c.set_batch_lanes(lanes)
            for form, dtype, et in (('uint16_sqrt_y', np.uint16, 1), ('float64_user', np.float64, 4)):
                try:
                    c.set_batch_cube(np.arange(8.0), np.ones((1, 8), dtype=dtype), et, np.ones((1, 8)) if et == 4 else None)
                except _lib.GadfitHipError as e:
                    if 'no GPU' not in str(e):
                        raise
                rec['%s_lanes%d_%s' % (name, lanes, form)] = r = kernel_registers(c.batch_source(list(range(n_pars))))
                if name == 'exp2' and any(k['scratch_bytes_per_lane'] != 0 for k in r.values()):
                    sys.exit('model_exp2 %s at %d lanes: scratch is not 0: %s' % (form, lanes, r))
    c.close()
    return rec


def cube_main(a):
    from tests import batch_records as RC
    rec = dict(method='per cell (model, lanes per fit, fits, points per spectrum) five data forms of the same spectra -- counts, round(%g x the model) -- '
                      'alternating launch by launch on one context of one card in one run, each launch behind the upload of its own data: the median and '
                      'the min-max of %d launches after %d warm-up launches; device = HIP events around the kernel; lambda0 = %g, max_iter = %d and no '
                      'other exit; all forms hold the same values and run the same passes (checked); upload_ms = wall time of the set call, median of 3; '
                      'the yardstick is the ragged form of the same run with precomputed SQRT_Y weights; wins = tests/batch_records.row_wins against '
                      'it; no counter pass was made' % (CUBE_SCALE, a.launches, a.warmup, LAMBDA0, MAX_ITER), measurements=[])
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        if 'registers' in old:
            rec['registers'] = old['registers']
    kw = dict(lambda_=LAMBDA0, max_iter=MAX_ITER)
    for cell in a.cells.split(','):
        name, lanes, nf, n = cell.split(':')
        lanes, nf, n = int(lanes), int(nf), int(n)
        m = ROW_MODELS[name]
        t0 = time.perf_counter()
        xs, y, _ = spectra_flat(name, nf, n)
        x = xs[:n].copy()
        counts = np.round(CUBE_SCALE * y).reshape(nf, n)
        del y
        if counts.min() < 1 or counts.max() > 65535:
            sys.exit('the counts leave uint16')
        w = 1.0 / np.sqrt(counts)                       # SQRT_Y on the host, as a caller of set_batch_data forms it
        data = {'float64': counts, 'float32': counts.astype(np.float32), 'uint16': counts.astype(np.uint16)}
        off = np.arange(nf + 1, dtype=np.int64) * n
        amp = np.where(np.arange(m['n_pars']) % 2 == 0, CUBE_SCALE, 1.0) if name == 'exp4' else np.array([CUBE_SCALE, 1.0, 1.0, CUBE_SCALE])
        start = np.tile(m['start'] * amp, (nf, 1))
        print('%-6s %3d lanes %6d fits x %5d points: data in %.1f s' % (name, lanes, nf, n, time.perf_counter() - t0), flush=True)
        ctx = _lib.Context(0)
        ctx.set_model(trace_model(m['model'], m['n_pars']))
        ctx.set_batch_lanes(lanes)

        def upload(form, dtype, et):
            t = time.perf_counter()
            if dtype is None:
                ctx.set_batch_data(off, xs, counts.reshape(-1), w.reshape(-1))
            else:
                ctx.set_batch_cube(x, data[np.dtype(dtype).name], et, w if et == 4 else None)
            return time.perf_counter() - t
        entry = dict(model=name, what=m['what'], n_active=len(m['active']), lanes=lanes, fits=nf, points=n, forms={})
        dev = {f[0]: [] for f in CUBE_FORMS}; up = {f[0]: [] for f in CUBE_FORMS}
        out = {}
        for it in range(a.warmup + a.launches):
            for form, dtype, et in CUBE_FORMS:       # the forms alternate launch by launch: a drift of the card's clock meets all alike
                t_up = upload(form, dtype, et)
                p, r, sec = ctx.fit_batch(start, m['active'], **kw)
                want = 'ragged' if dtype is None else ('cube', (np.float64, np.float32, np.uint16).index(dtype), et)
                if ctx.batch_lanes_used() != lanes or ctx.batch_form_used() != want:
                    sys.exit('the launch did not take the form asked for')
                if it >= a.warmup:
                    dev[form].append(sec)
                    if len(up[form]) < 3:
                        up[form].append(t_up)
                out[form] = (p, r)
        ctx.close()
        p0, r0 = out['ragged']
        for form, dtype, et in CUBE_FORMS:
            p, r = out[form]
            if not (np.array_equal(p, p0) and all(np.array_equal(r[f], r0[f]) for f in ('n_sweeps', 'n_chi2', 'n_omega', 'exit_reason', 'iterations'))):
                sys.exit('%s does not return what the ragged form returns' % form)
            d = statistics.median(dev[form])
            entry['forms'][form] = dict(device_ms=1e3 * d, device_ms_min=1e3 * min(dev[form]), device_ms_max=1e3 * max(dev[form]),
                                        upload_ms=1e3 * statistics.median(up[form]),
                                        bytes_per_point=24 if dtype is None else np.dtype(dtype).itemsize + (8 if et == 4 else 0))
        entry['passes'] = dict(sweeps=int(r0['n_sweeps'].sum()), chi2=int(r0['n_chi2'].sum()), omega=int(r0['n_omega'].sum()))
        entry['exit_reasons'] = {str(int(v)): int(np.sum(r0['exit_reason'] == v)) for v in sorted(set(r0['exit_reason'].tolist()))}
        entry['finite'] = bool(np.all(np.isfinite(p0)))
        for form, _, _ in CUBE_FORMS[1:]:
            e = entry['forms'][form]
            e['over_ragged_device_time'] = e['device_ms'] / entry['forms']['ragged']['device_ms']
            e['over_ragged_upload_time'] = e['upload_ms'] / entry['forms']['ragged']['upload_ms']
            e['wins'] = bool(RC.row_wins(e, entry['forms']['ragged']))
            e['loses'] = bool(RC.row_wins(entry['forms']['ragged'], e))
        rec['measurements'].append(entry)
        print('\n'.join('   %-15s device %9.3f ms [%.3f, %.3f], upload %9.1f ms%s' % (
            f, e['device_ms'], e['device_ms_min'], e['device_ms_max'], e['upload_ms'],
            '' if f == 'ragged' else ', %.2f of ragged%s' % (e['over_ragged_device_time'], ' -> wins' if e['wins'] else ' -> loses' if e['loses'] else ''))
            for f, e in entry['forms'].items()), flush=True)
        with open(a.out, 'w') as fh:          # (after every cell: a run that is cut short leaves what it measured)
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write('\n')
        del xs, counts, w, data
    print('wrote', a.out)


def cov_main(a):
    """fit_batch_errors against fit_batch alone and against fit_batch + batch_pass + numpy.linalg.inv (see the module's text)"""
    n_points, lanes = int(a.points or 1000), int(a.lanes or 64)
    rec = dict(method='per (model, fits) three routes alternating call by call on one context of one card in one run: fit = fit_batch alone, errors = '
                      'fit_batch_errors(scale=True), host = fit_batch + batch_pass at the fitted parameters + numpy.linalg.inv of the batch and its scaling '
                      'by chi2 / dof on the host; the median and the min-max of %d calls after %d warm-up calls; wall = around the route, device = what the '
                      'library reports (HIP events around the fit kernel, and around the fit kernel and gfh_k_batch_cov together); %d points per '
                      'spectrum, %d lanes per fit, lambda0 = %g, max_iter = %d; no events surround gfh_k_batch_pass, so its device time is not recorded; '
                      'no counter pass was made' % (a.launches, a.warmup, n_points, lanes, LAMBDA0, MAX_ITER), measurements=[])
    kw = dict(lambda_=LAMBDA0, max_iter=MAX_ITER)
    for name in ('gauss4', 'exp4'):
        m = ROW_MODELS[name]
        na = len(m['active'])
        for nf in [int(s) for s in a.sizes.split(',')]:
            xs, ys, ws = spectra_flat(name, nf, n_points)
            ctx = _lib.Context(0)
            ctx.set_model(trace_model(m['model'], m['n_pars']))
            ctx.set_batch_lanes(lanes)
            ctx.set_batch_data(np.arange(nf + 1, dtype=np.int64) * n_points, xs, ys, ws)
            del xs, ys, ws
            start = np.tile(m['start'], (nf, 1))
            wall = dict(fit=[], errors=[], host=[]); dev = dict(fit=[], errors=[])
            for it in range(a.warmup + a.launches):
                t0 = time.perf_counter()
                p, r, sec = ctx.fit_batch(start, m['active'], **kw)
                t1 = time.perf_counter()
                pe, re_, (cov, sigma, info), sec_e = ctx.fit_batch_errors(start, m['active'], scale=True, **kw)
                t2 = time.perf_counter()
                ph, rh, _ = ctx.fit_batch(start, m['active'], **kw)
                JTJ, _, chi2 = ctx.batch_pass(ph, m['active'])
                cov_h = np.linalg.inv(JTJ) * (chi2 / rh['dof'])[:, None, None]
                sigma_h = np.sqrt(np.diagonal(cov_h, axis1=1, axis2=2))
                t3 = time.perf_counter()
                if it >= a.warmup:
                    wall['fit'].append(t1 - t0); wall['errors'].append(t2 - t1); wall['host'].append(t3 - t2)
                    dev['fit'].append(sec); dev['errors'].append(sec_e)
            ctx.close()
            if not (np.array_equal(p, pe) and np.array_equal(p, ph) and np.all(info == 0)):
                sys.exit('the routes do not fit alike, or a covariance failed')
            entry = dict(model=name, what=m['what'], n_active=na, fits=nf, points=n_points, lanes=lanes,
                         worst_relative_sigma_difference_to_the_host_route=float(np.max(np.abs(sigma - sigma_h) / sigma_h)))
            for k, v in wall.items():
                entry['wall_ms_' + k] = dict(median=1e3 * statistics.median(v), min=1e3 * min(v), max=1e3 * max(v))
            for k, v in dev.items():
                entry['device_ms_' + k] = dict(median=1e3 * statistics.median(v), min=1e3 * min(v), max=1e3 * max(v))
            entry['device_ms_cov_kernel_by_difference'] = entry['device_ms_errors']['median'] - entry['device_ms_fit']['median']
            entry['wall_errors_over_fit'] = entry['wall_ms_errors']['median'] / entry['wall_ms_fit']['median']
            entry['wall_host_route_over_errors'] = entry['wall_ms_host']['median'] / entry['wall_ms_errors']['median']
            rec['measurements'].append(entry)
            print('%-6s %7d fits: wall fit %.2f ms, errors %.2f ms, host route %.2f ms; device fit %.3f ms, fit + cov %.3f ms; sigma differs from the host route by %.1e'
                  % (name, nf, entry['wall_ms_fit']['median'], entry['wall_ms_errors']['median'], entry['wall_ms_host']['median'],
                     entry['device_ms_fit']['median'], entry['device_ms_errors']['median'], entry['worst_relative_sigma_difference_to_the_host_route']), flush=True)
            with open(a.out, 'w') as fh:
                json.dump(rec, fh, indent=1, sort_keys=True)
                fh.write('\n')
    print('wrote', a.out)


# --bounds: one binding box per model -- the amplitude of the gaussian held below its truth of 3.0, the slowest decay time of the four
# exponentials below its truth of 30; the other sides keep the fits physical without touching them
BOUNDS_BOXES = {
    'gauss4': ([0.0, 0.0, 0.1, 0.0], [2.8, 10.0, np.inf, np.inf]),
    'exp4': ([0.0] * 8, [np.inf] * 7 + [29.0]),
}


def bounds_main(a):
    """fit_batch against fit_batch_bounded under infinite bounds and under a binding box (see the module's text)"""
    n_points, lanes = int(a.points or 1000), int(a.lanes or 64)
    rec = dict(method='per model three routes alternating call by call on one context of one card in one run: fit = fit_batch (the kernel '
                      'gfh_k_fit_batch, which is the parent commit\'s), bounded_inf = fit_batch_bounded with every bound infinite (gfh_k_fit_batch_bounded; '
                      'the same bits, checked), bounded_box = fit_batch_bounded with the binding box written down per entry; device time (HIP events '
                      'around the kernel) and wall time around the call, the median and the min-max of %d calls after %d warm-up calls; %d points per '
                      'spectrum, %d lanes per fit, lambda0 = %g, max_iter = %d; device_bounded_inf_over_fit = the medians\' ratio, beyond_spread = it '
                      'differs from 1 by more than the two routes\' min-max spreads together; no counter pass was made'
                      % (a.launches, a.warmup, n_points, lanes, LAMBDA0, MAX_ITER), measurements=[])
    kw = dict(lambda_=LAMBDA0, max_iter=MAX_ITER)
    for name in ('gauss4', 'exp4'):
        m = ROW_MODELS[name]
        na = len(m['active'])
        lo, hi = BOUNDS_BOXES[name]
        for nf in [int(s) for s in a.sizes.split(',')]:
            xs, ys, ws = spectra_flat(name, nf, n_points)
            ctx = _lib.Context(0)
            ctx.set_model(trace_model(m['model'], m['n_pars']))
            ctx.set_batch_lanes(lanes)
            ctx.set_batch_data(np.arange(nf + 1, dtype=np.int64) * n_points, xs, ys, ws)
            del xs, ys, ws
            start = np.tile(m['start'], (nf, 1))
            wall = dict(fit=[], bounded_inf=[], bounded_box=[]); dev = dict(fit=[], bounded_inf=[], bounded_box=[])
            for it in range(a.warmup + a.launches):
                t0 = time.perf_counter()
                p, r, sec = ctx.fit_batch(start, m['active'], **kw)
                t1 = time.perf_counter()
                pi, ri, ati, sec_i = ctx.fit_batch_bounded(start, m['active'], [-np.inf] * na, [np.inf] * na, **kw)
                t2 = time.perf_counter()
                pb, rb, atb, sec_b = ctx.fit_batch_bounded(start, m['active'], lo, hi, **kw)
                t3 = time.perf_counter()
                if it >= a.warmup:
                    wall['fit'].append(t1 - t0); wall['bounded_inf'].append(t2 - t1); wall['bounded_box'].append(t3 - t2)
                    dev['fit'].append(sec); dev['bounded_inf'].append(sec_i); dev['bounded_box'].append(sec_b)
            ctx.close()
            if not (np.array_equal(p, pi) and np.array_equal(r['chi2'], ri['chi2']) and np.array_equal(r['iterations'], ri['iterations']) and np.all(ati == 0)):
                sys.exit('infinite bounds changed a fit')
            A = np.array(m['active'])
            if not (np.all(pb[:, A] >= lo) and np.all(pb[:, A] <= hi)):
                sys.exit('a fit left the box')
            entry = dict(model=name, what=m['what'], n_active=na, fits=nf, points=n_points, lanes=lanes,
                         box=dict(lower=[float(v) if np.isfinite(v) else str(v) for v in lo], upper=[float(v) if np.isfinite(v) else str(v) for v in hi]),
                         fits_on_a_bound_under_the_box=int(np.sum(atb != 0)),
                         passes={k: dict(sweeps=int(q['n_sweeps'].sum()), chi2=int(q['n_chi2'].sum()), omega=int(q['n_omega'].sum()))
                                 for k, q in (('fit', r), ('bounded_inf', ri), ('bounded_box', rb))})
            for k in wall:
                entry['wall_ms_' + k] = _spread(wall[k]); entry['device_ms_' + k] = _spread(dev[k])
            f, b = entry['device_ms_fit'], entry['device_ms_bounded_inf']
            entry['device_bounded_inf_over_fit'] = b['median'] / f['median']
            entry['beyond_spread'] = bool(abs(b['median'] - f['median']) > (f['max'] - f['min']) + (b['max'] - b['min']))
            rec['measurements'].append(entry)
            print('%-6s %7d fits: device fit %.3f ms [%.3f, %.3f], bounded (no bound) %.3f ms [%.3f, %.3f], ratio %.4f%s; bounded (box) %.3f ms, %d fits on a bound'
                  % (name, nf, f['median'], f['min'], f['max'], b['median'], b['min'], b['max'], entry['device_bounded_inf_over_fit'],
                     ' (beyond the spread)' if entry['beyond_spread'] else '', entry['device_ms_bounded_box']['median'], entry['fits_on_a_bound_under_the_box']), flush=True)
            with open(a.out, 'w') as fh:
                json.dump(rec, fh, indent=1, sort_keys=True)
                fh.write('\n')
    print('wrote', a.out)


# --loss
LOSS_SIGMA, LOSS_NAMES = 1.0e-3, ('linear', 'cauchy', 'huber')


def loss_registers_record():
    """{model_lanesN_<loss>: the compiler's figures of the unit's kernels, gfh_k_fit_batch_bounded (a unit of its own) among them}"""
    from tests import models as M
    rec = {}
    c = _lib.Context(-1)
    for name, fn, n_pars in (('exp2', M.model_exp2, 4), ('exp4', M.model_exp4, 8)):
        c.set_model(trace_model(fn, n_pars))
        for lanes in (64, 16, 256):
            c.set_batch_lanes(lanes)
            for loss, lname in enumerate(LOSS_NAMES):
                c.set_batch_loss(loss, 1.0)
                r = kernel_registers(c.batch_source(list(range(n_pars))))
                r.update(kernel_registers(c.batch_source(list(range(n_pars)), bounded=True)))
                r.pop('gfh_k_batch_eval', None)
                rec['%s_lanes%d_%s' % (name, lanes, lname)] = r
    c.close()
    return rec


def loss_main(a):
    """the linear, Cauchy and Huber units against each other (see the module's text)"""
    n_points, lanes = int(a.points or 1000), int(a.lanes or 64)
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec.update(method='per model the three losses alternating call by call on one context of one card in one run: linear = the unit of the parent '
                      'commit, whose text did not change; cauchy, huber = set_batch_loss(1 / 2, 1.0).  weights 1 / sigma with sigma = %g (the ripple of '
                      'the spectra), every sample with (7919 k + 104729 i) %% 100 == 0 (k the fit, i the point: 1 %%) displaced by +12 sigma.  pass = '
                      'batch_pass at the start parameters, fit = fit_batch with lambda0 = %g, max_iter = %d, accth = 0.9; device time (HIP events around '
                      'the kernel), the median and the min-max of %d calls after %d warm-up calls; %d points per spectrum, %d lanes per fit; passes = '
                      'the fits\' total sweeps, chi2 passes and omega passes; no counter pass was made and no ratio is asserted'
                      % (LOSS_SIGMA, LAMBDA0, MAX_ITER, a.launches, a.warmup, n_points, lanes), measurements=[])
    kw = dict(lambda_=LAMBDA0, max_iter=MAX_ITER, accth=0.9)
    for name in ('gauss4', 'exp4'):
        m = ROW_MODELS[name]
        for nf in [int(s) for s in a.sizes.split(',')]:
            xs, ys, ws = spectra_flat(name, nf, n_points)
            hit = (7919 * np.arange(nf, dtype=np.int64)[:, None] + 104729 * np.arange(n_points, dtype=np.int64)[None, :]) % 100 == 0
            ys[hit.reshape(-1)] += 12.0 * LOSS_SIGMA
            ws[:] = 1.0 / LOSS_SIGMA
            ctx = _lib.Context(0)
            ctx.set_model(trace_model(m['model'], m['n_pars']))
            ctx.set_batch_lanes(lanes)
            ctx.set_batch_data(np.arange(nf + 1, dtype=np.int64) * n_points, xs, ys, ws)
            del xs, ys, ws
            start = np.tile(m['start'], (nf, 1))
            dev = {k: dict(pass_=[], fit=[]) for k in LOSS_NAMES}
            last = {}
            for it in range(a.warmup + a.launches):
                for loss, lname in enumerate(LOSS_NAMES):
                    ctx.set_batch_loss(loss, 1.0)
                    ctx.batch_pass(start, m['active'])
                    sec_p = ctx.batch_pass_seconds()
                    p, r, sec = ctx.fit_batch(start, m['active'], **kw)
                    last[lname] = (p, r)
                    if it >= a.warmup:
                        dev[lname]['pass_'].append(sec_p); dev[lname]['fit'].append(sec)
            ctx.close()
            entry = dict(model=name, what=m['what'], n_active=len(m['active']), fits=nf, points=n_points, lanes=lanes, displaced_samples=int(hit.sum()))
            for lname in LOSS_NAMES:
                p, r = last[lname]
                entry[lname] = dict(device_ms_pass=_spread(dev[lname]['pass_']), device_ms_fit=_spread(dev[lname]['fit']),
                                    passes=dict(sweeps=int(r['n_sweeps'].sum()), chi2=int(r['n_chi2'].sum()), omega=int(r['n_omega'].sum())),
                                    exits={str(k): int(np.sum(r['exit_reason'] == k)) for k in sorted(set(r['exit_reason'].tolist()))},
                                    median_parameters=[float(v) for v in np.median(p, axis=0)])
                e = entry[lname]
                print('%-6s %7d fits %-6s: pass %.4f ms [%.4f, %.4f], fit %.3f ms [%.3f, %.3f], sweeps %d chi2 %d omega %d'
                      % (name, nf, lname, e['device_ms_pass']['median'], e['device_ms_pass']['min'], e['device_ms_pass']['max'],
                         e['device_ms_fit']['median'], e['device_ms_fit']['min'], e['device_ms_fit']['max'],
                         e['passes']['sweeps'], e['passes']['chi2'], e['passes']['omega']), flush=True)
            rec['measurements'].append(entry)
            with open(a.out, 'w') as fh:
                json.dump(rec, fh, indent=1, sort_keys=True)
                fh.write('\n')
    print('wrote', a.out)


# --estimator
ESTIMATOR_NAMES = ('lsq', 'poisson')
ESTIMATOR_CELLS = 'gauss4:64:16384:1000,exp4:64:16384:1000,gauss4:16:131072:64,gauss4:256:256:65536'


def estimator_registers_record():
    """{model_lanesN_<estimator>: the compiler's figures of the unit's kernels, gfh_k_fit_batch_bounded (a unit of its own) among them}"""
    from tests import models as M
    rec = {}
    c = _lib.Context(-1)
    for name, fn, n_pars in (('exp2', M.model_exp2, 4), ('exp4', M.model_exp4, 8)):
        c.set_model(trace_model(fn, n_pars))
        for lanes in (64, 16, 256):
            c.set_batch_lanes(lanes)
            for est, ename in enumerate(ESTIMATOR_NAMES):
                c.set_batch_estimator(est)
                r = kernel_registers(c.batch_source(list(range(n_pars))))
                r.update(kernel_registers(c.batch_source(list(range(n_pars)), bounded=True)))
                r.pop('gfh_k_batch_eval', None)
                rec['%s_lanes%d_%s' % (name, lanes, ename)] = r
                print('%s %3d lanes %-7s: %s' % (name, lanes, ename, {k: (v['vgprs'], v['scratch_bytes_per_lane'], v['waves_per_simd']) for k, v in sorted(r.items())}), flush=True)
    c.close()
    return rec


def estimator_main(a):
    """the least-squares and the Poisson unit against each other (see the module's text)"""
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec.update(method='per cell the two estimators alternating call by call on one context of one card in one run: lsq = the unit of the parent '
                      'commit, whose text did not change; poisson = set_batch_estimator(1).  counts = round(%g x the model\'s spectrum), ragged form, '
                      'weights 1 / sqrt(y) (the Poisson unit reads them as a mask).  pass = batch_pass at the start parameters, fit = fit_batch with '
                      'lambda0 = %g, max_iter = %d; device time (HIP events around the kernel), the median and the min-max of %d calls after %d '
                      'warm-up calls; per_pass_in_fit = fit time / (sweeps + chi2 passes of all fits) x fits: the time of one pass over the batch '
                      'made inside a fit; no counter pass was made and no ratio is asserted' % (CUBE_SCALE, LAMBDA0, MAX_ITER, a.launches, a.warmup),
               measurements=[])
    kw = dict(lambda_=LAMBDA0, max_iter=MAX_ITER)
    for cell in a.cells.split(','):
        name, lanes, nf, n_points = cell.split(':')
        lanes, nf, n_points = int(lanes), int(nf), int(n_points)
        m = ROW_MODELS[name]
        xs, ys, ws = spectra_flat(name, nf, n_points)
        np.rint(CUBE_SCALE * ys, out=ys)
        np.divide(1.0, np.sqrt(ys), out=ws, where=ys > 0.0)
        ws[ys <= 0.0] = 0.0
        scale = np.where(np.arange(m['n_pars']) % 2 == 0, CUBE_SCALE, 1.0) if name == 'exp4' else np.array([CUBE_SCALE, 1.0, 1.0, CUBE_SCALE])
        ctx = _lib.Context(0)
        ctx.set_model(trace_model(m['model'], m['n_pars']))
        ctx.set_batch_lanes(lanes)
        ctx.set_batch_data(np.arange(nf + 1, dtype=np.int64) * n_points, xs, ys, ws)
        del xs, ys, ws
        start = np.tile(m['start'] * scale, (nf, 1))
        dev = {k: dict(pass_=[], fit=[]) for k in ESTIMATOR_NAMES}
        last = {}
        for it in range(a.warmup + a.launches):
            for est, ename in enumerate(ESTIMATOR_NAMES):
                ctx.set_batch_estimator(est)
                ctx.batch_pass(start, m['active'])
                sec_p = ctx.batch_pass_seconds()
                p, r, sec = ctx.fit_batch(start, m['active'], **kw)
                if ctx.batch_estimator_used() != est or ctx.batch_lanes_used() != lanes:
                    sys.exit('the launch did not run the unit asked for')
                last[ename] = (p, r)
                if it >= a.warmup:
                    dev[ename]['pass_'].append(sec_p); dev[ename]['fit'].append(sec)
        ctx.close()
        entry = dict(model=name, what=m['what'], n_active=len(m['active']), fits=nf, points=n_points, lanes=lanes)
        for ename in ESTIMATOR_NAMES:
            p, r = last[ename]
            passes = int(r['n_sweeps'].sum()) + int(r['n_chi2'].sum())
            entry[ename] = e = dict(device_ms_pass=_spread(dev[ename]['pass_']), device_ms_fit=_spread(dev[ename]['fit']),
                                    device_ms_per_pass_in_fit=_spread([v * nf / passes for v in dev[ename]['fit']]),
                                    passes=dict(sweeps=int(r['n_sweeps'].sum()), chi2=int(r['n_chi2'].sum())),
                                    exits={str(k): int(np.sum(r['exit_reason'] == k)) for k in sorted(set(r['exit_reason'].tolist()))},
                                    median_parameters=[float(v) for v in np.median(p, axis=0)])
            print('%-6s %3d lanes %7d x %5d %-7s: pass %.4f ms [%.4f, %.4f], fit %.3f ms [%.3f, %.3f], per pass in fit %.4f ms, sweeps %d chi2 %d'
                  % (name, lanes, nf, n_points, ename, e['device_ms_pass']['median'], e['device_ms_pass']['min'], e['device_ms_pass']['max'],
                     e['device_ms_fit']['median'], e['device_ms_fit']['min'], e['device_ms_fit']['max'], e['device_ms_per_pass_in_fit']['median'],
                     e['passes']['sweeps'], e['passes']['chi2']), flush=True)
        entry['poisson_over_lsq'] = dict(pass_=entry['poisson']['device_ms_pass']['median'] / entry['lsq']['device_ms_pass']['median'],
                                         per_pass_in_fit=entry['poisson']['device_ms_per_pass_in_fit']['median'] / entry['lsq']['device_ms_per_pass_in_fit']['median'])
        print('  poisson / lsq: pass %.3f, per pass in fit %.3f' % (entry['poisson_over_lsq']['pass_'], entry['poisson_over_lsq']['per_pass_in_fit']), flush=True)
        rec['measurements'].append(entry)
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write('\n')
    print('wrote', a.out)


EVAL_CELLS = 'gauss4:64:16384:1000,gauss4:64:131072:1000,gauss4:16:131072:64,gauss4:256:256:65536'


def eval_registers_record():
    """{model_lanesN: the compiler's figures of gfh_k_batch_eval}"""
    from tests import models as M
    rec = {}
    c = _lib.Context(-1)
    for name, fn, n_pars in (('exp2', M.model_exp2, 4), ('exp4', M.model_exp4, 8)):
        c.set_model(trace_model(fn, n_pars))
        for lanes in (64, 16, 256):
            c.set_batch_lanes(lanes)
            rec['%s_lanes%d' % (name, lanes)] = r = kernel_registers(c.batch_source(list(range(n_pars))))['gfh_k_batch_eval']
            if r['scratch_bytes_per_lane'] != 0 or r['lds_bytes_per_block'] != 0:
                sys.exit('gfh_k_batch_eval of %s at %d lanes has scratch or LDS: %s' % (name, lanes, r))
    c.close()
    return rec


def _spread(v):
    return dict(median=1e3 * statistics.median(v), min=1e3 * min(v), max=1e3 * max(v))


def eval_main(a):
    """batch_eval against batch_pass on the same batch in the same run, and against the bytes it must move (see the module's text)"""
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec = {k: v for k, v in rec.items() if k in ('registers', 'observed')}
    rec['method'] = ('per cell (model, lanes per fit, fits, points per spectrum) and data form -- ragged doubles with precomputed SQRT_Y weights, and '
                     'the uint16 cube under SQRT_Y of the same counts, round(%g x the model) -- three calls alternating on one context of one card in '
                     'one run: batch_pass, batch_eval(model) and batch_eval(model, residual, band) at the start parameters with the covariance '
                     'batch_covariance returns there; min, median and max of %d calls after %d warm-up calls; device = HIP events around the kernel, '
                     'wall = around the call (parameters and covariances down, launch, outputs back into numpy arrays); bytes_per_point = what the '
                     "form's load reads per point (ragged 24; uint16 2, the grid is shared) + 8 per requested output; fraction_of_8TBps = bytes_moved "
                     '/ device time / 8e12; over_batch_pass_device_time = the medians\' ratio; no counter pass was made' % (CUBE_SCALE, a.launches, a.warmup))
    rec['measurements'] = []
    for cell in a.cells.split(','):
        name, lanes, nf, n = cell.split(':')
        lanes, nf, n = int(lanes), int(nf), int(n)
        m = ROW_MODELS[name]
        t0 = time.perf_counter()
        xs, y, _ = spectra_flat(name, nf, n)
        x = xs[:n].copy()
        counts = np.round(CUBE_SCALE * y).reshape(nf, n)
        del y
        if counts.min() < 1 or counts.max() > 65535:
            sys.exit('the counts leave uint16')
        amp = np.where(np.arange(m['n_pars']) % 2 == 0, CUBE_SCALE, 1.0) if name == 'exp4' else np.array([CUBE_SCALE, 1.0, 1.0, CUBE_SCALE])
        pars = np.tile(m['start'] * amp, (nf, 1))
        print('%-6s %3d lanes %6d fits x %5d points: data in %.1f s' % (name, lanes, nf, n, time.perf_counter() - t0), flush=True)
        ctx = _lib.Context(0)
        ctx.set_model(trace_model(m['model'], m['n_pars']))
        ctx.set_batch_lanes(lanes)
        entry = dict(model=name, what=m['what'], n_active=len(m['active']), lanes=lanes, fits=nf, points=n, forms={})
        outs = {}
        for form, read in (('ragged', 24), ('uint16_sqrt_y', 2)):
            if form == 'ragged':
                ctx.set_batch_data(np.arange(nf + 1, dtype=np.int64) * n, xs, counts.reshape(-1), (1.0 / np.sqrt(counts)).reshape(-1))
            else:
                ctx.set_batch_cube(x, counts.astype(np.uint16), 1)
            cov, _, info = ctx.batch_covariance(pars, m['active'])
            if np.any(info != 0):
                sys.exit('a covariance failed')
            dev = dict(model=[], all=[]); wall = dict(model=[], all=[]); dev_pass = []
            for it in range(a.warmup + a.launches):
                ctx.batch_pass(pars, m['active'])
                sec_pass = ctx.batch_pass_seconds()
                t0 = time.perf_counter()
                o1 = ctx.batch_eval(pars, m['active'])
                t1 = time.perf_counter()
                o3 = ctx.batch_eval(pars, m['active'], cov=cov, residuals=True)
                t2 = time.perf_counter()
                want = 'ragged' if form == 'ragged' else ('cube', 2, 1)
                if ctx.batch_lanes_used() != lanes or ctx.batch_form_used() != want:
                    sys.exit('the launch did not take the form asked for')
                if it >= a.warmup:
                    dev_pass.append(sec_pass); dev['model'].append(o1[4]); dev['all'].append(o3[4])
                    wall['model'].append(t1 - t0); wall['all'].append(t2 - t1)
            outs[form] = [np.ravel(v) for v in o3[:3]]
            if not all(np.all(np.isfinite(v)) for v in outs[form]):
                sys.exit('an output is not finite')
            del o1, o3
            e = dict(pass_device_ms=_spread(dev_pass), outputs={})
            for what, n_out in (('model', 1), ('all', 3)):
                o = dict(device_ms=_spread(dev[what]), wall_ms=_spread(wall[what]), bytes_per_point=read + 8 * n_out)
                o['bytes_moved'] = o['bytes_per_point'] * nf * n
                o['fraction_of_8TBps'] = o['bytes_moved'] / (1e-3 * o['device_ms']['median']) / 8e12
                o['over_batch_pass_device_time'] = o['device_ms']['median'] / e['pass_device_ms']['median']
                e['outputs'][what] = o
            entry['forms'][form] = e
            print('   %-14s pass %8.3f ms | model %8.3f ms [%.3f, %.3f] %.2f of pass, %.3f of 8 TB/s, wall %8.1f ms | all %8.3f ms [%.3f, %.3f] %.2f of pass, '
                  '%.3f of 8 TB/s, wall %8.1f ms' % (form, e['pass_device_ms']['median'],
                  *[v for w_ in ('model', 'all') for o in [e['outputs'][w_]] for v in (o['device_ms']['median'], o['device_ms']['min'], o['device_ms']['max'],
                                                                                     o['over_batch_pass_device_time'], o['fraction_of_8TBps'], o['wall_ms']['median'])]),
                  flush=True)
        ctx.close()
        entry['the_cube_returns_the_ragged_forms_bits'] = bool(all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(outs['ragged'], outs['uint16_sqrt_y'])))
        rec['measurements'].append(entry)
        with open(a.out, 'w') as fh:          # (after every cell: a run that is cut short leaves what it measured)
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write('\n')
        del xs, counts, outs
    print('wrote', a.out)


FRAMES_CELLS = 'uint16:1:64:131072:1000,uint16:1:16:131072:64,uint16:1:256:256:65536,float32:1:64:16384:1000,float64:4:64:16384:1000'
FRAMES_ROUTES = ('cube', 'host_transpose', 'frames', 'frames_one_put', 'frames_8_puts')
FRAMES_MUST_WIN = ('uint16', 131072, 1000)


def _as_row(e):
    """a wall-time record in the keys tests/batch_records.row_wins reads"""
    return dict(device_ms=e['wall_ms'], device_ms_min=e['wall_ms_min'], device_ms_max=e['wall_ms_max'])


def frames_main(a):
    """a stack of frames (gfh_set_batch_frames) against the two routes a caller had before (see the module's text)"""
    from tests import batch_records as RC
    rec = dict(method='per cell (sample type, weight rule, lanes per fit, fits, points per spectrum) one stack of counts F [points][fits] -- round(%g x the '
                      'gauss4 model), the data of --cube transposed -- set through five routes that alternate call by call on one context of one card in one '
                      'run: cube = set_batch_cube of the already transposed array (the floor: the upload alone), host_transpose = '
                      'np.ascontiguousarray(F.T) + set_batch_cube (the route before this call existed; under USER the weights are transposed too), '
                      'frames = set_batch_frames with the default pieces (default_frames_per_put: where it equals points, the default IS one put and '
                      'the two routes are one call), frames_one_put = set_batch_frames with one put of the whole stack, frames_8_puts = eight pieces; '
                      'each round of the five begins one route later than the round before; wall time around the call(s), the median and the min-max of %d calls after %d warm-up calls; kernel_ms = device time of the transposing '
                      'kernels of one set (HIP events, summed over the puts, and under USER over both kernels), kernel_GB_per_s = bytes read plus '
                      'bytes written over it; fit_batch (lambda0 = %g, max_iter = %d) returns the same parameters and counts from cube, '
                      'host_transpose and frames (checked); wins = tests/batch_records.row_wins on the wall times; no counter pass was made, no '
                      'share of a peak is claimed' % (CUBE_SCALE, a.launches, a.warmup, LAMBDA0, MAX_ITER), measurements=[])
    kw = dict(lambda_=LAMBDA0, max_iter=MAX_ITER)
    m = ROW_MODELS['gauss4']
    for cell in a.cells.split(','):
        tname, et, lanes, nf, n = cell.split(':')
        et, lanes, nf, n = int(et), int(lanes), int(nf), int(n)
        dtype = np.dtype(tname)
        t0 = time.perf_counter()
        xs, y, _ = spectra_flat('gauss4', nf, n)
        x = xs[:n].copy()
        del xs
        counts = np.round(CUBE_SCALE * y).reshape(nf, n)
        del y
        if counts.min() < 1 or counts.max() > 65535:
            sys.exit('the counts leave uint16')
        Y = counts.astype(dtype)
        W = 1.0 / np.sqrt(counts) if et == 4 else None
        del counts
        F = np.ascontiguousarray(Y.T)                   # the stack as the instrument delivers it
        WF = None if W is None else np.ascontiguousarray(W.T)
        start = np.tile(m['start'] * np.array([CUBE_SCALE, 1.0, 1.0, CUBE_SCALE]), (nf, 1))
        print('%-8s rule %d %3d lanes %6d fits x %5d points: data in %.1f s' % (tname, et, lanes, nf, n, time.perf_counter() - t0), flush=True)
        ctx = _lib.Context(0)
        ctx.set_model(trace_model(m['model'], m['n_pars']))
        ctx.set_batch_lanes(lanes)

        def route(name):
            t = time.perf_counter()
            if name == 'cube':
                ctx.set_batch_cube(x, Y, et, W)
            elif name == 'host_transpose':
                ctx.set_batch_cube(x, np.ascontiguousarray(F.T), et, None if WF is None else np.ascontiguousarray(WF.T))
            else:
                ctx.set_batch_frames(x, F, et, WF, frames_per_put=n if name == 'frames_one_put' else (n + 7) // 8 if name == 'frames_8_puts' else 0)
            return time.perf_counter() - t
        wall = {r: [] for r in FRAMES_ROUTES}; kern = {r: [] for r in FRAMES_ROUTES[2:]}
        for it in range(a.warmup + a.launches):
            # the routes alternate call by call, and the round begins one route later each time: a drift of the host or the card meets
            # all alike, and no route is always the one behind the host transpose's half second of CPU work
            for r in FRAMES_ROUTES[it % len(FRAMES_ROUTES):] + FRAMES_ROUTES[:it % len(FRAMES_ROUTES)]:
                t = route(r)
                if it >= a.warmup:
                    wall[r].append(t)
                    if r in kern:
                        kern[r].append(ctx.batch_frames_seconds())
        out = {}
        for r in FRAMES_ROUTES[:3]:
            route(r)
            p, res, _ = ctx.fit_batch(start, m['active'], **kw)
            if ctx.batch_lanes_used() != lanes or ctx.batch_form_used() != ('cube', (np.float64, np.float32, np.uint16).index(dtype.type), et):
                sys.exit('the launch did not take the form asked for')
            out[r] = (p, res)
        p0, r0 = out['cube']
        for r in FRAMES_ROUTES[1:3]:
            p, res = out[r]
            if not (np.array_equal(p.view(np.uint64), p0.view(np.uint64)) and
                    all(np.array_equal(res[f], r0[f]) for f in ('n_sweeps', 'n_chi2', 'n_omega', 'exit_reason', 'iterations'))):
                sys.exit('%s does not return what set_batch_cube returns' % r)
        mem = ctx.device_memory()['workspace_pool']
        ctx.close()
        per_frame = nf * (dtype.itemsize + (8 if et == 4 else 0))
        moved = 2 * n * per_frame
        entry = dict(sample_type=tname, error_type=et, lanes=lanes, fits=nf, points=n, stack_MB=n * per_frame / 1e6,
                     default_frames_per_put=int(min(n, max(1, (256 << 20) // per_frame))), routes={}, fits_equal=True,
                     finite=bool(np.all(np.isfinite(p0))), device_bytes_held=int(mem))
        for r in FRAMES_ROUTES:
            e = dict(wall_ms=1e3 * statistics.median(wall[r]), wall_ms_min=1e3 * min(wall[r]), wall_ms_max=1e3 * max(wall[r]))
            if r in kern:
                k = statistics.median(kern[r])
                e.update(kernel_ms=1e3 * k, kernel_ms_min=1e3 * min(kern[r]), kernel_ms_max=1e3 * max(kern[r]), kernel_GB_per_s=moved / k / 1e9)
            entry['routes'][r] = e
        for r in FRAMES_ROUTES[1:]:
            e = entry['routes'][r]
            e['over_cube_wall_time'] = e['wall_ms'] / entry['routes']['cube']['wall_ms']
        for r in FRAMES_ROUTES[2:]:
            e = entry['routes'][r]
            e['over_host_transpose_wall_time'] = e['wall_ms'] / entry['routes']['host_transpose']['wall_ms']
            e['wins'] = bool(RC.row_wins(_as_row(e), _as_row(entry['routes']['host_transpose'])))
            e['loses'] = bool(RC.row_wins(_as_row(entry['routes']['host_transpose']), _as_row(e)))
        one, dflt = entry['routes']['frames_one_put'], entry['routes']['frames']
        entry['default_pieces_against_one_put'] = ('faster' if RC.row_wins(_as_row(dflt), _as_row(one)) else
                                                   'slower' if RC.row_wins(_as_row(one), _as_row(dflt)) else 'within the spreads')
        rec['measurements'].append(entry)
        print('\n'.join('   %-15s wall %9.2f ms [%.2f, %.2f]%s%s' % (
            r, e['wall_ms'], e['wall_ms_min'], e['wall_ms_max'],
            '' if r == 'cube' else ', %.2f x the upload alone' % e['over_cube_wall_time'],
            '' if 'kernel_ms' not in e else ', kernel %.3f ms = %.0f GB/s, %.3f of host_transpose%s' % (
                e['kernel_ms'], e['kernel_GB_per_s'], e['over_host_transpose_wall_time'], ' -> wins' if e['wins'] else ' -> loses' if e['loses'] else ''))
            for r, e in entry['routes'].items()), flush=True)
        with open(a.out, 'w') as fh:          # (after every cell: a run that is cut short leaves what it measured)
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write('\n')
        if (tname, nf, n) == FRAMES_MUST_WIN and not entry['routes']['frames']['wins']:
            sys.exit('at %d x %d %s the frames route does not beat the host transpose by more than the two spreads' % (nf, n, tname))
        del Y, W, F, WF
    print('wrote', a.out)


def rows_main(a, points, lanes_list):
    """the two forms against each other over spectrum lengths (see the module's text)"""
    from tests import batch_records as RC
    nf = int(a.sizes.split(',')[0])
    rec = dict(method='%d fits per launch; per (model, length, form) the median and the min-max of %d launches after %d warm-up launches; device = HIP '
                      'events around the kernel, wall = around the call; lambda0 = %g, max_iter = %d and no other exit, so both forms run the same passes up to the accept / reject decisions that rounding takes past convergence (the totals are in each record); '
                      'the forms alternate on one context, one card, one run' % (nf, a.launches, a.warmup, LAMBDA0, MAX_ITER),
               n_fits=nf, measurements=[])
    if os.path.exists(a.out):          # (--registers and --observed of earlier calls stay)
        old = json.load(open(a.out))
        for k in ('registers', 'observed_maxima_against_the_oracle'):
            if k in old:
                rec[k] = old[k]
    kw = dict(lambda_=LAMBDA0, max_iter=MAX_ITER)
    for name, m in ROW_MODELS.items():
        ctx = _lib.Context(0)
        ctx.set_model(trace_model(m['model'], m['n_pars']))
        for n in points:
            if name == 'gauss4':
                x, y, _ = spectra(nf, n)
            else:
                x, y = spectra_exp4(nf, n)
            off = np.arange(nf + 1, dtype=np.int64) * n
            ctx.set_batch_data(off, np.tile(x, nf), y.ravel(), np.ones(nf * n))
            del y
            start = np.tile(m['start'], (nf, 1))
            entry = dict(model=name, what=m['what'], n_active=len(m['active']), points=n, lanes={})
            times = {l: ([], []) for l in lanes_list}
            out = {}
            for it in range(a.warmup + a.launches):
                for l in lanes_list:          # the forms alternate launch by launch: a drift of the card's clock meets both alike
                    t0 = time.perf_counter()
                    p, r, sec = ctx.fit_batch(start, m['active'], lanes_per_fit=l, **kw)
                    t1 = time.perf_counter()
                    if ctx.batch_lanes_used() != l:
                        sys.exit('the launch did not take the form asked for')
                    if it >= a.warmup:
                        times[l][0].append(sec); times[l][1].append(t1 - t0)
                    out[l] = (p, r)
            for l in lanes_list:
                dev, wall = times[l]
                p, r = out[l]
                d = statistics.median(dev); w = statistics.median(wall)
                entry['lanes'][str(l)] = dict(
                    device_ms=1e3 * d, device_ms_min=1e3 * min(dev), device_ms_max=1e3 * max(dev), wall_ms=1e3 * w, wall_ms_min=1e3 * min(wall),
                    wall_ms_max=1e3 * max(wall), device_us_per_fit=1e6 * d / nf, wall_us_per_fit=1e6 * w / nf,
                    passes=dict(sweeps=int(r['n_sweeps'].sum()), chi2=int(r['n_chi2'].sum()), omega=int(r['n_omega'].sum())),
                    exit_reasons={str(int(v)): int(np.sum(r['exit_reason'] == v)) for v in sorted(set(r['exit_reason'].tolist()))},
                    finite=bool(np.all(np.isfinite(p))))
            if '16' in entry['lanes'] and '64' in entry['lanes']:
                a16, a64 = out[16], out[64]
                entry['fits_with_equal_counts_in_both_forms'] = int(np.sum((a16[1]['n_sweeps'] == a64[1]['n_sweeps']) & (a16[1]['n_chi2'] == a64[1]['n_chi2']) &
                                                                           (a16[1]['exit_reason'] == a64[1]['exit_reason'])))
                entry['row_over_wave_device_time'] = entry['lanes']['16']['device_ms'] / entry['lanes']['64']['device_ms']
                entry['row_wins'] = bool(RC.row_wins(entry['lanes']['16'], entry['lanes']['64']))
            rec['measurements'].append(entry)
            print('%-6s %5d points: %s%s' % (name, n, ', '.join('%s lanes %9.3f ms [%.3f, %.3f] (%.4f us per fit)' % (
                l, e['device_ms'], e['device_ms_min'], e['device_ms_max'], e['device_us_per_fit']) for l, e in sorted(entry['lanes'].items())),
                ' -> row form wins' if entry.get('row_wins') else ''), flush=True)
        ctx.close()
    if all('row_wins' in m for m in rec['measurements']):
        rule = RC.implied_rule(rec)
        rec['auto_rule'] = dict(sixteen_lanes_up_to={str(k): v for k, v in rule.items()},
                                text='per active-count class (measured at 4 and at 8 active parameters; 1 ... 4 take the first, 5 ... 8 the second): 16 lanes '
                                     'up to the largest measured length at which the row form beat the wave form by more than the two min-max spreads; '
                                     '0: nowhere, auto stays at 64 lanes')
    if a.observed:
        rec['observed_maxima_against_the_oracle'] = json.load(open(a.observed))
    with open(a.out, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', a.out)


def workgroup_main(a, points, sizes, models):
    """the 256-lane form against the 64-lane form over points per spectrum and fits per launch (see the module's text)"""
    from tests import batch_records as RC
    lanes_list = [64, 256]
    rec = dict(method='per (model, fits per launch, points per spectrum, form) the median and the min-max of %d launches after %d warm-up launches; device = HIP '
                      'events around the kernel, wall = around the call; lambda0 = %g, max_iter = %d and no other exit, so both forms run the same passes up to the '
                      'accept / reject decisions that rounding takes past convergence (the totals are in each record); the forms alternate launch by launch on one '
                      'context, one card, one run; cells above 2^30 points in total are dropped; no counter pass was made' % (a.launches, a.warmup, LAMBDA0, MAX_ITER),
               measurements=[])
    if os.path.exists(a.out):          # (--registers and --observed of earlier calls stay, and the models this call does not measure)
        old = json.load(open(a.out))
        for k in ('registers', 'observed_maxima_against_the_oracle'):
            if k in old:
                rec[k] = old[k]
        rec['measurements'] = [m for m in old.get('measurements', []) if m['model'] not in models]
    kw = dict(lambda_=LAMBDA0, max_iter=MAX_ITER)
    for name in models:
        m = ROW_MODELS[name]
        ctx = _lib.Context(0)
        ctx.set_model(trace_model(m['model'], m['n_pars']))
        for nf in sizes:
            for n in points:
                if nf * n > 2 ** 30:
                    continue
                t0 = time.perf_counter()
                x, y, w = spectra_flat(name, nf, n)
                ctx.set_batch_data(np.arange(nf + 1, dtype=np.int64) * n, x, y, w)
                del x, y, w
                print('%-6s %5d fits x %5d points: data in %.1f s' % (name, nf, n, time.perf_counter() - t0), flush=True)
                start = np.tile(m['start'], (nf, 1))
                entry = dict(model=name, what=m['what'], n_active=len(m['active']), fits=nf, points=n, lanes={})
                times = {l: ([], []) for l in lanes_list}
                out = {}
                for it in range(a.warmup + a.launches):
                    for l in lanes_list:          # the forms alternate launch by launch: a drift of the card's clock meets both alike
                        t0 = time.perf_counter()
                        p, r, sec = ctx.fit_batch(start, m['active'], lanes_per_fit=l, **kw)
                        t1 = time.perf_counter()
                        if ctx.batch_lanes_used() != l:
                            sys.exit('the launch did not take the form asked for')
                        if it >= a.warmup:
                            times[l][0].append(sec); times[l][1].append(t1 - t0)
                        out[l] = (p, r)
                for l in lanes_list:
                    dev, wall = times[l]
                    p, r = out[l]
                    d = statistics.median(dev); wl = statistics.median(wall)
                    entry['lanes'][str(l)] = dict(
                        device_ms=1e3 * d, device_ms_min=1e3 * min(dev), device_ms_max=1e3 * max(dev), wall_ms=1e3 * wl, wall_ms_min=1e3 * min(wall),
                        wall_ms_max=1e3 * max(wall), device_us_per_fit=1e6 * d / nf, wall_us_per_fit=1e6 * wl / nf,
                        passes=dict(sweeps=int(r['n_sweeps'].sum()), chi2=int(r['n_chi2'].sum()), omega=int(r['n_omega'].sum())),
                        exit_reasons={str(int(v)): int(np.sum(r['exit_reason'] == v)) for v in sorted(set(r['exit_reason'].tolist()))},
                        finite=bool(np.all(np.isfinite(p))))
                a256, a64 = out[256], out[64]
                entry['fits_with_equal_counts_in_both_forms'] = int(np.sum((a256[1]['n_sweeps'] == a64[1]['n_sweeps']) & (a256[1]['n_chi2'] == a64[1]['n_chi2']) &
                                                                           (a256[1]['exit_reason'] == a64[1]['exit_reason'])))
                entry['workgroup_over_wave_device_time'] = entry['lanes']['256']['device_ms'] / entry['lanes']['64']['device_ms']
                entry['workgroup_wins'] = bool(RC.row_wins(entry['lanes']['256'], entry['lanes']['64']))
                rec['measurements'].append(entry)
                print('%-6s %5d fits x %5d points: %s%s' % (name, nf, n, ', '.join('%s lanes %9.3f ms [%.3f, %.3f]' % (
                    l, e['device_ms'], e['device_ms_min'], e['device_ms_max']) for l, e in sorted(entry['lanes'].items(), key=lambda it: int(it[0]))),
                    ' -> workgroup form wins' if entry['workgroup_wins'] else ''), flush=True)
                with open(a.out, 'w') as fh:          # (after every cell: a run that is cut short leaves what it measured)
                    json.dump(rec, fh, indent=1, sort_keys=True)
                    fh.write('\n')
        ctx.close()
    if a.observed:
        rec['observed_maxima_against_the_oracle'] = json.load(open(a.observed))
    with open(a.out, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', a.out)


def main():
    global N_POINTS
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', default=None, help='points per spectrum (default 1000); with --rows a list (default 8,16,32,64,128,256,1000)')
    ap.add_argument('--lanes', default=None, help='lanes per fit, 64, 16 or 256 (default 64); with --rows a list (default 64,16)')
    ap.add_argument('--rows', action='store_true', help='the two forms of the batch kernels against each other, into profiles/batch_rows.json')
    ap.add_argument('--workgroup', action='store_true', help='the 256-lane form of the batch kernels against the 64-lane form, into profiles/batch_workgroup.json')
    ap.add_argument('--cube', action='store_true', help='a batch as a data cube against the ragged form of the same spectra, into profiles/batch_cube.json')
    ap.add_argument('--frames', action='store_true', help='a stack of frames against the host transpose and the upload alone, into profiles/batch_frames.json')
    ap.add_argument('--cov', action='store_true', help='fit_batch_errors against fit_batch alone and against the host route, into profiles/batch_cov.json')
    ap.add_argument('--bounds', action='store_true', help='fit_batch_bounded under infinite bounds and under a binding box against fit_batch, into profiles/batch_bounds.json')
    ap.add_argument('--loss', action='store_true', help='the Cauchy and Huber units of the batch kernels against the linear unit, into profiles/batch_loss.json')
    ap.add_argument('--estimator', action='store_true', help='the Poisson unit of the batch kernels against the least-squares unit, into profiles/batch_mle.json')
    ap.add_argument('--eval', action='store_true', help='batch_eval against batch_pass and against the bytes it moves, into profiles/batch_eval.json')
    ap.add_argument('--cells', default=None, help='with --cube and --eval: model:lanes:fits:points, ...; with --frames: sample type:error type:lanes:fits:points, ...')
    ap.add_argument('--models', default='gauss4,exp4', help='with --workgroup: the models measured by this call (the record keeps the others)')
    ap.add_argument('--registers', action='store_true', help='with --rows or --workgroup: only the register figures of the four kernels into the record; no GPU is needed')
    ap.add_argument('--sizes', default='1024,16384,131072')
    ap.add_argument('--launches', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--one-at-a-time', type=int, default=200)
    ap.add_argument('--rate-fits', type=int, default=16384)
    ap.add_argument('--observed', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--observed-only', action='store_true', help='replace observed_maxima_against_the_oracle of the record at --out by --observed; '
                                                                 'nothing is timed, no GPU is needed')
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'batch_mle.json' if a.estimator else 'batch_loss.json' if a.loss else 'batch_bounds.json' if a.bounds else 'batch_eval.json' if a.eval else 'batch_cov.json' if a.cov else 'batch_frames.json' if a.frames else 'batch_cube.json' if a.cube else 'batch_workgroup.json' if a.workgroup else 'batch_rows.json' if a.rows else 'batch_fits.json')
    if a.cells is None:
        a.cells = ESTIMATOR_CELLS if a.estimator else FRAMES_CELLS if a.frames else EVAL_CELLS if a.eval else CUBE_CELLS
    if (a.loss or a.estimator) and a.registers:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
        rec['registers'] = estimator_registers_record() if a.estimator else loss_registers_record()
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write('\n')
        print('wrote', a.out)
        return
    if a.eval and (a.registers or a.observed):
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
        if a.registers:
            rec['registers'] = eval_registers_record()
        if a.observed:
            rec['observed'] = {k: v for k, v in json.load(open(a.observed)).items() if k.startswith('eval_')}
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write('\n')
        print(json.dumps({k: rec[k] for k in ('registers', 'observed') if k in rec}, indent=1, sort_keys=True))
        print('wrote', a.out)
        return
    if (a.rows or a.workgroup or a.cube) and a.registers:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
        rec['registers'] = cube_registers_record() if a.cube else registers_record((256,) if a.workgroup else (64, 16))
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write('\n')
        print(json.dumps(rec['registers'], indent=1, sort_keys=True))
        print('wrote', a.out)
        return
    sizes = [int(s) for s in a.sizes.split(',')]
    if a.observed and not os.path.exists(a.observed):
        sys.exit('--observed %s: no such file (run tests/test_gpu_batch_shapes.py tests/test_gpu_batch.py in one pytest process under GADFIT_BATCH_OBSERVE first)' % a.observed)
    if a.observed_only:
        if not a.observed:
            sys.exit('--observed-only needs --observed FILE')
        rec = json.load(open(a.out))
        rec['observed_maxima_against_the_oracle'] = json.load(open(a.observed))
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write('\n')
        print('wrote', a.out)
        return
    if a.launches < 5:
        sys.exit('at least 5 timed launches')
    if a.eval:
        return eval_main(a)
    if a.estimator:
        return estimator_main(a)
    if a.bounds:
        if a.sizes == '1024,16384,131072':
            a.sizes = '16384'
        return bounds_main(a)
    if a.loss:
        if a.sizes == '1024,16384,131072':
            a.sizes = '16384'
        return loss_main(a)
    if a.cov:
        if a.sizes == '1024,16384,131072':
            a.sizes = '16384,131072'
        return cov_main(a)
    if a.frames:
        return frames_main(a)
    if a.cube:
        return cube_main(a)
    if a.workgroup:
        if a.sizes == '1024,16384,131072':
            a.sizes = '64,256,1024,16384'
        return workgroup_main(a, [int(v) for v in (a.points or '1000,4096,16384,65536').split(',')], [int(v) for v in a.sizes.split(',')], a.models.split(','))
    if a.rows:
        if a.sizes == '1024,16384,131072':
            a.sizes = '131072'
        return rows_main(a, [int(v) for v in (a.points or '8,16,32,64,128,256,1000').split(',')], [int(v) for v in (a.lanes or '64,16').split(',')])
    N_POINTS = int(a.points or 1000)
    lanes = int(a.lanes or 64)
    tape = trace_model(model, 4)
    x, y, pos = spectra(max(sizes + [a.one_at_a_time, a.rate_fits if a.rate_fits else 0]))
    rec = dict(problem=dict(points=N_POINTS, parameters=4, max_iter=MAX_ITER, lambda0=LAMBDA0, model='gaussian on a background',
                            source='tests/fortran/bench_many_small_fits.F90'),
               method='median of %d launches after %d warm-up launches; device = HIP events around the kernel, wall = around the call' % (a.launches, a.warmup),
               batches=[])
    kw = dict(lambda_=LAMBDA0, max_iter=MAX_ITER)
    ctx = _lib.Context(0)
    ctx.set_model(tape)
    ctx.set_batch_lanes(lanes)
    rec['problem']['lanes_per_fit'] = lanes
    batch_out = {}
    for nf in sizes:
        xs = np.tile(x, nf); ys = np.ascontiguousarray(y[:nf]).ravel(); ws = np.ones(nf * N_POINTS)
        off = np.arange(nf + 1, dtype=np.int64) * N_POINTS
        t0 = time.perf_counter()
        ctx.set_batch_data(off, xs, ys, ws)
        t_upload = time.perf_counter() - t0
        start = np.tile(START, (nf, 1))
        dev, wall = [], []
        for it in range(a.warmup + a.launches):
            t0 = time.perf_counter()
            p, r, sec = ctx.fit_batch(start, ACTIVE, **kw)
            t1 = time.perf_counter()
            if it >= a.warmup:
                dev.append(sec); wall.append(t1 - t0)
        if not np.all(np.abs(p[:, 1] - pos[:nf]) < 1e-2):
            sys.exit('a fit of the batch is off')
        passes = dict(sweeps=int(r['n_sweeps'].sum()), chi2=int(r['n_chi2'].sum()), omega=int(r['n_omega'].sum()))
        d = statistics.median(dev); w = statistics.median(wall)
        b = dict(n_fits=nf, device_ms=1e3 * d, device_ms_min=1e3 * min(dev), device_ms_max=1e3 * max(dev), wall_ms=1e3 * w,
                 wall_ms_min=1e3 * min(wall), wall_ms_max=1e3 * max(wall), upload_ms=1e3 * t_upload,
                 device_us_per_fit=1e6 * d / nf, wall_us_per_fit=1e6 * w / nf, passes=passes,
                 iterations=sorted(set(int(v) for v in r['iterations'])), exit_reasons=sorted(set(int(v) for v in r['exit_reason'])),
                 point_evaluations_per_s=(passes['sweeps'] + passes['chi2'] + passes['omega']) * N_POINTS / d)
        rec['batches'].append(b)
        batch_out[nf] = (p, r)
        print('batch of %7d fits: device %9.3f ms (%.3f us per fit), wall %9.3f ms (%.3f us per fit), upload %.1f ms' % (
            nf, b['device_ms'], b['device_us_per_fit'], b['wall_ms'], b['wall_us_per_fit'], b['upload_ms']), flush=True)
    ctx.close()

    # yardstick 1: one at a time, set_data + fit on one context of this process (the parent commit's capability)
    n1 = a.one_at_a_time
    if n1 > 0:
        c = _lib.Context(0)
        c.set_model(tape)
        c.set_keep_jacobian(2)                      # as the procedural API runs its fits: the Jacobian is written only if read
        ones = np.ones(N_POINTS)
        outs, t_cycle, t_fit, same = [], [], [], 0
        for k in range(-3, n1):                     # three warm-up spectra
            j = max(k, 0)
            t0 = time.perf_counter()
            c.set_data(x, y[j], ones, [0, N_POINTS])
            c.init_weights(0)                       # gadf_set_errors(NONE), as the procedural API does per spectrum
            t1 = time.perf_counter()
            out, r1 = c.fit([START], ACTIVE, [0] * 4, **kw)
            t2 = time.perf_counter()
            if k >= 0:
                t_cycle.append(t2 - t0); t_fit.append(t2 - t1); outs.append(out.ravel())
                pb, rb = batch_out[sizes[0]]
                if j < sizes[0]:
                    same += int((r1.iterations, r1.n_sweeps, r1.n_chi2, r1.exit_reason) ==
                                (int(rb['iterations'][j]), int(rb['n_sweeps'][j]), int(rb['n_chi2'][j]), int(rb['exit_reason'][j])))
        c.close()
        m = min(n1, sizes[0])
        pb = batch_out[sizes[0]][0][:m]
        one = dict(n_fits=n1, ms_per_fit_set_data_and_fit=1e3 * statistics.median(t_cycle), ms_per_fit_fit_only=1e3 * statistics.median(t_fit),
                   ms_per_fit_mean=1e3 * sum(t_cycle) / n1,
                   same_counts_as_batch='%d of %d' % (same, m),
                   worst_relative_parameter_difference_to_batch=float(np.max(np.abs(np.array(outs[:m]) - pb) / np.abs(pb))))
        rec['one_at_a_time'] = one
        print('one at a time: %.3f ms per fit (set_data + fit), %.3f ms fit only; counts equal to the batch in %s' % (
            one['ms_per_fit_set_data_and_fit'], one['ms_per_fit_fit_only'], one['same_counts_as_batch']), flush=True)
        for b in rec['batches']:
            b['speedup_wall_over_one_at_a_time'] = one['ms_per_fit_set_data_and_fit'] * 1e3 / b['wall_us_per_fit']
            b['speedup_device_over_one_at_a_time'] = one['ms_per_fit_set_data_and_fit'] * 1e3 / b['device_us_per_fit']
            print('  %7d fits: %.0f x per fit by wall time, %.0f x by device time' % (
                b['n_fits'], b['speedup_wall_over_one_at_a_time'], b['speedup_device_over_one_at_a_time']))

    # yardstick 2: the N-sized kernels of the same model on the batch's points as ONE dataset
    if a.rate_fits > 0:
        nf = a.rate_fits
        c = _lib.Context(0)
        c.set_model(tape)
        c.set_keep_jacobian(0)                      # the batch kernel writes no Jacobian either
        n = nf * N_POINTS
        c.set_data(np.tile(x, nf), np.ascontiguousarray(y[:nf]).ravel(), np.ones(n), [0, n])
        c.init_weights(0)
        jac, dim = c.jacobian_indices(ACTIVE, [0] * 4)
        c.sweep([START], ACTIVE, jac, dim)
        c.chi2([START])
        c.time_kernel(0, 3); c.time_kernel(2, 3)
        t_sweep = statistics.median(c.time_kernel(0, 10) for _ in range(5)) * 1e-3
        t_chi2 = statistics.median(c.time_kernel(2, 10) for _ in range(5)) * 1e-3
        c.close()
        rate = dict(points=n, sweep_ns_per_point=1e9 * t_sweep / n, chi2_ns_per_point=1e9 * t_chi2 / n)
        rec['n_sized_kernels'] = rate
        print('N-sized kernels on %d points: sweep %.4f ns per point, chi2 %.4f ns per point' % (n, rate['sweep_ns_per_point'], rate['chi2_ns_per_point']))
        for b in rec['batches']:
            full = (b['passes']['sweeps'] * t_sweep + b['passes']['chi2'] * t_chi2) / n * N_POINTS      # the same passes at the full card's rates
            b['n_sized_kernels_time_for_the_same_passes_ms'] = 1e3 * full
            b['n_sized_kernels_time_over_batch_time'] = full / (1e-3 * b['device_ms'])
            print('  %7d fits: the same passes through the N-sized kernels %.3f ms = %.2f x the batch kernel\'s time' % (
                b['n_fits'], 1e3 * full, b['n_sized_kernels_time_over_batch_time']))
    if a.observed:
        rec['observed_maxima_against_the_oracle'] = json.load(open(a.observed))
    with open(a.out, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
