"""Batched independent fits (gfh_fit_batch) measured against what the project offered for them before, on the problem of
profiles/r05_small_fits.txt: 1000 points, a Gaussian on a background, 4 parameters, lambda0 = 1, max_iter = 30.

    python tools/bench_batch.py [--sizes 1024,16384,131072] [--launches 7] [--warmup 2] [--one-at-a-time 200]
                                [--observed FILE [--observed-only]] [--out profiles/batch_fits.json]

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
process, so a module run alone writes its own keys only).  --observed-only: the record's timings stay, its maxima are replaced."""
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

N_POINTS, MAX_ITER, LAMBDA0 = 1000, 30, 1.0
START = np.array([2.5, 4.3, 1.0, 0.3])
ACTIVE = [0, 1, 2, 3]


def model(p, x):
    return p[0] * exp(-((x - p[1]) / p[2]) ** 2) + p[3]


def spectra(n_fits):
    """bench_many_small_fits.F90's spectrum k, with the peak position spread over [4, 5) so that a large batch holds no two alike"""
    x = 10.0 * (np.arange(N_POINTS) + 0.5) / N_POINTS
    k = np.arange(1, n_fits + 1, dtype=np.float64)
    pos = 4.0 + np.mod(k * 0.6180339887498949, 1.0)
    y = np.empty((n_fits, N_POINTS))
    for lo in range(0, n_fits, 8192):
        hi = min(n_fits, lo + 8192)
        y[lo:hi] = 3.0 * np.exp(-((x[None, :] - pos[lo:hi, None]) / 0.8) ** 2) + 0.5 + 1.0e-3 * np.sin(977.0 * x[None, :] + k[lo:hi, None])
    return x, y, pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1024,16384,131072')
    ap.add_argument('--launches', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--one-at-a-time', type=int, default=200)
    ap.add_argument('--rate-fits', type=int, default=16384)
    ap.add_argument('--observed', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'batch_fits.json'))
    ap.add_argument('--observed-only', action='store_true', help='replace observed_maxima_against_the_oracle of the record at --out by --observed; '
                                                                 'nothing is timed, no GPU is needed')
    a = ap.parse_args()
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
    tape = trace_model(model, 4)
    x, y, pos = spectra(max(sizes + [a.one_at_a_time, a.rate_fits if a.rate_fits else 0]))
    rec = dict(problem=dict(points=N_POINTS, parameters=4, max_iter=MAX_ITER, lambda0=LAMBDA0, model='gaussian on a background',
                            source='tests/fortran/bench_many_small_fits.F90'),
               method='median of %d launches after %d warm-up launches; device = HIP events around the kernel, wall = around the call' % (a.launches, a.warmup),
               batches=[])
    kw = dict(lambda_=LAMBDA0, max_iter=MAX_ITER)
    ctx = _lib.Context(0)
    ctx.set_model(tape)
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
