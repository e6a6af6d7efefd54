"""The curves of a plain fit, measured (gfh_eval; the kernels of device/eval.hip) -> profiles/plain_eval.json.

    python tools/bench_eval.py --registers     the compiler's figures of the four kernels per unit of REGISTER_UNITS; needs no GPU
    python tools/bench_eval.py                 the timings below on card 0 (the registers of the record are kept)

Sizes: the headline, N = 1e7 points x model_gauss8 with 32 active parameters, and BASELINE config 2, N = 1e7 x model_exp4 with 8.
Per size the device time of the kernel (HIP events round the launch, Context.eval's `seconds`) for
  (a) model + residual          gfh_k_eval
  (b) model + residual + band   gfh_k_eval_band, with the covariance Context.covariance returns at the same parameters.
Each figure is the median (and the min and max) of LAUNCHES calls; in every call the kernel is launched WARM + 1 times back to back
(Context.debug_eval_launches) and the last launch is the one timed: a call ends with the copy of 80 ... 240 MB back to the host,
an idle gap for the card, and the first twenty launches behind such a gap run slow (the cold_start of the bench line).
Yardstick 2, same context, same run: gfh_k_chi2 without its residual store (Context.time_kernel(2) after a fit under keep_jacobian
mode 2; WARM launches untimed, then LAUNCHES x REPS timed).  chi2 reads x, y, w: 24 B per point; (a) reads the same and writes two
doubles: 40 B.  The expectation stated before anything was measured: (a) <= 1.25 x (40 / 24) x chi2.  The record holds the ratio and
whether it is met.
(b): the fraction of the FP64 floor of its own instruction count.  Per point the band adds na^2 + na multiplications and as many
additions (no contraction: two instructions where an FMA would be one) to the body of gfh_k_sweep's point function; counted from the
kernel's own assembly as the FP64 vector instructions per lane, at 4 cycles per wave and instruction on a SIMD (MI355X: 256 CUs x 4
SIMDs x 16 lanes, 2.4 GHz): floor = instructions x N / (256 x 4 x 16 lanes x 2.4e9 / s).  No ratio is fixed in advance.
Yardstick 1, wall time against wall time, at N_HOST = 1e6 points (at 1e7 x 32 the host would hold a 2.56 GB Jacobian twice): what a
user did before -- Context.sweep with a stored Jacobian, Context.jacobian() read back, the band in numpy with the same covariance --
against Context.covariance + Context.eval(model, residual, band).  No counter pass was made."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gadfit_amd import _lib  # noqa: E402
from gadfit_amd.ad import trace_model  # noqa: E402
from tests import models as M  # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'plain_eval.json')
KERNELS = ('gfh_k_eval', 'gfh_k_eval_band', 'gfh_k_eval_grid', 'gfh_k_eval_grid_band')
REGISTER_UNITS = ('exp2_4active', 'exp4_8active', 'gauss3_12active', 'gauss8_32active', 'gauss9_36active', 'global7_7active')
WARM, LAUNCHES, REPS = 24, 7, 20
N, N_HOST = 10_000_000, 1_000_000
PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9          # FP64 vector instructions per lane and second, one per lane every 4 cycles of a 16-lane SIMD


def _compile(src, flag):
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, 'unit.hip')
        with open(f, 'w') as fh:
            fh.write('#include <hip/hip_runtime.h>\n' + src)
        out = os.path.join(d, 'unit.s')
        r = subprocess.run([os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', 'hipcc'), '-O3', '-std=c++17', '--offload-arch=gfx950',
                            '-ffp-contract=on', '--cuda-device-only', flag, f, '-o', out, '-Rpass-analysis=kernel-resource-usage'],
                           capture_output=True, text=True, check=True)
        return r.stderr, open(out).read() if flag == '-S' else ''


def kernel_registers(src):
    """{kernel: {vgprs, agprs, sgprs, scratch_bytes_per_lane, waves_per_simd, lds_bytes_per_block, fp64_valu, scalar_loads}} of the
    eval kernels of a generated source, as hipcc compiles it with hiprtc's options"""
    remarks, asm = _compile(src, '-S')
    out, name = {}, None
    keys = {'VGPRs': 'vgprs', 'AGPRs': 'agprs', 'TotalSGPRs': 'sgprs', 'ScratchSize [bytes/lane]': 'scratch_bytes_per_lane',
            'Occupancy [waves/SIMD]': 'waves_per_simd', 'LDS Size [bytes/block]': 'lds_bytes_per_block'}
    for line in remarks.splitlines():
        m = re.search(r'remark:\s+(.*?): (\S+) \[-Rpass', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            name = m.group(2) if m.group(2) in KERNELS else None
            if name:
                out[name] = {}
        elif name and m.group(1) in keys:
            out[name][keys[m.group(1)]] = int(m.group(2))
    for k in out:          # the body between the kernel's label and its s_endpgm
        body = asm[asm.index('\n%s:' % k):]
        body = body[:body.index('s_endpgm')]
        out[k]['fp64_valu'] = len(re.findall(r'\n\s+v_(?:fma|mul|add|fmac|rcp|sqrt|div_\w+|trig_preop|ldexp|frexp_\w+|rndne|fract|min|max)_f64', body))
        out[k]['scalar_loads'] = len(re.findall(r'\n\s+s_load_dword', body))
    return out


def _units():
    g7 = trace_model(M.model_global7, 7)
    return {'exp2_4active': (trace_model(M.model_exp2, 4), list(range(4))), 'exp4_8active': (trace_model(M.model_exp4, 8), list(range(8))),
            'gauss3_12active': (trace_model(M.make_model_gaussK(3), 12), list(range(12))),
            'gauss8_32active': (trace_model(M.model_gauss8, 32), list(range(32))),
            'gauss9_36active': (trace_model(M.make_model_gaussK(9), 36), list(range(36))), 'global7_7active': (g7, list(range(7)))}


def load_record():
    return json.load(open(OUT)) if os.path.exists(OUT) else {}


def save_record(rec):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')


def registers_main():
    rec = load_record()
    rec['registers'] = {}
    c = _lib.Context(-1)
    for label, (tape, active) in _units().items():          # (the source of a context without data: the one-dataset form)
        c.set_model(tape)
        rec['registers'][label] = r = kernel_registers(c.eval_source(active))
        for k, v in r.items():
            print(label, k, v)
            if v['scratch_bytes_per_lane'] or v['lds_bytes_per_block']:
                sys.exit('%s of %s has scratch or LDS' % (k, label))
    c.close()
    save_record(rec)
    print('wrote', OUT)


def _spread(v):
    return dict(median=1e3 * statistics.median(v), min=1e3 * min(v), max=1e3 * max(v))


def measure(label, model, fn_numpy, truth, lo, fp64_band):
    na = truth.size
    active, glob = list(range(na)), [0] * na
    x, y, s = M.make_single(fn_numpy, truth, N, lo, 100.0)
    start = M.start_values(truth).reshape(1, na)
    ctx = _lib.Context(0)
    ctx.set_model(trace_model(model, na))
    ctx.set_data(x, y, 1.0 / s, [0, N])
    del y, s
    cov, _, info = ctx.covariance(start, active, glob)
    if info:
        sys.exit('the covariance failed')
    entry = dict(size=label, points=N, n_active=na)
    ctx.debug_eval_launches(WARM + 1)
    dev = dict(a=[], b=[])
    for _ in range(LAUNCHES):
        dev['a'].append(ctx.eval(start, active, glob, residuals=True)[3])
        dev['b'].append(ctx.eval(start, active, glob, cov=cov, residuals=True)[3])
    ctx.debug_eval_launches(1)
    # yardstick 2: gfh_k_chi2 without its residual store, and with it
    chi2 = {}
    for name, mode, nbytes in (('chi2_no_res_store', 2, 24), ('chi2', 1, 32)):
        ctx.set_keep_jacobian(mode)
        ctx.fit(start, active, glob, lambda_=1.0, max_iter=1)
        ctx.time_kernel(2, WARM)
        ms = [ctx.time_kernel(2, REPS) for _ in range(LAUNCHES)]
        chi2[name] = dict(device_ms=dict(median=statistics.median(ms), min=min(ms), max=max(ms)), bytes_per_point=nbytes)
    ctx.set_keep_jacobian(1)
    ctx.close()
    entry['a_model_residual'] = a = dict(device_ms=_spread(dev['a']), bytes_per_point=40)
    a['fraction_of_8TBps'] = 40 * N / (1e-3 * a['device_ms']['median']) / 8e12
    entry['b_model_residual_band'] = b = dict(device_ms=_spread(dev['b']), bytes_per_point=48, fp64_valu_per_point=fp64_band)
    b['fp64_floor_ms'] = 1e3 * fp64_band * N / PEAK_LANE_OPS
    b['fp64_floor_over_device_time'] = b['fp64_floor_ms'] / b['device_ms']['median']
    entry['yardstick_chi2'] = chi2
    ref = chi2['chi2_no_res_store']['device_ms']['median']
    a['over_chi2_no_res_store'] = a['device_ms']['median'] / ref
    a['expected_at_most'] = 1.25 * 40 / 24
    a['expectation_met'] = bool(a['over_chi2_no_res_store'] <= a['expected_at_most'])
    print('%s: (a) %.3f ms [%.3f, %.3f] = %.2f x chi2 without the store (%.3f ms; expected <= %.2f: %s), %.2f of 8 TB/s | (b) %.3f ms [%.3f, %.3f], '
          'FP64 floor %.3f ms = %.2f of it' % (label, a['device_ms']['median'], a['device_ms']['min'], a['device_ms']['max'], a['over_chi2_no_res_store'], ref,
                                                  a['expected_at_most'], a['expectation_met'], a['fraction_of_8TBps'], b['device_ms']['median'],
                                                  b['device_ms']['min'], b['device_ms']['max'], b['fp64_floor_ms'], b['fp64_floor_over_device_time']), flush=True)
    # yardstick 1 at N_HOST: wall against wall
    xh, yh, sh = M.make_single(fn_numpy, truth, N_HOST, lo, 100.0)
    ctx = _lib.Context(0)
    ctx.set_model(trace_model(model, na))
    ctx.set_data(xh, yh, 1.0 / sh, [0, N_HOST])
    jac, dim = ctx.jacobian_indices(active, glob)
    wall = dict(host_route=[], eval_route=[])
    for it in range(2 + 3):
        t0 = time.perf_counter()
        JTJ, _, _ = ctx.sweep(start, active, jac, dim)
        Ch = np.linalg.inv(JTJ)
        g = ctx.jacobian(na) / ctx.weights()[:, None]
        res_h = ctx.residuals()
        band_h = np.sqrt(np.maximum(np.einsum('ia,ab,ib->i', g, Ch, g), 0.0))
        t1 = time.perf_counter()
        C2, _, _ = ctx.covariance(start, active, glob)
        m2, r2, b2, _ = ctx.eval(start, active, glob, cov=C2, residuals=True)
        t2 = time.perf_counter()
        if it >= 2:
            wall['host_route'].append(t1 - t0); wall['eval_route'].append(t2 - t1)
    ctx.close()
    entry['yardstick_host_route'] = dict(points=N_HOST, wall_ms_host_route=_spread(wall['host_route']), wall_ms_covariance_and_eval=_spread(wall['eval_route']),
                                         host_route_over_eval=statistics.median(wall['host_route']) / statistics.median(wall['eval_route']),
                                         worst_relative_band_difference=float(np.max(np.abs(b2 - band_h) / band_h)),
                                         residuals_equal=bool(np.array_equal(r2, res_h)))
    print('   host route at N = %d: %.1f ms against covariance + eval %.1f ms; bands differ by %.1e' %
          (N_HOST, entry['yardstick_host_route']['wall_ms_host_route']['median'], entry['yardstick_host_route']['wall_ms_covariance_and_eval']['median'],
           entry['yardstick_host_route']['worst_relative_band_difference']), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--registers', action='store_true', help='only the compiler\'s figures into the record; no GPU is needed')
    a = ap.parse_args()
    if a.registers:
        return registers_main()
    rec = load_record()
    if 'registers' not in rec:
        sys.exit('run with --registers first: the FP64 floor of (b) is counted from the kernels\' assembly')
    rec['method'] = __doc__.split('\n\n', 2)[2]
    rec['measurements'] = []
    for label, model, fn, truth, lo, unit in (('headline: N = 1e7 x model_gauss8, 32 active', M.model_gauss8, M.gauss8_numpy, M.gauss8_truth(), 0.0, 'gauss8_32active'),
                                              ('BASELINE config 2: N = 1e7 x model_exp4, 8 active', M.model_exp4, M.exp4_numpy, M.EXP4_TRUTH, 0.0, 'exp4_8active')):
        rec['measurements'].append(measure(label, model, fn, truth, lo, rec['registers'][unit]['gfh_k_eval_band']['fp64_valu']))
        save_record(rec)          # (after every size: a run that is cut short leaves what it measured)
    print('wrote', OUT)


if __name__ == '__main__':
    main()
