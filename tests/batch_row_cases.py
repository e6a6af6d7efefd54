"""The inputs of tests/test_gpu_batch_rows.py: the 16-lane form of the batch kernels (gfh_set_batch_lanes(16): a DPP row per fit, four
fits per wave, sixteen per workgroup).  tests/test_cpu_batch_rows.py runs the selection rule and the compilations without a GPU.
Everything here is deterministic and needs no GPU; the spectra, the starts, the scenarios and the rule (select) are those of
tests/batch_cases.py and tests/test_gpu_batch.py, imported, not restated.

Part R1: model_exp2, tests.batch_cases.spectrum_n(n, s), s = 0 ... 5, with lengths at the ROW's edges -- n = na, one below / at /
one above 8, 16, 32, 48 and 64 (a quarter, one, two, three and four rows of points), 80 and 257 (the row loop) -- in an order that
puts short spectra beside long ones, so that the four fits of a wave differ in their trip counts.
The active counts 1 ... 8 come from Part 2 of tests/batch_cases.py as it stands (part2, exp4_sets, EXP4_ARGS, EXP4_ORDER)."""
import functools

import numpy as np

from gadfit_amd.ad import trace_model
from tests import batch_cases as BC
from tests import models as M
from tests.test_gpu_batch import SCENARIOS, start_of

LENGTHS = (4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 257)
ACTIVE = [0, 1, 2, 3]
FIT_SCENARIOS = ('a', 'b', 'c')
ONE_ACTIVE = [1]
ONE_SCENARIOS = ('a', 'b')
ONE_ACTIVE_CAP = 0.05              # of the one-parameter fits (both scenarios together) may fail the rule; none of the four-parameter fits
SAME_BITS_MAX_N = 16               # up to here a fit has at most one point per lane in both forms: the two forms return the same bits
LARGE_MAX_N = 33                   # the large batch tiles the spectra up to this length
LARGE_FITS = 2 ** 17 + 3
CUTS = (17, 16, 15, 5, 4, 3, 1)    # batch sizes that leave rows, waves and (17) all but one row of a last workgroup without a fit


def r1_order():
    """(n, s) of the 114 spectra in batch order: per s the lengths from both ends inwards (4, 257, 5, 80, 7, 65, ...), as
    batch_cases.part1_order, the middle length last"""
    per_s = []
    for i in range(len(LENGTHS) // 2):
        per_s += [LENGTHS[i], LENGTHS[-1 - i]]
    per_s.append(LENGTHS[len(LENGTHS) // 2])
    return [(n, s) for s in range(6) for n in per_s]


@functools.lru_cache(maxsize=None)
def r1():
    """(tape, order [(n, s)], truths [114][4], Batch)"""
    order = r1_order()
    sp = [BC.spectrum_n(n, s) for n, s in order]
    return trace_model(M.model_exp2, 4), order, np.array([it[0] for it in sp]), BC.Batch([it[1:4] for it in sp])


def r1_starts(off, active=ACTIVE):
    """only the active parameters are moved off truth, as batch_cases.part1_starts"""
    truths = r1()[2]
    starts = truths.copy()
    starts[:, active] = np.array([start_of(t, off) for t in truths])[:, active]
    return starts


@functools.lru_cache(maxsize=None)
def r1_selection(name, one_active=False):
    """batch_cases.select over the 114 spectra under a scenario of test_gpu_batch.py: [(kept, oracle result, self-difference, margin)]"""
    tape, _, _, batch = r1()
    active = ONE_ACTIVE if one_active else ACTIVE
    off, kw = SCENARIOS[name]
    starts = r1_starts(off, active)
    return [BC.select(tape, *batch.items[b], starts[b], active, kw) for b in range(len(batch.items))]


def sub_batch(indices):
    """the spectra `indices` of R1 as a batch of their own, in that order"""
    items = r1()[3].items
    return BC.Batch([items[k] for k in indices])


def row_units():
    """[(tape, active list)]: every batch translation unit tests/test_gpu_batch_rows.py asks for, each in BOTH forms (the row form is
    the one under test; the wave form of the same unit is what two of the tests compare it with)"""
    units = [(r1()[0], ACTIVE), (r1()[0], ONE_ACTIVE)]
    seen = set()
    for a in [a for name in sorted(BC.EXP4_ARGS) for a in BC.exp4_sets(name)] + [o[0] for pair in BC.EXP4_ORDER.values() for o in pair]:
        if tuple(a) not in seen:
            seen.add(tuple(a))
            units.append((BC.part2()[0], list(a)))
    return units


# ---- the auto rule, as profiles/batch_rows.json implies it -----------------------------------------------------------------------
def row_wins(row, wave):
    """Is the row form faster than the wave form at one measured (model, length)?  row, wave: the two forms' records of one run on
    one card (device_ms the median, device_ms_min, device_ms_max of the timed launches).  Faster by more than the two forms' own
    min-max spread: the medians differ by more than the sum of the two spreads."""
    gain = wave['device_ms'] - row['device_ms']
    return gain > (row['device_ms_max'] - row['device_ms_min']) + (wave['device_ms_max'] - wave['device_ms_min'])


def implied_rule(record):
    """{n_active class: the largest measured length at which the row form wins (0: nowhere)} from a record of tools/bench_batch.py --rows"""
    out = {}
    for m in record['measurements']:
        k = int(m['n_active'])
        out.setdefault(k, 0)
        if row_wins(m['lanes']['16'], m['lanes']['64']):
            out[k] = max(out[k], int(m['points']))
    return out
