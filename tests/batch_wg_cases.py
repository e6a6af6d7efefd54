"""The inputs of tests/test_gpu_batch_wg.py: the 256-lane form of the batch kernels (gfh_set_batch_lanes(256): a workgroup of four
waves per fit, grid = number of fits).  tests/test_cpu_batch_wg.py runs the selection rule and the compilations without a GPU.
Everything here is deterministic and needs no GPU; the spectra, the starts, the scenarios and the rule (select) are those of
tests/batch_cases.py and tests/test_gpu_batch.py, imported, not restated.

Part W1: model_exp2, tests.batch_cases.spectrum_n(n, s), s = 0 ... 5, with lengths at the edges of the WORKGROUP's row of 256 points:
n = na and na + 1, one below / at / one above 64, 128, 192 (the edges of each wave's share of the first row), 256, 512, 768 (one,
two, three rows), 1000 and 1025 (the fourth row, one live lane in a fifth), and 4097 (a row loop of 16, one live lane in the 17th) -- in an order that puts
short spectra beside long ones.
The active counts 1 ... 8 come from Part 2 of tests/batch_cases.py as it stands (part2, exp4_sets, EXP4_ARGS, EXP4_ORDER)."""
import functools

import numpy as np

from gadfit_amd.ad import trace_model
from tests import batch_cases as BC
from tests import models as M
from tests.test_gpu_batch import SCENARIOS, start_of

LENGTHS = (4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1000, 1025, 4097)
ACTIVE = [0, 1, 2, 3]
FIT_SCENARIOS = ('a', 'b', 'c')
ONE_ACTIVE = [1]
ONE_SCENARIOS = ('a',)             # (scenario b with one parameter fails the rule on 23 of the 138 and is left out)
ONE_ACTIVE_MAX_DROPPED = 3         # of the 138 one-parameter fits may fail the rule (2 %); none of the 414 four-parameter fits
SAME_BITS_MAX_N = 64               # up to here waves 1 ... 3 add exact zeros: the workgroup form returns the wave form's bits
LARGE_MAX_N = 257                  # the large batch tiles the spectra up to this length
LARGE_FITS = 70003                 # more workgroups than 65535
CUTS = (5, 2, 1)


def w1_order():
    """(n, s) of the 138 spectra in batch order: per s the lengths from both ends inwards (4, 4097, 5, 1025, 63, 1000, ...), as
    batch_cases.part1_order, the middle length last"""
    per_s = []
    for i in range(len(LENGTHS) // 2):
        per_s += [LENGTHS[i], LENGTHS[-1 - i]]
    per_s.append(LENGTHS[len(LENGTHS) // 2])
    return [(n, s) for s in range(6) for n in per_s]


@functools.lru_cache(maxsize=None)
def w1():
    """(tape, order [(n, s)], truths [138][4], Batch)"""
    order = w1_order()
    sp = [BC.spectrum_n(n, s) for n, s in order]
    return trace_model(M.model_exp2, 4), order, np.array([it[0] for it in sp]), BC.Batch([it[1:4] for it in sp])


def w1_starts(off, active=ACTIVE):
    """only the active parameters are moved off truth, as batch_cases.part1_starts"""
    truths = w1()[2]
    starts = truths.copy()
    starts[:, active] = np.array([start_of(t, off) for t in truths])[:, active]
    return starts


@functools.lru_cache(maxsize=None)
def w1_selection(name, one_active=False):
    """batch_cases.select over the 138 spectra under a scenario of test_gpu_batch.py: [(kept, oracle result, self-difference, margin)]"""
    tape, _, _, batch = w1()
    active = ONE_ACTIVE if one_active else ACTIVE
    off, kw = SCENARIOS[name]
    starts = w1_starts(off, active)
    return [BC.select(tape, *batch.items[b], starts[b], active, kw) for b in range(len(batch.items))]


def sub_batch(indices):
    """the spectra `indices` of W1 as a batch of their own, in that order"""
    items = w1()[3].items
    return BC.Batch([items[k] for k in indices])


def wg_units():
    """[(tape, active list)]: every batch translation unit tests/test_gpu_batch_wg.py asks for in the 256-lane form (the W1 units are
    asked for in the 64-lane form too, which tests/batch_row_cases.row_units already lists)"""
    units = [(w1()[0], ACTIVE), (w1()[0], ONE_ACTIVE)]
    seen = set()
    for a in [a for name in sorted(BC.EXP4_ARGS) for a in BC.exp4_sets(name)] + [o[0] for pair in BC.EXP4_ORDER.values() for o in pair]:
        if tuple(a) not in seen:
            seen.add(tuple(a))
            units.append((BC.part2()[0], list(a)))
    return units


# ---- profiles/batch_workgroup.json ------------------------------------------------------------------------------------------------
MUST_WIN = tuple((model, 256, points) for model in ('gauss4', 'exp4') for points in (16384, 65536))


def cell(record, model, fits, points):
    """the measurement of one (model, fits per launch, points per spectrum) of a record of tools/bench_batch.py --workgroup, or None"""
    for m in record['measurements']:
        if (m['model'], int(m['fits']), int(m['points'])) == (model, fits, points):
            return m
    return None
