"""The three forms of the batch kernels (64, 16 and 256 lanes per fit: a wave, a DPP row, a workgroup of four waves) as a table, and
the inputs of the suite in tests/batch_form_suite.py written once over it.  tests/test_cpu_batch_cases.py runs the selection rule
over every form without a GPU.  Everything here is deterministic and needs no GPU; the spectra (spectrum_n), the rule (select) and Parts 2 and 3
are those of tests/batch_cases.py, the scenarios those of tests/batch_common.py.

Part 1 of a form: model_exp2, batch_cases.spectrum_n(n, s), s = 0 ... 5, with n over the form's `lengths` -- the edges of ITS row of
lanes -- from both ends inwards, so that short spectra lie beside long ones:
  64: n = na, n < 64, one below / at / one above 64, 128, 192, and rows enough that the row loop dominates (20001: 313 rows);
  16: n = na, one below / at / one above 8, 16, 32, 48 and 64 (a quarter, one, two, three and four rows), 80 and 257 (the row loop);
 256: n = na and na + 1, one below / at / one above 64, 128, 192 (each wave's share of the first row), 256, 512, 768 (one, two, three
      rows), 1000 and 1025 (the fourth row, one live lane in a fifth), and 4097 (a row loop of 16, one live lane in the 17th).
A field is in the table because two forms differ in it.  Where they differ for no reason that anybody wrote down, the table keeps
what each form's tests did when they were three modules, and says so."""
import dataclasses
import functools

import numpy as np

from gadfit_amd.ad import trace_model
from tests import batch_cases as BC
from tests import models as M
from tests.batch_common import SCENARIOS, TOL_CHI2, TOL_FIT, TOL_PARS, start_of

ACTIVE = [0, 1, 2, 3]
FIT_SCENARIOS = ('a', 'b', 'c')
ONE_ACTIVE = [1]
SAMPLES = 6                        # spectra per length (s = 0 ... 5)


def _one_at_a_time(n):
    """the 64-lane form's clean masks: one spectrum clean, for the first and the last, a short one between long ones, a long one
    between short ones, two in the middle and three that end with a full row"""
    n = n.tolist()
    last = len(n) - 1
    short_between_long = next(k for k in range(1, last) if n[k - 1] > 4096 and n[k] < 64 and n[k + 1] > 4096)
    long_between_short = next(k for k in range(1, last) if n[k - 1] < 64 and n[k] > 4096 and n[k + 1] < 64)
    exact_rows = [k for k in range(len(n)) if n[k] in (64, 128, 192)][:3]
    return [np.arange(len(n)) == k for k in [0, last, short_between_long, long_between_short, 53, 54] + exact_rows]


def _residues(*moduli):
    """clean masks: the fits of each residue class of each modulus in turn"""
    return lambda n: [np.arange(n.size) % m == k for m in moduli for k in range(m)]


@dataclasses.dataclass(frozen=True)
class Form:
    lanes: int
    prefix: str                    # of the form's keys in the record of observed maxima
    lengths: tuple
    spectra: int                   # SAMPLES of each length
    edges: frozenset               # lengths the list must hold
    short_beside_long: object      # n [spectra] -> bool: what the batch order is there for
    # active = [1]: the scenarios run, and those that also take the pass.  (b) with one parameter fails the rule on 23 of the 138
    # spectra of the 256-lane form and is left out there; why the 64-lane form takes the pass under (a) alone is not recorded.
    one_scenarios: tuple
    one_pass_scenarios: tuple
    one_cap_each: object           # so many of the one-parameter fits may fail the rule in one scenario (None: not held) ...
    one_cap_total: object          # ... and so many in all its scenarios together (None: not held)
    one_kept_per_length: int       # every length keeps that many of its six one-parameter fits, in each scenario
    same_bits_max_n: object        # up to here the form returns the wave form's bits (None: it is the wave form) ...
    same_bits_lengths: tuple       # ... which are these of its lengths
    large_max_n: int               # the large batch tiles the spectra up to this length, ...
    large_spectra: int             # ... which are this many, ...
    large_fits: int                # ... to this many fits
    every_single_fit_and_reversed: bool          # isolation: each fit alone and the batch reversed (not recorded why not at 64 lanes)
    cuts: tuple                    # isolation: the batch cut to its first k fits
    nan_clean: object              # n [spectra] -> the masks of fits left clean while the others are NaN
    nan_scenarios: tuple           # (not recorded why (c) alone at 64 lanes)
    part1_tol: tuple               # bounds on Part 1's fitted parameters and chi2 (Part 2's are TOL_FIT in every form)
    observes_order_between: bool   # the caller's-order test records the difference between its two orders (only ever at 64 lanes)


WAVE = Form(
    lanes=64, prefix='shapes',
    lengths=(4, 5, 6, 8, 17, 31, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000, 4097, 20001), spectra=108,
    edges=frozenset({63, 64, 65, 127, 128, 129, 191, 192, 193}),
    # a long spectrum between two short ones and a short one between two long ones
    short_beside_long=lambda n: (any(n[k - 1] < 64 and n[k] > 4096 and n[k + 1] < 64 for k in range(1, len(n) - 1))
                                 and any(n[k - 1] > 4096 and n[k] < 64 and n[k + 1] > 4096 for k in range(1, len(n) - 1))),
    one_scenarios=('a', 'b'), one_pass_scenarios=('a',),
    # under (b) every seventh one-parameter fit makes a chi2 comparison closer than MARGIN: no scenario loses more than a quarter of 108
    one_cap_each=27, one_cap_total=None, one_kept_per_length=1,
    same_bits_max_n=None, same_bits_lengths=(), large_max_n=193, large_spectra=90, large_fits=2 ** 17 + 3,
    every_single_fit_and_reversed=False,
    cuts=(107, 106, 105, 7, 5, 3, 2),          # 3, 2, 1 live waves in the last workgroup, and small batches
    nan_clean=_one_at_a_time, nan_scenarios=('c',), part1_tol=(TOL_FIT, TOL_FIT), observes_order_between=True)
ROWS = Form(
    lanes=16, prefix='rows',
    lengths=(4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 257), spectra=114,
    edges=frozenset({7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65}),
    # four neighbours (the rows of a wave) with trip counts that differ: one row of points beside five and more
    short_beside_long=lambda n: any(min(n[k:k + 4]) <= 16 and max(n[k:k + 4]) > 64 for k in range(0, len(n) - 2, 4)),
    one_scenarios=('a', 'b'), one_pass_scenarios=('a', 'b'),
    one_cap_each=None, one_cap_total=0.05 * 2 * 114, one_kept_per_length=4,
    same_bits_max_n=16, same_bits_lengths=(4, 5, 7, 8, 9, 15, 16),          # at most one point per lane in both forms
    large_max_n=33, large_spectra=66, large_fits=2 ** 17 + 3,
    every_single_fit_and_reversed=True,
    cuts=(17, 16, 15, 5, 4, 3, 1),             # rows, waves and (17) all but one row of a last workgroup without a fit
    nan_clean=_residues(2, 4),                 # both parities, then each of the four rows of a wave in turn the only clean one
    nan_scenarios=('a', 'c'), part1_tol=(TOL_FIT, TOL_FIT), observes_order_between=False)
WORKGROUP = Form(
    lanes=256, prefix='wg',
    lengths=(4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1000, 1025, 4097),
    spectra=138,
    edges=frozenset(64 * k + e for k in (1, 2, 3, 4, 8, 12) for e in (-1, 0, 1)),
    short_beside_long=lambda n: any(n[k] <= 64 and n[k + 1] > 1024 for k in range(len(n) - 1)),
    one_scenarios=('a',), one_pass_scenarios=('a',),
    one_cap_each=None, one_cap_total=3, one_kept_per_length=4,
    same_bits_max_n=64, same_bits_lengths=(4, 5, 63, 64),          # waves 1 ... 3 add exact zeros
    large_max_n=257, large_spectra=84, large_fits=70003,         # more workgroups than 65535
    every_single_fit_and_reversed=True,
    cuts=(5, 2, 1),
    nan_clean=_residues(2), nan_scenarios=('a', 'c'), part1_tol=(TOL_PARS, TOL_CHI2), observes_order_between=False)
FORMS = (WAVE, ROWS, WORKGROUP)


def order(form):
    """(n, s) of the form's spectra in batch order: per s the lengths from both ends inwards (4, 20001, 5, 4097, 6, 1000, ... at 64
    lanes), the middle length last when their count is odd"""
    ln = form.lengths
    per_s = [n for i in range(len(ln) // 2) for n in (ln[i], ln[-1 - i])] + list(ln[len(ln) // 2:(len(ln) + 1) // 2])
    return [(n, s) for s in range(SAMPLES) for n in per_s]


@functools.lru_cache(maxsize=None)
def batch(form):
    """(tape, order [(n, s)], truths [spectra][4], Batch)"""
    sp = [BC.spectrum_n(n, s) for n, s in order(form)]
    return trace_model(M.model_exp2, 4), order(form), np.array([it[0] for it in sp]), BC.Batch([it[1:4] for it in sp])


def starts(form, off, active=ACTIVE):
    """only the active parameters are moved off truth"""
    truths = batch(form)[2]
    out = truths.copy()
    out[:, active] = np.array([start_of(t, off) for t in truths])[:, active]
    return out


@functools.lru_cache(maxsize=None)
def selection(form, name, one_active=False):
    """batch_cases.select over the form's spectra under a scenario: [(kept, oracle result, self-difference, margin)]"""
    tape, _, _, b = batch(form)
    active = ONE_ACTIVE if one_active else ACTIVE
    off, kw = SCENARIOS[name]
    st = starts(form, off, active)
    return [BC.select(tape, *item, st[k], active, kw) for k, item in enumerate(b.items)]


def sub_batch(form, indices):
    """the spectra `indices` of the form's batch as a batch of their own, in that order"""
    items = batch(form)[3].items
    return BC.Batch([items[k] for k in indices])


def units(form):
    """[(tape, active list)]: every translation unit the suite of tests/batch_form_suite.py asks for per form (the 16- and 256-lane tests ask
    for the 64-lane form of them too; Part 3 runs at 64 lanes only: batch_cases.operator_units)"""
    tape = batch(form)[0]
    return [(tape, ACTIVE), (tape, ONE_ACTIVE)] + BC.part2_units()
