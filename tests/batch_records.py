"""How the records of tools/bench_batch.py are read: when one form counts as faster than another, the auto rule that
profiles/batch_rows.json implies, and the cells of profiles/batch_workgroup.json.  tools/bench_batch.py writes its verdicts with the same
functions the CPU tests (tests/test_cpu_batch_rows.py, tests/test_cpu_batch_wg.py) read them with."""


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


# ---- profiles/batch_workgroup.json ------------------------------------------------------------------------------------------------
MUST_WIN = tuple((model, 256, points) for model in ('gauss4', 'exp4') for points in (16384, 65536))


def cell(record, model, fits, points):
    """the measurement of one (model, fits per launch, points per spectrum) of a record of tools/bench_batch.py --workgroup, or None"""
    for m in record['measurements']:
        if (m['model'], int(m['fits']), int(m['points'])) == (model, fits, points):
            return m
    return None
