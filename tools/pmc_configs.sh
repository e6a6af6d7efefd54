# HBM traffic of the dominant kernel of BASELINE configs 2 and 3 (the HBM-bound ones): separate --pmc passes of
# `bench.py --full --legs configs --only-config N` (FETCH_SIZE, WRITE_SIZE), per launch of gfh_k_sweep_gram (the stored form the line times);
# FETCH_SIZE x 2 on gfx950 (MI355X_MICROARCH.md, HBM section).  -> OUT_DIR/r06_configs_traffic.json (copied to profiles/)
# Usage: bash tools/pmc_configs.sh OUT_DIR   (relative to the repository root, or absolute)
OUT=${1:?usage: bash tools/pmc_configs.sh OUT_DIR}
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
mkdir -p "$OUT/pmc_cfg"
for c in 2 3; do
  for ctr in FETCH_SIZE WRITE_SIZE; do
    rocprofv3 --pmc $ctr --output-format csv -d "$OUT/pmc_cfg/cfg${c}_$ctr" -- python3 bench.py --full --legs configs --only-config $c > "$OUT/pmc_cfg/cfg${c}_$ctr.log" 2>&1
  done
done
python3 - "$OUT" <<'PY'
import csv, glob, json, collections, sys
d = sys.argv[1]
out = {}
for c in (2, 3):
    v = {}
    for ctr in ('FETCH_SIZE', 'WRITE_SIZE'):
        f = max(glob.glob('%s/pmc_cfg/cfg%d_%s/*/*_counter_collection.csv' % (d, c, ctr)), key=lambda p: __import__('os').path.getmtime(p))
        vals = [float(r['Counter_Value']) for r in csv.DictReader(open(f)) if r['Kernel_Name'] == 'gfh_k_sweep_gram' and r['Counter_Name'] == ctr]
        v[ctr] = sum(vals) / len(vals); v[ctr + '_launches'] = len(vals)
    out['cfg%d' % c] = dict(v, hbm_bytes_per_launch=2 * v['FETCH_SIZE'] * 1024 + v['WRITE_SIZE'] * 1024)
json.dump(out, open('%s/r06_configs_traffic.json' % d, 'w'), indent=1)
print(json.dumps(out))
PY
