#!/bin/bash
# L2-miss (FETCH_SIZE) traffic of the factor-build kernels in a short bench.py --full run
#   bash tools/pmc_fetch_quick.sh OUT_DIR          (OUT_DIR relative to the repository root)
OUT=${1:?usage: bash tools/pmc_fetch_quick.sh OUT_DIR}
export TMPDIR=/tmp; cd "$(dirname "$0")/.." || exit 1
mkdir -p "$OUT"; rm -rf "$OUT/fetch"
timeout -k 10 600 python3 bench.py --full --no-cpu-baseline --steps 1 --warmup 1 > /dev/null 2>&1 || exit $?
timeout -k 10 400 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$OUT/fetch" -- python3 bench.py --full --no-cpu-baseline --steps 2 --warmup 1 > "$OUT/fetch.log" 2>&1 || exit $?
OUT="$OUT" python3 - <<'PY'
import csv, glob, collections, os
f = glob.glob(os.path.join(os.environ["OUT"], "fetch", "*", "*counter_collection.csv"))[0]
acc = collections.defaultdict(lambda: [0.0, 0])
for r in csv.DictReader(open(f)):
    if r["Counter_Name"] == "FETCH_SIZE" and "syrk" in r["Kernel_Name"]:
        k = r["Kernel_Name"].split("(")[0]
        acc[k][0] += float(r["Counter_Value"]); acc[k][1] += 1
for k, (v, n) in acc.items():
    print(f"{k}: FETCH_SIZE {v / n * 1024 / 1e9 * 1.0:.3f} GB per launch raw-KiB*1024 ({n} launches; gfx950 correction as in tools/parse_pmc.py not applied)")
PY
