#!/bin/bash
# The factor-build traffic file of bench.py's `roofline.traffic`: FETCH_SIZE / WRITE_SIZE / SQ passes of the headline run
# and the --factor-build summary of tools/parse_pmc.py, written to OUT_DIR/syrk_pmc.json (commit it as
# profiles/r06_syrk_pmc.json)
#   bash tools/collect_syrk_pmc.sh OUT_DIR          (OUT_DIR relative to the repository root)
OUT=${1:?usage: bash tools/collect_syrk_pmc.sh OUT_DIR}
export TMPDIR=/tmp; cd "$(dirname "$0")/.." || exit 1
mkdir -p "$OUT"; rm -rf "$OUT/fetch" "$OUT/write" "$OUT/sq"
B="python3 bench.py"
timeout -k 10 600 $B --steps 1 --warmup 1 > "$OUT/warm.log" 2>&1 || exit $?
timeout -k 10 400 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$OUT/fetch" -- $B --steps 2 --warmup 1 > "$OUT/fetch.log" 2>&1 || exit $?
timeout -k 10 400 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$OUT/write" -- $B --steps 2 --warmup 1 > "$OUT/write.log" 2>&1 || exit $?
timeout -k 10 400 rocprofv3 --kernel-trace --pmc SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES --output-format csv -d "$OUT/sq" -- $B --steps 2 --warmup 1 > "$OUT/sq.log" 2>&1 || exit $?
python3 tools/parse_pmc.py "$OUT" --factor-build > "$OUT/syrk_pmc.json" || exit $?
rm -rf "$OUT/fetch" "$OUT/write" "$OUT/sq"
OUT="$OUT" python3 -c "
import json, os; d = json.load(open(os.path.join(os.environ['OUT'], 'syrk_pmc.json')))
print(d['source_sha16'], '%.2f GB per update' % (d['hbm_bytes_per_launch'] / 1e9))"
