#!/bin/bash
# full validation of a tree on an MI355X: the GPU suite, smoke() and the whole benchmark (bench.py --full)
#   bash tools/gpu_full.sh OUT_DIR          (OUT_DIR relative to the repository root)
# A step that times out or crashes (abort, segmentation fault) ends the script: nothing more is started on the GPU.
OUT=${1:?usage: bash tools/gpu_full.sh OUT_DIR}
cd "$(dirname "$0")/.." || exit 1
mkdir -p "$OUT"

stop_on_crash() {
    case $1 in 124|134|137|139) echo "$2: rc=$1, stopping"; exit "$1";; esac
}

timeout -k 10 1500 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > "$OUT/pytest.txt" 2>&1
rc=$?; echo "pytest rc=$rc" >> "$OUT/pytest.txt"; stop_on_crash $rc pytest
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.txt" 2>&1
stop_on_crash $? smoke
timeout -k 10 900 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
stop_on_crash $? bench
grep -E "passed|failed|FAILED|rc=|Error" "$OUT/pytest.txt" | head -20; tail -2 "$OUT/smoke.txt"; cat "$OUT/bench.json"
