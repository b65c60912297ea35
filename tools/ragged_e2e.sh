#!/bin/bash
# End-to-end img/s (loader workers → pinned batches → copy stream → device augmentation → ResNet-50 step) of the three input-pipeline
# configs in ONE session, one after the other: uniform frames (head), ragged frames (simple family), ragged frames (body family, 256 x 256).
# Every run is a process of its own under its own time limit; a failing run ends the script.   tools/ragged_e2e.sh [out-file]
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/ragged_e2e.txt}
TMP=$(mktemp -d)
export PFR_LIMIT_TRAIN_BATCHES=${PFR_LIMIT_TRAIN_BATCHES:-60} PFR_VAL_IDS=${PFR_VAL_IDS:-8} PFR_WORKERS=${PFR_WORKERS:-16}
echo "# tools/ragged_e2e.sh: main.py --config, $PFR_LIMIT_TRAIN_BATCHES train batches of 256, $PFR_WORKERS loader workers; throughput clock starts after batch 5" > "$TMP/out"
run() {
  ( cd "$TMP" && timeout -k 10 420 python "$OLDPWD/main.py" --config "$OLDPWD/pets-face-recognition_amd/configs/synthetic/$1.py" ) > "$TMP/$1.log" 2>&1 || { tail -20 "$TMP/$1.log"; return 1; }
  echo "$1: $(grep -h 'train throughput' "$TMP/$1.log" | tail -1)" >> "$TMP/out"
}
run fe_r50_mi355x_pipeline && run fe_r50_mi355x_pipeline_simple && run fe_r50_mi355x_pipeline_body && cp "$TMP/out" "$OUT" && cat "$OUT"
