#!/bin/bash
# Recipe 1: the GPU test suite and the full bench line.   usage (on the GPU box): bash tools/run/tests_and_bench.sh <round> <out dir>
# (<out dir> relative to the repository root) -> <out dir>/<round>_gpu_tests.log, <out dir>/<round>_bench.json (copy the latter to profiles/<round>_final_bench.json)
R=${1:-r05}
OUT=${2:?usage: tools/run/tests_and_bench.sh <round> <out dir>}
cd "$(dirname "$0")/../.."
mkdir -p "$OUT"
python -m pytest tests -m gpu -q 2>&1 | tail -15 > "$OUT/${R}_gpu_tests.log"
python bench.py --full > "$OUT/${R}_bench.json" 2> "$OUT/${R}_bench.err"
tail -3 "$OUT/${R}_gpu_tests.log"; tail -c 400 "$OUT/${R}_bench.json"
