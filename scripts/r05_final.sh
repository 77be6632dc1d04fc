#!/bin/bash
# round-5 collection: all profiles (scripts/collect_profiles.sh r05) + the three-leg bench line + the NT GEMM table
set -e -o pipefail
bash scripts/collect_profiles.sh r05
PROF=$(ls -d ./*/prof_r05)      # the folder collect_profiles.sh filled above
python3 bench.py --full --steps 10 --warmup 3 > "$PROF/r05_bench_line.json" 2> "$PROF/bench.err" || { tail -20 "$PROF/bench.err"; exit 1; }
python3 scripts/perf_gemm_table.py > gpurun_out/prof_r05/r05_gemm_table.txt 2>&1
ls -la gpurun_out/prof_r05
