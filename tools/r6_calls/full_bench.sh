#!/bin/bash
# round 6: the default bench line (extra legs + CPU baseline), as the driver runs it
cd "${GRAFT_REPO_ROOT:-/root/repo}"
out=${BENCH_LOG_DIR:-bench_logs}
mkdir -p "$out"
timeout 1200 python bench.py --full > "$out/r6_bench.log" 2>&1
tail -c 3000 "$out/r6_bench.log"
