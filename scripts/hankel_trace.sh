#!/bin/bash
# Kernel time of the Hankel propagator: one rocprofv3 kernel trace per shape (tracing only, no counters), then the
# summary appended to the timing file.  Run on the GPU after scripts/hankel_timing.py:
#   scripts/hankel_trace.sh OUTDIR TIMING_FILE
set -o pipefail
out=${1:-hankel_trace}
timing=${2:-profiles/hankel_timing.txt}
for shape in 512,1,512 512,32,512 512,32,1 2048,1,2048 2048,32,2048 2048,1,1 2048,32,1 4096,1,4096 4096,32,4096 4096,1,1 4096,32,1; do
  d="$out/${shape//,/_}"
  mkdir -p "$d"
  timeout -k 10 120 rocprofv3 --kernel-trace --stats -d "$d" -o run --output-format csv -- \
    python3 scripts/hankel_timing.py --trace "$shape" > "$d/log.txt" 2>&1 || exit $?
done
timeout -k 10 60 python3 scripts/hankel_timing.py --trace-summary "$out" --out "$timing"
