#!/bin/bash
# rocprofv3 kernel statistics of the anchor-map regime beside the 60-anchor permuted path (tools/gpu/anchor_map_time.py)
# usage: tools/gpu/anchor_map_trace.sh [OUT]   -> OUT (default ./anchor_map.txt; the record kept as profiles/anchor_map.txt)
set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
out=${1:-anchor_map.txt}
mkdir -p "$(dirname "$out")"
prof=$(mktemp -d)
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$prof" -o p --output-format csv -- python tools/gpu/anchor_map_time.py 2>&1 | grep anchors > "$out" || { echo "profiled run failed"; exit 1; }
f=$(find "$prof" -name "*kernel_stats.csv" | head -1)
python - "$f" >> "$out" <<'P'
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
steps = 5.0     # launches per configuration: one warm-up + four timed steps
print('\nrocprofv3 --kernel-trace --stats of that run (both anchor counts; per step = total / 5 steps):')
for r in rows[:32]:
    n = r['Name'].replace('(anonymous namespace)::', '').replace('void ', '')
    print(f"{n[:120]:120s} calls {r['Calls']:>4s} avg {float(r['AverageNs'])/1e6:8.3f} ms  per step {float(r['TotalDurationNs'])/1e6/steps:7.2f} ms")
P
cat "$out"
