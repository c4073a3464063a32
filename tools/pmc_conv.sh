#!/bin/bash
# FETCH_SIZE / WRITE_SIZE / TCC hit-miss passes (separate runs) on the 148^2 refinenet 3x3 conv
# (tools/pmc_conv.py) -> $OUT/pmc_conv.json (OUT defaults to profile_out).  Run on the GPU box from the repo root.
set -o pipefail
OUT="${OUT:-profile_out}"
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
mkdir -p "$OUT" || exit 1
for pass in "FETCH_SIZE:fetch" "WRITE_SIZE:write" "TCC_HIT_sum TCC_MISS_sum:hit"; do
  ctr=${pass%%:*}; d=${pass##*:}
  timeout -s KILL 90 rocprofv3 --pmc $ctr --output-format csv -d "$OUT/pmcc_$d" -o run \
    -- python3 tools/pmc_conv.py 5 > "$OUT/pmcc_$d.log" 2>&1 || exit 1
done
python3 tools/pmc_summary.py "$OUT/pmcc_fetch/run_counter_collection.csv" "$OUT/pmcc_write/run_counter_collection.csv" \
  "hconv" "$OUT/pmc_conv.json" $(( (3 * 32 * 148 * 148 * 256 + 9 * 256 * 256) * 2 )) "$OUT/pmcc_hit/run_counter_collection.csv"
