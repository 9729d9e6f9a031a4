#!/bin/bash
# GPU box: the widened victim table.  Output: $O/part2.txt
# (The victim-side build variants this script once ran first were removed with their patch; they live in git history.)
cd "$(dirname "$0")/../.."
O=gpurun_out/r06_costream
mkdir -p $O
export WT_EXPERIMENT=1
{
for mt in 4 5 6; do
  for agg in res2 res4; do
    echo "== aggressor $agg MT=$mt"
    WD_SPLIT_MT=$mt AGGRESSOR=$agg timeout 600 python tools/costream/victims_table.py 2>&1 | tail -30
  done
done
echo "== control: no aggressor"
AGGRESSOR=none REPS=50 timeout 600 python tools/costream/victims_table.py 2>&1 | tail -30
echo "== positive control: MT=2 aggressor, all victims"
WD_SPLIT_MT=2 AGGRESSOR=res2 timeout 600 python tools/costream/victims_table.py 2>&1 | tail -30
} > $O/part2.txt 2>&1
