#!/bin/bash
# DEVELOPER-ONLY: in-run A/B of switches on the headline workload (same box, alternating, settled)
# usage: bash tools/ab_spectrum.sh "ENV=.." "ENV=.. ENV2=.." ...
o=${OUT_DIR:-out}  # where the results land
mkdir -p "$o"
for rep in 1 2; do
  for v in "$@"; do
    env $v python3 bench.py --full --steps 300 --warmup 10 --headline-only --no-cpu-baseline > $o/ab.json 2>/dev/null || exit 1
    python3 -c "
import json,sys; d=json.load(open('$o/ab.json')); r=d['roofline']; print('$v', 'step', d['ms_per_step'], 'spectrum co', r['avg_launch_ms'], 'alone', r.get('avg_launch_ms_alone'))"
  done
done
