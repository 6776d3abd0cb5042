#!/bin/bash
# GPU box: A/B of another build of the library against the tree's own on the inference step (bench.py's headline leg only):
# value, ms per step, the four block stages.   scripts/ab_block.sh <path of the other libepcnet_hip.so>
for i in 1 2; do for v in "" "$1"; do
  echo "lib ${v:-default}"
  EPCNET_LIB=$v python bench.py --full --no-configs --no-cpu-baseline --precision f32 --regions 3 2>/dev/null | python3 -c '
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d["value"], d["ms_per_step"], {k:v for k,v in d["stage_ms"].items() if k.startswith("block") or k=="knn"})'
done; done
