#!/bin/bash
# same-box A/B of bf16 plan knobs on one architecture: tools/ab_arch.sh <arch> "<ENV=1 ...>" ...   (first variant "" = default)
arch=$1; shift
for rep in 1 2; do
  for v in "" "$@"; do
    r=$(env $v python bench.py --full --arch $arch --steps 20 --warmup 5 --no-extra --no-cpu-baseline 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], d['roofline']['whole_net_frac'])")
    echo "rep $rep [${v:-default}] $r"
  done
done
