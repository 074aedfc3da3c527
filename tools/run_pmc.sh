#!/bin/bash
# usage: tools/run_pmc.sh <tag> <out dir> <pmc counters...>   (run on the GPU box)
tag=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
out=$(mkdir -p "$1" && cd "$1" && pwd); shift
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d $out/$tag -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $out/$tag.log 2>&1
echo "$tag rc=$?"
