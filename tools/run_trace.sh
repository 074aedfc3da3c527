#!/bin/bash
# usage: tools/run_trace.sh <tag> <out dir> [bench args]   (GPU box): kernel-trace + stats of bench.py --full
tag=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
out=$(mkdir -p "$1" && cd "$1" && pwd); shift
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out/$tag -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline "$@" > $out/$tag.log 2>&1
echo "$tag rc=$?"
grep '^{' $out/$tag.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['kernel_us'])"
