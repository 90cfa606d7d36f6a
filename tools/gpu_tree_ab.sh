#!/bin/bash
# usage: OUT=<dir> tools/gpu_tree_ab.sh <tag> <other tree (path relative to the repo)> [rounds]  -- same-box interleaved A/B of the headline (bench.py --gpus 1:
# B = 64 tiles of 64 x 64 x 8, T = 1000) of THIS tree against ANOTHER checkout that carries its own built library (say `git archive <commit>` unpacked next to a
# build of that commit).  tools/gpu_lib_ab.sh swaps only the library under one binding, which stops working once a change adds exports (the binding resolves
# every symbol of include/ddif.h at load); this one runs each tree with its own binding.  One JSON line per run in $OUT, a summary line per run on stdout.
set -o pipefail
tag=$1; other=$2; rounds=${3:-3}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT:?set OUT to the directory the results are written to}" && cd "$OUT" && pwd)
for rep in $(seq 1 "$rounds"); do
  for v in this other; do
    if [ $v = other ]; then cd "$R/$other"; else cd "$R"; fi
    timeout -k 10 300 python3 bench.py --gpus 1 --steps 2 --warmup 1 --no-cpu-baseline 2> /dev/null | tail -1 > "$OUT/${tag}_${v}_$rep.json" || exit $?
    python3 -c "
import json; r=json.load(open('$OUT/${tag}_${v}_$rep.json')); print('$v', $rep, 'ms per job %.1f' % r['ms_per_step'], 'build', r.get('build_id'))"
  done
done
