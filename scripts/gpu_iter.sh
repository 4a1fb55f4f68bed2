#!/bin/bash
# Iteration run: GPU parity tests, then the bench (default and any A/B env given as args).
# usage: scripts/gpu_iter.sh TAG [ENV=VAL ...]   (logs under ${BA3C_OUT:-out}/TAG/)
set -o pipefail
tag=$1; shift
O=${BA3C_OUT:-out}/$tag
mkdir -p $O
S=scripts/gpu_step.sh
$S 600 $O/pytest_gpu.log python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread && \
$S 300 $O/bench.log python bench.py --full --no-cpu-baseline --no-overlap && \
for ab in "$@"; do
  $S 300 $O/bench_$ab.log env $ab python bench.py --full --no-cpu-baseline --no-overlap --no-b32 || exit $?
done
tail -3 $O/pytest_gpu.log
grep -h '^{' $O/bench*.log | python -c "
import sys,json
for l in sys.stdin:
    d=json.loads(l); print(d['value'], d['ms_per_step'], json.dumps(d.get('kernel_ms_per_step')))"
