#!/bin/bash
# GPU parity tests, then the bench (default tree) and any A/B env settings given as args,
# each without the CPU baseline / overlap legs.  usage: scripts/gpu_ab.sh TAG [ENV=VAL ...]
# (logs under ${BA3C_OUT:-out}/TAG/)
set -o pipefail
tag=$1; shift
O=${BA3C_OUT:-out}/$tag
mkdir -p $O
S=scripts/gpu_step.sh
$S 900 $O/pytest_gpu.log python -u -m pytest tests -m gpu -v --timeout 240 --timeout-method thread
tail -1 $O/pytest_gpu.log
grep -E "^FAILED|^E  " $O/pytest_gpu.log | head -20
$S 300 $O/bench.log python bench.py --full --no-cpu-baseline --no-overlap || exit $?
for ab in "$@"; do
  $S 300 $O/bench_$ab.log env $ab python bench.py --full --no-cpu-baseline --no-overlap || exit $?
done
grep -h '^{' $O/bench*.log | python -c "
import sys,json
for l in sys.stdin:
    d=json.loads(l); print(d['value'], d['ms_per_step'], d['b32']['value'] if 'b32' in d else '', json.dumps(d.get('kernel_ms_per_step')))"
