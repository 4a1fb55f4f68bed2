#!/bin/bash
# Round check: GPU parity tests, smoke(), the full default bench line, and a rocprofv3 kernel
# stats run of the bench workload.  usage: scripts/gpu_round.sh TAG [pytest -k expr]
# (logs under ${BA3C_OUT:-out}/TAG/)
set -o pipefail
T=${1:-r02}
K=${2:-}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
O=${BA3C_OUT:-out}/$T
mkdir -p $O
S=scripts/gpu_step.sh
export TMPDIR=/tmp     # rocprofv3's scratch files
if [ -n "$K" ]; then KA=(-k "$K"); else KA=(); fi
$S 900 $O/pytest_gpu.log python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread "${KA[@]}" && \
$S 300 $O/smoke.log python -c "import __graft_entry__ as g; g.smoke()" && \
$S 600 $O/bench.log python bench.py --full && \
$S 300 $O/rocprof.log rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o run -- python bench.py --steps 10 --warmup 2
tail -3 $O/pytest_gpu.log; tail -1 $O/smoke.log; grep '^{' $O/bench.log | cut -c1-1500
$S 300 $O/rocprof32.log rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats32 -o run -- python bench.py --batch 32 --fc_neurons 128 --fc_splits 4 --steps 50 --warmup 5
