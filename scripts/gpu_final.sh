#!/bin/bash
# Round-end check: GPU parity tests, smoke(), full bench line.  usage: scripts/gpu_final.sh TAG
# (logs under ${BA3C_OUT:-out}/TAG/)
set -o pipefail
T=${1:-r01final}
O=${BA3C_OUT:-out}/$T
mkdir -p $O
S=scripts/gpu_step.sh
$S 600 $O/pytest_gpu.log python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread && \
$S 300 $O/smoke.log python -c "import __graft_entry__ as g; g.smoke()" && \
$S 600 $O/bench.log python bench.py --full
tail -2 $O/pytest_gpu.log; tail -1 $O/smoke.log; grep '^{' $O/bench.log
