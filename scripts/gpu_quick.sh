#!/bin/bash
# Quick iteration: selected GPU tests (pytest -k expression, or all with "all"), then same-box
# A/B probes of kernels over library builds.
# usage: scripts/gpu_quick.sh TAG "KEXPR|all" "KERNEL[,KERNEL...]" LIB...
# (logs under ${BA3C_OUT:-out}/TAG/)
set -o pipefail
T=$1; K=$2; KS=$3; shift 3
O=${BA3C_OUT:-out}/$T
mkdir -p $O
S=scripts/gpu_step.sh
if [ "$K" = all ]; then KA=(); else KA=(-k "$K"); fi
$S 600 $O/pytest_gpu.log python -u -m pytest tests -m gpu -v --timeout 120 --timeout-method thread "${KA[@]}" || exit $?
grep -E "FAILED|ERROR" $O/pytest_gpu.log | head -20
tail -2 $O/pytest_gpu.log | head -1
for k in ${KS//,/ }; do
  bash scripts/gpu_abk.sh $T/ab_$k $k default "$@" || exit $?
done
