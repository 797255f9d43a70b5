#!/bin/bash
# Quick GPU pass: the -m gpu suite, then a short single-GPU bench (--full)
# without the CPU baseline / configs / worst case / host rows (stage times,
# throughput). Logs go to $SEZKP_OUT (default out/).
set -euo pipefail
O=${SEZKP_OUT:-out}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/gpu_tests.log 2>&1
echo "tests ok"
timeout -k 10 300 python -u bench.py --full --steps 100 --no-cpu-baseline --no-configs --no-worst-case --no-host-rows --detail $O/quick_detail.json > $O/quick.log 2> $O/quick.err
echo "bench ok"
