#!/bin/bash
# One call that produces the round's evidence (run from the repo root on a
# machine with the GPU): the -m gpu suite, the full bench line (bench.py --full), and
# the rocprofv3 kernel-stats / PMC passes of tools/profile_round.sh. Each step
# has its own time limit; the first failure ends the script. Logs go to
# $SEZKP_OUT (default out/).
set -euo pipefail
O=${SEZKP_OUT:-out}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread > $O/gpu_tests.log 2>&1
echo "tests ok"
timeout -k 10 400 python -u bench.py --full --detail $O/bench_detail.json > $O/bench.log 2> $O/bench.err
echo "bench ok"
bash tools/profile_round.sh
