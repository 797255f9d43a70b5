#!/bin/bash
# A/B (bound is the default since): bench process bound to the GPU's NUMA-local CPUs (SEZKP_BENCH_NUMA=1)
# vs the scheduler's choice (default), alternating default-length lines (bench.py --full: the
# host -> proof and single-proof figures are read too). Results go to $SEZKP_OUT (default out/).
set -euo pipefail
O=${SEZKP_OUT:-out}
mkdir -p $O
for v in 0 1 0 1 0 1; do
  echo -n "$v " >> $O/ab_numa.txt
  SEZKP_BENCH_NUMA=$v timeout -k 10 300 python3 bench.py --full --no-cpu-baseline --no-configs --dntt-log-n 0 --detail $O/ab_numa_detail.json 2>/dev/null | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['host_to_proof']['value'], d['single_proof']['ms_per_proof'], json.load(open(d['detail'])).get('numa'))" >> $O/ab_numa.txt
done
echo done
